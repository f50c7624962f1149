// host_sanitize_bounce_class.cpp — the host builder of the bounce entries' direction classes (scene_build.cpp,
// rt_bounce_class_entries_host, rt_set_bounce_classes) in the AddressSanitizer + UndefinedBehaviorSanitizer build of the
// library, beside host_sanitize.cpp: RTIOW and a field of 3 000 small spheres in every form, the fall-back of form 2 at
// a lowered node limit, a scene with 32-bit references, the classes of a batch of rays and the argument checks.  Built
// and run by `make -C cudaraytracer_amd/csrc asan`; no GPU is needed.  Exit status 0 = every check held and the
// sanitizers reported nothing.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "../../include/rt_hip.h"

static int failures = 0;
#define CHECK(cond)                                                                  \
    do {                                                                             \
        if (!(cond)) {                                                               \
            std::fprintf(stderr, "CHECK failed at line %d: %s (%s)\n", __LINE__, #cond, \
                         rt_last_error());                                           \
            failures++;                                                              \
        }                                                                            \
    } while (0)

struct Scene {
    std::vector<rt_hittable_desc> h;
    std::vector<rt_material_desc> m;
    rt_scene_desc desc() const {
        rt_scene_desc d{};
        d.hittables = h.data();
        d.num_hittables = (uint32_t)h.size();
        d.materials = m.data();
        d.num_materials = (uint32_t)m.size();
        return d;
    }
};

static Scene rtiow() {
    Scene s;
    uint32_t nh = 0, nm = 0;
    CHECK(rt_builtin_scene(2, 1, nullptr, &nh, nullptr, &nm) == RT_OK);
    s.h.resize(nh);
    s.m.resize(nm);
    CHECK(rt_builtin_scene(2, 1, s.h.data(), &nh, s.m.data(), &nm) == RT_OK);
    return s;
}

// n small spheres over a ground sphere (cudaraytracer_amd/scenes.py sphere_field's shape, its own numbers)
static Scene field(const uint32_t n) {
    Scene s;
    s.m.resize(1);
    std::memset(s.m.data(), 0, sizeof(rt_material_desc));
    s.m[0].type = RT_LAMBERTIAN;
    s.m[0].albedo.type = RT_CONSTANT;
    s.m[0].albedo.image = -1;
    s.m[0].albedo.color[0] = s.m[0].albedo.color[1] = s.m[0].albedo.color[2] = 0.5f;
    s.h.resize(n + 1);
    std::memset(s.h.data(), 0, s.h.size() * sizeof(rt_hittable_desc));
    uint32_t x = 12345u;
    const auto next = [&x]() {  // uniform in [0, 1)
        x = x * 1664525u + 1013904223u;
        return (float)(x >> 8) * 0x1p-24f;
    };
    for (uint32_t i = 0; i <= n; i++) {
        rt_hittable_desc& h = s.h[i];
        h.type = RT_SPHERE;
        h.is_active = 1;
        if (i == 0) {
            h.center[1] = -1000.0f;
            h.radius = 1000.0f;
        } else {
            h.center[0] = -11.0f + 22.0f * next();
            h.center[1] = 0.05f + 2.45f * next();
            h.center[2] = -11.0f + 22.0f * next();
            h.radius = 0.03f + 0.12f * next();
        }
    }
    return s;
}

struct Built {
    rt_bounce_class_info info{};
    std::vector<uint32_t> records, refs;
    std::vector<float> nodes48;
    std::vector<double> regions;
};

static Built build(const Scene& s, const int form, const uint32_t node_limit) {
    Built b;
    const rt_scene_desc d = s.desc();
    CHECK(rt_bounce_class_entries_host(&d, form, node_limit, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0,
                                       nullptr, &b.info) == RT_OK);
    // exactly the sizes the header states: the sanitizer sees a write past any of them
    b.records.resize((size_t)b.info.num_records * 25 * 4);
    b.nodes48.resize((size_t)b.info.num_class_nodes * 12);
    b.refs.resize(b.info.num_class_nodes);
    b.regions.resize((size_t)b.info.num_records * 6);
    CHECK(rt_bounce_class_entries_host(&d, form, node_limit, b.records.data(), b.nodes48.data(), b.refs.data(),
                                       b.regions.data(), nullptr, nullptr, 0, nullptr, &b.info) == RT_OK);
    return b;
}

static void forms(const Scene& s, const char* name) {
    const rt_scene_desc d = s.desc();
    rt_bounce_entries_info e{};
    CHECK(rt_bounce_entries_host(&d, nullptr, nullptr, nullptr, nullptr, nullptr, &e) == RT_OK);
    CHECK(e.num_records > 0);
    // rt_bounce_entries_host's arrays keep their sizes whatever the thread's form is (the class nodes are not copied)
    for (int form = 0; form <= 2; form++) {
        CHECK(rt_set_bounce_classes(form) >= 0);
        const size_t total = (size_t)e.num_nodes + e.num_chain_nodes;
        std::vector<float> chain((size_t)e.num_chain_nodes * 16), n48(total * 12);
        std::vector<uint32_t> refs(total), rec((size_t)e.num_records * 4);
        std::vector<uint16_t> grid((size_t)e.grid_dim[0] * e.grid_dim[1] * e.grid_dim[2]);
        rt_bounce_entries_info e2{};
        CHECK(rt_bounce_entries_host(&d, chain.data(), n48.data(), refs.data(), rec.data(), grid.data(), &e2) == RT_OK);
        CHECK(e2.num_chain_nodes == e.num_chain_nodes && e2.num_records == e.num_records);
    }
    CHECK(rt_set_bounce_classes(0) == 2);
    const Built off = build(s, 0, 0), one = build(s, 1, 0), two = build(s, 2, 0);
    CHECK(off.info.form == 0 && off.info.num_class_nodes == 0 && off.info.num_records == e.num_records);
    CHECK(one.info.form == 1 && one.info.num_class_nodes == 0 && one.info.num_records == e.num_records);
    CHECK(two.info.form == 2 && two.info.num_class_nodes > 0);
    CHECK(two.info.first_class_node == e.num_nodes + e.num_chain_nodes);
    // every reference of a class record names a leaf, a node of the table or the pad
    const uint32_t nodes = two.info.first_class_node + two.info.num_class_nodes;
    size_t shorter = 0;
    for (size_t i = 0; i < two.records.size(); i++)
        for (int half = 0; half < 2; half++) {
            const uint32_t r = (two.records[i] >> (16 * half)) & 0xffffu;
            CHECK(r >= 0x8000u || r == 0x7fffu || r < nodes);
            if (r == 0x7fffu) shorter++;
        }
    CHECK(shorter > 0);
    // form 2 at a node limit it just fits, and one below: the fall-back to form 1
    const Built fits = build(s, 2, nodes + 1), back = build(s, 2, nodes);
    CHECK(fits.info.form == 2 && fits.records == two.records);
    CHECK(back.info.form == 1 && back.info.num_class_nodes == 0 && back.records == one.records);
    std::printf("%s: %u records, %u class nodes (form 2)\n", name, two.info.num_records, two.info.num_class_nodes);
}

static void ray_classes(const Scene& s) {
    const rt_scene_desc d = s.desc();
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    const float o[] = {0.0f, 0.5f, 0.0f, 0.0f, 0.5f, 0.0f, 0.0f, 0.5f, 0.0f, nan, 0.5f, 0.0f, 1e30f, 0.5f, 0.0f, 0.0f, 0.5f, 0.0f};
    const float v[] = {0.3f, 1.0f, -0.2f, 0.0f, 1.0f, 0.2f, inf, 1.0f, 0.2f, 0.3f, 1.0f, -0.2f, 0.3f, 1.0f, -0.2f, -1.0f, 0.5f, 0.5f};
    uint32_t cls[6] = {99, 99, 99, 99, 99, 99};
    rt_bounce_class_info info{};
    CHECK(rt_bounce_class_entries_host(&d, 1, 0, nullptr, nullptr, nullptr, nullptr, o, v, 6, cls, &info) == RT_OK);
    CHECK(cls[0] == 12 && cls[1] == 24 && cls[2] == 24 && cls[3] == 24 && cls[4] == 24 && cls[5] == 1);
    CHECK(rt_bounce_class_entries_host(&d, 1, 0, nullptr, nullptr, nullptr, nullptr, nullptr, v, 6, cls, &info) == RT_OK);
    CHECK(cls[0] == 12 && cls[3] == 12 && cls[4] == 12);
}

static void arguments(const Scene& s) {
    const rt_scene_desc d = s.desc();
    rt_bounce_class_info info{};
    const float v[3] = {1.0f, 1.0f, 1.0f};
    uint32_t cls = 0;
    CHECK(rt_bounce_class_entries_host(&d, 1, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, nullptr, nullptr) ==
          RT_ERR_INVALID_ARGUMENT);
    CHECK(rt_bounce_class_entries_host(&d, 3, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, nullptr, &info) ==
          RT_ERR_INVALID_ARGUMENT);
    CHECK(rt_bounce_class_entries_host(&d, -2, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, nullptr, &info) ==
          RT_ERR_INVALID_ARGUMENT);
    CHECK(rt_bounce_class_entries_host(&d, 1, 0x8000u, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, nullptr,
                                       &info) == RT_ERR_INVALID_ARGUMENT);
    CHECK(rt_bounce_class_entries_host(&d, 1, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 1, &cls, &info) ==
          RT_ERR_INVALID_ARGUMENT);
    CHECK(rt_bounce_class_entries_host(&d, 1, 0, nullptr, nullptr, nullptr, nullptr, nullptr, v, 1, nullptr, &info) ==
          RT_ERR_INVALID_ARGUMENT);
    CHECK(rt_bounce_class_entries_host(nullptr, 1, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, nullptr,
                                       &info) != RT_OK);
    CHECK(rt_set_bounce_classes(-1) == RT_ERR_INVALID_ARGUMENT && rt_set_bounce_classes(3) == RT_ERR_INVALID_ARGUMENT);
    CHECK(std::strstr(rt_last_error(), "rt_set_bounce_classes") != nullptr);
    // a scene with 32-bit references: no table in any form, and no classes to ask for
    const Scene big = field(9000);
    const rt_scene_desc bd = big.desc();
    for (int form = 0; form <= 2; form++) {
        CHECK(rt_bounce_class_entries_host(&bd, form, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, nullptr,
                                           &info) == RT_OK);
        CHECK(info.form == 0 && info.num_records == 0 && info.num_class_nodes == 0);
    }
    CHECK(rt_bounce_class_entries_host(&bd, 1, 0, nullptr, nullptr, nullptr, nullptr, v, v, 1, &cls, &info) ==
          RT_ERR_INVALID_ARGUMENT);
}

int main() {
    const Scene r = rtiow(), f = field(3000);
    forms(r, "rtiow");
    forms(f, "field");
    ray_classes(r);
    arguments(r);
    if (failures) {
        std::fprintf(stderr, "%d check(s) failed\n", failures);
        return 1;
    }
    std::printf("host_sanitize_bounce_class: all checks passed\n");
    return 0;
}
