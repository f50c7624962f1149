// host_sanitize_direct_light.cpp — the host paths of RT_RADIANCE_DIRECT_LIGHT (rt_radiance_rays' argument checks with the
// flag) and of rt_scene_lights_host (validation, the list, the capacity rule, tuning independence) in the
// AddressSanitizer + UndefinedBehaviorSanitizer build of the library, beside host_sanitize_radiance.cpp.  Built and run
// by `make -C cudaraytracer_amd/csrc asan`; no GPU is needed.  Exit status 0 = every check held and the sanitizers
// reported nothing.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
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

// A rejection: RT_ERR_INVALID_ARGUMENT with the function's name and `what` in the message.
#define REJECTED(who, call, what)                                  \
    do {                                                           \
        CHECK((call) == RT_ERR_INVALID_ARGUMENT);                  \
        CHECK(std::strstr(rt_last_error(), who) != nullptr);       \
        CHECK(std::strstr(rt_last_error(), what) != nullptr);      \
    } while (0)

// The flag's checks run with the others: before the first device call and before the scene is read.
static void flag_arguments() {
    const char* who = "rt_radiance_rays";
    const uint32_t n = 96;
    std::vector<float> rays(n * 8), sum(n * 4), mean(n * 4);
    std::vector<uint32_t> ids(n);
    std::vector<uint64_t> counters(RT_COUNTERS_WORDS);
    rt_radiance_args q{};
    q.rays = rays.data();
    q.stream_ids = ids.data();
    q.sum = sum.data();
    q.mean = mean.data();
    q.counters = counters.data();
    q.n = n;
    q.samples_per_ray = 1;
    q.max_depth = 8;
    q.flags = RT_RADIANCE_DIRECT_LIGHT;
    const rt_scene* fake = reinterpret_cast<const rt_scene*>(&q);
    REJECTED(who, rt_radiance_rays(nullptr, &q, nullptr), "NULL scene");  // the flag is valid
    rt_radiance_args b = q;
    b.flags = RT_RADIANCE_DIRECT_LIGHT | RT_FLAG_RIUS_LEFT_TO_RIGHT;
    b.max_depth = 4096;
    b.count_tests = 1;
    REJECTED(who, rt_radiance_rays(nullptr, &b, nullptr), "NULL scene");  // ... with the fill order, at the depth limit
    for (uint32_t bad : {4097u, 0x10000u, 0xffffffffu}) {
        b = q;
        b.max_depth = bad;
        REJECTED(who, rt_radiance_rays(fake, &b, nullptr), "max_depth");
        b.flags = 0;  // (without the flag the depth is not limited)
        REJECTED(who, rt_radiance_rays(nullptr, &b, nullptr), "NULL scene");
    }
    for (uint32_t bad : {1u, 2u, 4u, 16u, (uint32_t)RT_FLAG_RNG_PHILOX, 64u, 128u, 512u, 0x80000000u}) {
        b = q;
        b.flags = RT_RADIANCE_DIRECT_LIGHT | bad;
        REJECTED(who, rt_radiance_rays(fake, &b, nullptr), "flags");
    }
    for (int k = 0; k < 3; k++) {
        b = q;
        b.reserved[k] = 1;
        REJECTED(who, rt_radiance_rays(fake, &b, nullptr), "reserved");
    }
    b = q;
    b.n = 0;  // nothing to trace: no device call, the scene is not read
    CHECK(rt_radiance_rays(nullptr, &b, nullptr) == RT_OK);
    b.max_depth = 4097;  // ... but the arguments are still checked
    REJECTED(who, rt_radiance_rays(nullptr, &b, nullptr), "max_depth");
}

static rt_material_desc mat(int32_t type, int32_t intensity) {
    rt_material_desc m{};
    m.type = type;
    m.ir = 1.5f;
    m.light_intensity = intensity;
    m.albedo.type = RT_CONSTANT;
    m.albedo.image = -1;
    m.albedo.color[0] = m.albedo.color[1] = m.albedo.color[2] = 0.5f;
    return m;
}

static rt_hittable_desc rect(int32_t type, float x, float y, float z, float w, float h, int32_t material, int32_t active = 1) {
    rt_hittable_desc r{};
    r.type = type;
    r.is_active = active;
    r.center[0] = x;
    r.center[1] = y;
    r.center[2] = z;
    r.width = w;
    r.height = h;
    r.material = material;
    return r;
}

static rt_hittable_desc ball(float x, float y, float z, float radius, int32_t material) {
    rt_hittable_desc s{};
    s.type = RT_SPHERE;
    s.is_active = 1;
    s.center[0] = x;
    s.center[1] = y;
    s.center[2] = z;
    s.radius = radius;
    s.material = material;
    return s;
}

static void light_lists() {
    const char* who = "rt_scene_lights_host";
    std::vector<rt_material_desc> mats = {mat(RT_LAMBERTIAN, 0), mat(RT_DIFFUSELIGHT, 4), mat(RT_DIFFUSELIGHT, 0)};
    std::vector<rt_hittable_desc> hs = {
        ball(0, 3, 0, 0.5f, 1),                        // 0: a light, but a sphere
        rect(RT_XZRECT, 0, 0, 0, 10, 10, 0),           // 1: Lambertian
        rect(RT_YZRECT, 2, 1, 0, 0.5f, 0.5f, 1),       // 2: valid
        rect(RT_XZRECT, 0, 2, 0, 1, 1, 1, 0),          // 3: inactive
        rect(RT_XZRECT, 1, 2, 0, 0, 1, 1),             // 4: zero width
        rect(RT_XYRECT, 0, 1, -2, 0.5f, 0.25f, 1),     // 5: valid
        rect(RT_XZRECT, -1, 2, 0, 1, 1, 2),            // 6: intensity 0
        rect(RT_XYRECT, 1, 1, -2, 1, -1, 1),           // 7: negative height
        rect(RT_XZRECT, 0.5f, 2, 0.5f, 0.6f, 0.4f, 1)  // 8: valid
    };
    for (int k = 0; k < 40; k++) hs.push_back(ball(0.3f * k - 6, 0.2f, 1.0f, 0.1f, 0));
    rt_scene_desc d{};
    d.hittables = hs.data();
    d.num_hittables = (uint32_t)hs.size();
    d.materials = mats.data();
    d.num_materials = (uint32_t)mats.size();
    uint32_t count = 77;
    CHECK(rt_scene_lights_host(&d, nullptr, 0, &count) == RT_OK && count == 3);
    for (uint32_t cap = 0; cap <= 5; cap++) {  // exactly min(N_L, capacity) entries, in exactly `capacity` words of heap
        std::vector<uint32_t> out(cap, 0xa5a5a5a5u);
        count = 0;
        CHECK(rt_scene_lights_host(&d, out.data(), cap, &count) == RT_OK && count == 3);
        const uint32_t want[3] = {2, 5, 8};
        for (uint32_t i = 0; i < cap; i++) CHECK(out[i] == (i < 3 ? want[i] : 0xa5a5a5a5u));
    }
    for (int leaf_max = 1; leaf_max <= 4; leaf_max++) {  // the list does not depend on the BVH
        const int prev = rt_set_tuning(RT_TUNE_LEAF_MAX, leaf_max);
        uint32_t out[3] = {0, 0, 0};
        CHECK(rt_scene_lights_host(&d, out, 3, &count) == RT_OK && count == 3 && out[0] == 2 && out[1] == 5 && out[2] == 8);
        rt_set_tuning(RT_TUNE_LEAF_MAX, prev);
    }
    mats[2].light_intensity = 1;  // a material edit: 6 becomes a light
    mats[1].type = RT_METAL;      // ... and 2, 5, 8 stop being lights
    uint32_t one[2] = {0, 0xa5a5a5a5u};
    CHECK(rt_scene_lights_host(&d, one, 1, &count) == RT_OK && count == 1 && one[0] == 6 && one[1] == 0xa5a5a5a5u);
    // errors: the call's own, then rt_scene_create's
    REJECTED(who, rt_scene_lights_host(&d, nullptr, 0, nullptr), "NULL count");
    REJECTED(who, rt_scene_lights_host(&d, nullptr, 2, &count), "NULL");
    REJECTED(who, rt_scene_lights_host(nullptr, nullptr, 0, &count), "NULL");
    rt_scene_desc bad = d;
    bad.hittables = nullptr;
    REJECTED(who, rt_scene_lights_host(&bad, nullptr, 0, &count), "NULL array");
    hs[5].material = 3;
    CHECK(rt_scene_lights_host(&d, nullptr, 0, &count) == RT_ERR_INVALID_SCENE && std::strstr(rt_last_error(), "material index"));
    hs[5].material = 1;
    hs[8].width = NAN;
    CHECK(rt_scene_lights_host(&d, nullptr, 0, &count) == RT_ERR_INVALID_SCENE && std::strstr(rt_last_error(), "non-finite"));
    hs[8].width = 0.6f;
    hs[2].type = 9;
    CHECK(rt_scene_lights_host(&d, nullptr, 0, &count) == RT_ERR_INVALID_SCENE);
    hs[2].type = RT_YZRECT;
    mats[0].type = 7;
    CHECK(rt_scene_lights_host(&d, nullptr, 0, &count) == RT_ERR_INVALID_SCENE);
    mats[0].type = RT_LAMBERTIAN;
    // empty and all-inactive scenes: no lights
    rt_scene_desc empty{};
    empty.materials = mats.data();
    empty.num_materials = (uint32_t)mats.size();
    count = 9;
    CHECK(rt_scene_lights_host(&empty, nullptr, 0, &count) == RT_OK && count == 0);
    for (rt_hittable_desc& h : hs) h.is_active = 0;
    count = 9;
    CHECK(rt_scene_lights_host(&d, nullptr, 0, &count) == RT_OK && count == 0);
}

int main() {
    flag_arguments();
    light_lists();
    if (failures) {
        std::fprintf(stderr, "%d check(s) failed\n", failures);
        return 1;
    }
    std::printf("host_sanitize_direct_light: all checks passed\n");
    return 0;
}
