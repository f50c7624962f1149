// host_sanitize_dynamic.cpp — the host paths of rt_scene_motion (every rule of the table), rt_temporal_dynamic (argument
// checks, the launch's error path) and rt_scene_edit (argument checks) in the AddressSanitizer +
// UndefinedBehaviorSanitizer build of the library, beside host_sanitize.cpp, host_sanitize_denoise.cpp and
// host_sanitize_temporal.cpp.  Built and run by `make -C cudaraytracer_amd/csrc asan`; no GPU is needed.  Exit status
// 0 = every check held and the sanitizers reported nothing.
#include <cmath>
#include <cstdio>
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

static rt_hittable_desc hittable(int type, float x, float y, float z, float radius, float width, float height) {
    rt_hittable_desc h{};
    h.type = type;
    h.is_active = 1;
    h.center[0] = x;
    h.center[1] = y;
    h.center[2] = z;
    h.radius = radius;
    h.width = width;
    h.height = height;
    return h;
}

static bool is(const float* m, float x, float y, float z, float s) {
    const float want[4] = {x, y, z, s};
    return std::memcmp(m, want, sizeof(want)) == 0;
}

// rt_scene_motion touches no device: every rule, on one list.
static void motion() {
    const rt_hittable_desc sphere = hittable(RT_SPHERE, 1.1f, -0.35f, 0.6f, 0.65f, 0, 0);
    const rt_hittable_desc rect = hittable(RT_XZRECT, 1.0f, 2.6f, -1.0f, 0, 2.0f, 3.0f);
    std::vector<rt_hittable_desc> prev, cur;
    const auto add = [&](const rt_hittable_desc& p, const rt_hittable_desc& c) {
        prev.push_back(p);
        cur.push_back(c);
    };
    rt_hittable_desc h = sphere;
    add(sphere, sphere);  // 0: at rest
    h.center[0] = 1.25f;
    h.center[2] = 0.5f;
    add(sphere, h);  // 1: translated
    h = sphere;
    h.radius = 0.5f;
    add(sphere, h);  // 2: resized
    h = rect;
    h.center[0] = 0.8f;
    add(rect, h);  // 3: a rectangle moved
    h = rect;
    h.width = 2.5f;
    add(rect, h);  // 4: resized: no history
    h = rect;
    h.type = RT_XYRECT;
    add(rect, h);  // 5: another type
    h = sphere;
    h.is_active = 0;
    add(sphere, h);  // 6, 7: inactive on either side
    add(h, sphere);
    h = sphere;
    h.radius = 0.0f;
    add(sphere, h);  // 8, 9: radius 0 on either side
    add(h, sphere);
    h = sphere;
    h.material = 3;
    add(sphere, h);  // 10: a material edit is the caller's to zero
    add(rect, rect);  // 11
    h = sphere;
    h.type = 17;
    add(h, h);  // 12: not a hittable type
    const uint32_t n = (uint32_t)cur.size();
    std::vector<float> table(4 * (size_t)n, -1.0f);
    CHECK(rt_scene_motion(prev.data(), cur.data(), n, table.data()) == RT_OK);
    const float* m = table.data();
    CHECK(is(m + 0, 0, 0, 0, 1));
    CHECK(is(m + 4, 1.1f - 1.25f, 0.0f, 0.6f - 0.5f, 1));
    const float s = 0.65f / 0.5f;
    const volatile float sx = s * 1.1f, sy = s * -0.35f, sz = s * 0.6f;  // (one rounding each, then the subtraction)
    CHECK(is(m + 8, 1.1f - sx, -0.35f - sy, 0.6f - sz, s));
    CHECK(is(m + 12, 1.0f - 0.8f, 0.0f, 0.0f, 1));
    for (int i : {4, 5, 6, 7, 8, 9, 12}) CHECK(is(m + 4 * i, 0, 0, 0, 0));
    CHECK(is(m + 40, 0, 0, 0, 1));
    CHECK(is(m + 44, 0, 0, 0, 1));
    CHECK(rt_scene_motion(nullptr, cur.data(), n, table.data()) == RT_ERR_INVALID_ARGUMENT);
    CHECK(rt_scene_motion(prev.data(), nullptr, n, table.data()) == RT_ERR_INVALID_ARGUMENT);
    CHECK(rt_scene_motion(prev.data(), cur.data(), n, nullptr) == RT_ERR_INVALID_ARGUMENT);
    CHECK(std::strstr(rt_last_error(), "rt_scene_motion") != nullptr);
    CHECK(rt_scene_motion(nullptr, nullptr, 0, nullptr) == RT_OK);
    // exactly n entries are written
    std::vector<float> two(8, -1.0f);
    CHECK(rt_scene_motion(prev.data(), cur.data(), 1, two.data()) == RT_OK);
    CHECK(is(two.data(), 0, 0, 0, 1) && is(two.data() + 4, -1, -1, -1, -1));
}

static bool rejected(const rt_temporal_args& a, const float* table, uint32_t n, const char* word) {
    return rt_temporal_dynamic(&a, table, n, nullptr) == RT_ERR_INVALID_ARGUMENT &&
           std::strstr(rt_last_error(), word) != nullptr;
}

// Every argument check runs before the first device call, so a GPU-less host sees status codes.
static void temporal_dynamic() {
    const uint32_t W = 16, H = 8, N = 4;
    std::vector<float> color(W * H * 4), nd(W * H * 4), prev_hist(W * H * 4), prev_nd(W * H * 4), hist(W * H * 4);
    std::vector<float> motion(W * H * 2);
    std::vector<int32_t> ids(W * H), prev_ids(W * H);
    std::vector<uint32_t> pos(W * H);
    alignas(16) float table[4 * N] = {0, 0, 0, 1, 0.5f, 0, 0, 1, 0, 0, 0, 0, 1, 2, 3, 1.5f};
    const float eye[3] = {0, 2, 12}, fwd[3] = {0, 0, -1}, up[3] = {0, 1, 0}, bg[3] = {1, 1, 1};
    rt_temporal_args a{};
    a.color = color.data();
    a.normal_depth = nd.data();
    a.prim_id = ids.data();
    a.prev_history = prev_hist.data();
    a.prev_normal_depth = prev_nd.data();
    a.prev_prim_id = prev_ids.data();
    a.history = hist.data();
    a.motion = motion.data();
    a.pos = pos.data();
    a.width = W;
    a.height = H;
    a.max_history = 32;
    a.depth_tol = 0.05f;
    a.normal_tol = 0.2f;
    a.tiling = rt_tiling{H, 1, 0, H};
    rt_camera_inputs(eye, fwd, up, 45.0f, 0.1f, 10.0f, bg, bg, &a.inputs);
    a.prev_inputs = a.inputs;

    CHECK(rt_temporal_dynamic(nullptr, table, N, nullptr) == RT_ERR_INVALID_ARGUMENT);
    CHECK(std::strstr(rt_last_error(), "rt_temporal_dynamic") != nullptr);
    // the table's own checks
    CHECK(rejected(a, nullptr, N, "prim_motion"));
    CHECK(rejected(a, table + 1, N - 1, "aligned"));
    // (std::vector storage of these sizes is 16-byte aligned: operator new's guarantee)
    CHECK(rejected(a, hist.data(), N, "overlaps"));
    CHECK(rejected(a, hist.data() + 4 * (W * H - 1), N, "overlaps"));
    CHECK(rejected(a, motion.data() + 8, 1, "overlaps"));
    CHECK(rejected(a, (const float*)pos.data(), 2, "overlaps"));
    // rt_temporal's checks, under this entry point's name
    rt_temporal_args b = a;
    b.color = nullptr;
    CHECK(rejected(b, table, N, "NULL"));
    b = a;
    b.history = nullptr;
    CHECK(rejected(b, table, N, "history"));
    b = a;
    b.prev_prim_id = nullptr;
    CHECK(rejected(b, table, N, "prev_"));
    b = a;
    b.flags = 1u << 2;
    CHECK(rejected(b, table, N, "flags"));
    b = a;
    b.max_history = 4097;
    CHECK(rejected(b, table, N, "max_history"));
    b = a;
    b.depth_tol = std::nanf("");
    CHECK(rejected(b, table, N, "tol"));
    b = a;
    b.reserved[1] = 1;
    CHECK(rejected(b, table, N, "reserved"));
    b = a;
    b.tiling = rt_tiling{4, 2, 0, 4};
    CHECK(rejected(b, table, N, "tiling"));
    b = a;
    b.history = prev_hist.data() + 4 * 5;
    CHECK(rejected(b, table, N, "alias"));
    b = a;
    b.width = 0;  // an empty frame: nothing to do, no device call; the table is still checked
    CHECK(rt_temporal_dynamic(&b, table, N, nullptr) == RT_OK);
    CHECK(rt_temporal_dynamic(&b, table, 0, nullptr) == RT_OK);
    CHECK(rejected(b, nullptr, N, "prim_motion"));
    b.flags = RT_TEMPORAL_RESET;  // ... which RT_TEMPORAL_RESET makes optional
    CHECK(rt_temporal_dynamic(&b, nullptr, 0, nullptr) == RT_OK);

    // The launch's error path.  Only where no device is usable: the planes above are host memory, which a kernel must
    // never be handed, and without a device the launch fails before any kernel runs and must come back as a status.
    if (rt_set_device(0) != RT_OK) {
        CHECK(rt_temporal_dynamic(&a, table, N, nullptr) == RT_ERR_LAUNCH);
        CHECK(std::strstr(rt_last_error(), "rt_temporal_dynamic: kernel launch") != nullptr);
        b = a;
        b.flags = RT_TEMPORAL_RESET;
        b.prev_history = nullptr;
        b.prev_normal_depth = nullptr;
        b.prev_prim_id = nullptr;
        CHECK(rt_temporal_dynamic(&b, nullptr, 0, nullptr) == RT_ERR_LAUNCH);
    } else {
        std::printf("host_sanitize_dynamic: a device is present, the launch error path is not exercised\n");
    }
}

// rt_scene_edit without a base scene (creating one needs a device): the NULL checks, and that `out` is cleared.
static void scene_edit() {
    rt_hittable_desc h = hittable(RT_SPHERE, 0, 0, 0, 1, 0, 0);
    rt_scene* out = reinterpret_cast<rt_scene*>(&h);
    CHECK(rt_scene_edit(nullptr, &h, 1, &out) == RT_ERR_INVALID_ARGUMENT);
    CHECK(out == nullptr);
    CHECK(std::strstr(rt_last_error(), "rt_scene_edit") != nullptr);
    CHECK(rt_scene_edit(nullptr, &h, 1, nullptr) == RT_ERR_INVALID_ARGUMENT);
    CHECK(rt_scene_edit(nullptr, nullptr, 0, &out) == RT_ERR_INVALID_ARGUMENT);
    // with a device: the count check, a description rt_scene_create would refuse, and both orders of destruction
    rt_material_desc m{};
    m.type = RT_LAMBERTIAN;
    m.albedo.type = RT_CONSTANT;
    m.albedo.image = -1;
    rt_scene_desc d{};
    d.hittables = &h;
    d.num_hittables = 1;
    d.materials = &m;
    d.num_materials = 1;
    rt_scene* base = nullptr;
    if (rt_scene_create(&d, &base) != RT_OK) {
        CHECK(base == nullptr);
        return;
    }
    CHECK(rt_scene_edit(base, &h, 2, &out) == RT_ERR_INVALID_ARGUMENT && out == nullptr);
    CHECK(rt_scene_edit(base, nullptr, 1, &out) == RT_ERR_INVALID_ARGUMENT);
    rt_hittable_desc bad = h;
    bad.radius = -1.0f;
    CHECK(rt_scene_edit(base, &bad, 1, &out) == RT_ERR_INVALID_SCENE && out == nullptr);
    h.center[0] = 0.5f;
    CHECK(rt_scene_edit(base, &h, 1, &out) == RT_OK && out != nullptr);
    CHECK(rt_scene_destroy(base) == RT_OK);
    CHECK(rt_scene_destroy(out) == RT_OK);
}

int main() {
    motion();
    temporal_dynamic();
    scene_edit();
    if (failures) {
        std::fprintf(stderr, "%d check(s) failed\n", failures);
        return 1;
    }
    std::printf("host_sanitize_dynamic: all checks passed\n");
    return 0;
}
