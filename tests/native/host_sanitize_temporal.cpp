// host_sanitize_temporal.cpp — the host paths of rt_temporal (argument checks, the camera terms filled per call, the
// launch's error path) in the AddressSanitizer + UndefinedBehaviorSanitizer build of the library, beside
// host_sanitize.cpp and host_sanitize_denoise.cpp.  Built and run by `make -C cudaraytracer_amd/csrc asan`; no GPU is
// needed.  Exit status 0 = every check held and the sanitizers reported nothing.
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

static bool rejected(const rt_temporal_args& a, const char* word) {
    return rt_temporal(&a, nullptr) == RT_ERR_INVALID_ARGUMENT && std::strstr(rt_last_error(), word) != nullptr;
}

// Every argument check runs before the first device call, so a GPU-less host sees status codes.
static void temporal() {
    static_assert(sizeof(rt_temporal_args) == 264, "rt_temporal_args layout");
    const uint32_t W = 16, H = 8;
    std::vector<float> color(W * H * 4), nd(W * H * 4), prev_hist(W * H * 4), prev_nd(W * H * 4), hist(W * H * 4);
    std::vector<float> motion(W * H * 2);
    std::vector<int32_t> ids(W * H), prev_ids(W * H);
    std::vector<uint32_t> pos(W * H);
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

    CHECK(rt_temporal(nullptr, nullptr) == RT_ERR_INVALID_ARGUMENT);
    rt_temporal_args b = a;
    b.color = nullptr;
    CHECK(rejected(b, "NULL"));
    b = a;
    b.normal_depth = nullptr;
    CHECK(rejected(b, "NULL"));
    b = a;
    b.prim_id = nullptr;
    CHECK(rejected(b, "NULL"));
    b = a;
    b.history = nullptr;
    CHECK(rejected(b, "history"));
    b = a;
    b.prev_history = nullptr;
    CHECK(rejected(b, "prev_"));
    b = a;
    b.prev_normal_depth = nullptr;
    CHECK(rejected(b, "prev_"));
    b = a;
    b.prev_prim_id = nullptr;
    CHECK(rejected(b, "prev_"));
    b = a;
    b.flags = RT_TEMPORAL_RESET;  // ... with it the current planes are still required
    b.prim_id = nullptr;
    CHECK(rejected(b, "NULL"));
    b = a;
    b.flags = 1u << 2;
    CHECK(rejected(b, "flags"));
    for (uint32_t n : {0u, 4097u}) {
        b = a;
        b.max_history = n;
        CHECK(rejected(b, "max_history"));
    }
    for (float t : {0.0f, -1.0f, std::nanf("")}) {
        b = a;
        b.depth_tol = t;
        CHECK(rejected(b, "tol"));
        b = a;
        b.normal_tol = t;
        CHECK(rejected(b, "tol"));
    }
    for (int k = 0; k < 2; k++) {
        b = a;
        b.reserved[k] = 1;
        CHECK(rejected(b, "reserved"));
    }
    b = a;
    b.tiling = rt_tiling{4, 2, 0, 4};
    CHECK(rejected(b, "tiling"));
    b = a;
    b.tiling.local_rows = H / 2;
    CHECK(rejected(b, "tiling"));
    b = a;
    b.history = prev_hist.data();  // the alias case, whole and partial
    CHECK(rejected(b, "alias"));
    b.history = prev_hist.data() + 4 * 5;
    CHECK(rejected(b, "alias"));
    b = a;
    b.motion = prev_nd.data();
    CHECK(rejected(b, "overlaps"));
    b = a;
    b.width = 0;  // an empty frame: nothing to do, no device call
    CHECK(rt_temporal(&b, nullptr) == RT_OK);

    // The launch's error path.  Only where no device is usable: the planes above are host memory, which a kernel must
    // never be handed, and without a device the launch fails before any kernel runs and must come back as a status.
    if (rt_set_device(0) != RT_OK) {
        const int rc = rt_temporal(&a, nullptr);
        CHECK(rc == RT_ERR_LAUNCH);
        CHECK(std::strstr(rt_last_error(), "rt_temporal: kernel launch") != nullptr);
        b = a;
        b.flags = RT_TEMPORAL_RESET | RT_TEMPORAL_COLOR_IS_SUM;
        b.prev_history = nullptr;
        b.prev_normal_depth = nullptr;
        b.prev_prim_id = nullptr;
        b.motion = nullptr;
        b.pos = nullptr;
        CHECK(rt_temporal(&b, nullptr) == RT_ERR_LAUNCH);
    } else {
        std::printf("host_sanitize_temporal: a device is present, the launch error path is not exercised\n");
    }
}

int main() {
    temporal();
    if (failures) {
        std::fprintf(stderr, "%d check(s) failed\n", failures);
        return 1;
    }
    std::printf("host_sanitize_temporal: all checks passed\n");
    return 0;
}
