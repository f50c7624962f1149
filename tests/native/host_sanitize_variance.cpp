// host_sanitize_variance.cpp — the host paths of rt_temporal_moments, rt_denoise_variance and
// rt_denoise_variance_scratch_bytes (argument checks, the launch parameters filled per call, the launches' error paths) in
// the AddressSanitizer + UndefinedBehaviorSanitizer build of the library, beside host_sanitize_temporal.cpp and
// host_sanitize_denoise.cpp.  Built and run by `make -C cudaraytracer_amd/csrc asan`; no GPU is needed.  Exit status 0 =
// every check held and the sanitizers reported nothing.
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

static bool is_rejected(int rc, const char* word) {
    return rc == RT_ERR_INVALID_ARGUMENT && std::strstr(rt_last_error(), word) != nullptr;
}

// Every argument check runs before the first device call, so a GPU-less host sees status codes.
static void moments() {
    const uint32_t W = 16, H = 8, NP = 4;
    std::vector<float> color(W * H * 4), nd(W * H * 4), prev_hist(W * H * 4), prev_nd(W * H * 4), hist(W * H * 4);
    std::vector<float> motion(W * H * 2), prev_m(W * H * 2), m(W * H * 2);
    std::vector<int32_t> ids(W * H), prev_ids(W * H);
    std::vector<uint32_t> pos(W * H);
    alignas(16) float table[NP * 4] = {};
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
    const auto call = [&](const rt_temporal_args& args, const float* t, uint32_t n, const float* pm, float* mo) {
        return rt_temporal_moments(&args, t, n, pm, mo, nullptr);
    };

    CHECK(is_rejected(rt_temporal_moments(nullptr, table, NP, prev_m.data(), m.data(), nullptr), "rt_temporal_moments"));
    rt_temporal_args b = a;
    b.color = nullptr;  // rt_temporal's checks, under this entry point's name
    CHECK(is_rejected(call(b, table, NP, prev_m.data(), m.data()), "rt_temporal_moments: NULL"));
    b = a;
    b.flags = 1u << 2;
    CHECK(is_rejected(call(b, nullptr, 0, prev_m.data(), m.data()), "flags"));
    b = a;
    b.max_history = 0;
    CHECK(is_rejected(call(b, nullptr, 0, prev_m.data(), m.data()), "max_history"));
    b = a;
    b.depth_tol = std::nanf("");
    CHECK(is_rejected(call(b, nullptr, 0, prev_m.data(), m.data()), "tol"));
    b = a;
    b.tiling = rt_tiling{4, 2, 0, 4};
    CHECK(is_rejected(call(b, nullptr, 0, prev_m.data(), m.data()), "tiling"));
    b = a;
    b.history = prev_hist.data() + 4 * 5;
    CHECK(is_rejected(call(b, nullptr, 0, prev_m.data(), m.data()), "alias"));
    // the table
    CHECK(is_rejected(call(a, nullptr, NP, prev_m.data(), m.data()), "prim_motion"));
    CHECK(is_rejected(call(a, table + 1, NP - 1, prev_m.data(), m.data()), "aligned"));
    CHECK(is_rejected(call(a, hist.data() + 8, NP, prev_m.data(), m.data()), "prim_motion"));
    // the moments planes
    CHECK(is_rejected(call(a, nullptr, 0, prev_m.data(), nullptr), "moments"));
    CHECK(is_rejected(call(a, table, NP, nullptr, m.data()), "prev_moments"));
    CHECK(is_rejected(call(a, nullptr, 0, prev_m.data(), prev_m.data()), "moments"));
    CHECK(is_rejected(call(a, nullptr, 0, prev_m.data(), prev_m.data() + 2 * 5), "moments"));
    CHECK(is_rejected(call(a, nullptr, 0, prev_m.data(), color.data()), "moments"));
    CHECK(is_rejected(call(a, nullptr, 0, prev_m.data(), (float*)ids.data()), "moments"));
    CHECK(is_rejected(call(a, nullptr, 0, prev_m.data(), prev_nd.data() + 2), "moments"));
    CHECK(is_rejected(call(a, nullptr, 0, prev_m.data(), hist.data() + 2), "moments"));
    CHECK(is_rejected(call(a, nullptr, 0, prev_m.data(), (float*)pos.data()), "moments"));
    CHECK(is_rejected(call(a, table, NP, prev_m.data(), table + 4), "moments"));
    b = a;
    b.motion = prev_m.data();
    CHECK(is_rejected(call(b, nullptr, 0, prev_m.data(), m.data()), "moments"));
    b = a;
    b.flags = RT_TEMPORAL_RESET;  // nothing is gathered: the prev_* planes may be NULL, this frame's may still not be hit
    b.prev_history = nullptr;
    b.prev_normal_depth = nullptr;
    b.prev_prim_id = nullptr;
    CHECK(is_rejected(call(b, nullptr, 0, nullptr, nd.data()), "moments"));
    b.width = 0;  // an empty frame: nothing to do, no device call
    CHECK(call(b, nullptr, 0, nullptr, m.data()) == RT_OK);
    b = a;
    b.height = 0;
    b.tiling = rt_tiling{H, 1, 0, 0};
    CHECK(call(b, table, NP, prev_m.data(), m.data()) == RT_OK);

    // The launches' error path.  Only where no device is usable: the planes above are host memory, which a kernel must
    // never be handed, and without a device the launch fails before any kernel runs and must come back as a status.
    if (rt_set_device(0) != RT_OK) {
        CHECK(call(a, nullptr, 0, prev_m.data(), m.data()) == RT_ERR_LAUNCH);
        CHECK(std::strstr(rt_last_error(), "rt_temporal_moments: kernel launch") != nullptr);
        CHECK(call(a, table, NP, prev_m.data(), m.data()) == RT_ERR_LAUNCH);
    } else {
        std::printf("host_sanitize_variance: a device is present, the launch error paths are not exercised\n");
    }
}

static void filter() {
    static_assert(sizeof(rt_denoise_variance_args) == 112, "rt_denoise_variance_args layout");
    static_assert(sizeof(rt_temporal_args) == 264 && sizeof(rt_denoise_args) == 104, "the existing layouts");
    const uint32_t W = 16, H = 8;
    CHECK(rt_denoise_variance_scratch_bytes(0, H, 3) == 0 && rt_denoise_variance_scratch_bytes(W, 0, 6) == 0);
    CHECK(rt_denoise_variance_scratch_bytes(W, H, 1) >= (uint64_t)W * H * 16);
    CHECK(rt_denoise_variance_scratch_bytes(W, H, 2) >= rt_denoise_variance_scratch_bytes(W, H, 1));
    CHECK(rt_denoise_variance_scratch_bytes(65535, 32767, 6) == (uint64_t)65535 * 32767 * 32);  // (no 32-bit overflow)
    std::vector<float> color(W * H * 4), mom(W * H * 2), nd(W * H * 4), out(W * H * 4);
    std::vector<int32_t> ids(W * H);
    std::vector<uint32_t> pos(W * H);
    std::vector<unsigned char> scratch(rt_denoise_variance_scratch_bytes(W, H, 6));
    rt_denoise_variance_args a{};
    a.color = color.data();
    a.moments = mom.data();
    a.normal_depth = nd.data();
    a.prim_id = ids.data();
    a.out_color = out.data();
    a.pos = pos.data();
    a.scratch = scratch.data();
    a.width = W;
    a.height = H;
    a.iterations = 3;
    a.sigma_l = 1.0f;
    a.sigma_n = 0.1f;
    a.sigma_z = 0.05f;
    a.min_history = 4;
    a.tiling = rt_tiling{H, 1, 0, H};
    const auto rejected = [](const rt_denoise_variance_args& args, const char* word) {
        return is_rejected(rt_denoise_variance(&args, nullptr), word);
    };

    CHECK(is_rejected(rt_denoise_variance(nullptr, nullptr), "rt_denoise_variance"));
    rt_denoise_variance_args b = a;
    b.color = nullptr;
    CHECK(rejected(b, "NULL"));
    b = a;
    b.moments = nullptr;
    CHECK(rejected(b, "NULL"));
    b = a;
    b.normal_depth = nullptr;
    CHECK(rejected(b, "NULL"));
    b = a;
    b.prim_id = nullptr;
    CHECK(rejected(b, "NULL"));
    b = a;
    b.out_color = nullptr;
    b.pos = nullptr;
    CHECK(rejected(b, "output"));
    b = a;
    b.flags = 1;
    CHECK(rejected(b, "flags"));
    for (int k = 0; k < 2; k++) {
        b = a;
        b.reserved[k] = 1;
        CHECK(rejected(b, "reserved"));
    }
    for (float s : {0.0f, -1.0f, std::nanf("")}) {
        b = a;
        b.sigma_l = s;
        CHECK(rejected(b, "sigma"));
        b = a;
        b.sigma_n = s;
        CHECK(rejected(b, "sigma"));
        b = a;
        b.sigma_z = s;
        CHECK(rejected(b, "sigma"));
    }
    for (uint32_t n : {0u, 7u}) {
        b = a;
        b.iterations = n;
        CHECK(rejected(b, "iterations"));
    }
    for (uint32_t n : {0u, 4097u}) {
        b = a;
        b.min_history = n;
        CHECK(rejected(b, "min_history"));
    }
    b = a;
    b.tiling = rt_tiling{4, 2, 0, 4};
    CHECK(rejected(b, "tiling"));
    b = a;
    b.tiling.local_rows = H / 2;
    CHECK(rejected(b, "tiling"));
    b = a;
    b.scratch = nullptr;
    CHECK(rejected(b, "scratch"));
    b = a;
    b.out_color = color.data();
    CHECK(rejected(b, "alias"));
    b.out_color = color.data() + 4 * 5;
    CHECK(rejected(b, "alias"));
    b = a;
    b.pos = (uint32_t*)mom.data();
    CHECK(rejected(b, "overlaps"));
    b = a;
    b.scratch = nd.data() + 4;  // (two planes long: it may reach a neighbouring output of the heap as well)
    CHECK(rejected(b, "overlap"));
    b = a;
    b.out_color = (float*)scratch.data() + 4;
    CHECK(rejected(b, "overlap"));
    b = a;
    b.width = 0;  // an empty frame: nothing to do, no device call, no scratch
    b.scratch = nullptr;
    CHECK(rt_denoise_variance(&b, nullptr) == RT_OK);

    if (rt_set_device(0) != RT_OK) {
        CHECK(rt_denoise_variance(&a, nullptr) == RT_ERR_LAUNCH);
        CHECK(std::strstr(rt_last_error(), "rt_denoise_variance: kernel launch") != nullptr);
        b = a;
        b.iterations = 1;
        b.out_color = nullptr;
        CHECK(rt_denoise_variance(&b, nullptr) == RT_ERR_LAUNCH);
    }
}

int main() {
    moments();
    filter();
    if (failures) {
        std::fprintf(stderr, "%d check(s) failed\n", failures);
        return 1;
    }
    std::printf("host_sanitize_variance: all checks passed\n");
    return 0;
}
