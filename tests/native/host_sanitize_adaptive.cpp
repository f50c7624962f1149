// host_sanitize_adaptive.cpp — the host paths of rt_adaptive_select and rt_adaptive_samples (every argument check, the
// overlap tests, the empty frame and the empty list) in the AddressSanitizer + UndefinedBehaviorSanitizer build of the
// library, beside host_sanitize_radiance.cpp.  Built and run by `make -C cudaraytracer_amd/csrc asan`; no GPU is needed.
// Exit status 0 = every check held and the sanitizers reported nothing.
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

static const uint32_t W = 12, H = 8, N = W * H, CAP = 40;

// Every check of rt_adaptive_select runs before the first device call, so a GPU-less host sees status codes.
static void select_arguments() {
    const char* who = "rt_adaptive_select";
    std::vector<float> history(N * 4), moments(N * 2);
    std::vector<int32_t> prim_id(N);
    std::vector<uint32_t> pixels(CAP), samples(CAP), count(2);
    std::vector<uint32_t> scratch(rt_adaptive_select_scratch_bytes(W, H) / 4);
    CHECK(rt_adaptive_select_scratch_bytes(W, H) == 8 && rt_adaptive_select_scratch_bytes(0, H) == 0);
    CHECK(rt_adaptive_select_scratch_bytes(0xffffffffu, 0xffffffffu) > (1ull << 50));
    rt_adaptive_select_args q{};
    q.history = history.data();
    q.moments = moments.data();
    q.prim_id = prim_id.data();
    q.pixels = pixels.data();
    q.samples = samples.data();
    q.count = count.data();
    q.scratch = scratch.data();
    q.width = W;
    q.height = H;
    q.capacity = CAP;
    q.max_samples = 4;
    q.min_history = 4;
    q.tau = 0.1f;
    q.lum_floor = 0.01f;
    q.tiling = rt_tiling{H, 1, 0, H};
    REJECTED(who, rt_adaptive_select(nullptr, nullptr), "NULL args");
    rt_adaptive_select_args b = q;
    b.history = nullptr;
    REJECTED(who, rt_adaptive_select(&b, nullptr), "NULL history");
    b = q;
    b.moments = nullptr;
    REJECTED(who, rt_adaptive_select(&b, nullptr), "NULL moments");
    b = q;
    b.pixels = nullptr;
    REJECTED(who, rt_adaptive_select(&b, nullptr), "NULL pixels");
    b = q;
    b.count = nullptr;
    REJECTED(who, rt_adaptive_select(&b, nullptr), "NULL count");
    b = q;
    b.scratch = nullptr;
    REJECTED(who, rt_adaptive_select(&b, nullptr), "NULL scratch");
    b = q;
    b.scratch = reinterpret_cast<char*>(scratch.data()) + 1;
    REJECTED(who, rt_adaptive_select(&b, nullptr), "aligned");
    for (float bad : {0.0f, -1.0f, NAN}) {
        b = q;
        b.tau = bad;
        REJECTED(who, rt_adaptive_select(&b, nullptr), "tau");
        b = q;
        b.lum_floor = bad;
        REJECTED(who, rt_adaptive_select(&b, nullptr), "lum_floor");
    }
    for (uint32_t bad : {4097u, 0xffffffffu}) {
        b = q;
        b.min_history = bad;
        REJECTED(who, rt_adaptive_select(&b, nullptr), "min_history");
    }
    for (uint32_t bad : {0u, 17u, 0xffffffffu}) {
        b = q;
        b.max_samples = bad;
        REJECTED(who, rt_adaptive_select(&b, nullptr), "max_samples");
    }
    for (uint32_t bad : {17u, 0xffffffffu}) {
        b = q;
        b.pixels_per_lane = bad;
        REJECTED(who, rt_adaptive_select(&b, nullptr), "pixels_per_lane");
    }
    for (uint32_t bad : {1u, 0x80000000u}) {
        b = q;
        b.flags = bad;
        REJECTED(who, rt_adaptive_select(&b, nullptr), "flags");
    }
    for (int k = 0; k < 3; k++) {
        b = q;
        b.reserved[k] = 1;
        REJECTED(who, rt_adaptive_select(&b, nullptr), "reserved");
    }
    b = q;
    b.tiling = rt_tiling{4, 2, 0, 4};
    REJECTED(who, rt_adaptive_select(&b, nullptr), "num_ranks");
    b = q;
    b.tiling.local_rows = H - 1;
    REJECTED(who, rt_adaptive_select(&b, nullptr), "local_rows");
    b = q;
    b.width = 0x10000u;  // 2^31 pixels; and 2^28 pixels of up to 16 samples: the products are taken in 64 bits
    b.height = 0x8000u;
    b.tiling = rt_tiling{0x8000u, 1, 0, 0x8000u};
    REJECTED(who, rt_adaptive_select(&b, nullptr), "too large");
    b.height = 0x1000u;
    b.tiling = rt_tiling{0x1000u, 1, 0, 0x1000u};
    b.max_samples = 16;
    REJECTED(who, rt_adaptive_select(&b, nullptr), "too large");
    // overlaps: an output against an input, and against another output
    b = q;
    b.pixels = reinterpret_cast<uint32_t*>(history.data() + 4 * N - 1);  // the plane's last float
    REJECTED(who, rt_adaptive_select(&b, nullptr), "pixels overlaps history");
    b = q;
    b.samples = reinterpret_cast<uint32_t*>(moments.data());
    REJECTED(who, rt_adaptive_select(&b, nullptr), "samples overlaps moments");
    b = q;
    b.count = reinterpret_cast<uint32_t*>(prim_id.data() + (N - 1));
    REJECTED(who, rt_adaptive_select(&b, nullptr), "count overlaps prim_id");
    b = q;
    b.scratch = history.data();
    REJECTED(who, rt_adaptive_select(&b, nullptr), "scratch overlaps history");
    b = q;
    b.samples = pixels.data() + (CAP - 1);
    REJECTED(who, rt_adaptive_select(&b, nullptr), "samples overlaps pixels");
    b = q;
    b.count = samples.data();
    REJECTED(who, rt_adaptive_select(&b, nullptr), "count overlaps samples");
    b = q;
    b.scratch = count.data() + 1;
    REJECTED(who, rt_adaptive_select(&b, nullptr), "scratch overlaps count");
    // an empty frame without count: RT_OK and no device call ... but the arguments are still checked
    b = q;
    b.height = 0;
    b.tiling = rt_tiling{1, 1, 0, 0};
    b.count = nullptr;
    CHECK(rt_adaptive_select(&b, nullptr) == RT_OK);
    b.history = nullptr;
    b.moments = nullptr;
    b.pixels = nullptr;
    b.scratch = nullptr;
    CHECK(rt_adaptive_select(&b, nullptr) == RT_OK);
    b.flags = 2;
    REJECTED(who, rt_adaptive_select(&b, nullptr), "flags");
}

// Every check of rt_adaptive_samples runs before the first device call and before the scene is read, so the scene
// pointer below is never dereferenced.
static void samples_arguments() {
    const char* who = "rt_adaptive_samples";
    std::vector<uint32_t> pixels(CAP), samples(CAP), count(2);
    std::vector<float> history(N * 4), moments(N * 2), accum(N * 4);
    std::vector<uint64_t> counters(RT_COUNTERS_WORDS);
    rt_adaptive_samples_args q{};
    q.pixels = pixels.data();
    q.samples = samples.data();
    q.count = count.data();
    q.history = history.data();
    q.moments = moments.data();
    q.accum = accum.data();
    q.counters = counters.data();
    q.capacity = CAP;
    q.width = W;
    q.height = H;
    q.samples_per_pixel = 1;
    q.max_samples = 4;
    q.sample_base = 1;
    q.max_depth = 8;
    q.max_history = 32;
    q.inputs.orientation[2] = -1.0f;
    q.inputs.up[1] = 1.0f;
    q.inputs.fov = 0.7f;
    q.inputs.near_plane = 0.1f;
    q.inputs.far_plane = 10.0f;
    const rt_scene* fake = reinterpret_cast<const rt_scene*>(&q);
    REJECTED(who, rt_adaptive_samples(fake, nullptr, nullptr), "NULL args");
    REJECTED(who, rt_adaptive_samples(nullptr, &q, nullptr), "NULL scene");  // valid arguments, NULL scene
    rt_adaptive_samples_args b = q;
    b.count_tests = 1;
    b.flags = RT_FLAG_RIUS_LEFT_TO_RIGHT;
    b.rays_per_lane = 16;
    b.max_depth = 0;
    b.samples = nullptr;
    b.count = nullptr;
    b.moments = nullptr;
    b.accum = nullptr;
    b.max_samples = 16;
    b.sample_base = RT_PHILOX_MAX_SPP - 16;
    b.max_history = 4096;
    REJECTED(who, rt_adaptive_samples(nullptr, &b, nullptr), "NULL scene");  // (all of these are valid)
    b = q;
    b.pixels = nullptr;
    REJECTED(who, rt_adaptive_samples(fake, &b, nullptr), "NULL pixels");
    b = q;
    b.history = nullptr;
    b.moments = nullptr;
    b.accum = nullptr;
    REJECTED(who, rt_adaptive_samples(fake, &b, nullptr), "no target");
    b = q;
    b.history = nullptr;
    REJECTED(who, rt_adaptive_samples(fake, &b, nullptr), "moments without history");
    for (uint32_t bad : {2u, 0x80000000u}) {
        b = q;
        b.count_tests = bad;
        REJECTED(who, rt_adaptive_samples(fake, &b, nullptr), "count_tests");
    }
    b = q;
    b.count_tests = 1;
    b.counters = nullptr;
    REJECTED(who, rt_adaptive_samples(fake, &b, nullptr), "without counters");
    for (uint32_t bad : {17u, 0xffffffffu}) {
        b = q;
        b.rays_per_lane = bad;
        REJECTED(who, rt_adaptive_samples(fake, &b, nullptr), "rays_per_lane");
    }
    for (uint32_t bad : {1u, (uint32_t)RT_FLAG_RNG_PHILOX, 0x80000000u, (uint32_t)RT_FLAG_RIUS_LEFT_TO_RIGHT | 1u}) {
        b = q;
        b.flags = bad;
        REJECTED(who, rt_adaptive_samples(fake, &b, nullptr), "flags");
    }
    for (int k = 0; k < 2; k++) {
        b = q;
        b.reserved[k] = 1;
        REJECTED(who, rt_adaptive_samples(fake, &b, nullptr), "reserved");
    }
    for (uint32_t bad : {0u, 17u, 0xffffffffu}) {
        b = q;
        b.max_samples = bad;
        REJECTED(who, rt_adaptive_samples(fake, &b, nullptr), "max_samples");
    }
    for (uint32_t bad : {0u, 4097u, 0xffffffffu}) {
        b = q;
        b.max_history = bad;
        REJECTED(who, rt_adaptive_samples(fake, &b, nullptr), "max_history");
    }
    b = q;
    b.samples = nullptr;
    b.samples_per_pixel = 0;
    REJECTED(who, rt_adaptive_samples(fake, &b, nullptr), "samples_per_pixel");
    const uint32_t windows[][2] = {{RT_PHILOX_MAX_SPP, 1u}, {RT_PHILOX_MAX_SPP - 3u, 4u}, {0xffffffffu, 16u}};  // (64-bit sum)
    for (const auto& w : windows) {
        b = q;
        b.sample_base = w[0];
        b.max_samples = w[1];
        REJECTED(who, rt_adaptive_samples(fake, &b, nullptr), "RT_PHILOX_MAX_SPP");
    }
    b = q;
    b.width = 0x10000u;
    b.height = 0x8000u;
    REJECTED(who, rt_adaptive_samples(fake, &b, nullptr), "too large");
    b = q;
    b.width = 0;
    REJECTED(who, rt_adaptive_samples(fake, &b, nullptr), "empty frame");
    // overlaps among the list, the count, the counters and the planes
    b = q;
    b.samples = pixels.data() + (CAP - 1);
    REJECTED(who, rt_adaptive_samples(fake, &b, nullptr), "samples overlaps pixels");
    b = q;
    b.count = samples.data();
    REJECTED(who, rt_adaptive_samples(fake, &b, nullptr), "count overlaps samples");
    b = q;
    b.counters = reinterpret_cast<uint64_t*>(count.data());
    REJECTED(who, rt_adaptive_samples(fake, &b, nullptr), "counters overlaps count");
    b = q;
    b.history = reinterpret_cast<float*>(pixels.data());
    REJECTED(who, rt_adaptive_samples(fake, &b, nullptr), "history overlaps pixels");
    b = q;
    b.moments = history.data() + 4 * N - 1;  // the plane's last float
    REJECTED(who, rt_adaptive_samples(fake, &b, nullptr), "moments overlaps history");
    b = q;
    b.accum = moments.data();
    REJECTED(who, rt_adaptive_samples(fake, &b, nullptr), "accum overlaps moments");
    b = q;
    b.accum = reinterpret_cast<float*>(counters.data() + (RT_COUNTERS_WORDS - 1));
    REJECTED(who, rt_adaptive_samples(fake, &b, nullptr), "accum overlaps counters");
    std::vector<float> both(N * 6);
    b = q;
    b.history = both.data();
    b.moments = both.data() + 4 * N;  // adjacent, not overlapping: passes the argument checks
    REJECTED(who, rt_adaptive_samples(nullptr, &b, nullptr), "NULL scene");
    b = q;
    b.capacity = 0;  // nothing to trace: no device call, the scene is not read
    CHECK(rt_adaptive_samples(nullptr, &b, nullptr) == RT_OK);
    b.pixels = nullptr;
    b.width = 0;
    CHECK(rt_adaptive_samples(nullptr, &b, nullptr) == RT_OK);
    b.flags = 1;  // ... but the arguments are still checked
    REJECTED(who, rt_adaptive_samples(nullptr, &b, nullptr), "flags");
}

int main() {
    select_arguments();
    samples_arguments();
    if (failures) {
        std::fprintf(stderr, "%d check(s) failed\n", failures);
        return 1;
    }
    std::printf("host_sanitize_adaptive: all checks passed\n");
    return 0;
}
