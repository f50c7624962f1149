// host_sanitize_occlusion.cpp — the host paths of rt_occluded_rays (every argument check, the overlap tests, n = 0) in
// the AddressSanitizer + UndefinedBehaviorSanitizer build of the library, beside host_sanitize_query.cpp.  Built and run
// by `make -C cudaraytracer_amd/csrc asan`; no GPU is needed.  Exit status 0 = every check held and the sanitizers
// reported nothing.
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
#define REJECTED(call, what)                                               \
    do {                                                                   \
        CHECK((call) == RT_ERR_INVALID_ARGUMENT);                          \
        CHECK(std::strstr(rt_last_error(), "rt_occluded_rays") != nullptr); \
        CHECK(std::strstr(rt_last_error(), what) != nullptr);              \
    } while (0)

// Every check of rt_occluded_rays runs before the first device call and before the scene is read, so a GPU-less host
// sees status codes and the scene pointer below is never dereferenced.
static void occlusion_arguments() {
    const uint32_t n = 96;
    std::vector<float> rays(n * 8);
    std::vector<uint8_t> occ(n);
    std::vector<int32_t> blk(n);
    std::vector<uint64_t> counters(RT_COUNTERS_WORDS);
    rt_occlusion_args q{};
    q.rays = rays.data();
    q.occluded = occ.data();
    q.blocker = blk.data();
    q.counters = counters.data();
    q.n = n;
    const rt_scene* fake = reinterpret_cast<const rt_scene*>(&q);
    REJECTED(rt_occluded_rays(fake, nullptr, nullptr), "NULL args");
    REJECTED(rt_occluded_rays(nullptr, &q, nullptr), "NULL scene");  // valid arguments, NULL scene
    rt_occlusion_args b = q;
    b.count_tests = 1;
    REJECTED(rt_occluded_rays(nullptr, &b, nullptr), "NULL scene");  // (count_tests = 1 with counters is valid)
    b = q;
    b.rays = nullptr;
    REJECTED(rt_occluded_rays(fake, &b, nullptr), "NULL rays");
    b = q;
    b.occluded = nullptr;
    b.blocker = nullptr;
    REJECTED(rt_occluded_rays(fake, &b, nullptr), "no output");
    for (uint32_t bad : {2u, 0x80000000u, 0xffffffffu}) {
        b = q;
        b.count_tests = bad;
        REJECTED(rt_occluded_rays(fake, &b, nullptr), "count_tests");
    }
    b = q;
    b.count_tests = 1;
    b.counters = nullptr;
    REJECTED(rt_occluded_rays(fake, &b, nullptr), "without counters");
    for (uint32_t bad : {17u, 0xffffffffu}) {
        b = q;
        b.rays_per_lane = bad;
        REJECTED(rt_occluded_rays(fake, &b, nullptr), "rays_per_lane");
    }
    b = q;
    b.flags = 1;
    REJECTED(rt_occluded_rays(fake, &b, nullptr), "flags");
    for (int k = 0; k < 2; k++) {
        b = q;
        b.reserved[k] = 1;
        REJECTED(rt_occluded_rays(fake, &b, nullptr), "reserved");
    }
    // overlaps: each output (counters included) against the rays ...
    b = q;
    b.occluded = reinterpret_cast<uint8_t*>(rays.data()) + 32 * n - 1;  // the rays' last byte
    REJECTED(rt_occluded_rays(fake, &b, nullptr), "overlaps rays");
    b = q;
    b.blocker = reinterpret_cast<int32_t*>(rays.data() + 8);
    REJECTED(rt_occluded_rays(fake, &b, nullptr), "overlaps rays");
    b = q;
    b.counters = reinterpret_cast<uint64_t*>(rays.data());
    REJECTED(rt_occluded_rays(fake, &b, nullptr), "overlaps rays");
    // ... and against each other
    b = q;
    b.occluded = reinterpret_cast<uint8_t*>(blk.data() + (n - 1));  // occluded's first byte is in blocker's last element
    REJECTED(rt_occluded_rays(fake, &b, nullptr), "overlap");
    b = q;
    b.counters = reinterpret_cast<uint64_t*>(blk.data());
    REJECTED(rt_occluded_rays(fake, &b, nullptr), "overlap");
    b = q;
    b.occluded = reinterpret_cast<uint8_t*>(counters.data() + (RT_COUNTERS_WORDS - 1));  // in the last counter word
    REJECTED(rt_occluded_rays(fake, &b, nullptr), "overlap");
    b = q;
    b.occluded = reinterpret_cast<uint8_t*>(blk.data() + n);  // adjacent, not overlapping: passes the argument checks
    b.blocker = blk.data();
    REJECTED(rt_occluded_rays(nullptr, &b, nullptr), "NULL scene");
    b = q;
    b.n = 0xffffffffu;  // the overlap tests count bytes in 64 bits: an output 2^36 bytes into the rays is still inside them
    b.blocker = nullptr;
    b.counters = nullptr;
    b.occluded = reinterpret_cast<uint8_t*>(reinterpret_cast<uintptr_t>(rays.data()) + (1ull << 36));
    REJECTED(rt_occluded_rays(fake, &b, nullptr), "overlaps rays");  // 2^32 rays of 32 B reach past 2^36
    b = q;
    b.n = 0;  // nothing to trace: no device call, the scene is not read
    CHECK(rt_occluded_rays(nullptr, &b, nullptr) == RT_OK);
    b.rays = nullptr;
    CHECK(rt_occluded_rays(nullptr, &b, nullptr) == RT_OK);
    b.flags = 1;  // ... but the arguments are still checked
    REJECTED(rt_occluded_rays(nullptr, &b, nullptr), "flags");
}

int main() {
    occlusion_arguments();
    if (failures) {
        std::fprintf(stderr, "%d check(s) failed\n", failures);
        return 1;
    }
    std::printf("host_sanitize_occlusion: all checks passed\n");
    return 0;
}
