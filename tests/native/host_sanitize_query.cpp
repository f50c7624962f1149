// host_sanitize_query.cpp — the host paths of rt_query_rays (every argument check, the overlap tests, n = 0) in the
// AddressSanitizer + UndefinedBehaviorSanitizer build of the library, beside host_sanitize.cpp.  Built and run by
// `make -C cudaraytracer_amd/csrc asan`; no GPU is needed.  Exit status 0 = every check held and the sanitizers reported
// nothing.
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

// Every check of rt_query_rays runs before the first device call and before the scene is read, so a GPU-less host sees
// status codes and the scene pointer below is never dereferenced.
static void query_arguments() {
    const uint32_t n = 96;
    std::vector<float> rays(n * 8), nd(n * 4), alb(n * 4), uv(n * 2);
    std::vector<int32_t> ids(n), mat(n), hits(n * 2);
    rt_query_args q{};
    q.rays = rays.data();
    q.normal_depth = nd.data();
    q.albedo = alb.data();
    q.prim_id = ids.data();
    q.uv = uv.data();
    q.material = mat.data();
    q.hits = hits.data();
    q.n = n;
    const rt_scene* fake = reinterpret_cast<const rt_scene*>(&q);
    CHECK(rt_query_rays(fake, nullptr, nullptr) == RT_ERR_INVALID_ARGUMENT);
    CHECK(std::strstr(rt_last_error(), "rt_query_rays") != nullptr);
    CHECK(rt_query_rays(nullptr, &q, nullptr) == RT_ERR_INVALID_ARGUMENT);  // valid arguments, NULL scene
    rt_query_args b = q;
    b.rays = nullptr;
    CHECK(rt_query_rays(fake, &b, nullptr) == RT_ERR_INVALID_ARGUMENT);
    b = q;
    b.normal_depth = b.albedo = b.uv = nullptr;
    b.prim_id = b.material = b.hits = nullptr;
    CHECK(rt_query_rays(fake, &b, nullptr) == RT_ERR_INVALID_ARGUMENT);
    for (uint32_t bad : {17u, 0xffffffffu}) {
        b = q;
        b.rays_per_lane = bad;
        CHECK(rt_query_rays(fake, &b, nullptr) == RT_ERR_INVALID_ARGUMENT);
    }
    b = q;
    b.flags = 1;
    CHECK(rt_query_rays(fake, &b, nullptr) == RT_ERR_INVALID_ARGUMENT);
    b = q;
    b.reserved = 1;
    CHECK(rt_query_rays(fake, &b, nullptr) == RT_ERR_INVALID_ARGUMENT);
    b = q;
    b.hits = reinterpret_cast<int32_t*>(rays.data() + 8);  // inside the rays
    CHECK(rt_query_rays(fake, &b, nullptr) == RT_ERR_INVALID_ARGUMENT);
    b = q;
    b.albedo = nd.data() + 4 * (n - 1);  // albedo's first element is normal_depth's last
    CHECK(rt_query_rays(fake, &b, nullptr) == RT_ERR_INVALID_ARGUMENT);
    b = q;
    b.material = ids.data();
    CHECK(rt_query_rays(fake, &b, nullptr) == RT_ERR_INVALID_ARGUMENT);
    b = q;
    b.n = 0xffffffffu;  // the overlap tests count bytes in 64 bits: an output 2^36 bytes into the rays is still inside them
    b.albedo = b.uv = nullptr;
    b.prim_id = b.material = b.hits = nullptr;
    b.normal_depth = reinterpret_cast<float*>(reinterpret_cast<uintptr_t>(rays.data()) + (1ull << 36));
    CHECK(rt_query_rays(fake, &b, nullptr) == RT_ERR_INVALID_ARGUMENT);  // 2^32 rays of 32 B reach past 2^36
    b = q;
    b.n = 0;  // nothing to trace: no device call, the scene is not read
    CHECK(rt_query_rays(nullptr, &b, nullptr) == RT_OK);
    b.rays = nullptr;
    CHECK(rt_query_rays(nullptr, &b, nullptr) == RT_OK);
}

int main() {
    query_arguments();
    if (failures) {
        std::fprintf(stderr, "%d check(s) failed\n", failures);
        return 1;
    }
    std::printf("host_sanitize_query: all checks passed\n");
    return 0;
}
