// host_sanitize_denoise.cpp — the host paths of rt_gbuffer / rt_denoise (argument checks, rt_denoise_scratch_bytes, the
// prim_id source tables of the host scene build) in the AddressSanitizer + UndefinedBehaviorSanitizer build of the
// library, beside host_sanitize.cpp.  Built and run by `make -C cudaraytracer_amd/csrc asan`; no GPU is needed.  Exit
// status 0 = every check held and the sanitizers reported nothing.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/rt_hip.h"
#include "../../cudaraytracer_amd/csrc/rt_internal.h"

static int failures = 0;
#define CHECK(cond)                                                                  \
    do {                                                                             \
        if (!(cond)) {                                                               \
            std::fprintf(stderr, "CHECK failed at line %d: %s (%s)\n", __LINE__, #cond, \
                         rt_last_error());                                           \
            failures++;                                                              \
        }                                                                            \
    } while (0)

// rt_gbuffer / rt_denoise: every argument check runs before the first device call, so a GPU-less host sees status codes;
// the prim_id tables of the host scene map BVH order and flat order back to the description, inactive entries counted.
static void gbuffer_and_denoise() {
    std::vector<float> plane(16 * 8 * 4);
    std::vector<float> out(16 * 8 * 4);
    std::vector<int32_t> ids(16 * 8);
    std::vector<uint32_t> pos(16 * 8);
    std::vector<uint8_t> scratch((size_t)rt_denoise_scratch_bytes(16, 8, 6));
    CHECK(rt_denoise_scratch_bytes(0, 8, 3) == 0 && rt_denoise_scratch_bytes(16, 8, 1) == 0);
    CHECK(scratch.size() >= 16 * 8 * 16);
    rt_gbuffer_args g{};
    g.prim_id = ids.data();
    g.width = 16;
    g.height = 8;
    g.tiling = rt_tiling{8, 1, 0, 8};
    CHECK(rt_gbuffer(nullptr, nullptr, nullptr) == RT_ERR_INVALID_ARGUMENT);
    CHECK(rt_gbuffer(nullptr, &g, nullptr) == RT_ERR_INVALID_ARGUMENT);  // NULL scene
    const rt_scene* fake = reinterpret_cast<const rt_scene*>(&g);         // never dereferenced by the calls below
    rt_gbuffer_args bad = g;
    bad.prim_id = nullptr;
    CHECK(rt_gbuffer(fake, &bad, nullptr) == RT_ERR_INVALID_ARGUMENT);
    bad = g;
    bad.reserved[1] = 1;
    CHECK(rt_gbuffer(fake, &bad, nullptr) == RT_ERR_INVALID_ARGUMENT);
    CHECK(std::strlen(rt_last_error()) > 0);

    rt_denoise_args a{};
    a.color = plane.data();
    a.normal_depth = plane.data();
    a.albedo = plane.data();
    a.prim_id = ids.data();
    a.out_color = out.data();
    a.pos = pos.data();
    a.scratch = scratch.data();
    a.width = 16;
    a.height = 8;
    a.iterations = 3;
    a.sigma_c = 0.6f;
    a.sigma_n = 0.1f;
    a.sigma_z = 0.05f;
    a.tiling = rt_tiling{8, 1, 0, 8};
    CHECK(rt_denoise(nullptr, nullptr) == RT_ERR_INVALID_ARGUMENT);
    rt_denoise_args b = a;
    for (uint32_t n : {0u, 7u}) {
        b.iterations = n;
        CHECK(rt_denoise(&b, nullptr) == RT_ERR_INVALID_ARGUMENT);
    }
    b = a;
    b.sigma_n = 0.0f;
    CHECK(rt_denoise(&b, nullptr) == RT_ERR_INVALID_ARGUMENT);
    b = a;
    b.sigma_c = std::nanf("");
    CHECK(rt_denoise(&b, nullptr) == RT_ERR_INVALID_ARGUMENT);
    b = a;
    b.tiling.num_ranks = 2;
    CHECK(rt_denoise(&b, nullptr) == RT_ERR_INVALID_ARGUMENT);
    b = a;
    b.scratch = nullptr;
    CHECK(rt_denoise(&b, nullptr) == RT_ERR_INVALID_ARGUMENT);
    b = a;
    b.out_color = nullptr;
    b.pos = nullptr;
    CHECK(rt_denoise(&b, nullptr) == RT_ERR_INVALID_ARGUMENT);
    b = a;
    b.reserved = 1;
    CHECK(rt_denoise(&b, nullptr) == RT_ERR_INVALID_ARGUMENT);
    b = a;
    b.out_color = plane.data();  // aliases color
    CHECK(rt_denoise(&b, nullptr) == RT_ERR_INVALID_ARGUMENT);
    b = a;
    b.width = 0;  // an empty frame: nothing to do, no device call
    CHECK(rt_denoise(&b, nullptr) == RT_OK);

    // the default world with its middle entry switched off: both id tables skip it and cover every other entry once
    uint32_t nh = 0, nm = 0;
    CHECK(rt_builtin_scene(0, 1, nullptr, &nh, nullptr, &nm) == RT_OK);
    std::vector<rt_hittable_desc> h(nh);
    std::vector<rt_material_desc> m(nm);
    CHECK(rt_builtin_scene(0, 1, h.data(), &nh, m.data(), &nm) == RT_OK);
    h[nh / 2].is_active = 0;
    rt_scene_desc d{h.data(), nh, m.data(), nm, nullptr, 0};
    rt::HostScene hs;
    std::string err;
    CHECK(rt::build_host_scene(&d, &hs, &err, false) == RT_OK);
    CHECK(hs.num_prims == nh - 1 && hs.prim_source.size() == hs.num_prims && hs.flat_source.size() == hs.num_prims);
    for (const std::vector<int32_t>* tab : {&hs.prim_source, &hs.flat_source}) {
        std::vector<int> seen(nh, 0);
        for (int32_t i : *tab) {
            CHECK(i >= 0 && (uint32_t)i < nh);
            if (i >= 0 && (uint32_t)i < nh) seen[i]++;
        }
        for (uint32_t i = 0; i < nh; i++) CHECK(seen[i] == (i == nh / 2 ? 0 : 1));
    }
    for (uint32_t i = 0; i < hs.num_prims; i++)  // the flat records are the description's entries, in the flat order
        CHECK(hs.prims_flat[(size_t)i * 8] == h[hs.flat_source[i]].center[h[hs.flat_source[i]].type == RT_SPHERE ? 0 : 1]);
}

int main() {
    gbuffer_and_denoise();
    if (failures) {
        std::fprintf(stderr, "%d check(s) failed\n", failures);
        return 1;
    }
    std::printf("host_sanitize_denoise: all checks passed\n");
    return 0;
}
