// gradient.hip — temporal gradients turned into history lengths (rt_history_adapt, include/rt_hip.h).
//
// rt_temporal_gradient (render.hip) traces one pixel per stride × stride stratum of the previous frame again in the
// edited scene and stores (δ, m) per stratum: how far the re-traced colour is from the stored one, and their level.
// This pass spreads that over the frame: every pixel sums δ and m over the (2r + 1)² strata around its
// own, takes λ = min(gain · D / max(M, lum_floor · n), 1) and multiplies its history length by (1 − λ)^power, so the
// next temporal pass weighs the new sample by 1 / (N·(1 − λ)^power + 1) there instead of 1 / (N + 1).
//   * one launch, one lane per pixel, 64×4-pixel workgroups as rt_temporal: a wave covers 64 consecutive pixels of a
//     row; its stencil reads at most ceil(64 / stride) + 2r strata per stratum row, which the L2 serves; no LDS, no
//     scratch, no atomics; a lane reads and writes its own pixel's length alone and the gradient plane is only read:
//     deterministic, in place;
//   * binary32 multiplications, additions, comparisons and one IEEE division, one rounding each (-ffp-contract=off),
//     in the header's order: tests/test_gradient_host.py adapt_reference restates it in numpy bit for bit.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "rt_internal.h"

namespace rt {
namespace dev {

constexpr int kGaTileW = 64, kGaTileH = 4;

struct AdaptParams {
    const float2* gradient;
    float4* history;
    uint32_t width, height;
    uint32_t sw, sh, stride;
    int32_t radius;
    uint32_t power;
    float gain, lum_floor;
};

__global__ __launch_bounds__(kGaTileW * kGaTileH) void history_adapt_kernel(const AdaptParams P) {
    const uint32_t x = blockIdx.x * kGaTileW + threadIdx.x, y = blockIdx.y * kGaTileH + threadIdx.y;
    if (x >= P.width || y >= P.height) return;
    const int32_t sx = (int32_t)(x / P.stride), sy = (int32_t)(y / P.stride);  // (below sw, sh)
    float D = 0.0f, M = 0.0f;
    uint32_t n = 0u;
    for (int32_t dy = -P.radius; dy <= P.radius; dy++) {
        const int32_t ty = sy + dy;
        if (ty < 0 || ty >= (int32_t)P.sh) continue;
        for (int32_t dx = -P.radius; dx <= P.radius; dx++) {
            const int32_t tx = sx + dx;
            if (tx < 0 || tx >= (int32_t)P.sw) continue;
            const float2 g = P.gradient[(size_t)ty * P.sw + (uint32_t)tx];  // (inside the sw × sh plane)
            D = D + g.x;
            M = M + g.y;
            n++;
        }
    }
    const float lo = P.lum_floor * (float)n;
    const float q = (P.gain * D) / (M > lo ? M : lo);
    const float lambda = q < 1.0f ? q : 1.0f;  // (a NaN gives 1)
    const float keep = 1.0f - lambda;
    float f = keep;
    for (uint32_t j = 1; j < P.power; j++) f = f * keep;
    float* const w = &P.history[(size_t)y * P.width + x].w;  // (rgb is not touched)
    *w = *w * f;
}

}  // namespace dev
}  // namespace rt

using namespace rt;

extern "C" {

int rt_history_adapt(const rt_history_adapt_args* a, rt_stream stream) {
    // (every argument check runs before the first device call)
    const auto bad = [](const std::string& what) {
        set_error("rt_history_adapt: " + what);
        return (int)RT_ERR_INVALID_ARGUMENT;
    };
    if (!a) return bad("NULL args");
    if (a->flags != 0) return bad("flags must be 0");
    if (a->reserved[0] != 0 || a->reserved[1] != 0) return bad("reserved must be 0");
    if (a->stride < 1u || a->stride > 8u) return bad("stride must be 1..8");
    if (a->radius > 3u) return bad("radius must be 0..3");
    if (a->power < 1u || a->power > 8u) return bad("power must be 1..8");
    if (!(a->gain > 0.0f)) return bad("gain must be > 0");
    if (!(a->lum_floor > 0.0f)) return bad("lum_floor must be > 0");
    if (a->tiling.num_ranks > 1) return bad("the pass works on a whole frame (tiling.num_ranks > 1)");
    if (a->tiling.local_rows != 0 && a->tiling.local_rows != a->height) return bad("tiling.local_rows is not the frame's height");
    const uint64_t n = (uint64_t)a->width * a->height;
    if (n > 0x7fffffffull) return bad("frame too large (width * height)");
    if (n == 0) return RT_OK;  // no pixel
    if (!a->gradient) return bad("NULL gradient");
    if (!a->history) return bad("NULL history");
    const uint32_t sw = (a->width + a->stride - 1u) / a->stride, sh = (a->height + a->stride - 1u) / a->stride;
    if (overlaps(a->gradient, (uint64_t)sw * sh * 8u, a->history, n * 16u)) return bad("gradient overlaps history");
    dev::AdaptParams P;
    P.gradient = (const float2*)a->gradient;
    P.history = (float4*)a->history;
    P.width = a->width;
    P.height = a->height;
    P.sw = sw;
    P.sh = sh;
    P.stride = a->stride;
    P.radius = (int32_t)a->radius;
    P.power = a->power;
    P.gain = a->gain;
    P.lum_floor = a->lum_floor;
    const dim3 block(dev::kGaTileW, dev::kGaTileH);
    const dim3 grid((a->width + dev::kGaTileW - 1) / dev::kGaTileW, (a->height + dev::kGaTileH - 1) / dev::kGaTileH);
    (void)hipGetLastError();
    hipLaunchKernelGGL(dev::history_adapt_kernel, grid, block, 0, (hipStream_t)stream, P);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        set_error(std::string("rt_history_adapt: kernel launch: ") + hipGetErrorString(e));
        return RT_ERR_LAUNCH;
    }
    return RT_OK;
}

}  // extern "C"
