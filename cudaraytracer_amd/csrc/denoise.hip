// denoise.hip — edge-avoiding à-trous wavelet filter for low-spp frames (rt_denoise, include/rt_hip.h).
//
// The reference has no denoiser: while the camera moves, its viewer shows the raw frame of LaunchKernel
// (CudaLayer.cpp:372-386).  The filter (Dammertz et al. 2010) runs N iterations of a 5×5 B3-spline kernel whose taps
// are 2^i pixels apart, each tap weighted by how close its normal, depth (rt_gbuffer's planes) and colour are to the
// centre's.  Design:
//   * one launch per iteration, one lane per pixel, 32×16-pixel workgroups; every pixel is written by exactly one lane
//     from values of the previous iteration's plane: no atomics, no cross-workgroup dependence, deterministic;
//   * steps 1, 2 and 4 stage the tile and its 2·step halo (colour + normal/depth, 32 B per pixel) in LDS: 36×20 pixels
//     (23 KB), 40×24 (30 KB) and 48×32 (48 KB), so the 25 taps of a pixel read LDS; larger steps read global memory directly — a
//     wave's tap is two runs of 32 consecutive float4 per plane, and the planes (33 MB at 1080p) stay in the
//     Infinity Cache between launches;
//   * demodulation by the albedo is fused into the first launch's loads, remodulation and the RGBA8 pack into the last
//     launch's stores; intermediate colour ping-pongs in the caller's scratch with the pixel's validity
//     (prim_id >= 0) in its w channel, so only the first launch reads prim_id;
//   * the guide planes stay float4 / int32 (no packed internal format).
// Arithmetic: binary32; the taps are summed in row-major order (dy outer, dx inner); the per-tap divisions by sigma_n,
// sigma_z·max(t_p, 1e-3) and (sigma_c·2^-i)² are multiplications by constants computed once per launch / pixel, the
// one exponential per tap is v_exp_f32 (see `tap`).  Against the float64 statement of the definition the result is
// within 1.1 × the spread of a float32 numpy run of it (tests/test_gpu_denoise.py allows 4 ×).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <string>

#include "rt_epilogue.h"
#include "rt_internal.h"

namespace rt {
namespace dev {

constexpr int kDnTileW = 32, kDnTileH = 16;
constexpr float kAlbedoFloor = 1.0f / 256.0f;

struct DnParams {
    const float4* in;       // c_i: the caller's colour (first launch) or a scratch plane (rgb, w = 1 valid / 0 miss)
    const float4* nd;       // normal.xyz, t
    const float4* albedo;   // first and last launch with RT_DENOISE_DEMODULATE
    const int32_t* prim;    // first launch
    float4* out;            // c_{i+1}: a scratch plane, or out_color (last launch; may be NULL)
    uint32_t* pos;          // last launch (may be NULL)
    uint32_t width, height;
    uint32_t step;          // 2^i
    uint32_t flags;         // rt_denoise_flags
    float k_n;              // -log2(e) / sigma_n
    float sigma_z;
    float k_c;              // -log2(e) / (sigma_c · 2^-i)²
};

__device__ __forceinline__ float3 albedo_floor(const float4 a) {
    return make_float3(fmaxf(a.x, kAlbedoFloor), fmaxf(a.y, kAlbedoFloor), fmaxf(a.z, kAlbedoFloor));
}

// c_0 of a pixel: the caller's colour (RT_DENOISE_COLOR_IS_SUM: rgb / w, 0 where w = 0), demodulated if asked; w = the
// pixel's validity
__device__ __forceinline__ float4 first_colour(const DnParams& P, const size_t i) {
    float4 c = P.in[i];
    if (P.flags & RT_DENOISE_COLOR_IS_SUM) {
        if (c.w == 0.0f) c = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        else c = make_float4(c.x / c.w, c.y / c.w, c.z / c.w, 0.0f);
    }
    if (P.flags & RT_DENOISE_DEMODULATE) {
        const float3 a = albedo_floor(P.albedo[i]);
        c.x = c.x / a.x;
        c.y = c.y / a.y;
        c.z = c.z / a.z;
    }
    c.w = P.prim[i] >= 0 ? 1.0f : 0.0f;
    return c;
}

// The centre pixel's terms and the running sums of its taps.  A tap's weight is h·exp(-(e_n + e_z + e_c)) evaluated as
// h·exp2(k_n·max(0, 1 - n_p·n_q) + k_z·|t_p - t_q| + k_c·|c_p - c_q|²) with k = -log2(e) / sigma terms folded on the
// host (k_n, k_c) and once per pixel (k_z): one v_exp_f32 per tap, explicit FMAs (the library is compiled with
// -ffp-contract=off), 23 VALU instructions per tap instead of the 48 of the expression written out with expf.
struct DnPixel {
    float4 c, n;    // c_i(p) (w: validity), (normal, t) of p
    float k_z;      // -log2(e) / (sigma_z · max(t_p, 1e-3))
    float sw, sr, sg, sb;
};
__device__ __forceinline__ void tap(DnPixel& p, const float k_n, const float k_c, const float h, const float4 cq,
                                    const float4 nq, const bool ok) {
    const float ndot = __builtin_fmaf(p.n.z, nq.z, __builtin_fmaf(p.n.y, nq.y, p.n.x * nq.x));
    const float dr = p.c.x - cq.x, dg = p.c.y - cq.y, db = p.c.z - cq.z;
    const float d2 = __builtin_fmaf(db, db, __builtin_fmaf(dg, dg, dr * dr));
    const float arg = __builtin_fmaf(d2, k_c, __builtin_fmaf(fabsf(p.n.w - nq.w), p.k_z, fmaxf(0.0f, 1.0f - ndot) * k_n));
    float w = h * __builtin_amdgcn_exp2f(arg);
    w = ok ? w : 0.0f;  // a miss or a pixel outside the frame: skipped
    p.sw = p.sw + w;
    p.sr = __builtin_fmaf(w, cq.x, p.sr);
    p.sg = __builtin_fmaf(w, cq.y, p.sg);
    p.sb = __builtin_fmaf(w, cq.z, p.sb);
}
constexpr float kLog2e = 1.4426950408889634f;
__device__ __forceinline__ DnPixel begin_pixel(const DnParams& P, const float4 c, const float4 n) {
    return DnPixel{c, n, -kLog2e / (P.sigma_z * fmaxf(n.w, 1e-3f)), 0.0f, 0.0f, 0.0f, 0.0f};
}
__device__ __forceinline__ float4 end_pixel(const DnPixel& p) {
    return make_float4(p.sr / p.sw, p.sg / p.sw, p.sb / p.sw, 1.0f);
}

// S: the step of the LDS builds (1, 2, 4), 0 = the global-memory build (any step).  FIRST: iteration 0 (S = 1).
// LAST: iteration N - 1.
template <int S, bool FIRST, bool LAST>
__global__ __launch_bounds__(kDnTileW * kDnTileH) void denoise_kernel(const DnParams P) {
    static_assert(!FIRST || S == 1, "the first iteration's step is 1");
    constexpr int R = 2 * S;                                   // halo
    constexpr int TW = kDnTileW + 2 * R, TH = kDnTileH + 2 * R;  // staged tile
    constexpr float h[5] = {1.0f / 16.0f, 1.0f / 4.0f, 3.0f / 8.0f, 1.0f / 4.0f, 1.0f / 16.0f};
    const int x0 = (int)blockIdx.x * kDnTileW, y0 = (int)blockIdx.y * kDnTileH;
    const int x = x0 + (int)threadIdx.x, y = y0 + (int)threadIdx.y;
    const int W = (int)P.width, H = (int)P.height;
    const bool inside = x < W && y < H;
    const size_t pix = (size_t)(inside ? y : 0) * P.width + (size_t)(inside ? x : 0);
    float4 cp;
    if constexpr (S > 0) {
        __shared__ float4 col[TW * TH];
        __shared__ float4 gd[TW * TH];
        const int tid = (int)(threadIdx.y * kDnTileW + threadIdx.x);
        for (int k = tid; k < TW * TH; k += kDnTileW * kDnTileH) {
            const int ly = k / TW, lx = k - ly * TW;
            const int gx = x0 - R + lx, gy = y0 - R + ly;
            float4 c = make_float4(0.0f, 0.0f, 0.0f, 0.0f), n = c;  // outside the frame: skipped like a miss
            if (gx >= 0 && gx < W && gy >= 0 && gy < H) {
                const size_t i = (size_t)gy * P.width + (size_t)gx;
                c = FIRST ? first_colour(P, i) : P.in[i];
                n = P.nd[i];
            }
            col[k] = c;
            gd[k] = n;
        }
        __syncthreads();
        if (!inside) return;
        const int lc = ((int)threadIdx.y + R) * TW + (int)threadIdx.x + R;
        cp = col[lc];
        if (cp.w > 0.5f) {
            DnPixel px = begin_pixel(P, cp, gd[lc]);
#pragma unroll
            for (int dy = -2; dy <= 2; dy++) {
#pragma unroll
                for (int dx = -2; dx <= 2; dx++) {
                    const int lq = lc + dy * S * TW + dx * S;
                    const float4 cq = col[lq];
                    tap(px, P.k_n, P.k_c, h[dx + 2] * h[dy + 2], cq, gd[lq], cq.w > 0.5f);
                }
            }
            cp = end_pixel(px);
        }
    } else {
        if (!inside) return;
        cp = P.in[pix];
        if (cp.w > 0.5f) {
            DnPixel px = begin_pixel(P, cp, P.nd[pix]);
            const int s = (int)P.step;
#pragma unroll
            for (int dy = -2; dy <= 2; dy++) {
                const int qy = y + dy * s;
                if (qy < 0 || qy >= H) continue;  // (wave-uniform but for the wave's two rows)
#pragma unroll
                for (int dx = -2; dx <= 2; dx++) {
                    const int qx = x + dx * s;
                    const bool in_frame = qx >= 0 && qx < W;
                    const size_t i = (size_t)qy * P.width + (size_t)(in_frame ? qx : x);
                    const float4 cq = P.in[i];
                    tap(px, P.k_n, P.k_c, h[dx + 2] * h[dy + 2], cq, P.nd[i], in_frame && cq.w > 0.5f);
                }
            }
            cp = end_pixel(px);
        }
    }
    if constexpr (LAST) {
        float3 c = make_float3(cp.x, cp.y, cp.z);
        if (P.flags & RT_DENOISE_DEMODULATE) {
            const float3 a = albedo_floor(P.albedo[pix]);
            c = make_float3(c.x * a.x, c.y * a.y, c.z * a.z);
        }
        if (P.out) P.out[pix] = make_float4(c.x, c.y, c.z, 1.0f);
        // the render kernels' epilogue (Kernel.cu:152-157)
        if (P.pos) P.pos[pix] = rgb_to_int(255.0f * sqrtf(c.x), 255.0f * sqrtf(c.y), 255.0f * sqrtf(c.z));
    } else {
        P.out[pix] = cp;
    }
}

}  // namespace dev
}  // namespace rt

using namespace rt;

static uint64_t scratch_planes(const uint32_t iterations) { return iterations <= 1 ? 0u : (iterations == 2 ? 1u : 2u); }

uint64_t rt_denoise_scratch_bytes(uint32_t width, uint32_t height, uint32_t iterations) {
    return (uint64_t)width * height * 16u * scratch_planes(iterations);
}

int rt_denoise(const rt_denoise_args* a, rt_stream stream) {
    const auto bad = [](const char* msg) {
        set_error(std::string("rt_denoise: ") + msg);
        return (int)RT_ERR_INVALID_ARGUMENT;
    };
    if (!a) return bad("NULL args");
    if (a->reserved != 0) return bad("reserved fields must be 0");
    if (a->flags & ~(uint32_t)(RT_DENOISE_DEMODULATE | RT_DENOISE_COLOR_IS_SUM)) return bad("unknown flags");
    if (a->iterations < 1 || a->iterations > 6) return bad("iterations must be 1..6");
    if (!(a->sigma_c > 0.0f) || !(a->sigma_n > 0.0f) || !(a->sigma_z > 0.0f)) return bad("sigma_c, sigma_n and sigma_z must be > 0");
    if (a->tiling.num_ranks > 1) return bad("the filter works on a whole frame (tiling.num_ranks > 1)");
    if (a->tiling.local_rows != 0 && a->tiling.local_rows != a->height) return bad("tiling.local_rows is not the frame's height");
    if (!a->color || !a->normal_depth || !a->albedo || !a->prim_id) return bad("NULL input plane");
    if (!a->out_color && !a->pos) return bad("no output buffer");
    const uint64_t n = (uint64_t)a->width * a->height;
    if (n > 0x7fffffffull) return bad("frame too large");
    const uint64_t scratch_bytes = rt_denoise_scratch_bytes(a->width, a->height, a->iterations);
    if (scratch_bytes && !a->scratch) return bad("NULL scratch (rt_denoise_scratch_bytes)");
    const void* ins[4] = {a->color, a->normal_depth, a->albedo, a->prim_id};
    const uint64_t in_bytes[4] = {n * 16u, n * 16u, n * 16u, n * 4u};
    const void* outs[3] = {a->out_color, a->pos, a->scratch};
    const uint64_t out_bytes[3] = {n * 16u, n * 4u, scratch_bytes};
    for (int o = 0; o < 3; o++) {
        for (int i = 0; i < 4; i++)
            if (overlaps(outs[o], out_bytes[o], ins[i], in_bytes[i]))
                return bad(o == 0 && i == 0 ? "out_color must not alias color" : "an output or scratch overlaps an input plane");
        for (int p = o + 1; p < 3; p++)
            if (overlaps(outs[o], out_bytes[o], outs[p], out_bytes[p])) return bad("outputs and scratch overlap each other");
    }
    if (n == 0) return RT_OK;
    dev::DnParams P{};
    P.nd = (const float4*)a->normal_depth;
    P.albedo = (const float4*)a->albedo;
    P.prim = a->prim_id;
    P.width = a->width;
    P.height = a->height;
    P.flags = a->flags;
    P.k_n = -dev::kLog2e / a->sigma_n;
    P.sigma_z = a->sigma_z;
    float4* const planes[2] = {(float4*)a->scratch, (float4*)a->scratch + n};
    const dim3 block(dev::kDnTileW, dev::kDnTileH);
    const dim3 grid((a->width + dev::kDnTileW - 1) / dev::kDnTileW, (a->height + dev::kDnTileH - 1) / dev::kDnTileH);
    hipStream_t s = (hipStream_t)stream;
    (void)hipGetLastError();
    const float4* in = (const float4*)a->color;
    for (uint32_t i = 0; i < a->iterations; i++) {
        const bool last = i + 1 == a->iterations;
        const float sc = a->sigma_c * std::ldexp(1.0f, -(int)i);  // sigma_c · 2^-i
        P.in = in;
        P.out = last ? (float4*)a->out_color : planes[i & 1u];
        P.pos = last ? a->pos : nullptr;
        P.step = 1u << i;
        P.k_c = -dev::kLog2e / (sc * sc);
        if (i == 0) {
            if (last) hipLaunchKernelGGL((dev::denoise_kernel<1, true, true>), grid, block, 0, s, P);
            else hipLaunchKernelGGL((dev::denoise_kernel<1, true, false>), grid, block, 0, s, P);
        } else if (i == 1) {
            if (last) hipLaunchKernelGGL((dev::denoise_kernel<2, false, true>), grid, block, 0, s, P);
            else hipLaunchKernelGGL((dev::denoise_kernel<2, false, false>), grid, block, 0, s, P);
        } else if (i == 2) {
            if (last) hipLaunchKernelGGL((dev::denoise_kernel<4, false, true>), grid, block, 0, s, P);
            else hipLaunchKernelGGL((dev::denoise_kernel<4, false, false>), grid, block, 0, s, P);
        } else {
            if (last) hipLaunchKernelGGL((dev::denoise_kernel<0, false, true>), grid, block, 0, s, P);
            else hipLaunchKernelGGL((dev::denoise_kernel<0, false, false>), grid, block, 0, s, P);
        }
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) {
            set_error(std::string("rt_denoise: kernel launch: ") + hipGetErrorString(e));
            return RT_ERR_LAUNCH;
        }
        in = P.out;
    }
    return RT_OK;
}
