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

// ---------------------------------------------------------------------------------------------------------------------
// rt_denoise_variance: the same filter with the colour tolerance of each pixel taken from its own
// luminance variance.  One launch computes var_0 from rt_temporal_moments' plane, then one launch per iteration from
// dnv_kernel, a template of its own beside denoise_kernel (whose instantiations keep their code objects).
// Planes between the launches: float4 (rgb, variance), a negative w marking a miss (or, in LDS, a pixel outside the frame).
// ---------------------------------------------------------------------------------------------------------------------
struct DnvParams {
    const float4* in;       // the caller's colour (variance stage: rgb, w = history length) or a scratch plane
    const float2* moments;  // variance stage
    const float4* nd;       // normal.xyz, t
    const int32_t* prim;    // variance stage
    float4* out;            // a scratch plane, or out_color (last launch; may be NULL)
    uint32_t* pos;          // last launch (may be NULL)
    uint32_t width, height;
    uint32_t step;          // 2^i
    float min_history;
    float k_n;              // -log2(e) / sigma_n
    float sigma_z;
    float sigma_l;
};

__device__ __forceinline__ float lum(const float4 c) { return (0.2126f * c.x + 0.7152f * c.y) + 0.0722f * c.z; }

constexpr int kVarR = 3;  // the spatial estimate's window: 7×7
// ... and the factor on it: with a history this short the window's own estimate is low (the centre's sample dominates
// its weighted mean), so it is multiplied by 4, as the SVGF sample code does (variance *= 4 / historyLength)
constexpr float kShortHistoryBoost = 4.0f;

// The variance stage: var_0 = max(0, m2 − m1²) / N from the pixel's own moments where its history is at least
// min_history long, else 4 · that of the moments of its 7×7 neighbours weighted by exp(−(e_n + e_z)).  The tile and its 3-pixel
// halo of moments, normal/depth and validity are staged in LDS (38×22 pixels of 28 B: 23 KB); only lanes with a short
// history walk the window.
__global__ __launch_bounds__(kDnTileW * kDnTileH) void dnv_variance_kernel(const DnvParams P) {
    constexpr int TW = kDnTileW + 2 * kVarR, TH = kDnTileH + 2 * kVarR;
    __shared__ float4 gd[TW * TH];
    __shared__ float2 mo[TW * TH];
    __shared__ float okq[TW * TH];  // 1 = a hit inside the frame, 0 = skipped
    const int x0 = (int)blockIdx.x * kDnTileW, y0 = (int)blockIdx.y * kDnTileH;
    const int x = x0 + (int)threadIdx.x, y = y0 + (int)threadIdx.y;
    const int W = (int)P.width, H = (int)P.height;
    const int tid = (int)(threadIdx.y * kDnTileW + threadIdx.x);
    for (int k = tid; k < TW * TH; k += kDnTileW * kDnTileH) {
        const int ly = k / TW, lx = k - ly * TW;
        const int gx = x0 - kVarR + lx, gy = y0 - kVarR + ly;
        float4 n = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        float2 m = make_float2(0.0f, 0.0f);
        float ok = 0.0f;
        if (gx >= 0 && gx < W && gy >= 0 && gy < H) {
            const size_t i = (size_t)gy * P.width + (size_t)gx;
            n = P.nd[i];
            m = P.moments[i];
            ok = P.prim[i] >= 0 ? 1.0f : 0.0f;
        }
        gd[k] = n;
        mo[k] = m;
        okq[k] = ok;
    }
    __syncthreads();
    if (x >= W || y >= H) return;
    const size_t pix = (size_t)y * P.width + (size_t)x;
    const int lc = ((int)threadIdx.y + kVarR) * TW + (int)threadIdx.x + kVarR;
    const float4 c = P.in[pix];
    float var = -1.0f;  // a miss
    if (okq[lc] > 0.5f) {
        const float N = fmaxf(c.w, 1.0f);
        float2 m = mo[lc];
        float boost = 1.0f;
        if (!(N >= P.min_history)) {
            boost = kShortHistoryBoost;
            const float4 n = gd[lc];
            const float k_z = -kLog2e / (P.sigma_z * fmaxf(n.w, 1e-3f));
            float sg = 0.0f, s1 = 0.0f, s2 = 0.0f;
            for (int dy = -kVarR; dy <= kVarR; dy++) {
#pragma unroll
                for (int dx = -kVarR; dx <= kVarR; dx++) {
                    const int lq = lc + dy * TW + dx;
                    const float4 nq = gd[lq];
                    const float2 mq = mo[lq];
                    const float ndot = __builtin_fmaf(n.z, nq.z, __builtin_fmaf(n.y, nq.y, n.x * nq.x));
                    const float arg = __builtin_fmaf(fabsf(n.w - nq.w), k_z, fmaxf(0.0f, 1.0f - ndot) * P.k_n);
                    float g = __builtin_amdgcn_exp2f(arg);
                    g = okq[lq] > 0.5f ? g : 0.0f;
                    sg = sg + g;
                    s1 = __builtin_fmaf(g, mq.x, s1);
                    s2 = __builtin_fmaf(g, mq.y, s2);
                }
            }
            m = make_float2(s1 / sg, s2 / sg);  // (the centre's g is 1: sg > 0)
        }
        var = (boost * fmaxf(0.0f, m.y - m.x * m.x)) / N;
    }
    P.out[pix] = make_float4(c.x, c.y, c.z, var);
}

// The centre pixel's terms and running sums: DnPixel's with the luminance in place of the colour distance and the
// variance sums beside the colour's.  A tap's weight is h·exp2(k_n·max(0, 1 − n_p·n_q) + k_z·|t_p − t_q| + k_l·|l_p − l_q|),
// k_l = −log2(e) / (sigma_l·sqrt(v~(p) + 1e-6)) once per pixel: one v_exp_f32 per tap, explicit FMAs.
struct DnvPixel {
    float4 c, n;     // c_i(p) (w: variance), (normal, t) of p
    float l;         // lum(c_i(p))
    float k_z, k_l;
    float sw, sr, sg, sb, sv;
};
__device__ __forceinline__ void tap_v(DnvPixel& p, const float k_n, const float h, const float4 cq, const float4 nq,
                                      const bool ok) {
    const float ndot = __builtin_fmaf(p.n.z, nq.z, __builtin_fmaf(p.n.y, nq.y, p.n.x * nq.x));
    const float dl = fabsf(p.l - lum(cq));
    const float arg = __builtin_fmaf(dl, p.k_l, __builtin_fmaf(fabsf(p.n.w - nq.w), p.k_z, fmaxf(0.0f, 1.0f - ndot) * k_n));
    float w = h * __builtin_amdgcn_exp2f(arg);
    w = ok ? w : 0.0f;  // a miss or a pixel outside the frame: skipped (its cq.w is negative)
    p.sw = p.sw + w;
    p.sr = __builtin_fmaf(w, cq.x, p.sr);
    p.sg = __builtin_fmaf(w, cq.y, p.sg);
    p.sb = __builtin_fmaf(w, cq.z, p.sb);
    p.sv = __builtin_fmaf(w * w, cq.w, p.sv);
}
__device__ __forceinline__ DnvPixel begin_pixel_v(const DnvParams& P, const float4 c, const float4 n, const float vbar) {
    return DnvPixel{c, n, lum(c), -kLog2e / (P.sigma_z * fmaxf(n.w, 1e-3f)), -kLog2e / (P.sigma_l * sqrtf(vbar + 1e-6f)),
                    0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
}
__device__ __forceinline__ float4 end_pixel_v(const DnvPixel& p) {
    return make_float4(p.sr / p.sw, p.sg / p.sw, p.sb / p.sw, p.sv / (p.sw * p.sw));
}

// S: the step of the LDS builds (1, 2, 4), 0 = the global-memory build (any step).  LAST: iteration N − 1.
template <int S, bool LAST>
__global__ __launch_bounds__(kDnTileW * kDnTileH) void dnv_kernel(const DnvParams P) {
    constexpr int R = 2 * S;                                   // halo (>= 2 where S > 0: the 3×3 pre-filter reads it too)
    constexpr int TW = kDnTileW + 2 * R, TH = kDnTileH + 2 * R;  // staged tile
    constexpr float h[5] = {1.0f / 16.0f, 1.0f / 4.0f, 3.0f / 8.0f, 1.0f / 4.0f, 1.0f / 16.0f};
    constexpr float k3[3] = {1.0f / 4.0f, 1.0f / 2.0f, 1.0f / 4.0f};
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
            float4 c = make_float4(0.0f, 0.0f, 0.0f, -1.0f), n = make_float4(0.0f, 0.0f, 0.0f, 0.0f);  // outside: a miss
            if (gx >= 0 && gx < W && gy >= 0 && gy < H) {
                const size_t i = (size_t)gy * P.width + (size_t)gx;
                c = P.in[i];
                n = P.nd[i];
            }
            col[k] = c;
            gd[k] = n;
        }
        __syncthreads();
        if (!inside) return;
        const int lc = ((int)threadIdx.y + R) * TW + (int)threadIdx.x + R;
        cp = col[lc];
        if (cp.w >= 0.0f) {
            float sk = 0.0f, skv = 0.0f;
#pragma unroll
            for (int dy = -1; dy <= 1; dy++) {
#pragma unroll
                for (int dx = -1; dx <= 1; dx++) {
                    const float vq = col[lc + dy * TW + dx].w;
                    const float k = vq >= 0.0f ? k3[dx + 1] * k3[dy + 1] : 0.0f;
                    sk = sk + k;
                    skv = __builtin_fmaf(k, vq, skv);
                }
            }
            DnvPixel px = begin_pixel_v(P, cp, gd[lc], skv / sk);
#pragma unroll
            for (int dy = -2; dy <= 2; dy++) {
#pragma unroll
                for (int dx = -2; dx <= 2; dx++) {
                    const int lq = lc + dy * S * TW + dx * S;
                    const float4 cq = col[lq];
                    tap_v(px, P.k_n, h[dx + 2] * h[dy + 2], cq, gd[lq], cq.w >= 0.0f);
                }
            }
            cp = end_pixel_v(px);
        }
    } else {
        if (!inside) return;
        cp = P.in[pix];
        if (cp.w >= 0.0f) {
            float sk = 0.0f, skv = 0.0f;
#pragma unroll
            for (int dy = -1; dy <= 1; dy++) {
                const int qy = y + dy;
                if (qy < 0 || qy >= H) continue;
#pragma unroll
                for (int dx = -1; dx <= 1; dx++) {
                    const int qx = x + dx;
                    const bool in_frame = qx >= 0 && qx < W;
                    const float vq = P.in[(size_t)qy * P.width + (size_t)(in_frame ? qx : x)].w;
                    const float k = in_frame && vq >= 0.0f ? k3[dx + 1] * k3[dy + 1] : 0.0f;
                    sk = sk + k;
                    skv = __builtin_fmaf(k, vq, skv);
                }
            }
            DnvPixel px = begin_pixel_v(P, cp, P.nd[pix], skv / sk);
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
                    tap_v(px, P.k_n, h[dx + 2] * h[dy + 2], cq, P.nd[i], in_frame && cq.w >= 0.0f);
                }
            }
            cp = end_pixel_v(px);
        }
    }
    if constexpr (LAST) {
        if (P.out) P.out[pix] = make_float4(cp.x, cp.y, cp.z, fmaxf(cp.w, 0.0f));  // (a miss: variance 0)
        // the render kernels' epilogue (Kernel.cu:152-157)
        if (P.pos) P.pos[pix] = rgb_to_int(255.0f * sqrtf(cp.x), 255.0f * sqrtf(cp.y), 255.0f * sqrtf(cp.z));
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

// rt_denoise_variance: the variance stage writes plane 0; the iterations ping-pong between the two planes and the last
// one writes the outputs, so a single iteration needs one plane and any more need two.
uint64_t rt_denoise_variance_scratch_bytes(uint32_t width, uint32_t height, uint32_t iterations) {
    return (uint64_t)width * height * 16u * (iterations <= 1 ? 1u : 2u);
}

int rt_denoise_variance(const rt_denoise_variance_args* a, rt_stream stream) {
    const auto bad = [](const char* msg) {
        set_error(std::string("rt_denoise_variance: ") + msg);
        return (int)RT_ERR_INVALID_ARGUMENT;
    };
    if (!a) return bad("NULL args");
    if (a->reserved[0] != 0 || a->reserved[1] != 0) return bad("reserved fields must be 0");
    if (a->flags != 0) return bad("unknown flags");
    if (a->iterations < 1 || a->iterations > 6) return bad("iterations must be 1..6");
    if (a->min_history < 1 || a->min_history > 4096) return bad("min_history must be 1..4096");
    if (!(a->sigma_l > 0.0f) || !(a->sigma_n > 0.0f) || !(a->sigma_z > 0.0f)) return bad("sigma_l, sigma_n and sigma_z must be > 0");
    if (a->tiling.num_ranks > 1) return bad("the filter works on a whole frame (tiling.num_ranks > 1)");
    if (a->tiling.local_rows != 0 && a->tiling.local_rows != a->height) return bad("tiling.local_rows is not the frame's height");
    if (!a->color || !a->moments || !a->normal_depth || !a->prim_id) return bad("NULL input plane");
    if (!a->out_color && !a->pos) return bad("no output buffer");
    const uint64_t n = (uint64_t)a->width * a->height;
    if (n > 0x7fffffffull) return bad("frame too large");
    const uint64_t scratch_bytes = rt_denoise_variance_scratch_bytes(a->width, a->height, a->iterations);
    if (scratch_bytes && !a->scratch) return bad("NULL scratch (rt_denoise_variance_scratch_bytes)");
    const void* ins[4] = {a->color, a->moments, a->normal_depth, a->prim_id};
    const uint64_t in_bytes[4] = {n * 16u, n * 8u, n * 16u, n * 4u};
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
    dev::DnvParams P{};
    P.moments = (const float2*)a->moments;
    P.nd = (const float4*)a->normal_depth;
    P.prim = a->prim_id;
    P.width = a->width;
    P.height = a->height;
    P.min_history = (float)a->min_history;
    P.k_n = -dev::kLog2e / a->sigma_n;
    P.sigma_z = a->sigma_z;
    P.sigma_l = a->sigma_l;
    float4* const planes[2] = {(float4*)a->scratch, (float4*)a->scratch + n};
    const dim3 block(dev::kDnTileW, dev::kDnTileH);
    const dim3 grid((a->width + dev::kDnTileW - 1) / dev::kDnTileW, (a->height + dev::kDnTileH - 1) / dev::kDnTileH);
    hipStream_t s = (hipStream_t)stream;
    (void)hipGetLastError();
    const auto launched = []() {
        const hipError_t e = hipGetLastError();
        if (e == hipSuccess) return true;
        set_error(std::string("rt_denoise_variance: kernel launch: ") + hipGetErrorString(e));
        return false;
    };
    P.in = (const float4*)a->color;
    P.out = planes[0];
    hipLaunchKernelGGL(dev::dnv_variance_kernel, grid, block, 0, s, P);
    if (!launched()) return RT_ERR_LAUNCH;
    for (uint32_t i = 0; i < a->iterations; i++) {
        const bool last = i + 1 == a->iterations;
        P.in = planes[i & 1u];
        P.out = last ? (float4*)a->out_color : planes[(i + 1u) & 1u];
        P.pos = last ? a->pos : nullptr;
        P.step = 1u << i;
        if (i == 0) {
            if (last) hipLaunchKernelGGL((dev::dnv_kernel<1, true>), grid, block, 0, s, P);
            else hipLaunchKernelGGL((dev::dnv_kernel<1, false>), grid, block, 0, s, P);
        } else if (i == 1) {
            if (last) hipLaunchKernelGGL((dev::dnv_kernel<2, true>), grid, block, 0, s, P);
            else hipLaunchKernelGGL((dev::dnv_kernel<2, false>), grid, block, 0, s, P);
        } else if (i == 2) {
            if (last) hipLaunchKernelGGL((dev::dnv_kernel<4, true>), grid, block, 0, s, P);
            else hipLaunchKernelGGL((dev::dnv_kernel<4, false>), grid, block, 0, s, P);
        } else {
            if (last) hipLaunchKernelGGL((dev::dnv_kernel<0, true>), grid, block, 0, s, P);
            else hipLaunchKernelGGL((dev::dnv_kernel<0, false>), grid, block, 0, s, P);
        }
        if (!launched()) return RT_ERR_LAUNCH;
    }
    return RT_OK;
}
