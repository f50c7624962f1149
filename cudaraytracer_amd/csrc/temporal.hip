// temporal.hip — reprojected temporal accumulation for moving cameras (rt_temporal, include/rt_hip.h).
//
// The reference has no temporal filter: while the camera moves, its viewer shows the raw frame of LaunchKernel
// (CudaLayer.cpp:372-386) and its accumulation restarts.  This pass takes the previous frame's accumulated colour where
// the surface seen at a pixel was in the previous frame, rejects it where that surface was hidden or is another one
// (primitive id, depth along the previous centre ray, normal: rt_gbuffer's planes of both frames) and blends the new
// sample in.  Design:
//   * one launch, one lane per pixel, 64×4-pixel workgroups: a wave covers 64 consecutive pixels of a row, so its loads
//     and stores of the float4 planes are whole 1-KB runs and a tap of the gather is one or two such runs of the
//     previous frame's row; no LDS, no scratch, no atomics; every pixel is written by exactly one lane from planes the
//     launch only reads: deterministic;
//   * a tap's primitive id (4 B) is tested before its history and normal/depth records (32 B) are loaded; the four
//     id loads, then the loads of the taps that passed, are issued together and consumed afterwards;
//   * the centre ray restates the few operations of render.hip's camera_ray_at / lane_camera (Kernel.cu:139-146 with
//     both jitter numbers 0.5) instead of sharing them, so the render kernels' code objects are untouched.
// Arithmetic: binary32, one rounding per written operation (-ffp-contract=off), IEEE division and square root; the
// operations and their order are those of the numpy restatement (tests/test_temporal_host.py temporal_reference in
// float32).  A resting camera snaps to its own pixel: one tap of weight 1, so the result is h + (1/N)·(c − h) bit for
// bit.
// rt_temporal_dynamic is a second kernel over the same body: between the world point and the camera
// inverse it moves the point by its hittable's entry of a per-hittable motion table (rt_scene_motion), so history
// survives object edits; tests/test_dynamic_host.py temporal_dynamic_reference restates it.
// rt_temporal_moments adds two more kernels over the same body: beside the colour they accumulate the
// first and second moment of the pixel's luminance (one 8-byte load per counting tap, issued with the history loads, and
// one 8-byte store), from which rt_denoise_variance takes each pixel's own noise level.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "rt_epilogue.h"
#include "rt_internal.h"

namespace rt {
namespace dev {

constexpr int kTpTileW = 64, kTpTileH = 4;
constexpr float kSnap = 1.0f / 256.0f;    // a coordinate this close to an integer becomes it
constexpr float kMinWeight = 1.0f / 100.0f;  // history exists from this sum of counting tap weights

struct v3 {
    float x, y, z;
};
__device__ __forceinline__ v3 ld3(const float* p) { return v3{p[0], p[1], p[2]}; }
__device__ __forceinline__ v3 operator+(const v3 a, const v3 b) { return v3{a.x + b.x, a.y + b.y, a.z + b.z}; }
__device__ __forceinline__ v3 operator-(const v3 a, const v3 b) { return v3{a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ v3 operator*(const float s, const v3 a) { return v3{s * a.x, s * a.y, s * a.z}; }
__device__ __forceinline__ float dot3(const v3 a, const v3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }

// where the camera ray through (u, v) starts (Kernel.cu:139-142): (near · dist + origin) + fov · forward
__device__ __forceinline__ v3 ray_start(const TemporalCamera& C, const float u, const float v, v3& dist) {
    dist = u * ld3(C.right) + v * ld3(C.up);
    return (C.near_plane * dist + ld3(C.origin)) + ld3(C.fov_fwd);
}

// The pass's body.  DYNAMIC = false is rt_temporal; DYNAMIC = true is rt_temporal_dynamic: step 1a, the
// hittable's motion entry table[id] = (o.xyz, s), moves the world point to where that surface point was in the previous
// scene before the camera inverse.  The static build holds none of it (if constexpr): temporal_kernel keeps the 63
// VGPRs and 905 instructions it had before the second kernel existed.
// MOMENTS = true is rt_temporal_moments: the counting taps also fetch prev_moments = (m1, m2) and the
// pixel's luminance l and l·l are blended into their weighted mean with the colour's alpha.  Again if constexpr: the
// two kernels without moments hold none of it.
template <bool DYNAMIC, bool MOMENTS>
__device__ __forceinline__ void temporal_body(const TemporalParams& P, const float4* table, const uint32_t num_prims,
                                              const float2* prev_moments, float2* moments) {
    const uint32_t x = blockIdx.x * kTpTileW + threadIdx.x, y = blockIdx.y * kTpTileH + threadIdx.y;
    if (x >= P.width || y >= P.height) return;
    const int W = (int)P.width, H = (int)P.height;
    const size_t pix = (size_t)y * P.width + x;
    // 0. colour
    float4 c = ((const float4*)P.color)[pix];
    if (P.flags & RT_TEMPORAL_COLOR_IS_SUM) {
        if (c.w == 0.0f) c = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        else c = make_float4(c.x / c.w, c.y / c.w, c.z / c.w, 0.0f);
    }
    float4 out = make_float4(c.x, c.y, c.z, 1.0f);
    float2 mv = make_float2(0.0f, 0.0f);
    float2 lm = make_float2(0.0f, 0.0f), mo = lm;  // (l, l·l) of this frame's colour; the moments written
    if constexpr (MOMENTS) {
        const float l = (0.2126f * c.x + 0.7152f * c.y) + 0.0722f * c.z;
        lm = mo = make_float2(l, l * l);
    }
    const int id = P.prim_id[pix];
    // 1a. the hittable's motion entry: one 16-byte load per lane (neighbouring lanes mostly share the entry: the table
    // is a few cache lines); an id beyond the table or s == 0 means no history
    float4 m = make_float4(0.0f, 0.0f, 0.0f, 1.0f);
    if constexpr (DYNAMIC) {
        if (id >= 0 && (uint32_t)id < num_prims && !(P.flags & RT_TEMPORAL_RESET)) m = table[id];
        else m.w = 0.0f;
    }
    if (id >= 0 && !(P.flags & RT_TEMPORAL_RESET) && m.w != 0.0f) {
        const float4 nd = ((const float4*)P.normal_depth)[pix];
        // 1. the world point on rt_gbuffer's centre ray
        const float u = (((float)(int)x - P.half_w) + 0.5f) / P.width_f;
        const float v = ((P.half_h - (float)(int)y) + 0.5f) / P.width_f;
        v3 dist;
        const v3 ro = ray_start(P.cur, u, v, dist);
        const v3 second = (P.cur.far_plane * dist + ld3(P.cur.k10_fwd)) + ld3(P.cur.origin);
        const v3 d = second - ro;
        const float inv = 1.0f / sqrtf(dot3(d, d));
        const v3 rd = inv * d;
        v3 Pw = ro + nd.w * rd;
        if constexpr (DYNAMIC) {
            // (0, 0, 0, 1) leaves the point as it is; else one multiply, then one add per component
            if (!(m.x == 0.0f && m.y == 0.0f && m.z == 0.0f && m.w == 1.0f)) Pw = m.w * Pw + v3{m.x, m.y, m.z};
        }
        // 2. the inverse of the ray construction under the previous camera
        const TemporalCamera& Q = P.prev;
        const v3 q = Pw - ld3(Q.origin);
        const float a = dot3(q, ld3(Q.right)), b = dot3(q, ld3(Q.up));
        const float cf = dot3(q, ld3(Q.fw)) / Q.fw_dot_fw;
        const float s = (cf - Q.fov) / (Q.k10 - Q.fov);
        const float den = Q.near_plane + s * (Q.far_plane - Q.near_plane);
        if (s > 0.0f && den > 0.0f) {
            const float up = a / den, vp = b / den;
            float px = (up * P.width_f + P.half_w) - 0.5f;
            float py = (P.half_h + 0.5f) - vp * P.width_f;
            v3 pdist;
            const v3 e = Pw - ray_start(Q, up, vp, pdist);
            const float t_exp = sqrtf(dot3(e, e));
            // 3. snap
            const float rx = rintf(px), ry = rintf(py);
            if (fabsf(px - rx) <= kSnap) px = rx;
            if (fabsf(py - ry) <= kSnap) py = ry;
            mv = make_float2(px - (float)(int)x, py - (float)(int)y);
            // 4. bilinear fetch of the taps that show the same surface
            if (px > -1.0f && px < P.width_f && py > -1.0f && py < (float)H) {  // (else no tap is inside the frame)
                const float x0f = floorf(px), y0f = floorf(py);
                const float fx = px - x0f, fy = py - y0f;
                const int x0 = (int)x0f, y0 = (int)y0f;
                const float wx[2] = {1.0f - fx, fx}, wy[2] = {1.0f - fy, fy};
                const float lim = P.depth_tol * fmaxf(t_exp, 1e-3f);
                float w[4];
                size_t at[4];
                bool ok[4];
                int pid[4];
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    const int xi = x0 + (k & 1), yj = y0 + (k >> 1);
                    w[k] = wx[k & 1] * wy[k >> 1];
                    ok[k] = w[k] > 0.0f && xi >= 0 && xi < W && yj >= 0 && yj < H;
                    at[k] = ok[k] ? (size_t)yj * P.width + (size_t)xi : pix;
                    pid[k] = id ^ 1;
                    if (ok[k]) pid[k] = P.prev_prim_id[at[k]];
                }
                float4 hq[4], nq[4];
                float2 mq[4];
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    hq[k] = nq[k] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                    mq[k] = make_float2(0.0f, 0.0f);
                    ok[k] = ok[k] && pid[k] == id;
                    if (ok[k]) {
                        hq[k] = ((const float4*)P.prev_history)[at[k]];
                        nq[k] = ((const float4*)P.prev_normal_depth)[at[k]];
                        if constexpr (MOMENTS) mq[k] = prev_moments[at[k]];
                    }
                }
                float S = 0.0f, sr = 0.0f, sg = 0.0f, sb = 0.0f, sl = 0.0f, sm1 = 0.0f, sm2 = 0.0f;
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    const float ndot = (nd.x * nq[k].x + nd.y * nq[k].y) + nd.z * nq[k].z;
                    const bool counts = ok[k] && hq[k].w > 0.0f && fabsf(nq[k].w - t_exp) <= lim && ndot >= P.min_ndot;
                    const float wk = counts ? w[k] : 0.0f;
                    S = S + wk;
                    sr = sr + wk * hq[k].x;
                    sg = sg + wk * hq[k].y;
                    sb = sb + wk * hq[k].z;
                    sl = sl + wk * hq[k].w;
                    if constexpr (MOMENTS) {
                        sm1 = sm1 + wk * mq[k].x;
                        sm2 = sm2 + wk * mq[k].y;
                    }
                }
                if (S >= kMinWeight) {
                    // 5. blend
                    const float hr = sr / S, hg = sg / S, hb = sb / S;
                    const float N = fminf(sl / S + 1.0f, P.max_history);
                    const float alpha = 1.0f / N;
                    out = make_float4(hr + alpha * (c.x - hr), hg + alpha * (c.y - hg), hb + alpha * (c.z - hb), N);
                    if constexpr (MOMENTS) {
                        const float m1 = sm1 / S, m2 = sm2 / S;
                        mo = make_float2(m1 + alpha * (lm.x - m1), m2 + alpha * (lm.y - m2));
                    }
                }
            }
        }
    }
    ((float4*)P.history)[pix] = out;
    if constexpr (MOMENTS) moments[pix] = mo;
    if (P.motion) ((float2*)P.motion)[pix] = mv;
    // the render kernels' epilogue (Kernel.cu:152-157)
    if (P.pos) P.pos[pix] = rgb_to_int(255.0f * sqrtf(out.x), 255.0f * sqrtf(out.y), 255.0f * sqrtf(out.z));
}

__global__ __launch_bounds__(kTpTileW * kTpTileH) void temporal_kernel(const TemporalParams P) {
    temporal_body<false, false>(P, nullptr, 0u, nullptr, nullptr);
}

// rt_temporal_dynamic: the same launch shape; `table` holds num_prims float4 entries (never read with RT_TEMPORAL_RESET)
__global__ __launch_bounds__(kTpTileW * kTpTileH) void temporal_dynamic_kernel(const TemporalParams P,
                                                                               const float4* __restrict__ table,
                                                                               const uint32_t num_prims) {
    temporal_body<true, false>(P, table, num_prims, nullptr, nullptr);
}

// rt_temporal_moments without and with a motion table: the bodies above plus the moments (prev_moments is never read with
// RT_TEMPORAL_RESET)
__global__ __launch_bounds__(kTpTileW * kTpTileH) void temporal_moments_kernel(const TemporalParams P,
                                                                               const float2* __restrict__ prev_moments,
                                                                               float2* __restrict__ moments) {
    temporal_body<false, true>(P, nullptr, 0u, prev_moments, moments);
}

__global__ __launch_bounds__(kTpTileW * kTpTileH) void temporal_dynamic_moments_kernel(
    const TemporalParams P, const float4* __restrict__ table, const uint32_t num_prims,
    const float2* __restrict__ prev_moments, float2* __restrict__ moments) {
    temporal_body<true, true>(P, table, num_prims, prev_moments, moments);
}

}  // namespace dev

int launch_temporal(const TemporalParams& P, void* stream) {
    const dim3 block(dev::kTpTileW, dev::kTpTileH);
    const dim3 grid((P.width + dev::kTpTileW - 1) / dev::kTpTileW, (P.height + dev::kTpTileH - 1) / dev::kTpTileH);
    (void)hipGetLastError();
    hipLaunchKernelGGL(dev::temporal_kernel, grid, block, 0, (hipStream_t)stream, P);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        set_error(std::string("rt_temporal: kernel launch: ") + hipGetErrorString(e));
        return RT_ERR_LAUNCH;
    }
    return RT_OK;
}

int launch_temporal_dynamic(const TemporalParams& P, const float* prim_motion, uint32_t num_prims, void* stream) {
    const dim3 block(dev::kTpTileW, dev::kTpTileH);
    const dim3 grid((P.width + dev::kTpTileW - 1) / dev::kTpTileW, (P.height + dev::kTpTileH - 1) / dev::kTpTileH);
    (void)hipGetLastError();
    hipLaunchKernelGGL(dev::temporal_dynamic_kernel, grid, block, 0, (hipStream_t)stream, P, (const float4*)prim_motion,
                       num_prims);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        set_error(std::string("rt_temporal_dynamic: kernel launch: ") + hipGetErrorString(e));
        return RT_ERR_LAUNCH;
    }
    return RT_OK;
}

int launch_temporal_moments(const TemporalParams& P, const bool dynamic, const float* prim_motion, uint32_t num_prims,
                            const float* prev_moments, float* moments, void* stream) {
    const dim3 block(dev::kTpTileW, dev::kTpTileH);
    const dim3 grid((P.width + dev::kTpTileW - 1) / dev::kTpTileW, (P.height + dev::kTpTileH - 1) / dev::kTpTileH);
    (void)hipGetLastError();
    if (dynamic)
        hipLaunchKernelGGL(dev::temporal_dynamic_moments_kernel, grid, block, 0, (hipStream_t)stream, P,
                           (const float4*)prim_motion, num_prims, (const float2*)prev_moments, (float2*)moments);
    else
        hipLaunchKernelGGL(dev::temporal_moments_kernel, grid, block, 0, (hipStream_t)stream, P,
                           (const float2*)prev_moments, (float2*)moments);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        set_error(std::string("rt_temporal_moments: kernel launch: ") + hipGetErrorString(e));
        return RT_ERR_LAUNCH;
    }
    return RT_OK;
}

}  // namespace rt
