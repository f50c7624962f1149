// adaptive.hip — which pixels of a frame need how many more samples (rt_adaptive_select, include/rt_hip.h).
//
// The pass reads rt_temporal_moments' planes (history length, luminance moments) and writes the list of the pixels whose
// mean is not yet known to the relative standard error asked for, in ascending pixel order, with a sample count each
// (DESIGN.md §18).  The list is what rt_adaptive_samples (render.hip) traces.
//   * The rule (select_k) uses binary32 multiplications, additions and comparisons only, one rounding each
//     (-ffp-contract=off): tests/test_adaptive_host.py select_reference restates it in numpy bit for bit.
//   * The compaction is the multi-launch kind.  Launch 1: workgroup b counts the listed pixels and the samples of its
//     block of pixels into scratch[2b], scratch[2b + 1].  Launch 2: workgroup b sums the counts of the workgroups before
//     it (the scan; at most a few thousand 8-byte loads that hit the L2), evaluates the rule again and writes its pixels at
//     the positions an in-workgroup ballot scan gives them; the last workgroup writes `count`.  No workgroup waits for
//     another, there is no atomic, and every position is a function of the planes alone: the list does not depend on the
//     launch shape or the schedule.
//   * A workgroup is 256 lanes; it covers 256 · pixels_per_lane consecutive pixels, row `it` of them being the 256
//     pixels from base + 256 · it, so a wave reads 64 consecutive elements of each plane and the rows are in pixel order.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "rt_internal.h"

namespace rt {
namespace dev {

constexpr uint32_t kSelBlock = 256;  // lanes per workgroup (four waves)

struct SelectParams {
    const float4* history;
    const float2* moments;
    const int32_t* prim_id;
    uint32_t* pixels;
    uint32_t* samples;
    uint32_t* count;
    uint32_t* scratch;  // (listed pixels, samples) per workgroup
    uint32_t n, capacity, per_lane, max_samples;
    float min_history, tau2, lum_floor;
};

// k(p) of rt_adaptive_select_args: the operations and their order are the header's
__device__ __forceinline__ uint32_t select_k(const SelectParams& P, const uint32_t p) {
    if (P.prim_id && P.prim_id[p] < 0) return 0u;
    const float w = P.history[p].w;
    const float2 mo = P.moments[p];
    const float N = w > 1.0f ? w : 1.0f;
    const float d = mo.y - mo.x * mo.x;
    const float v = d > 0.0f ? d : 0.0f;
    const float m = mo.x > P.lum_floor ? mo.x : P.lum_floor;
    const float T = P.tau2 * (m * m);
    uint32_t k = 0u;
    for (uint32_t j = 0; j < P.max_samples; j++) {
        const float Nj = N + (float)j;
        if (Nj < P.min_history || v > Nj * T) k++;
    }
    return k;
}

// Sum of `v` over the workgroup's 256 lanes, in every lane (`part`: 4 words of LDS; two barriers)
__device__ __forceinline__ uint32_t block_sum(uint32_t v, uint32_t* part) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    __syncthreads();  // (the words' readers of the call before are done)
    if ((threadIdx.x & 63u) == 0u) part[threadIdx.x >> 6] = v;
    __syncthreads();
    return (part[0] + part[1]) + (part[2] + part[3]);
}

__global__ __launch_bounds__(kSelBlock) void adaptive_count_kernel(const SelectParams P) {
    __shared__ uint32_t part[4];
    const uint32_t base = blockIdx.x * (kSelBlock * P.per_lane);  // (the grid covers n: base < n <= 2^31 - 1)
    uint32_t listed = 0u, ksum = 0u;
    for (uint32_t it = 0; it < P.per_lane; it++) {
        const uint32_t off = it * kSelBlock + threadIdx.x;  // (< 4096)
        if (off < P.n - base) {
            const uint32_t k = select_k(P, base + off);
            listed += k != 0u ? 1u : 0u;
            ksum += k;
        }
    }
    listed = block_sum(listed, part);
    ksum = block_sum(ksum, part);
    if (threadIdx.x == 0u) {
        P.scratch[2 * (size_t)blockIdx.x] = listed;
        P.scratch[2 * (size_t)blockIdx.x + 1] = ksum;
    }
}

__global__ __launch_bounds__(kSelBlock) void adaptive_write_kernel(const SelectParams P) {
    __shared__ uint32_t part[4];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    // the scan: listed pixels of the workgroups before this one (the last one also totals the frame)
    const bool last = blockIdx.x == gridDim.x - 1u;
    uint32_t before = 0u, ktotal = 0u;
    for (uint32_t b = threadIdx.x; b < blockIdx.x; b += kSelBlock) before += P.scratch[2 * (size_t)b];
    before = block_sum(before, part);
    if (last) {
        for (uint32_t b = threadIdx.x; b < gridDim.x; b += kSelBlock) ktotal += P.scratch[2 * (size_t)b + 1];
        ktotal = block_sum(ktotal, part);
        if (threadIdx.x == 0u) {
            P.count[0] = before + P.scratch[2 * (size_t)blockIdx.x];
            P.count[1] = ktotal;
        }
    }
    if (before >= P.capacity) return;  // (workgroup-uniform: the list is full before this block's first pixel)
    const uint32_t base = blockIdx.x * (kSelBlock * P.per_lane);
    uint32_t pos = before;  // workgroup-uniform: the list position of the row's first listed pixel
    for (uint32_t it = 0; it < P.per_lane; it++) {
        const uint32_t off = it * kSelBlock + threadIdx.x;
        const uint32_t k = off < P.n - base ? select_k(P, base + off) : 0u;
        const uint64_t m = __ballot(k != 0u);
        const uint32_t below = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
        __syncthreads();  // (the words' readers of the row before are done)
        if (lane == 0u) part[wave] = (uint32_t)__popcll(m);
        __syncthreads();
        uint32_t at = pos + below;
        for (uint32_t w = 0; w < wave; w++) at += part[w];
        if (k != 0u && at < P.capacity) {  // (at < capacity: inside pixels / samples)
            P.pixels[at] = base + off;
            if (P.samples) P.samples[at] = k;
        }
        pos += (part[0] + part[1]) + (part[2] + part[3]);
    }
}

}  // namespace dev
}  // namespace rt

using namespace rt;

extern "C" {

uint64_t rt_adaptive_select_scratch_bytes(uint32_t width, uint32_t height) {
    const uint64_t n = (uint64_t)width * height;
    return (n + dev::kSelBlock - 1) / dev::kSelBlock * 8u;  // (a workgroup covers at least 256 pixels)
}

int rt_adaptive_select(const rt_adaptive_select_args* a, rt_stream stream) {
    // (every argument check runs before the first device call)
    const auto bad = [](const std::string& what) {
        set_error("rt_adaptive_select: " + what);
        return (int)RT_ERR_INVALID_ARGUMENT;
    };
    if (!a) return bad("NULL args");
    if (a->flags != 0) return bad("flags must be 0");
    if (a->reserved[0] != 0 || a->reserved[1] != 0 || a->reserved[2] != 0) return bad("reserved must be 0");
    if (!(a->tau > 0.0f)) return bad("tau must be > 0");
    if (!(a->lum_floor > 0.0f)) return bad("lum_floor must be > 0");
    if (a->min_history > 4096u) return bad("min_history must be 0..4096");
    if (a->max_samples < 1u || a->max_samples > 16u) return bad("max_samples must be 1..16");
    if (a->pixels_per_lane > 16u) return bad("pixels_per_lane above 16");
    if (a->tiling.num_ranks > 1) return bad("the pass works on a whole frame (tiling.num_ranks > 1)");
    if (a->tiling.local_rows != 0 && a->tiling.local_rows != a->height) return bad("tiling.local_rows is not the frame's height");
    const uint64_t n = (uint64_t)a->width * a->height;
    if (n * a->max_samples > 0xffffffffull || n > 0x7fffffffull) return bad("frame too large (width * height * max_samples beyond 32 bits)");
    if (!a->count && n != 0) return bad("NULL count");
    const uint64_t cap = a->capacity;
    const bool listing = n != 0 && cap != 0;
    const uint64_t scratch_bytes = rt_adaptive_select_scratch_bytes(a->width, a->height);
    if (n != 0) {
        if (!a->history) return bad("NULL history");
        if (!a->moments) return bad("NULL moments");
        if (!a->scratch) return bad("NULL scratch");
        if ((uintptr_t)a->scratch % 4u) return bad("scratch must be 4-byte aligned");
    }
    if (listing && !a->pixels) return bad("NULL pixels");
    const char* const in_names[3] = {"history", "moments", "prim_id"};
    const void* const ins[3] = {a->history, a->moments, a->prim_id};
    const uint64_t in_bytes[3] = {n * 16u, n * 8u, n * 4u};
    const char* const out_names[4] = {"pixels", "samples", "count", "scratch"};
    const void* const outs[4] = {a->pixels, a->samples, a->count, a->scratch};
    const uint64_t out_bytes[4] = {n ? cap * 4u : 0u, n ? cap * 4u : 0u, 8u, scratch_bytes};
    for (int o = 0; o < 4; o++) {
        for (int i = 0; i < 3; i++)
            if (overlaps(outs[o], out_bytes[o], ins[i], in_bytes[i]))
                return bad(std::string(out_names[o]) + " overlaps " + in_names[i]);
        for (int p = 0; p < o; p++)
            if (overlaps(outs[o], out_bytes[o], outs[p], out_bytes[p]))
                return bad(std::string(out_names[o]) + " overlaps " + out_names[p]);
    }
    hipStream_t s = (hipStream_t)stream;
    if (n == 0) {  // an empty frame lists nothing: count = (0, 0), the call's one device call (none without count)
        if (!a->count) return RT_OK;
        const hipError_t e = hipMemsetAsync(a->count, 0, 8, s);
        if (e != hipSuccess) {
            set_error(std::string("rt_adaptive_select: clearing count: ") + hipGetErrorString(e));
            return RT_ERR_DEVICE;
        }
        return RT_OK;
    }
    dev::SelectParams P;
    P.history = (const float4*)a->history;
    P.moments = (const float2*)a->moments;
    P.prim_id = a->prim_id;
    P.pixels = a->pixels;
    P.samples = a->samples;
    P.count = a->count;
    P.scratch = (uint32_t*)a->scratch;
    P.n = (uint32_t)n;
    P.capacity = a->capacity;  // (0: the write launch stores count alone)
    P.per_lane = a->pixels_per_lane ? a->pixels_per_lane : 4u;
    P.max_samples = a->max_samples;
    P.min_history = (float)a->min_history;
    P.tau2 = a->tau * a->tau;
    P.lum_floor = a->lum_floor;
    const uint32_t per_group = dev::kSelBlock * P.per_lane;
    const uint32_t grid = (uint32_t)((n + per_group - 1) / per_group);
    (void)hipGetLastError();
    hipLaunchKernelGGL(dev::adaptive_count_kernel, dim3(grid), dim3(dev::kSelBlock), 0, s, P);
    hipLaunchKernelGGL(dev::adaptive_write_kernel, dim3(grid), dim3(dev::kSelBlock), 0, s, P);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        set_error(std::string("rt_adaptive_select: kernel launch: ") + hipGetErrorString(e));
        return RT_ERR_LAUNCH;
    }
    return RT_OK;
}

}  // extern "C"
