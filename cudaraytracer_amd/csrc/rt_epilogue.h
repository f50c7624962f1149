// rt_epilogue.h — the reference's RGBA8 pack (RgbToInt, Kernel.cu:12-19) as device code shared by the render kernels
// (render.hip) and the denoiser's last launch (denoise.hip).  Include after <hip/hip_runtime.h>.
#pragma once

#include <cstdint>

namespace rt {
namespace dev {

__device__ __forceinline__ float clampf(float x, float a, float b) { return (x < a) ? a : ((x > b) ? b : x); }

__device__ __forceinline__ uint32_t f2u8(float f) { return f != f ? 0u : (uint32_t)(int)f; }

// RgbToInt (Kernel.cu:12-19)
__device__ __forceinline__ uint32_t rgb_to_int(float r, float g, float b) {
    r = clampf(r, 0.0f, 255.0f);
    g = clampf(g, 0.0f, 255.0f);
    b = clampf(b, 0.0f, 255.0f);
    return (255u << 24) | (f2u8(b) << 16) | (f2u8(g) << 8) | f2u8(r);
}

}  // namespace dev
}  // namespace rt
