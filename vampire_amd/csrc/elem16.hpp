// The 16-bit element conversions of the layer and task-head kernels: bf16 and IEEE half, as bit patterns, to and from
// fp32.  Host and device, so that a host program can run them over every bit pattern.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace vamp {

__host__ __device__ __forceinline__ float bf16_to_f32(uint16_t u) {
  return __builtin_bit_cast(float, (uint32_t) u << 16);
}

// four packed bf16 (element 0 in the low half of .x) -> fp32
__host__ __device__ __forceinline__ float4 bf16x4_to_f32(uint2 u) {
  return make_float4(__builtin_bit_cast(float, u.x << 16), __builtin_bit_cast(float, u.x & 0xffff0000u),
                     __builtin_bit_cast(float, u.y << 16), __builtin_bit_cast(float, u.y & 0xffff0000u));
}

// fp32 -> bf16, round to nearest even; a NaN keeps its sign and upper payload and gets the quiet bit
__host__ __device__ __forceinline__ uint16_t f32_to_bf16(float f) {
  uint32_t u = __builtin_bit_cast(uint32_t, f);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t) ((u >> 16) | 0x40u);
  u += 0x7fffu + ((u >> 16) & 1u);
  return (uint16_t) (u >> 16);
}

// the same with c10's NaN rule: every NaN becomes the canonical 0x7fc0
__host__ __device__ __forceinline__ uint16_t f32_to_bf16_c10(float f) {
  const uint32_t u = __builtin_bit_cast(uint32_t, f);
  if (f != f) return 0x7fc0;
  return (uint16_t) ((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}

__host__ __device__ __forceinline__ float f16_to_f32(uint16_t u) { return (float) __builtin_bit_cast(_Float16, u); }

// fp32 -> IEEE half, round to nearest even
__host__ __device__ __forceinline__ uint16_t f32_to_f16(float f) { return __builtin_bit_cast(uint16_t, (_Float16) f); }

// fp32 -> the 16-bit element type of a kernel instantiated for bf16 or (F16) IEEE half
template <bool F16>
__host__ __device__ __forceinline__ uint16_t f32_to_e16(float f) {
  if constexpr (F16) return f32_to_f16(f);
  else return f32_to_bf16(f);
}

}  // namespace vamp
