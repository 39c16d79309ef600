// What the 16-bit 3x3x3 convolutions share (conv3d_bf16.hip: stride 1, conv3d_bf16_s2.hip: stride 2): the register
// vector types, the matrix-core product on bf16 or IEEE half operands, the channel tile and shape rule, and the second
// launch of the weight gradient (the fixed-order sum of the workgroups' partials).
#pragma once
#include "common.hpp"
#include "elem16.hpp"       // f32_to_e16: the fp32 -> 16-bit rounding of the stores

namespace vamp {
namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef short bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef u32x4 __attribute__((aligned(2))) u32x4_u;     // a 16-byte global load at 2-byte alignment
typedef bf16x8 __attribute__((aligned(2))) bf16x8_u;

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

// the 16-bit matrix-core product: bf16 or (F16) IEEE half operands, fp32 accumulate; same fragment maps
template <bool F16>
__device__ __forceinline__ f32x4 mfma16(const bf16x8& a, const bf16x8& b, const f32x4& c) {
  if constexpr (F16) {
    f16x8 ha, hb;
    __builtin_memcpy(&ha, &a, 16);
    __builtin_memcpy(&hb, &b, 16);
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(ha, hb, c, 0, 0, 0);
  } else {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
  }
}

// dw[co][ci][tap] (bf16 or fp32 out) = sum over workgroups of part[wg][tap][co][ci]
__global__ void __launch_bounds__(256)
conv3d_bf16_wreduce_kernel(const float* __restrict__ part, float* __restrict__ dw, int cin, int cout, int nwg,
                           int cin_r, int cout_r) {
  const int e = blockIdx.x * 64 + (threadIdx.x & 63), wv = threadIdx.x >> 6;
  __shared__ float red[4][64];
  const int n = 27 * cout * cin;
  float s = 0.f;
  if (e < n) {
    int g = wv;
    for (; g + 28 < nwg; g += 32) {
      float v[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) v[i] = part[(size_t) (g + 4 * i) * n + e];
#pragma unroll
      for (int i = 0; i < 8; ++i) s += v[i];
    }
    for (; g < nwg; g += 4) s += part[(size_t) g * n + e];
  }
  red[wv][threadIdx.x & 63] = s;
  __syncthreads();
  if (wv == 0 && e < n) {
    s = (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
    const int ci = e % cin, co = (e / cin) % cout, tap = e / (cin * cout);
    if (co < cout_r && ci < cin_r) dw[((size_t) co * cin_r + ci) * 27 + tap] = s;
  }
}

constexpr int kWgradWgs = 512;       // two workgroups per CU

int tile_ch(int c) { return c <= 16 ? 16 : 32; }       // channel tile a real channel count runs under

bool bf16_shape_ok(const VampConvDesc* d) {
  return d && d->cin >= 1 && d->cin <= 32 && d->cout >= 1 && d->cout <= 32 && d->B > 0 && d->Z > 0 &&
         d->Y > 0 && d->X >= 8 && d->X % 4 == 0 &&
         (long) d->Z * d->Y * d->X * 32 * 2 < 0x7fffffffL;
}

}  // namespace
}  // namespace vamp
