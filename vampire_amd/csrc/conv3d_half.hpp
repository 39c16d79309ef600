// What the 16-bit 3x3x3 convolutions share (conv3d_bf16.hip: stride 1, conv3d_bf16_s2.hip: stride 2): the register
// vector types, the matrix-core product on bf16 or IEEE half operands, the staged box (the stride-2 kernels'; the
// stride-1 forward keeps it written out), the tile decode, the plain tile store, the weight gradients' partial store and
// second launch (the fixed-order sum of the workgroups' partials); on the host the channel tile and shape rule, the entry points' argument check and dispatch, the workspace
// size and the launcher of the kernels with dynamic LDS.
#pragma once
#include "common.hpp"
#include "elem16.hpp"       // f32_to_e16: the fp32 -> 16-bit rounding of the stores

#include <type_traits>

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

// A persistent tile's coordinates: tiles run x fastest, then y, then the nz planes of a sample, then the batch
struct TileIx {
  int tx, ty, z, b;
};
__device__ __forceinline__ TileIx tile_ix(long tile, int tiles_x, int tiles_y, int nz) {
  TileIx t;
  t.tx = (int) (tile % tiles_x);
  long r = tile / tiles_x;
  t.ty = (int) (r % tiles_y);
  r /= tiles_y;
  t.z = (int) (r % nz);
  t.b = (int) (r / nz);
  return t;
}

// The staged box: NZ x NY rows of HX voxels (HX even) from (z0, y0, x0), x0 even, of a [ch, Zt, Yt, Xt] sample
// (Xt even), in LDS CHANNEL-INNER at VS bytes per voxel.  Item = (row, x pair, 8-channel group): eight dword loads
// through a buffer descriptor (planes beyond the real count and voxels outside the volume read 0), v_perm into the two
// voxels' 16-byte channel vectors, two 16-byte LDS stores.  `fetch` fills registers only, so that the next tile's
// loads fly during the MFMAs; `commit` writes them.
// A voxel takes 2 KC + 16 bytes (padded: bank spread): the pitch of consecutive voxels is then 3 (KC 16) or 5 (KC 32)
// 16-byte slots, and at the stride-2 forward's two-voxel pitch 6 or 10, == 2 mod 4, so the 8 lanes of a ds_read_b128
// group that share a k-chunk fall on 8 different even slots and the other 8 on the odd ones.
template <int KC, int NZ, int NY, int HX>
struct Box {
  static constexpr int CG = KC / 8, VS = KC * 2 + 16, ROWS = NZ * NY;
  static constexpr int NITEM = ROWS * (HX / 2) * CG, NI = (NITEM + 255) / 256;
  static constexpr size_t bytes = (size_t) ROWS * HX * VS;

  static __device__ __forceinline__ void fetch(unsigned (&st)[NI][8], const unsigned short* sample, int ch, int Zt,
                                               int Yt, int Xt, int z0, int y0, int x0, int tid) {
    const long plane = (long) Zt * Yt * Xt;
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<unsigned short*>(sample), 0, (int) ((size_t) ch * plane * 2), 0x00020000);   // planes >= ch read 0
#pragma unroll
    for (int i = 0; i < NI; ++i) {
      const int it = tid + i * 256;
      const int px = it % (HX / 2), rr = (it / (HX / 2)) % ROWS, cg = it / ((HX / 2) * ROWS);
      const int zz = z0 + rr / NY, yy = y0 + rr % NY, xx = x0 + 2 * px;
      const bool ok = it < NITEM && zz >= 0 && zz < Zt && yy >= 0 && yy < Yt && xx >= 0 && xx < Xt;
      const unsigned voff = ok ? (unsigned) ((((long) cg * 8 * Zt + zz) * Yt + yy) * Xt + xx) * 2u : 0xfffffff0u;
#pragma unroll
      for (int j = 0; j < 8; ++j) st[i][j] = __builtin_amdgcn_raw_buffer_load_b32(rs, voff, (unsigned) (j * plane * 2), 0);
    }
  }

  static __device__ __forceinline__ void commit(const unsigned (&st)[NI][8], unsigned char* in_s, int tid) {
#pragma unroll
    for (int i = 0; i < NI; ++i) {
      const int it = tid + i * 256;
      if (it < NITEM) {
        const int px = it % (HX / 2), rr = (it / (HX / 2)) % ROWS, cg = it / ((HX / 2) * ROWS);
        u32x4 lo, hi;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          lo[q] = __builtin_amdgcn_perm(st[i][2 * q + 1], st[i][2 * q], 0x05040100u);   // the even-x voxel: low halves
          hi[q] = __builtin_amdgcn_perm(st[i][2 * q + 1], st[i][2 * q], 0x07060302u);   // the odd-x voxel: high halves
        }
        unsigned char* p = in_s + ((size_t) rr * HX + 2 * px) * VS + cg * 16;
        *reinterpret_cast<u32x4*>(p) = lo;
        *reinterpret_cast<u32x4*>(p + VS) = hi;
      }
    }
  }
};

// The plain store of a forward tile: acc[m][n] is the D fragment of M tile m (row = channel 16 m + 4 kg + reg) and
// N tile n (column = voxel x0 + 16 n + li) of the row at `ob` ([cout] planes of `plane` elements, X voxels long)
template <bool F16, int MT, int NN>
__device__ __forceinline__ void store_tile16(const f32x4 (&acc)[MT][NN], unsigned short* ob, long plane, int x0, int X,
                                             int cout, int kg, int li) {
#pragma unroll
  for (int m = 0; m < MT; ++m)
#pragma unroll
    for (int n = 0; n < NN; ++n) {
      const int x = x0 + n * 16 + li;
      if (x < X) {
#pragma unroll
        for (int rg = 0; rg < 4; ++rg)
          if (m * 16 + 4 * kg + rg < cout) ob[(long) (m * 16 + 4 * kg + rg) * plane + x] = f32_to_e16<F16>(acc[m][n][rg]);
      }
    }
}

// The weight gradients' partial sums: part[workgroup][tap][co][ci], wave wv holds the taps 9 wv .. 9 wv + 8; D row
// (co) = 4 kg + reg, column (ci) = li
template <int CIN, int COUT>
__device__ __forceinline__ void store_wgrad_partials(const f32x4 (&acc)[9][COUT / 16][CIN / 16], float* part, int wv,
                                                     int kg, int li) {
  float* pb = part + (size_t) blockIdx.x * 27 * COUT * CIN;
#pragma unroll
  for (int t = 0; t < 9; ++t) {
    const int tap = wv * 9 + t;
#pragma unroll
    for (int m = 0; m < COUT / 16; ++m)
#pragma unroll
      for (int n = 0; n < CIN / 16; ++n)
#pragma unroll
        for (int rg = 0; rg < 4; ++rg) pb[((size_t) tap * COUT + m * 16 + 4 * kg + rg) * CIN + n * 16 + li] = acc[t][m][n][rg];
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

// ---------------------------------------------------------------------------
// host side of the entry points
// ---------------------------------------------------------------------------
// What every 16-bit entry point asks of its arguments, in this order; `supported` names the file's shape rule for the
// message, `tensors`: none of the entry point's tensors is NULL
int half_args_ok(const char* func, const char* supported, const VampConvDesc* d, int32_t dtype, bool tensors) {
  if (!bf16_shape_ok(d)) {
    snprintf(g_err, sizeof(g_err), "%s: requirement failed: unsupported shape: see %s", func, supported);
    return VAMP_EINVAL;
  }
  if (!tensors) return fail(VAMP_EINVAL, "%s: requirement failed: NULL tensor", func);
  if (dtype != VAMP_BF16 && dtype != VAMP_F16)
    return fail(VAMP_EINVAL, "%s: requirement failed: dtype must be VAMP_BF16 or VAMP_F16", func);
  return VAMP_OK;
}

// the weight gradients' workspace: kWgradWgs partial sums [27][cout tile][cin tile] fp32
size_t half_workspace_bytes(const VampConvDesc* d) {
  if (!bf16_shape_ok(d)) return 0;
  return (size_t) kWgradWgs * 27 * tile_ch(d->cin) * tile_ch(d->cout) * sizeof(float);
}

// f(CI, CO, F16) with the channel tiles of the real counts ci / co and the dtype as compile-time constants
template <class F>
int dispatch_half(int ci, int co, int32_t dtype, F&& f) {
  return dispatch_tiles(tile_ch(ci), tile_ch(co), [&](auto CI, auto CO) {
    return dtype == VAMP_F16 ? f(CI, CO, std::true_type()) : f(CI, CO, std::false_type());
  });
}

// One launch of a 256-thread kernel with `lds` bytes of dynamic LDS (raised before every launch) under profile `slot`
template <class K, class... Args>
int launch_lds(K kernel, const char* name, size_t lds, unsigned grid, int slot, hipStream_t s, Args... args) {
  if (hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int) lds) != hipSuccess)
    return fail(VAMP_EHIP, "%s: cannot raise dynamic LDS", name);
  VAMP_TIMED(slot, s, (kernel<<<grid, 256, lds, s>>>(args...)));
  return check_launch(name);
}

}  // namespace
}  // namespace vamp
