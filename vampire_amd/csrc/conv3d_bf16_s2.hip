// 3x3x3 / stride 2 / pad 1 Conv3d of the UNet under a 16-bit autocast (Hourglass3D.conv1 / conv3,
// base_vampire2.py:34-46), gfx950: bf16 or IEEE half in, fp32 accumulate on v_mfma_f32_16x16x32_{bf16,f16}, 16-bit
// out; NCDHW tensors, weight [cout, cin, 3, 3, 3].  Output sizes Zo = (Z - 1) / 2 + 1, likewise Yo, Xo.
//
// Forward and data gradient stage a box of their input tensor in LDS CHANNEL-INNER like the stride-1 kernel
// (conv3d_bf16.hip): x-pairs of 8 channel planes through a buffer descriptor (planes beyond the real count and voxels
// outside the volume read 0), v_perm into the two voxels' 16-byte channel vectors, ds_write_b128.  The weights lie in
// LDS as [28 taps][M rows][K channels], tap 27 all zero: with 32 K-channels an MFMA k-step is one tap, with 16 it is
// two taps (lanes 32..63 take the second), and a tap without a partner pairs with tap 27.
//
//   forward:  out[co, vo] = sum w[co, ci, t] in[ci, 2 vo + t - 1].  A tile is 1 zo x TY yo x 32 xo -> a box of
//     3 x (2 TY + 1) x 66 voxels; the B fragment is read at a two-voxel pitch.  A voxel takes 2 cin + 16 bytes: the
//     pitch of 16 consecutive lanes is then 6 (cin 16) or 10 (cin 32) 16-byte slots, == 2 mod 4, so the 8 lanes of a
//     ds_read_b128 group that share a k-chunk fall on 8 different even slots and the other 8 on the odd ones.
//     cin 16: TY = 4, a wave owns a row and its two 16-voxel N tiles; cin 32: TY = 2 (the box and the weight image
//     must share 160 KiB), a wave owns a row and ONE of the two N tiles.  The N-tile count stays a compile-time
//     constant of the MFMA loop.
//   data gradient: a gather over grad_out.  z = 2 zo + dz - 1: an even z is reached through dz = 1 from z / 2, an odd
//     one through dz = 0 from (z + 1) / 2 and dz = 2 from (z - 1) / 2; likewise y and x: the parity classes of
//     (z, y, x) have 1 .. 8 taps.  A tile is 1 z x 4 y x 64 x; the z and y tap lists are wave-uniform run-time loops
//     (1 or 2 entries), the x parity is a compile-time property of the N tile: N tile e_j holds the 16 even x
//     x0 + 32 j + 2 i, o_j the 16 odd ones, so lane i ends with both x of a pair and stores them as one dword --
//     every element of grad_in is written exactly once, no atomics.
//   weight gradient: dw[co, ci, t] = sum_vo dout[co, vo] in[ci, 2 vo + t - 1], K = 32 xo of one output row per
//     MFMA.  A = 8 xo of dout; B: the aligned window of 16 input x, split by v_perm into the even-x stream (dx = 1)
//     and the odd-x stream (dx = 2); the odd stream shifted by one element (v_alignbit, the neighbouring lane
//     group's last dword through ds_bpermute) is dx = 0.  No LDS.  Rows of dout are only 4-byte aligned when
//     Xo % 4 == 2: the windows are loaded in naturally aligned pieces (16 / 8 / 4 bytes for dout, 16 / 16 / 8 for
//     the input), chosen by X % 16, X % 8, X % 4.  Per-workgroup partials, then the fixed-order reduce of the
//     stride-1 kernel: bitwise repeatable.
#include "conv3d_epilogue.hpp"   // the EPI instantiations' store
#include "conv3d_half.hpp"

#include <algorithm>
#include <type_traits>

namespace vamp {
namespace {

struct S2P {
  int B, Z, Y, X;          // the layer's input volume
  int Zo, Yo, Xo;          // its output volume
  int cin, cout;           // real channel counts of the layer
};

S2P make_params(const VampConvDesc* d) {
  return S2P{d->B, d->Z, d->Y, d->X, (d->Z - 1) / 2 + 1, (d->Y - 1) / 2 + 1, (d->X - 1) / 2 + 1, d->cin, d->cout};
}

constexpr char kShapeRule[] = "vamp_conv3d_half_s2_supported";      // where a refused shape's message points

constexpr int kFwdTX = 32;        // output x per forward tile (two 16-voxel N tiles)
constexpr int kFwdHX = 66;        // staged x: 2 xo0 - 2 .. 2 xo0 + 63 (pairs at even x)
constexpr int kDgTY = 4;          // grad_in rows per tile = waves per workgroup
constexpr int kDgTX = 64;         // grad_in x per tile: N tiles e0, o0, e1, o1
constexpr int kDgHX = 34;         // staged xo: x0 / 2 .. x0 / 2 + 33
constexpr int kFwdWgs = 256;      // persistent grids: the forward's LDS (98 .. 133 KiB) leaves one workgroup per CU,
constexpr int kDgWgs = 512;       // the data gradient's (23 .. 72 KiB) two

// weight image w_s[tap][m][k]; TR = false (forward): m = co, k = ci; TR = true (data gradient): m = ci, k = co
template <int KC, int M, bool TR>
__device__ __forceinline__ void load_wimage(unsigned char* w_s, const unsigned short* __restrict__ w, int cin, int cout,
                                            int tid) {
  static_assert(28 * M * KC % 256 == 0, "whole passes of the workgroup");
#pragma unroll 8                       // eight independent 2-byte loads in flight per thread
  for (int i = 0; i < 28 * M * KC / 256; ++i) {
    const int e = tid + i * 256;
    const int k = e % KC, m = (e / KC) % M, tap = e / (KC * M);
    const int co = TR ? k : m, ci = TR ? m : k;
    unsigned short v = 0;
    if (tap < 27 && ci < cin && co < cout) v = w[((long) co * cin + ci) * 27 + tap];
    reinterpret_cast<unsigned short*>(w_s)[e] = v;
  }
}

// this lane's 16 bytes of the A fragment (weights of `tap`, row `row`) / of the B fragment (staged voxel `vox`):
// 32 K-channels: chunk kg of the one tap; 16: chunk kg & 1 of the tap that kg >> 1 selected
template <int KC>
__device__ __forceinline__ bf16x8 frag_a(const unsigned char* w_s, int M, int tap, int row, int kg) {
  return *reinterpret_cast<const bf16x8*>(w_s + ((size_t) (tap * M + row) * KC * 2 + (KC == 16 ? (kg & 1) : kg) * 16));
}
template <int KC>
__device__ __forceinline__ bf16x8 frag_b(const unsigned char* in_s, int vox, int kg) {
  return *reinterpret_cast<const bf16x8*>(in_s + ((size_t) vox * (KC * 2 + 16) + (KC == 16 ? (kg & 1) : kg) * 16));
}

// ---------------------------------------------------------------------------
// forward
// ---------------------------------------------------------------------------
template <int CIN>
struct FwdTile {
  static constexpr int TY = CIN == 16 ? 4 : 2;          // output rows per tile
  static constexpr int NNW = CIN == 16 ? 2 : 1;         // N tiles per wave
  static constexpr int NY = 2 * TY + 1;
};

template <int CIN, int COUT>
struct FwdLds {
  using B = Box<CIN, 3, FwdTile<CIN>::NY, kFwdHX>;
  static constexpr size_t w_bytes = (size_t) 28 * COUT * CIN * 2;
  static constexpr size_t bytes = w_bytes + B::bytes;
};

// EPI: the accumulators go through the epilogue `ep` (conv3d_epilogue.hpp) into its segments' tensors instead of `out`
template <int CIN, int COUT, bool F16, bool EPI, bool OF32 = false>
__device__ __forceinline__ void conv3d_s2_fwd_body(const S2P& P, const unsigned short* __restrict__ in,
                                                   const unsigned short* __restrict__ w,
                                                   unsigned short* __restrict__ out, int tiles_x, int tiles_y,
                                                   long ntiles, const VampConvEpilogue* ep) {
  using T = FwdTile<CIN>;
  using L = FwdLds<CIN, COUT>;
  using BX = typename L::B;
  constexpr int MT = COUT / 16, TY = T::TY, NNW = T::NNW, NY = T::NY, HX = kFwdHX;
  constexpr int NTP = CIN == 16 ? 14 : 27;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  unsigned char* w_s = smem;
  unsigned char* in_s = smem + L::w_bytes;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int li = lane & 15, kg = lane >> 4;
  const long plane_i = (long) P.Z * P.Y * P.X, plane_o = (long) P.Zo * P.Yo * P.Xo;

  load_wimage<CIN, COUT, false>(w_s, w, P.cin, P.cout, tid);

  unsigned st[BX::NI][8];
  auto fetch = [&](long tile) {
    const TileIx t = tile_ix(tile, tiles_x, tiles_y, P.Zo);
    BX::fetch(st, in + (long) t.b * P.cin * plane_i, P.cin, P.Z, P.Y, P.X, 2 * t.z - 1, 2 * t.ty * TY - 1, 2 * t.tx * kFwdTX - 2, tid);
  };

  // this wave's row of the tile and its first N tile
  const int wr = CIN == 16 ? wv : wv >> 1, n0 = CIN == 16 ? 0 : (wv & 1);

  long tile = blockIdx.x;
  if (tile < ntiles) fetch(tile);
  for (; tile < ntiles; tile += gridDim.x) {
    __syncthreads();                           // the previous tile's readers (and the weight image)
    BX::commit(st, in_s, tid);
    __syncthreads();
    if (tile + gridDim.x < ntiles) fetch(tile + gridDim.x);

    const TileIx t = tile_ix(tile, tiles_x, tiles_y, P.Zo);
    const int zo = t.z, b = t.b, yo = t.ty * TY + wr, xo0 = t.tx * kFwdTX + n0 * 16;
    const int nnt = max(0, min(NNW, (P.Xo - xo0 + 15) / 16));       // N tiles of this wave inside the volume (uniform)
    f32x4 acc[MT][NNW];
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
      for (int n = 0; n < NNW; ++n) acc[m][n] = f32x4{0.f, 0.f, 0.f, 0.f};
    // NN = N tiles computed, a compile-time count: no branch between the LDS reads and the MFMAs of a k-step
    auto run = [&](auto nn_tag) {
      constexpr int NN = decltype(nn_tag)::value;
      // staged voxel of (row wr, xo0 + 16 n + li) at tap (0, 0, 0): x index 2 (xo - tile xo0) + dx + 1
      const int vbase = (2 * wr) * HX + 2 * (n0 * 16 + li) + 1;
#pragma unroll
      for (int tp = 0; tp < NTP; ++tp) {
        int tap, voff;
        if (CIN == 16) {
          const int t0 = 2 * tp, t1 = 2 * tp + 1;               // t1 = 27: the zero tap, read at t0's voxel
          const int o0 = ((t0 / 9) * NY + (t0 / 3) % 3) * HX + t0 % 3;
          const int o1 = t1 < 27 ? ((t1 / 9) * NY + (t1 / 3) % 3) * HX + t1 % 3 : o0;
          tap = (kg >> 1) ? t1 : t0;
          voff = (kg >> 1) ? o1 : o0;
        } else {
          tap = tp;
          voff = ((tp / 9) * NY + (tp / 3) % 3) * HX + tp % 3;
        }
        bf16x8 a[MT], bv[NN];
#pragma unroll
        for (int m = 0; m < MT; ++m) a[m] = frag_a<CIN>(w_s, COUT, tap, m * 16 + li, kg);
#pragma unroll
        for (int n = 0; n < NN; ++n) bv[n] = frag_b<CIN>(in_s, vbase + 32 * n + voff, kg);
#pragma unroll
        for (int n = 0; n < NN; ++n)
#pragma unroll
          for (int m = 0; m < MT; ++m) acc[m][n] = mfma16<F16>(a[m], bv[n], acc[m][n]);
      }
    };
    if (nnt == 2) {
      if constexpr (NNW == 2) run(std::integral_constant<int, 2>());
    } else if (nnt == 1) {
      run(std::integral_constant<int, 1>());
    }
    if constexpr (EPI) {
      if (yo < P.Yo)
        epi_store_tile<F16 ? kEpiF16 : kEpiBF16, OF32, MT, NNW>(*ep, acc, kg, li, b, plane_o, ((long) zo * P.Yo + yo) * P.Xo, xo0,
                                                               P.Xo, w);
    } else if (yo < P.Yo) {
      store_tile16<F16, MT, NNW>(acc, out + (long) b * P.cout * plane_o + ((long) zo * P.Yo + yo) * P.Xo, plane_o, xo0, P.Xo,
                                 P.cout, kg, li);
    }
  }
}

template <int CIN, int COUT, bool F16>
__global__ void __launch_bounds__(256)
conv3d_s2_fwd_kernel(S2P P, const unsigned short* __restrict__ in, const unsigned short* __restrict__ w,
                     unsigned short* __restrict__ out, int tiles_x, int tiles_y, long ntiles) {
  conv3d_s2_fwd_body<CIN, COUT, F16, false>(P, in, w, out, tiles_x, tiles_y, ntiles, nullptr);
}

// the forward with the epilogue: the same tiles, the segments' tensors instead of `out`
template <int CIN, int COUT, bool F16, bool OF32>
__global__ void __launch_bounds__(256)
conv3d_s2_fwd_epi_kernel(S2P P, const unsigned short* __restrict__ in, const unsigned short* __restrict__ w,
                         VampConvEpilogue ep, int tiles_x, int tiles_y, long ntiles) {
  conv3d_s2_fwd_body<CIN, COUT, F16, true, OF32>(P, in, w, nullptr, tiles_x, tiles_y, ntiles, &ep);
}

// ---------------------------------------------------------------------------
// data gradient: CO = the K-channel tile (grad_out's channels), CI = the M tile (grad_in's channels)
// ---------------------------------------------------------------------------
template <int CO, int CI>
struct DgLds {
  using B = Box<CO, 2, kDgTY / 2 + 1, kDgHX>;
  static constexpr size_t w_bytes = (size_t) 28 * CI * CO * 2;
  static constexpr size_t bytes = w_bytes + B::bytes;
};

template <int CO, int CI, bool F16>
__global__ void __launch_bounds__(256)
conv3d_s2_dgrad_kernel(S2P P, const unsigned short* __restrict__ gout, const unsigned short* __restrict__ w,
                       unsigned short* __restrict__ gin, int tiles_x, int tiles_y, long ntiles) {
  using L = DgLds<CO, CI>;
  using BX = typename L::B;
  constexpr int MT = CI / 16, NY = kDgTY / 2 + 1, HX = kDgHX;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  unsigned char* w_s = smem;
  unsigned char* in_s = smem + L::w_bytes;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int li = lane & 15, kg = lane >> 4;
  const long plane_i = (long) P.Z * P.Y * P.X, plane_o = (long) P.Zo * P.Yo * P.Xo;

  load_wimage<CO, CI, true>(w_s, w, P.cin, P.cout, tid);

  unsigned st[BX::NI][8];
  auto fetch = [&](long tile) {
    const TileIx t = tile_ix(tile, tiles_x, tiles_y, P.Z);
    BX::fetch(st, gout + (long) t.b * P.cout * plane_o, P.cout, P.Zo, P.Yo, P.Xo, t.z >> 1, t.ty * (kDgTY / 2), t.tx * (kDgTX / 2), tid);
  };

  long tile = blockIdx.x;
  if (tile < ntiles) fetch(tile);
  for (; tile < ntiles; tile += gridDim.x) {
    __syncthreads();
    BX::commit(st, in_s, tid);
    __syncthreads();
    if (tile + gridDim.x < ntiles) fetch(tile + gridDim.x);

    const TileIx t = tile_ix(tile, tiles_x, tiles_y, P.Z);
    const int z = t.z, b = t.b, y = t.ty * kDgTY + wv, x0 = t.tx * kDgTX;
    const int npair = min(2, (P.X - x0 + 31) / 32);         // (even, odd) N-tile pairs inside the volume (uniform)
    // the z and y tap lists of this wave's row: (tap index, staged plane / row); an even coordinate has the one tap
    // d = 1 from c / 2, an odd one d = 0 from (c + 1) / 2 and d = 2 from (c - 1) / 2
    const int nz = 1 + (z & 1), ny = 1 + (wv & 1);
    f32x4 acce[MT][2], acco[MT][2];
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
      for (int j = 0; j < 2; ++j) acce[m][j] = acco[m][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    auto run = [&](auto np_tag) {
      constexpr int NP = decltype(np_tag)::value;
      for (int iz = 0; iz < nz; ++iz) {
        const int dz = (z & 1) ? 2 * iz : 1, zp = (z & 1) ? 1 - iz : 0;
        for (int iy = 0; iy < ny; ++iy) {
          const int dy = (wv & 1) ? 2 * iy : 1, yr = (wv & 1) ? (iy ? (wv - 1) / 2 : (wv + 1) / 2) : wv / 2;
          const int tb = dz * 9 + dy * 3, vrow = (zp * NY + yr) * HX;
          if constexpr (CO == 32) {
            bf16x8 a0[MT], a1[MT], a2[MT], lo[NP], hi[NP];
#pragma unroll
            for (int m = 0; m < MT; ++m) {
              a0[m] = frag_a<CO>(w_s, CI, tb + 0, m * 16 + li, kg);
              a1[m] = frag_a<CO>(w_s, CI, tb + 1, m * 16 + li, kg);
              a2[m] = frag_a<CO>(w_s, CI, tb + 2, m * 16 + li, kg);
            }
#pragma unroll
            for (int j = 0; j < NP; ++j) {
              lo[j] = frag_b<CO>(in_s, vrow + 16 * j + li, kg);            // xo = x0 / 2 + 16 j + li
              hi[j] = frag_b<CO>(in_s, vrow + 16 * j + li + 1, kg);
            }
#pragma unroll
            for (int j = 0; j < NP; ++j)
#pragma unroll
              for (int m = 0; m < MT; ++m) {
                acce[m][j] = mfma16<F16>(a1[m], lo[j], acce[m][j]);         // x even: dx = 1 from x / 2
                acco[m][j] = mfma16<F16>(a0[m], hi[j], acco[m][j]);         // x odd: dx = 0 from (x + 1) / 2
                acco[m][j] = mfma16<F16>(a2[m], lo[j], acco[m][j]);         //        dx = 2 from (x - 1) / 2
              }
          } else {
            // two taps per MFMA: even x pairs dx = 1 with the zero tap, odd x pairs dx = 0 with dx = 2
            const int sel = kg >> 1;
            bf16x8 ae[MT], ao[MT], be[NP], bo[NP];
#pragma unroll
            for (int m = 0; m < MT; ++m) {
              ae[m] = frag_a<CO>(w_s, CI, sel ? 27 : tb + 1, m * 16 + li, kg);
              ao[m] = frag_a<CO>(w_s, CI, sel ? tb + 2 : tb + 0, m * 16 + li, kg);
            }
#pragma unroll
            for (int j = 0; j < NP; ++j) {
              be[j] = frag_b<CO>(in_s, vrow + 16 * j + li, kg);
              bo[j] = frag_b<CO>(in_s, vrow + 16 * j + li + (sel ? 0 : 1), kg);
            }
#pragma unroll
            for (int j = 0; j < NP; ++j)
#pragma unroll
              for (int m = 0; m < MT; ++m) {
                acce[m][j] = mfma16<F16>(ae[m], be[j], acce[m][j]);
                acco[m][j] = mfma16<F16>(ao[m], bo[j], acco[m][j]);
              }
          }
        }
      }
    };
    if (npair == 2) run(std::integral_constant<int, 2>());
    else run(std::integral_constant<int, 1>());
    if (y < P.Y) {
      unsigned short* ob = gin + (long) b * P.cin * plane_i + ((long) z * P.Y + y) * P.X;
#pragma unroll
      for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          const int x = x0 + 32 * j + 2 * li;                   // even; X is even, so x + 1 is inside with it
          if (x < P.X) {
#pragma unroll
            for (int rg = 0; rg < 4; ++rg)
              if (m * 16 + 4 * kg + rg < P.cin)
                *reinterpret_cast<unsigned*>(ob + (long) (m * 16 + 4 * kg + rg) * plane_i + x) =
                    (unsigned) f32_to_e16<F16>(acce[m][j][rg]) | ((unsigned) f32_to_e16<F16>(acco[m][j][rg]) << 16);
          }
        }
    }
  }
}

// ---------------------------------------------------------------------------
// weight gradient.  M = co, N = ci, K = 32 consecutive xo of one (b, zo, yo) output row per MFMA.  Wave = dz, nine
// accumulator sets (dy, dx); per-workgroup partials [27][cout][cin].
// AL = bytes of the naturally aligned pieces a dout window is loaded in (16: X % 16 == 0, 8: X % 8 == 0, 4: else);
// the input window (16 elements) comes in pieces of min(2 AL, 16) bytes.
// ---------------------------------------------------------------------------
template <int BYTES>
__device__ __forceinline__ void load_piece(const unsigned short* p, unsigned* dst) {
  if constexpr (BYTES == 16) {
    const u32x4 t = *reinterpret_cast<const u32x4*>(p);
    dst[0] = t[0]; dst[1] = t[1]; dst[2] = t[2]; dst[3] = t[3];
  } else if constexpr (BYTES == 8) {
    const u32x2 t = *reinterpret_cast<const u32x2*>(p);
    dst[0] = t[0]; dst[1] = t[1];
  } else {
    dst[0] = *reinterpret_cast<const unsigned*>(p);
  }
}

template <int CIN, int COUT, int AL, bool F16>
__global__ void __launch_bounds__(192)
conv3d_s2_wgrad_kernel(S2P P, const unsigned short* __restrict__ in, const unsigned short* __restrict__ dout,
                       float* __restrict__ part, long nrows) {
  constexpr int MT = COUT / 16, NT = CIN / 16;
  constexpr int GB = AL, GE = GB / 2, GN = 8 / GE;                       // dout pieces: bytes, elements, count
  constexpr int IB = AL >= 8 ? 16 : 8, IE = IB / 2, INP = 16 / IE;        // input pieces
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;           // wave = dz
  const int li = lane & 15, kg = lane >> 4;
  const long plane_i = (long) P.Z * P.Y * P.X, plane_o = (long) P.Zo * P.Yo * P.Xo;
  f32x4 acc[9][MT][NT];
#pragma unroll
  for (int t = 0; t < 9; ++t)
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
      for (int n = 0; n < NT; ++n) acc[t][m][n] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int ksteps = (P.Xo + 31) / 32;
  // All loads are unconditional, from rows and piece starts clamped into the volume (a piece never straddles a row
  // end: the row lengths are multiples of the piece); what lies outside is zeroed in registers afterwards.
  struct Step {
    unsigned a[MT][4];
    unsigned v[3][NT][8];
    int zo, yo, xb;
  };
  auto load = [&](Step& S, long step) {
    const long row = blockIdx.x + (step / ksteps) * (long) gridDim.x;
    const int ks = (int) (step % ksteps);
    S.yo = (int) (row % P.Yo);
    S.zo = (int) ((row / P.Yo) % P.Zo);
    const int b = (int) (row / ((long) P.Yo * P.Zo));
    S.xb = ks * 32 + 8 * kg;
    const unsigned short* gb = dout + (long) b * P.cout * plane_o + ((long) S.zo * P.Yo + S.yo) * P.Xo;
    const unsigned short* ib = in + (long) b * P.cin * plane_i;
    const int zz = min(max(2 * S.zo + wv - 1, 0), P.Z - 1);
#pragma unroll
    for (int m = 0; m < MT; ++m) {
      const unsigned short* rowp = gb + (long) min(m * 16 + li, P.cout - 1) * plane_o;
#pragma unroll
      for (int p = 0; p < GN; ++p) load_piece<GB>(rowp + min(S.xb + p * GE, P.Xo - GE), &S.a[m][p * (GE / 2)]);
    }
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      const int yy = min(max(2 * S.yo + r - 1, 0), P.Y - 1);
#pragma unroll
      for (int n = 0; n < NT; ++n) {
        const unsigned short* rowp = ib + (((long) min(n * 16 + li, P.cin - 1) * P.Z + zz) * P.Y + yy) * P.X;
#pragma unroll
        for (int p = 0; p < INP; ++p) load_piece<IB>(rowp + min(2 * S.xb + p * IE, P.X - IE), &S.v[r][n][p * (IE / 2)]);
      }
    }
  };
  auto as_frag = [](const u32x4& v) {
    bf16x8 f;
    __builtin_memcpy(&f, &v, 16);
    return f;
  };
  const u32x4 zero4 = u32x4{0u, 0u, 0u, 0u};
  // prev3[r][n]: the last dword of the previous step's odd-x stream (the input x just left of lane group 0's window)
  unsigned prev3[3][NT];
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int n = 0; n < NT; ++n) prev3[r][n] = 0u;
  auto compute = [&](const Step& S) {
    const bool in_row = S.xb < P.Xo;
    bf16x8 a[MT];
#pragma unroll
    for (int m = 0; m < MT; ++m) {
      u32x4 t;
#pragma unroll
      for (int d = 0; d < 4; ++d) t[d] = (S.xb + 2 * d < P.Xo && m * 16 + li < P.cout) ? S.a[m][d] : 0u;
      a[m] = as_frag(t);
    }
    const int zz = 2 * S.zo + wv - 1;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      const int yy = 2 * S.yo + r - 1;
      const bool row_ok = zz >= 0 && zz < P.Z && yy >= 0 && yy < P.Y;       // wave-uniform
#pragma unroll
      for (int n = 0; n < NT; ++n) {
        const bool lane_ok = row_ok && n * 16 + li < P.cin;
        unsigned v[8];
#pragma unroll
        for (int d = 0; d < 8; ++d) v[d] = (lane_ok && 2 * S.xb + 2 * d < P.X) ? S.v[r][n][d] : 0u;
        u32x4 ev, od;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          ev[q] = __builtin_amdgcn_perm(v[2 * q + 1], v[2 * q], 0x05040100u);   // x = 2 (xb + 2 q), 2 (xb + 2 q + 1)
          od[q] = __builtin_amdgcn_perm(v[2 * q + 1], v[2 * q], 0x07060302u);   // the same + 1
        }
        // the odd-x dword left of this lane's window: lane group kg - 1 (same step), or the previous step's group 3
        const unsigned lsend = kg == 3 ? prev3[r][n] : od[3];
        unsigned left = (unsigned) __shfl((int) lsend, (lane + 48) & 63, 64);
        if (S.xb == 0 || !lane_ok) left = 0u;                         // x = -1: padding
        u32x4 os = u32x4{__builtin_amdgcn_alignbit(od[0], left, 16), __builtin_amdgcn_alignbit(od[1], od[0], 16),
                         __builtin_amdgcn_alignbit(od[2], od[1], 16), __builtin_amdgcn_alignbit(od[3], od[2], 16)};
        if (!in_row) os = zero4;
        const bf16x8 b0 = as_frag(os), b1 = as_frag(ev), b2 = as_frag(od);
#pragma unroll
        for (int m = 0; m < MT; ++m) {
          acc[r * 3 + 0][m][n] = mfma16<F16>(a[m], b0, acc[r * 3 + 0][m][n]);
          acc[r * 3 + 1][m][n] = mfma16<F16>(a[m], b1, acc[r * 3 + 1][m][n]);
          acc[r * 3 + 2][m][n] = mfma16<F16>(a[m], b2, acc[r * 3 + 2][m][n]);
        }
        prev3[r][n] = od[3];
      }
    }
  };
  const long my_rows = blockIdx.x < nrows ? (nrows - blockIdx.x + gridDim.x - 1) / gridDim.x : 0;
  const long nsteps = my_rows * ksteps;
  Step cur, nxt;
  if (nsteps > 0) load(cur, 0);
  for (long st = 0; st < nsteps; ++st) {
    load(nxt, min(st + 1, nsteps - 1));
    compute(cur);
    cur = nxt;
  }
  store_wgrad_partials<CIN, COUT>(acc, part, wv, kg, li);
}

// ep: through the epilogue (EPI; OF32: fp32 outputs) instead of into `out`
template <int CIN, int COUT, bool F16, bool EPI = false, bool OF32 = false>
int launch_fwd(const VampConvDesc* d, const void* in, const void* w, void* out, hipStream_t s,
               const VampConvEpilogue* ep = nullptr) {
  using L = FwdLds<CIN, COUT>;
  const S2P P = make_params(d);
  const int tiles_x = (P.Xo + kFwdTX - 1) / kFwdTX, tiles_y = (P.Yo + FwdTile<CIN>::TY - 1) / FwdTile<CIN>::TY;
  const long ntiles = (long) P.B * P.Zo * tiles_y * tiles_x;
  static_assert(L::bytes <= 160 * 1024, "the box and the weight image share the LDS");
  const unsigned grid = (unsigned) std::min<long>(ntiles, kFwdWgs);
  const unsigned short* ip = static_cast<const unsigned short*>(in);
  const unsigned short* wp = static_cast<const unsigned short*>(w);
  if constexpr (EPI)
    return launch_lds(conv3d_s2_fwd_epi_kernel<CIN, COUT, F16, OF32>, "conv3d_s2_fwd_epi_kernel", L::bytes, grid,
                      kProfConvFwd, s, P, ip, wp, *ep, tiles_x, tiles_y, ntiles);
  else
    return launch_lds(conv3d_s2_fwd_kernel<CIN, COUT, F16>, "conv3d_s2_fwd_kernel", L::bytes, grid, kProfConvFwd, s, P, ip,
                      wp, static_cast<unsigned short*>(out), tiles_x, tiles_y, ntiles);
}

template <int CO, int CI, bool F16>
int launch_dgrad(const VampConvDesc* d, const void* gout, const void* w, void* gin, hipStream_t s) {
  using L = DgLds<CO, CI>;
  const S2P P = make_params(d);
  const int tiles_x = (P.X + kDgTX - 1) / kDgTX, tiles_y = (P.Y + kDgTY - 1) / kDgTY;
  const long ntiles = (long) P.B * P.Z * tiles_y * tiles_x;
  static_assert(2 * L::bytes <= 160 * 1024, "two workgroups per CU");
  const unsigned grid = (unsigned) std::min<long>(ntiles, kDgWgs);
  return launch_lds(conv3d_s2_dgrad_kernel<CO, CI, F16>, "conv3d_s2_dgrad_kernel", L::bytes, grid, kProfConvDgrad, s, P,
                    static_cast<const unsigned short*>(gout), static_cast<const unsigned short*>(w),
                    static_cast<unsigned short*>(gin), tiles_x, tiles_y, ntiles);
}

template <int CIN, int COUT, bool F16>
int launch_wgrad(const VampConvDesc* d, const void* in, const void* dout, float* dw, float* ws, hipStream_t s) {
  const S2P P = make_params(d);
  const long nrows = (long) P.B * P.Zo * P.Yo;
  const int nwg = (int) std::min<long>(nrows, kWgradWgs);
  const unsigned short* ip = static_cast<const unsigned short*>(in);
  const unsigned short* gp = static_cast<const unsigned short*>(dout);
  if (d->X % 16 == 0)
    VAMP_TIMED(kProfConvWgrad, s, (conv3d_s2_wgrad_kernel<CIN, COUT, 16, F16><<<nwg, 192, 0, s>>>(P, ip, gp, ws, nrows)));
  else if (d->X % 8 == 0)
    VAMP_TIMED(kProfConvWgrad, s, (conv3d_s2_wgrad_kernel<CIN, COUT, 8, F16><<<nwg, 192, 0, s>>>(P, ip, gp, ws, nrows)));
  else
    VAMP_TIMED(kProfConvWgrad, s, (conv3d_s2_wgrad_kernel<CIN, COUT, 4, F16><<<nwg, 192, 0, s>>>(P, ip, gp, ws, nrows)));
  if (int e = check_launch("conv3d_s2_wgrad_kernel")) return e;
  const int n = 27 * CIN * COUT;
  VAMP_TIMED(kProfConvWgrad, s, (conv3d_bf16_wreduce_kernel<<<(n + 63) / 64, 256, 0, s>>>(ws, dw, CIN, COUT, nwg, d->cin, d->cout)));
  return check_launch("conv3d_bf16_wreduce_kernel");
}

}  // namespace
}  // namespace vamp

using namespace vamp;

extern "C" {

// the descriptor holds the INPUT volume; one rule for the three entry points (the stride-1 16-bit rule: X % 4 == 0
// makes Xo even)
int vamp_conv3d_half_s2_supported(const VampConvDesc* d) { return bf16_shape_ok(d) ? 1 : 0; }

size_t vamp_conv3d_half_s2_workspace_bytes(const VampConvDesc* d) { return half_workspace_bytes(d); }

// Hourglass3D.conv1 / conv3 forward (base_vampire2.py:34-46) under a 16-bit autocast
int vamp_conv3d_half_s2_forward(const VampConvDesc* d, int32_t dtype, const void* in, const void* weight, void* out,
                                void* stream) {
  if (int e = half_args_ok(__func__, kShapeRule, d, dtype, in && weight && out)) return e;
  hipStream_t s = static_cast<hipStream_t>(stream);
  return dispatch_half(d->cin, d->cout, dtype, [&](auto CI, auto CO, auto F16) {
    return launch_fwd<CI(), CO(), F16()>(d, in, weight, out, s);
  });
}

// the forward through the epilogue (conv3d_epilogue.hpp; the contract is in vampire_hip.h)
int vamp_conv3d_half_s2_epilogue_forward(const VampConvDesc* d, int32_t dtype, const VampConvEpilogue* epi,
                                         const void* in, const void* weight, void* stream) {
  if (int e = half_args_ok(__func__, kShapeRule, d, dtype, true)) return e;
  if (int e = epi_check(__func__, d, epi, true, 1)) return e;
  VAMP_REQUIRE(in && weight, "NULL tensor");
  VAMP_REQUIRE(aligned(in, 16) && aligned(weight, 16), "in / weight must start on a 16-byte boundary");
  hipStream_t s = static_cast<hipStream_t>(stream);
  return dispatch_half(d->cin, d->cout, dtype, [&](auto CI, auto CO, auto F16) {
    return epi->seg[0].out_f32 ? launch_fwd<CI(), CO(), F16(), true, true>(d, in, weight, nullptr, s, epi)
                               : launch_fwd<CI(), CO(), F16(), true, false>(d, in, weight, nullptr, s, epi);
  });
}

// autograd's data gradient of the same layers (base_vampire2.py:34-46): grad_in is fully overwritten
int vamp_conv3d_half_s2_backward_data(const VampConvDesc* d, int32_t dtype, const void* grad_out, const void* weight,
                                      void* grad_in, void* stream) {
  if (int e = half_args_ok(__func__, kShapeRule, d, dtype, grad_out && weight && grad_in)) return e;
  hipStream_t s = static_cast<hipStream_t>(stream);
  // the tiles swapped: the kernel's K channels are grad_out's (cout), its M rows grad_in's (cin)
  return dispatch_half(d->cout, d->cin, dtype, [&](auto CO, auto CI, auto F16) {
    return launch_dgrad<CO(), CI(), F16()>(d, grad_out, weight, grad_in, s);
  });
}

// autograd's weight gradient of the same layers (base_vampire2.py:34-46): fp32 [cout, cin, 3, 3, 3], fully overwritten
int vamp_conv3d_half_s2_backward_weight(const VampConvDesc* d, int32_t dtype, const void* in, const void* grad_out,
                                        float* grad_weight, void* workspace, size_t workspace_bytes, void* stream) {
  if (int e = half_args_ok(__func__, kShapeRule, d, dtype, in && grad_out && grad_weight)) return e;
  const size_t need = half_workspace_bytes(d);
  if (int e = workspace_fits(__func__, workspace, workspace_bytes, need)) return e;
  hipStream_t s = static_cast<hipStream_t>(stream);
  float* ws = static_cast<float*>(workspace);
  return dispatch_half(d->cin, d->cout, dtype, [&](auto CI, auto CO, auto F16) {
    return launch_wgrad<CI(), CO(), F16()>(d, in, grad_out, grad_weight, ws, s);
  });
}

}  // extern "C"
