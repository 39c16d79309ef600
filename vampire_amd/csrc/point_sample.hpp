// What the two point-resampling files share (sample_points.hip: one volume per call; point_queries.hip: the four
// queries of a step in one call): the tap coordinates of a point, the eight taps of the forward with their weights
// and fma order, and the per-record accumulation of the backward's per-voxel gather (cell_list.hpp).
#pragma once
#include "cell_list.hpp"

namespace vamp {

struct SampleParams {
  int B, C, Z, Y, X, Pb;
  float lo[3], span[3];
  int border, mask_outside, activation, channel_last;
  int density_mode;
  float sdf_bias, beta_min;
  int n0, n12;             // lattice hint: n0 points along axis 0, n1 * n2 per axis-0 step (0 = none)
};

// density parameters when the activation is on (beta is only read then)
__device__ __forceinline__ DensityParams pts_density(const SampleParams& P, const float* __restrict__ beta_raw) {
  if (P.activation) return load_density(P.density_mode, beta_raw, P.beta_min, P.sdf_bias);
  DensityParams dp;
  dp.mode = VAMP_DENSITY_SIGMOID; dp.beta = 1.f; dp.ib = 1.f; dp.bias = 0.f;
  return dp;
}

// continuous tap coordinates of a point (aten: normalise by the bounds, unnormalise with
// align_corners=True, clip for 'border'), and the reference's inside mask
struct PointTap {
  float fx, fy, fz;
  bool inside;       // all(-1 <= n <= 1)        (bv2:587-589)
};
// point_tap's border clip on its own, for a caller that needs a point's clipped and unclipped taps
__device__ __forceinline__ void clip_tap(const SampleParams& P, PointTap& t) {
  t.fx = fminf((float) (P.X - 1), fmaxf(t.fx, 0.f));
  t.fy = fminf((float) (P.Y - 1), fmaxf(t.fy, 0.f));
  t.fz = fminf((float) (P.Z - 1), fmaxf(t.fz, 0.f));
}
__device__ __forceinline__ PointTap point_tap(const SampleParams& P, const float* __restrict__ pt) {
  const float gx = ((pt[0] - P.lo[0]) / P.span[0]) * 2.0f - 1.0f;
  const float gy = ((pt[1] - P.lo[1]) / P.span[1]) * 2.0f - 1.0f;
  const float gz = ((pt[2] - P.lo[2]) / P.span[2]) * 2.0f - 1.0f;
  PointTap t;
  t.inside = gx >= -1.0f && gx <= 1.0f && gy >= -1.0f && gy <= 1.0f && gz >= -1.0f && gz <= 1.0f;
  t.fx = ((gx + 1.0f) / 2.0f) * (float) (P.X - 1);
  t.fy = ((gy + 1.0f) / 2.0f) * (float) (P.Y - 1);
  t.fz = ((gz + 1.0f) / 2.0f) * (float) (P.Z - 1);
  if (P.border) {                     // clip_coordinates: min(size - 1, max(coord, 0)); nan -> 0
    t.fx = fminf((float) (P.X - 1), fmaxf(t.fx, 0.f));
    t.fy = fminf((float) (P.Y - 1), fmaxf(t.fy, 0.f));
    t.fz = fminf((float) (P.Z - 1), fmaxf(t.fz, 0.f));
  }
  return t;
}

// the eight taps of a point: weights, (clamped) voxel offsets inside one channel, and which of them are voxels
struct Taps8 {
  float wt[8];
  long at[8];
  unsigned inm;      // taps that are voxels: the others are skipped, not multiplied by 0 (aten)
};
__device__ __forceinline__ Taps8 point_taps8(const SampleParams& P, const PointTap& t) {
  const float flx = floorf(t.fx), fly = floorf(t.fy), flz = floorf(t.fz);
  // out-of-range coordinates (zeros mode) are clamped before the int conversion; their taps
  // get zero weight below
  const int ix0 = (int) fminf(fmaxf(flx, -2.f), (float) P.X), iy0 = (int) fminf(fmaxf(fly, -2.f), (float) P.Y),
            iz0 = (int) fminf(fmaxf(flz, -2.f), (float) P.Z);
  const float wx1 = t.fx - flx, wx0 = (flx + 1.0f) - t.fx;
  const float wy1 = t.fy - fly, wy0 = (fly + 1.0f) - t.fy;
  const float wz1 = t.fz - flz, wz0 = (flz + 1.0f) - t.fz;
  const bool finite = (t.fx == t.fx) && (t.fy == t.fy) && (t.fz == t.fz) &&
                      fabsf(t.fx) < 1e9f && fabsf(t.fy) < 1e9f && fabsf(t.fz) < 1e9f;
  Taps8 q;
  q.inm = 0;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const int iz = iz0 + (k >> 2), iy = iy0 + ((k >> 1) & 1), ix = ix0 + (k & 1);
    const bool in = finite && iz >= 0 && iz < P.Z && iy >= 0 && iy < P.Y && ix >= 0 && ix < P.X;
    q.inm |= (unsigned) in << k;
    q.wt[k] = in ? ((k & 1) ? wx1 : wx0) * ((k & 2) ? wy1 : wy0) * ((k & 4) ? wz1 : wz0) : 0.f;
    q.at[k] = ((long) min(max(iz, 0), P.Z - 1) * P.Y + min(max(iy, 0), P.Y - 1)) * P.X + min(max(ix, 0), P.X - 1);
  }
  return q;
}

// one channel of one point: sum_k wt[k] * v[k] in tap order, v through the density activation when `act`
template <typename T>
__device__ __forceinline__ float taps8_sample(const Taps8& q, const T* __restrict__ vol, long cb, bool act,
                                              const DensityParams& dp) {
  float s = 0.f;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    float v = ldf(vol, cb + q.at[k]);
    if (act) v = density_fwd(dp, v);
    if (!((q.inm >> k) & 1u)) v = 0.f;          // the clamped address may hold a non-finite value: 0 * v is NaN
    s = __builtin_fmaf(q.wt[k], v, s);
  }
  return s;
}

// The k-th record of a voxel's ranges into the voxel's accumulators: its trilinear weight at the voxel times its
// gradient row G[record's source index][CP].  SPLIT: the row's entry 0 goes to acc[0] for a source index below
// `split_at` and to `acc_b` for the others (point_queries.hip keeps the raw and the activated density gradient apart).
template <int CP4, bool SPLIT>
__device__ __forceinline__ void record_accumulate(const CellRanges& cr, int k, const float4* __restrict__ R,
                                                  const float* __restrict__ G, float fix, float fiy,
                                                  float fiz, float (&acc)[CP4 * 4], int split_at, float& acc_b) {
  constexpr int CP = CP4 * 4;
  const bool in = k < cr.tot;
  const float4 a = R[cell_pos(cr, min(k, cr.tot - 1))];
  const float wt = in ? cell_tap_weight(a.x, fix) * cell_tap_weight(a.y, fiy) * cell_tap_weight(a.z, fiz) : 0.f;
  const int src = __float_as_int(a.w);
  const float4* g4 = reinterpret_cast<const float4*>(G + (long) src * CP);
#pragma unroll
  for (int c4 = 0; c4 < CP4; ++c4) {
    const float4 f = g4[c4];
    if (SPLIT && c4 == 0) {
      const bool first = src < split_at;
      acc[0] = __builtin_fmaf(wt, first ? f.x : 0.f, acc[0]);
      acc_b = __builtin_fmaf(wt, first ? 0.f : f.x, acc_b);
    } else {
      acc[c4 * 4] = __builtin_fmaf(wt, f.x, acc[c4 * 4]);
    }
    acc[c4 * 4 + 1] = __builtin_fmaf(wt, f.y, acc[c4 * 4 + 1]);
    acc[c4 * 4 + 2] = __builtin_fmaf(wt, f.z, acc[c4 * 4 + 2]);
    acc[c4 * 4 + 3] = __builtin_fmaf(wt, f.w, acc[c4 * 4 + 3]);
  }
}

template <int CP4>
__device__ __forceinline__ void point_accumulate(const CellRanges& cr, int k, const float4* __restrict__ R,
                                                 const float* __restrict__ G, float fix, float fiy,
                                                 float fiz, float (&acc)[CP4 * 4]) {
  float unused = 0.f;
  record_accumulate<CP4, false>(cr, k, R, G, fix, fiy, fiz, acc, 0, unused);
}

// The workspace of either file's backward (cell_list.hpp's lists over the source rows, then the gradient rows), every
// region 256-byte aligned and back to back.  `rows`: source rows of all samples; `CP`: floats of a gradient row;
// `nbeta`: d beta partial sums.  `workspace` may be nullptr (only `bytes` is of use then).
struct PointWs {
  int *cnt, *off, *bsum, *boff, *aux, *heavy, *key, *rank;
  float4 *F, *R;
  float *G, *beta_part;
  size_t bytes;
};
inline PointWs point_ws(int B, int Z, int Y, int X, size_t rows, int CP, size_t nbeta, void* workspace) {
  Carve c(workspace);
  PointWs w;
  take_scan(c, (size_t) cell_count_padded(B, Z, Y, X), w.cnt, w.off, w.bsum, w.boff, w.aux);
  w.heavy = c.take<int>((size_t) B * Z * Y * X);
  w.key = c.take<int>(rows);
  w.rank = c.take<int>(rows);
  w.F = c.take<float4>(rows);
  w.R = c.take<float4>(rows);
  w.G = c.take<float>(rows * CP);
  w.beta_part = c.take<float>(nbeta);
  w.bytes = c.off;
  return w;
}

}  // namespace vamp
