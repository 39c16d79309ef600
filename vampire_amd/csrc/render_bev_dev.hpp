// Device helpers shared by the BEV forward (render_bev_fwd.hip) and the BEV backward (render_bev.hip).
#pragma once
#include "render_common.hpp"

namespace vamp {

constexpr int kBevMaxOZ = 64;         // heights whose taps fit the LDS table

// bev_density_kernel and bev_scan_kernel take the heights kHChunk at a time: a column is one thread
// and the grid is only oY * oX / 64 waves, so the loads of one height cannot hide behind other
// waves -- the taps of a whole chunk are issued together instead of one round trip per height.
constexpr int kHChunk = 5;

// x/y part of a column's taps (shared by all heights) and the z part per height
struct AxisTap {
  int i0;
  float w0, w1;
};

__device__ __forceinline__ AxisTap axis_tap(float pos, float lo, float span, int n) {
  const float g = ((pos - lo) / span) * 2.0f - 1.0f;
  const float f = ((g + 1.0f) / 2.0f) * (float) (n - 1);
  const float fl = floorf(f);
  AxisTap t;
  t.i0 = (int) fl;
  t.w1 = f - fl;
  t.w0 = (fl + 1.0f) - f;
  return t;
}

template <typename T>
__device__ __forceinline__ float sample8(const RenderParams& P, const T* __restrict__ vol, long cb,
                                         const AxisTap& tx, const AxisTap& ty, const AxisTap& tz) {
  // aten tap order: x fastest, then y, then z; zero padding outside the volume
  // branch-free: out-of-volume taps are clamped to a legal address and given zero weight, so
  // the eight loads are independent (a bounds branch per tap serialises the round trips)
  float s = 0.f;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const int iz = tz.i0 + (k >> 2), iy = ty.i0 + ((k >> 1) & 1), ix = tx.i0 + (k & 1);
    const bool in = iz >= 0 && iz < P.Z && iy >= 0 && iy < P.Y && ix >= 0 && ix < P.X;
    const float wt = in ? ((k & 1) ? tx.w1 : tx.w0) * ((k & 2) ? ty.w1 : ty.w0) * ((k & 4) ? tz.w1 : tz.w0) : 0.f;
    const long at = ((long) min(max(iz, 0), P.Z - 1) * P.Y + min(max(iy, 0), P.Y - 1)) * P.X + min(max(ix, 0), P.X - 1);
    s = __builtin_fmaf(wt, ldf(vol, cb + at), s);
  }
  return s;
}

// bilinear (x, y) sample of one volume plane, zero padding (also for a plane outside the volume)
template <typename T>
__device__ __forceinline__ float bilinear_plane(const RenderParams& P, const T* __restrict__ vol,
                                                long cb, const AxisTap& tx, const AxisTap& ty, int iz) {
  const bool zin = iz >= 0 && iz < P.Z;
  const int izc = min(max(iz, 0), P.Z - 1);
  float s = 0.f;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int iy = ty.i0 + (k >> 1), ix = tx.i0 + (k & 1);
    const bool in = zin && iy >= 0 && iy < P.Y && ix >= 0 && ix < P.X;
    const float wt = in ? ((k & 1) ? tx.w1 : tx.w0) * ((k & 2) ? ty.w1 : ty.w0) : 0.f;
    s = __builtin_fmaf(wt, ldf(vol, cb + ((long) izc * P.Y + min(max(iy, 0), P.Y - 1)) * P.X + min(max(ix, 0), P.X - 1)), s);
  }
  return s;
}

}  // namespace vamp
