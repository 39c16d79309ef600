// BEV (top-down) branch of the renderer for gfx950, the two-kernel forward: base_vampire2.py:408-418, 442-461.
// (The one-kernel forward is render_bev_fused.hip, the backward render_bev.hip.)
//
// The det-grid sample lattice is regular, so every access pattern here is coalesced
// (lanes along x) and the work splits per channel:
//
//  bev_density   thread per column: density samples -> sigma_j (= voxel_density)
//                and the height expectation
//  bev_channels  thread per (channel, column): trilinear samples of one channel at
//                the oZ heights; composite (sem / rgb) with weights rebuilt from
//                voxel_density, or pass through (base -> voxel_output)
#include "render_bev_dev.hpp"

namespace vamp {

template <typename T>
__global__ void __launch_bounds__(256)
bev_density_kernel(RenderParams P, const float* __restrict__ oxs, const float* __restrict__ oys,
                   const float* __restrict__ ozs, const float* __restrict__ bev_mids,
                   const float* __restrict__ beta_raw, const T* __restrict__ dens,
                   float* __restrict__ voxel_density, float* __restrict__ bev_height,
                   float* __restrict__ s0_save) {
  const int x = blockIdx.x * 64 + (threadIdx.x & 63);
  const int y = blockIdx.y * 4 + (threadIdx.x >> 6);
  const int b = blockIdx.z;
  if (x >= P.oX || y >= P.oY) return;
  const DensityParams dp = load_density(P.density_mode, beta_raw, P.beta_min, P.sdf_bias);
  const long V = (long) P.Z * P.Y * P.X, OYX = (long) P.oY * P.oX, col = (long) y * P.oX + x;
  const AxisTap tx = axis_tap(oxs[x], P.lo[0], P.span[0], P.X);
  const AxisTap ty = axis_tap(oys[y], P.lo[1], P.span[1], P.Y);
  float cum = 0.f, height = 0.f;
  for (int j0 = 0; j0 < P.oZ; j0 += kHChunk) {
    float s0[kHChunk];
#pragma unroll
    for (int u = 0; u < kHChunk; ++u) {
      const int j = min(j0 + u, P.oZ - 1);
      const AxisTap tz = axis_tap(ozs[P.oZ - 1 - j], P.lo[2], P.span[2], P.Z);     // flip (bv2:443)
      s0[u] = sample8(P, dens, (long) b * V, tx, ty, tz);
    }
#pragma unroll
    for (int u = 0; u < kHChunk; ++u) {
      const int j = j0 + u;
      if (j >= P.oZ) break;
      const float sigma = density_fwd(dp, s0[u]);
      voxel_density[((long) b * P.oZ + j) * OYX + col] = sigma;
      if (s0_save) s0_save[((long) b * P.oZ + j) * OYX + col] = s0[u];           // for the backward's scan
      const float tau = sigma * (1.0f * P.z_step);                                  // bv2:451-453
      height = __builtin_fmaf((1.0f - expf(-tau)) * expf(-cum), bev_mids[j], height);
      cum += tau;
    }
  }
  bev_height[(long) b * OYX + col] = height;
}

// channel index space of bev_channels: [0, K) semantic, [K, K+3) rgb, [K+3, K+3+C) base.
// A thread owns one BEV column and NC consecutive channels: the column's compositing weights
// (two exps per height) and the height taps are worked out once and shared by its channels --
// with a thread per (channel, column) this kernel spent 80 % of its time in the vector ALU
// redoing them 38 times -- and the 8 * NC plane loads of a height go out together.
// cfg-B, us per launch: one thread per (channel, column) 55; NC = 1 / 2 / 4 / 8: 46 / 41.5 / 50 / 48
// (fewer waves per CU hide less latency past NC = 2).
#ifndef VAMP_BEV_NC
#define VAMP_BEV_NC 2
#endif
constexpr int kBevNC = VAMP_BEV_NC;   // channels per thread

template <typename T, int NC>
__global__ void __launch_bounds__(256)
bev_channels_kernel(RenderParams P, const float* __restrict__ oxs, const float* __restrict__ oys,
                    const float* __restrict__ ozs, const T* __restrict__ sem,
                    const T* __restrict__ rgb, const T* __restrict__ base,
                    const float* __restrict__ voxel_density, float* __restrict__ bev_rgb,
                    float* __restrict__ bev_seg, float* __restrict__ voxel_output,
                    float* __restrict__ ss_save) {
  __shared__ int tz_i0[kBevMaxOZ];
  __shared__ float tz_w0[kBevMaxOZ], tz_w1[kBevMaxOZ];
  if ((int) threadIdx.x < P.oZ) {
    const AxisTap tz = axis_tap(ozs[P.oZ - 1 - threadIdx.x], P.lo[2], P.span[2], P.Z);   // flip (bv2:443)
    tz_i0[threadIdx.x] = tz.i0; tz_w0[threadIdx.x] = tz.w0; tz_w1[threadIdx.x] = tz.w1;
  }
  __syncthreads();
  const int x = blockIdx.x * 64 + (threadIdx.x & 63);
  const int y = blockIdx.y * 4 + (threadIdx.x >> 6);
  const int nch = P.K + 3 + P.C;
  const int ngrp = (nch + NC - 1) / NC;
  const int b = blockIdx.z / ngrp, c0 = (blockIdx.z % ngrp) * NC;
  if (x >= P.oX || y >= P.oY) return;
  const long V = (long) P.Z * P.Y * P.X, OYX = (long) P.oY * P.oX, col = (long) y * P.oX + x;
  const int CO = P.C + (P.cat_seg ? P.K : 0);
  const AxisTap tx = axis_tap(oxs[x], P.lo[0], P.span[0], P.X);
  const AxisTap ty = axis_tap(oys[y], P.lo[1], P.span[1], P.Y);
  // the four (y, x) taps of the column: clamped offsets and weights (zero outside the volume)
  long off4[4];
  float w4[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int iy = ty.i0 + (k >> 1), ix = tx.i0 + (k & 1);
    const bool in = iy >= 0 && iy < P.Y && ix >= 0 && ix < P.X;
    w4[k] = in ? ((k & 1) ? tx.w1 : tx.w0) * ((k & 2) ? ty.w1 : ty.w0) : 0.f;
    off4[k] = (long) min(max(iy, 0), P.Y - 1) * P.X + min(max(ix, 0), P.X - 1);
  }
  const T* vol[NC];
  long cb[NC];
  bool on[NC];
#pragma unroll
  for (int u = 0; u < NC; ++u) {
    const int ch = min(c0 + u, nch - 1);
    on[u] = c0 + u < nch;
    if (ch < P.K) { vol[u] = sem; cb[u] = ((long) b * P.K + ch) * V; }
    else if (ch < P.K + 3) { vol[u] = rgb; cb[u] = ((long) b * 3 + (ch - P.K)) * V; }
    else { vol[u] = base; cb[u] = ((long) b * P.C + (ch - P.K - 3)) * V; }
  }
  auto plane = [&](int u, int iz) -> float {
    const bool zin = iz >= 0 && iz < P.Z;
    const long zo = cb[u] + (long) min(max(iz, 0), P.Z - 1) * P.Y * P.X;
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k) s = __builtin_fmaf(zin ? w4[k] : 0.f, ldf(vol[u], zo + off4[k]), s);
    return s;
  };
  float cum = 0.f, acc[NC];
#pragma unroll
  for (int u = 0; u < NC; ++u) acc[u] = 0.f;
  const bool any_comp = c0 < P.K + 3;
  // Heights kHChunk at a time.  A wave's life is (heights) x (memory round trip) -- 2.3 us per
  // height under load -- so the volume planes of a whole chunk are fetched in one go: the chunk's
  // heights step down the volume by at most one plane each (det and seg grids have about the same
  // spacing), so its kHChunk + 1 planes below the first height's upper plane cover it; a height
  // outside that window (other spacings) fetches its two planes itself.
  for (int j0 = 0; j0 < P.oZ; j0 += kHChunk) {
    const int top = tz_i0[j0] + 1;
    float pl[NC][kHChunk + 1], tau[kHChunk];
#pragma unroll
    for (int t = 0; t <= kHChunk; ++t)
#pragma unroll
      for (int u = 0; u < NC; ++u) pl[u][t] = plane(u, top - t);
#pragma unroll
    for (int h = 0; h < kHChunk; ++h)
      tau[h] = any_comp ? voxel_density[((long) b * P.oZ + min(j0 + h, P.oZ - 1)) * OYX + col] * (1.0f * P.z_step) : 0.f;   // bv2:451-458
#pragma unroll
    for (int h = 0; h < kHChunk; ++h) {
      const int j = j0 + h;
      if (j >= P.oZ) break;
      const int i0 = tz_i0[j];
      const float wz0 = tz_w0[j], wz1 = tz_w1[j];
      const int d = top - 1 - i0;                  // planes below the chunk's first height (uniform)
      float n_lo[NC], n_hi[NC];
      bool found = false;
#pragma unroll
      for (int t = 0; t < kHChunk; ++t)
        if (d == t) {
#pragma unroll
          for (int u = 0; u < NC; ++u) { n_hi[u] = pl[u][t]; n_lo[u] = pl[u][t + 1]; }
          found = true;
        }
      if (!found) {
#pragma unroll
        for (int u = 0; u < NC; ++u) { n_hi[u] = plane(u, i0 + 1); n_lo[u] = plane(u, i0); }
      }
      const float wj = (1.0f - expf(-tau[h])) * expf(-cum);
      cum += tau[h];
#pragma unroll
      for (int u = 0; u < NC; ++u) {
        const float sv = __builtin_fmaf(wz1, n_hi[u], wz0 * n_lo[u]);
        const int ch = c0 + u;
        if (!on[u]) continue;
        if (ch < P.K + 3) {
          acc[u] = __builtin_fmaf(wj, sv, acc[u]);
          // training: the backward's q_j = sum_c G_c s_j[c] reads the samples back
          if (ss_save) ss_save[(((long) b * (P.K + 3) + ch) * P.oZ + j) * OYX + col] = sv;
          if (ch < P.K && P.cat_seg)
            voxel_output[(((long) b * CO + P.C + ch) * P.oZ + j) * OYX + col] = sv;     // bv2:449-450
        } else {
          voxel_output[(((long) b * CO + (ch - P.K - 3)) * P.oZ + j) * OYX + col] = sv;
        }
      }
    }
  }
#pragma unroll
  for (int u = 0; u < NC; ++u) {
    const int ch = c0 + u;
    if (!on[u]) continue;
    if (ch < P.K) bev_seg[((long) b * P.K + ch) * OYX + col] = acc[u];
    else if (ch < P.K + 3) bev_rgb[((long) b * 3 + (ch - P.K)) * OYX + col] = acc[u];
  }
}

// the two launches for volumes of type T
template <typename T>
static int launch_bev_fwd_two(const VampRenderDesc* d, const RenderParams& P, const float* oxs, const float* oys,
                              const float* ozs, const float* bev_mids, const float* beta, const void* dens,
                              const void* sem, const void* rgb, const void* base, float* bev_rgb, float* bev_seg,
                              float* bev_height, float* voxel_density, float* voxel_output, float* s0_save,
                              float* ss_save, hipStream_t s) {
  const dim3 g1((d->oX + 63) / 64, (d->oY + 3) / 4, d->B);
  const dim3 g2((d->oX + 63) / 64, (d->oY + 3) / 4, d->B * ((d->K + 3 + d->C + kBevNC - 1) / kBevNC));
  VAMP_TIMED(kProfBevFwd, s, (bev_density_kernel<T><<<g1, 256, 0, s>>>(
      P, oxs, oys, ozs, bev_mids, beta, (const T*) dens, voxel_density, bev_height, s0_save)));
  if (int e = check_launch("bev_density_kernel")) return e;
  VAMP_TIMED(kProfBevFwdCh, s, (bev_channels_kernel<T, kBevNC><<<g2, 256, 0, s>>>(
      P, oxs, oys, ozs, (const T*) sem, (const T*) rgb, (const T*) base, voxel_density, bev_rgb, bev_seg,
      voxel_output, ss_save)));
  return check_launch("bev_channels_kernel");
}

}  // namespace vamp

using namespace vamp;

extern "C" {

int vamp_render_bev_forward_ex(const VampRenderDesc* d, const float* oxs, const float* oys,
                               const float* ozs, const float* bev_mids, const float* beta,
                               const void* density_feature, const void* semantic, const void* rgb,
                               const void* base, float* bev_rgb, float* bev_seg, float* bev_height,
                               float* voxel_density, float* voxel_output, const float* ozs_host,
                               void* workspace, size_t workspace_bytes, int flags, void* stream) {
  if (int e = validate(d)) return e;
  float *s0_save = nullptr, *ss_save = nullptr;
  if (flags & VAMP_BEVFWD_SAVE) {
    const BevWorkspace w = bev_workspace(d, workspace);
    if (int e = workspace_fits(__func__, workspace, workspace_bytes, w.bytes)) return e;
    s0_save = w.s0_saved;
    ss_save = w.ss_saved;
  }
  VAMP_REQUIRE(d->oZ > 0 && d->oY > 0 && d->oX > 0, "det grid must be non-empty");
  VAMP_REQUIRE(oxs && oys && ozs && bev_mids && density_feature && semantic && rgb, "null pointer");
  VAMP_REQUIRE(base || d->C == 0, "base is NULL");
  VAMP_REQUIRE(bev_rgb && bev_seg && bev_height && voxel_density && voxel_output, "null output");
  VAMP_REQUIRE(beta || d->density_mode == VAMP_DENSITY_SIGMOID, "beta is NULL");
  const RenderParams P = to_params(d);
  hipStream_t s = static_cast<hipStream_t>(stream);
  // the one-kernel forward only for heights the library has checked against its plane slabs (bev_fused_heights_fit)
  if (!(flags & VAMP_BEVFWD_TWO_KERNELS) && bev_fwd_fused_supported(d) && bev_fused_heights_fit(d, ozs_host))
    return launch_bev_fwd_fused(d, P, oxs, oys, ozs, bev_mids, beta, density_feature, semantic, rgb, base, bev_rgb,
                                bev_seg, bev_height, voxel_density, voxel_output, s0_save, ss_save, s);
  VAMP_REQUIRE(d->oZ <= kBevMaxOZ, "at most 64 det-grid heights");
  return (d->in_dtype == VAMP_F32 ? launch_bev_fwd_two<float> : launch_bev_fwd_two<__hip_bfloat16>)(
      d, P, oxs, oys, ozs, bev_mids, beta, density_feature, semantic, rgb, base, bev_rgb, bev_seg, bev_height,
      voxel_density, voxel_output, s0_save, ss_save, s);
}

int vamp_render_bev_forward(const VampRenderDesc* d, const float* oxs, const float* oys,
                            const float* ozs, const float* bev_mids, const float* beta,
                            const void* density_feature, const void* semantic, const void* rgb,
                            const void* base, float* bev_rgb, float* bev_seg, float* bev_height,
                            float* voxel_density, float* voxel_output, void* stream) {
  return vamp_render_bev_forward_ex(d, oxs, oys, ozs, bev_mids, beta, density_feature, semantic, rgb, base,
                                    bev_rgb, bev_seg, bev_height, voxel_density, voxel_output, nullptr, nullptr, 0, 0,
                                    stream);
}

}  // extern "C"
