// Rgb loss on the device: mean smooth-L1 (beta 1) + 1 - MS-SSIM of the rendered image against the label
// (base_exp.py:286, 539-549; the definition is multitask.ms_ssim with its defaults: Gaussian 11 / 1.5 window as a
// valid correlation, five scales, betas 0.0448 0.2856 0.3001 0.2363 0.1333, 2x2 average pooling with floor between
// the scales, the per-image contrast-structure means relu-ed), forward and gradient with respect to the prediction,
// without a host synchronisation, without float atomics and with bitwise repeatable results.
//
//  forward   rgb_fwd_kernel, one launch per scale s = 0 .. 4.  A 256-lane workgroup owns a 16 x 32 tile of one
//            plane's valid region.  It loads the tile plus the window's reach (26 x 42 pixels of x and of y) into LDS,
//            runs the 11 taps along the rows over the five moments x, y, xx, yy, xy into a float64 LDS buffer and then
//            along the columns, two pixels per lane.  The window sums and sigma = E[..] - mu^2 are float64: on a flat
//            region the difference cancels against c2 = 9e-4, and fp32 sums would put 1e-5 into the gradient there.
//            From sigma on a pixel is fp32: cs = (2 sxy + c2) / (sxx + syy + c2), on the last scale times
//            l = (2 mux muy + c1) / (mux^2 + muy^2 + c1).  The workgroup stores the tile's sum as one float64
//            partial, and per pixel the three UNIT adjoints d value / d mux, d value / d E[xx], d value / d E[xy]
//            (fp32).  They are kept and not recomputed by the backward: the factor that multiplies them,
//            d loss / d v[n, s], is one number per image and scale, so it can be applied behind the transposed window,
//            and the backward then needs neither the five-moment pass again nor a 20-pixel reach.  The price is
//            12 bytes of workspace per valid pixel.  The same launch writes the 2x2-pooled x and y of the pixels the
//            tile owns for the next scale, and at scale 0 the float64 partial of the smooth-L1 sum (a tile owns its
//            16 x 32 pixels; the last tile of a row or column also owns the 10 pixels behind the valid region).
//  finish    rgb_finish_kernel, one workgroup: the partials of every (image, scale) in index order (lane-strided,
//            then a butterfly), v[n, s] = relu(sum / (C Hv Wv)); per image prod = PROD v^beta and the backward's
//            factors fac[n, s] = -beta_s prod / v[n, s] / (N C Hv Wv) = d loss / d value at a pixel of scale s;
//            ms_ssim = mean_n prod, terms = (mean smooth-L1, ms_ssim), loss = terms[0] + 1 - terms[1].
//            Where some v[n, s] is 0 after the relu, prod is 0 and every fac[n, .] is exactly 0: the image's MS-SSIM
//            gradient is DEFINED as zero.  This is the one difference from the torch expression, where the gradient
//            of relu(v) ** beta at 0 is inf * 0 = NaN (a NaN that a relu backward which selects may drop again).
//  backward  rgb_bwd_kernel, one launch per scale, coarse to fine.  A workgroup owns a 16 x 32 tile of one plane of
//            scale s.  It loads the three unit adjoints over the tile and the 10 valid positions before it (zero
//            outside the valid region) into LDS and applies the window's transpose (the window is symmetric: the
//            same 11 taps, rows then columns, float64 sums), then g = fac (Amu + 2 x Axx + y Axy), plus a quarter of
//            the coarser scale's gradient at the pooled position (rows and columns the pooling dropped get none).
//            Scales 4 .. 1 store g in the workspace; scale 0 adds the smooth-L1 gradient clamp(x - y, -1, 1) / numel,
//            multiplies by the upstream grad_loss[0] (a device scalar; the last factor, so a scaled loss scales every
//            element with one rounding) and writes grad_pred once.
// The workspace needs no initialisation; the backward reads what the forward left there.  Eleven launches in all.
#include <cmath>

#include "common.hpp"
#include "wave_reduce.hpp"

namespace vamp {
namespace {

constexpr int kRgbScales = 5;
constexpr int kRgbTaps = 11;
constexpr int kRgbReach = kRgbTaps - 1;              // 10
constexpr int kRgbMinSide = 176;                     // the fifth scale still holds one window: 176 / 16 = 11
constexpr int kRgbMaxSide = 16384;
constexpr int kRgbBlock = 256;
constexpr int kRgbWaves = kRgbBlock / 64;
constexpr int kTW = 32, kTH = 16;                    // tile: 32 columns x 16 rows, two rows per lane
constexpr int kLW = kTW + kRgbReach, kLH = kTH + kRgbReach;   // 42 x 26 loaded
constexpr int kLP = kLW + 1;                         // LDS row pitch (odd: the column pass of the loads spreads over banks)
constexpr double kRgbBetas[kRgbScales] = {0.0448, 0.2856, 0.3001, 0.2363, 0.1333};

struct RgbParams {
  const float* x0;                                   // pred   [P, H, W]
  const float* y0;                                   // target [P, H, W]
  const float* grad_loss;
  float* grad;                                       // grad_pred
  float* loss;
  float* terms;
  float* vals;
  double* part;                                      // partial sums: scale s at part_off[s], smooth-L1 at part_off[5]
  double* vd;                                        // [N, 5] v in float64
  double* fac;                                       // [N, 5]
  double* prodn;                                     // [N]
  float* pyr;                                        // x_s at pyr_off[s], y_s behind it (s >= 1)
  float* adj;                                        // three maps of P Hv Wv floats at adj_off[s]
  float* gco;                                        // gradient of scale s at g_off[s] (s >= 1)
  long part_off[kRgbScales + 1], pyr_off[kRgbScales], adj_off[kRgbScales], g_off[kRgbScales];
  int H[kRgbScales], W[kRgbScales], tx[kRgbScales], ty[kRgbScales];   // tiles of the VALID region (forward)
  int N, C, P;
  float c1, c2;
  double w[kRgbTaps];
};

// ---------------------------------------------------------------------------------------------------------
// forward
// ---------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kRgbBlock) rgb_fwd_kernel(RgbParams p, int s) {
  __shared__ float sx[kLH][kLP], sy[kLH][kLP];
  __shared__ double hb[5][kLH][kTW];
  __shared__ double red[kRgbWaves];
  const int tid = threadIdx.x;
  const int Hs = p.H[s], Ws = p.W[s], Hv = Hs - kRgbReach, Wv = Ws - kRgbReach;
  const int tiles = p.tx[s] * p.ty[s];
  const int plane = blockIdx.x / tiles, t = blockIdx.x % tiles, ty = t / p.tx[s], tx = t % p.tx[s];
  const int r0 = ty * kTH, c0 = tx * kTW;
  const long psz = (long) Hs * Ws;
  const float* xs = s == 0 ? p.x0 : p.pyr + p.pyr_off[s];
  const float* ys = s == 0 ? p.y0 : xs + (long) p.P * psz;
  xs += plane * psz;
  ys += plane * psz;
  for (int i = tid; i < kLH * kLW; i += kRgbBlock) {
    const int r = i / kLW, c = i % kLW, gr = r0 + r, gc = c0 + c;
    const bool in = gr < Hs && gc < Ws;
    sx[r][c] = in ? xs[(long) gr * Ws + gc] : 0.0f;
    sy[r][c] = in ? ys[(long) gr * Ws + gc] : 0.0f;
  }
  __syncthreads();
  // the window along the rows
  for (int i = tid; i < kLH * kTW; i += kRgbBlock) {
    const int r = i / kTW, c = i % kTW;
    double mx = 0.0, my = 0.0, xx = 0.0, yy = 0.0, xy = 0.0;
#pragma unroll
    for (int k = 0; k < kRgbTaps; ++k) {
      const double a = sx[r][c + k], b = sy[r][c + k], w = p.w[k];
      mx = __builtin_fma(w, a, mx);
      my = __builtin_fma(w, b, my);
      xx = __builtin_fma(w, a * a, xx);
      yy = __builtin_fma(w, b * b, yy);
      xy = __builtin_fma(w, a * b, xy);
    }
    hb[0][r][c] = mx; hb[1][r][c] = my; hb[2][r][c] = xx; hb[3][r][c] = yy; hb[4][r][c] = xy;
  }
  __syncthreads();
  // along the columns, then the pixel's value and unit adjoints
  double acc = 0.0;
  const long vsz = (long) Hv * Wv;
  float* adj = p.adj + p.adj_off[s] + plane * vsz;
  const long msz = (long) p.P * vsz;
  const double c2 = (double) p.c2;
  const bool last = s == kRgbScales - 1;
#pragma unroll
  for (int o = 0; o < 2; ++o) {
    const int r = (tid >> 5) + o * (kTH / 2), c = tid & 31, gr = r0 + r, gc = c0 + c;
    double m[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int k = 0; k < kRgbTaps; ++k) {
      const double w = p.w[k];
#pragma unroll
      for (int j = 0; j < 5; ++j) m[j] = __builtin_fma(w, hb[j][r + k][c], m[j]);
    }
    if (gr < Hv && gc < Wv) {
      const double sxx = m[2] - m[0] * m[0], syy = m[3] - m[1] * m[1], sxy = m[4] - m[0] * m[1];
      const float mux = (float) m[0], muy = (float) m[1];
      const float D = (float) (sxx + syy + c2), A = (float) (2.0 * sxy + c2);
      const float invD = 1.0f / D, cs = A / D;
      float val, umu, uxx, uxy;
      if (last) {
        const float E = (mux * mux + muy * muy) + p.c1;
        const float l = ((2.0f * mux) * muy + p.c1) / E;
        val = l * cs;
        uxy = l * (2.0f * invD);
        uxx = -(l * cs) * invD;
        umu = (-(muy * uxy) - (2.0f * mux) * uxx) + cs * ((2.0f * muy - (2.0f * mux) * l) / E);
      } else {
        val = cs;
        uxy = 2.0f * invD;
        uxx = -cs * invD;
        umu = -(muy * uxy) - (2.0f * mux) * uxx;
      }
      const long e = (long) gr * Wv + gc;
      adj[e] = umu;
      adj[msz + e] = uxx;
      adj[2 * msz + e] = uxy;
      acc += (double) val;
    }
  }
  const double tot = block_sum<kRgbWaves>(acc, red);
  if (tid == 0) p.part[p.part_off[s] + blockIdx.x] = tot;
  // the pixels this tile owns: its 16 x 32, and what lies behind the valid region for the last tile of a row / column
  const int lrows = ty == p.ty[s] - 1 ? Hs - r0 : kTH, lcols = tx == p.tx[s] - 1 ? Ws - c0 : kTW;
  if (!last) {
    const int Hn = p.H[s + 1], Wn = p.W[s + 1], npr = lrows / 2, npc = lcols / 2;
    float* xn = p.pyr + p.pyr_off[s + 1] + (long) plane * Hn * Wn;
    float* yn = xn + (long) p.P * Hn * Wn;
    for (int i = tid; i < npr * npc; i += kRgbBlock) {
      const int pi = i / npc, pj = i % npc, a = 2 * pi, b = 2 * pj;
      const long e = (long) (r0 / 2 + pi) * Wn + (c0 / 2 + pj);
      xn[e] = ((sx[a][b] + sx[a][b + 1]) + (sx[a + 1][b] + sx[a + 1][b + 1])) * 0.25f;
      yn[e] = ((sy[a][b] + sy[a][b + 1]) + (sy[a + 1][b] + sy[a + 1][b + 1])) * 0.25f;
    }
  }
  if (s == 0) {
    double sl = 0.0;
    for (int i = tid; i < lrows * lcols; i += kRgbBlock) {
      const int r = i / lcols, c = i % lcols;
      const double d = (double) sx[r][c] - (double) sy[r][c], ad = fabs(d);
      sl += ad < 1.0 ? 0.5 * d * d : ad - 0.5;
    }
    const double st = block_sum<kRgbWaves>(sl, red);
    if (tid == 0) p.part[p.part_off[kRgbScales] + blockIdx.x] = st;
  }
}

__global__ void __launch_bounds__(kRgbBlock) rgb_finish_kernel(RgbParams p) {
  __shared__ double red[kRgbWaves];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  for (int pr = wave; pr < p.N * kRgbScales; pr += kRgbWaves) {
    const int n = pr / kRgbScales, s = pr % kRgbScales;
    const int cnt = p.C * p.tx[s] * p.ty[s];
    const double* q = p.part + p.part_off[s] + (long) n * cnt;
    double a = 0.0;
    for (int j = lane; j < cnt; j += 64) a += q[j];
    a = wave_sum(a);
    if (lane == 0) {
      const double M = (double) p.C * (p.H[s] - kRgbReach) * (p.W[s] - kRgbReach);
      double v = a / M;
      v = v > 0.0 ? v : 0.0;                          // (a NaN mean counts as 0)
      p.vd[pr] = v;
      p.vals[pr] = (float) v;
    }
  }
  __syncthreads();
  for (int n = tid; n < p.N; n += kRgbBlock) {
    double prod = 1.0;
    bool pos = true;
    for (int s = 0; s < kRgbScales; ++s) {
      const double v = p.vd[n * kRgbScales + s];
      pos = pos && v > 0.0;
      prod *= pow(v, kRgbBetas[s]);
    }
    if (!pos) prod = 0.0;
    for (int s = 0; s < kRgbScales; ++s) {
      const double M = (double) p.C * (p.H[s] - kRgbReach) * (p.W[s] - kRgbReach);
      p.fac[n * kRgbScales + s] = pos ? -(kRgbBetas[s] * prod / p.vd[n * kRgbScales + s]) / ((double) p.N * M) : 0.0;
    }
    p.prodn[n] = prod;
  }
  __syncthreads();
  double a = 0.0, b = 0.0;
  for (int n = tid; n < p.N; n += kRgbBlock) a += p.prodn[n];
  const long nsl = (long) p.P * p.tx[0] * p.ty[0];
  const double* q = p.part + p.part_off[kRgbScales];
  for (long j = tid; j < nsl; j += kRgbBlock) b += q[j];
  const double ms = block_sum<kRgbWaves>(a, red) / (double) p.N;
  const double sl = block_sum<kRgbWaves>(b, red) / ((double) p.P * p.H[0] * p.W[0]);
  if (tid == 0) {
    p.terms[0] = (float) sl;
    p.terms[1] = (float) ms;
    p.loss[0] = (float) (sl + 1.0 - ms);
  }
}

// ---------------------------------------------------------------------------------------------------------
// backward
// ---------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kRgbBlock) rgb_bwd_kernel(RgbParams p, int s, int btx, int bty) {
  __shared__ float sa[3][kLH][kLP];
  __shared__ double hb[3][kLH][kTW];
  const int tid = threadIdx.x;
  const int Hs = p.H[s], Ws = p.W[s], Hv = Hs - kRgbReach, Wv = Ws - kRgbReach;
  const int tiles = btx * bty;
  const int plane = blockIdx.x / tiles, t = blockIdx.x % tiles, ty = t / btx, tx = t % btx;
  const int r0 = ty * kTH, c0 = tx * kTW;
  const long vsz = (long) Hv * Wv, msz = (long) p.P * vsz;
  const float* adj = p.adj + p.adj_off[s] + plane * vsz;
  // the unit adjoints at the valid positions r0 - 10 .. r0 + 15, c0 - 10 .. c0 + 31; zero outside the valid region
  for (int i = tid; i < kLH * kLW; i += kRgbBlock) {
    const int r = i / kLW, c = i % kLW, pr = r0 - kRgbReach + r, pc = c0 - kRgbReach + c;
    const bool in = pr >= 0 && pr < Hv && pc >= 0 && pc < Wv;
    const long e = (long) pr * Wv + pc;
#pragma unroll
    for (int m = 0; m < 3; ++m) sa[m][r][c] = in ? adj[m * msz + e] : 0.0f;
  }
  __syncthreads();
  for (int i = tid; i < kLH * kTW; i += kRgbBlock) {
    const int r = i / kTW, c = i % kTW;
    double a[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int k = 0; k < kRgbTaps; ++k) {
      const double w = p.w[k];
#pragma unroll
      for (int m = 0; m < 3; ++m) a[m] = __builtin_fma(w, (double) sa[m][r][c + k], a[m]);
    }
#pragma unroll
    for (int m = 0; m < 3; ++m) hb[m][r][c] = a[m];
  }
  __syncthreads();
  const long psz = (long) Hs * Ws;
  const float* xs = s == 0 ? p.x0 : p.pyr + p.pyr_off[s];
  const float* ys = s == 0 ? p.y0 : xs + (long) p.P * psz;
  const double fac = p.fac[(plane / p.C) * kRgbScales + s];
#pragma unroll
  for (int o = 0; o < 2; ++o) {
    const int r = (tid >> 5) + o * (kTH / 2), c = tid & 31, gr = r0 + r, gc = c0 + c;
    if (gr >= Hs || gc >= Ws) continue;
    double a[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int k = 0; k < kRgbTaps; ++k) {
      const double w = p.w[k];
#pragma unroll
      for (int m = 0; m < 3; ++m) a[m] = __builtin_fma(w, hb[m][r + k][c], a[m]);
    }
    const long e = plane * psz + (long) gr * Ws + gc;
    const double x = xs[e], y = ys[e];
    double g = fac * ((a[0] + (2.0 * x) * a[1]) + y * a[2]);
    if (s < kRgbScales - 1) {
      const int Hn = p.H[s + 1], Wn = p.W[s + 1];
      if ((gr >> 1) < Hn && (gc >> 1) < Wn)
        g += 0.25 * (double) p.gco[p.g_off[s + 1] + (long) plane * Hn * Wn + (long) (gr >> 1) * Wn + (gc >> 1)];
    }
    if (s == 0) {
      const double d = x - y;
      g += (d >= 1.0 ? 1.0 : d <= -1.0 ? -1.0 : d) / ((double) p.P * psz);
      p.grad[e] = (float) ((double) p.grad_loss[0] * g);
    } else {
      p.gco[p.g_off[s] + e] = (float) g;
    }
  }
}

// ---------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------
static_assert(sizeof(VampRgbLossDesc) == 28, "VampRgbLossDesc layout: part of the ABI (the binding reads it from include/vampire_hip.h)");
static_assert(sizeof(RgbParams) <= 4096, "kernel arguments");

int rgb_validate(const VampRgbLossDesc* d) {
  VAMP_REQUIRE(d, "desc is NULL");
  VAMP_REQUIRE(d->N >= 1, "N must be positive");
  VAMP_REQUIRE(d->C >= 1 && d->C <= 4, "C must be in [1, 4]");
  VAMP_REQUIRE(d->H >= kRgbMinSide && d->W >= kRgbMinSide, "H, W must be at least 176");
  VAMP_REQUIRE(d->H <= kRgbMaxSide && d->W <= kRgbMaxSide, "H, W must be at most 16384");
  VAMP_REQUIRE((long) d->N * d->C * d->H * d->W < (1L << 31), "N * C * H * W must be below 2^31");
  VAMP_REQUIRE(std::isfinite(d->data_range) && d->data_range > 0.0f, "data_range must be positive and finite");
  VAMP_REQUIRE(std::isfinite(d->k1) && d->k1 > 0.0f && std::isfinite(d->k2) && d->k2 > 0.0f,
               "k1, k2 must be positive and finite");
  return VAMP_OK;
}

// the shapes of *q, and its regions carved from `workspace` (NULL: only the size, which is returned, is of use)
size_t rgb_params(const VampRgbLossDesc* d, RgbParams* q, void* workspace) {
  q->N = d->N; q->C = d->C; q->P = d->N * d->C;
  const long P = q->P;
  long npart = 0, npyr = 0, nadj = 0, ng = 0;
  int h = d->H, w = d->W;
  for (int s = 0; s < kRgbScales; ++s) {
    q->H[s] = h; q->W[s] = w;
    const long hv = h - kRgbReach, wv = w - kRgbReach;
    q->tx[s] = (int) ((wv + kTW - 1) / kTW);
    q->ty[s] = (int) ((hv + kTH - 1) / kTH);
    q->part_off[s] = npart;
    npart += P * q->tx[s] * q->ty[s];
    q->adj_off[s] = nadj;
    nadj += 3 * P * hv * wv;
    q->pyr_off[s] = npyr;
    q->g_off[s] = ng;
    if (s > 0) {
      npyr += 2 * P * h * w;
      ng += P * h * w;
    }
    h /= 2; w /= 2;
  }
  q->part_off[kRgbScales] = npart;
  npart += P * q->tx[0] * q->ty[0];
  const double c1 = (double) d->k1 * d->data_range, c2 = (double) d->k2 * d->data_range;
  q->c1 = (float) (c1 * c1);
  q->c2 = (float) (c2 * c2);
  double sum = 0.0;
  for (int k = 0; k < kRgbTaps; ++k) {
    const double a = k - (kRgbTaps - 1) / 2.0;
    q->w[k] = std::exp(-(a * a) / (2.0 * 1.5 * 1.5));
    sum += q->w[k];
  }
  for (int k = 0; k < kRgbTaps; ++k) q->w[k] /= sum;
  Carve c(workspace);
  q->part = c.take<double>((size_t) npart);
  q->vd = c.take<double>((size_t) d->N * kRgbScales);
  q->fac = c.take<double>((size_t) d->N * kRgbScales);
  q->prodn = c.take<double>((size_t) d->N);
  q->pyr = c.take<float>((size_t) npyr);
  q->adj = c.take<float>((size_t) nadj);
  q->gco = c.take<float>((size_t) ng);
  return c.off;
}

}  // namespace
}  // namespace vamp

using namespace vamp;

extern "C" {

size_t vamp_rgb_loss_workspace_bytes(const VampRgbLossDesc* d) {
  if (rgb_validate(d)) return 0;
  RgbParams q{};
  return rgb_params(d, &q, nullptr);
}

int vamp_rgb_loss_forward(const VampRgbLossDesc* d, const float* pred, const float* target, float* loss, float* terms,
                          float* vals, void* workspace, size_t workspace_bytes, void* stream) {
  if (int e = rgb_validate(d)) return e;
  if (!pred || !target || !loss || !terms || !vals)
    return fail(VAMP_ENOSPC, "%s: an input or output pointer is NULL", __func__);
  RgbParams q{};
  if (int e = workspace_fits(__func__, workspace, workspace_bytes, rgb_params(d, &q, workspace))) return e;
  if (!aligned(workspace, 8))
    return fail(VAMP_ENOSPC, "%s: the workspace must be 8-byte aligned", __func__);
  q.x0 = pred; q.y0 = target; q.loss = loss; q.terms = terms; q.vals = vals;
  hipStream_t st = static_cast<hipStream_t>(stream);
  for (int s = 0; s < kRgbScales; ++s) {
    const int grid = q.P * q.tx[s] * q.ty[s];
    VAMP_TIMED(kProfAux, st, (rgb_fwd_kernel<<<grid, kRgbBlock, 0, st>>>(q, s)));
  }
  VAMP_TIMED(kProfAux, st, (rgb_finish_kernel<<<1, kRgbBlock, 0, st>>>(q)));
  return check_launch("rgb_loss_forward");
}

int vamp_rgb_loss_backward(const VampRgbLossDesc* d, const float* pred, const float* target, const float* grad_loss,
                           float* grad_pred, void* workspace, size_t workspace_bytes, void* stream) {
  if (int e = rgb_validate(d)) return e;
  if (!pred || !target || !grad_loss || !grad_pred)
    return fail(VAMP_ENOSPC, "%s: an input or output pointer is NULL", __func__);
  RgbParams q{};
  if (int e = workspace_fits(__func__, workspace, workspace_bytes, rgb_params(d, &q, workspace))) return e;
  if (!aligned(workspace, 8))
    return fail(VAMP_ENOSPC, "%s: the workspace must be 8-byte aligned", __func__);
  q.x0 = pred; q.y0 = target; q.grad_loss = grad_loss; q.grad = grad_pred;
  hipStream_t st = static_cast<hipStream_t>(stream);
  for (int s = kRgbScales - 1; s >= 0; --s) {
    const int btx = (q.W[s] + kTW - 1) / kTW, bty = (q.H[s] + kTH - 1) / kTH;
    VAMP_TIMED(kProfAux, st, (rgb_bwd_kernel<<<q.P * btx * bty, kRgbBlock, 0, st>>>(q, s, btx, bty)));
  }
  return check_launch("rgb_loss_backward");
}

}  // extern "C"
