// Detection post-processing on the device: the reference head's get_bboxes (bev_depth_head.py:381-494) --
// sigmoid, top-K, box decode, score / centre filters, circle / size-aware-circle / rotated-IoU NMS, the task
// merge -- for every task of a head and every sample in four launches that never synchronise with the host:
//
//  (a) det_select_kernel, one 1024-lane workgroup per (sample, task): the score of every heatmap element is
//      mapped to an order-preserving uint32 key (stored to the workspace, L2-resident), the K-th largest key
//      is found by an 11 + 11 + 10-bit radix select over LDS histograms, the keys above it and the
//      lowest-index keys equal to it are gathered by a block scan over contiguous per-lane chunks, and at
//      most 1024 (key, ~index) pairs are bitonic-sorted in LDS: score descending, index ascending.  The
//      sorted candidates are decoded, filtered and compacted into the workspace.
//  (b) det_mask_kernel, one wave per (sample, task, row block, column block >= row block): 64-bit words of
//      the upper triangle of the K x K suppression matrix.  Rotated IoU first rejects pairs whose
//      circumscribed circles do not meet.
//  (c) det_scan_kernel, one wave per (sample, task): the greedy walk.  Only the word of the current 64-row
//      block is needed to decide its rows (scalar registers), the words of later blocks are ORed from the
//      kept rows, staged in LDS; the walk stops at post_max_size kept boxes.
//  (d) det_merge_kernel, one workgroup per sample: the kept rows of the tasks in task order, labels offset by
//      the earlier tasks' class counts, zero tail, counts.
// No atomics outside LDS histograms (integer counts), no host synchronisation: the output is a pure function
// of the inputs and the launches can be captured in a graph.
#include <algorithm>

#include "common.hpp"
#include "elem16.hpp"

namespace vamp {
namespace {

constexpr int kDetMaxT = 8;
constexpr int kDetMaxK = 1024;
constexpr int kDetMaxNcls = 4;
constexpr int kSelBlock = 1024;
constexpr int kMaxWords = kDetMaxK / 64;
constexpr int kRow = 12;               // candidate row: x y z dx dy dz rot vx vy score label pad (fp32 / int bits)

struct DetParams {
  VampDetTask task[kDetMaxT];
  int ncls[kDetMaxT], K[kDetMaxT], flag[kDetMaxT];
  float min_radius[kDetMaxT], thresh_scale[kDetMaxT], nms_thr[kDetMaxT];
  int B, T, H, W, P, pre_max, kind, has_vel, norm_bbox, use_thr, use_rng, cs;
  float thr, osf, vs0, vs1, pc0, pc1, rng[6];
  int KP, nblk;
  long nstride;                        // keys per (sample, task) row of the workspace
  uint32_t* keys;
  float* cand;
  int* ncand;
  uint64_t* masks;
  int* kept;
  int* nkept;
};

template <int DT>
__device__ __forceinline__ float ld(const void* p, long i) {
  if constexpr (DT == VAMP_F32) return static_cast<const float*>(p)[i];
  else if constexpr (DT == VAMP_BF16) return bf16_to_f32(static_cast<const uint16_t*>(p)[i]);
  else return f16_to_f32(static_cast<const uint16_t*>(p)[i]);
}
// a value torch computes in the input dtype (sigmoid, exp, atan2 of 16-bit tensors): rounded to it, widened back
template <int DT>
__device__ __forceinline__ float rnd(float f) {
  if constexpr (DT == VAMP_F32) return f;
  else if constexpr (DT == VAMP_BF16) return bf16_to_f32(f32_to_bf16_c10(f));
  else return f16_to_f32(f32_to_f16(f));
}

// aten's sigmoid: 1 / (1 + exp(-x)) in fp32 with the accurate expf, rounded to the input dtype
template <int DT>
__device__ __forceinline__ float score_of(float x) { return rnd<DT>(1.0f / (1.0f + expf(-x))); }

// order-preserving key: a larger float has a larger key, every NaN the largest (topk ranks a NaN first)
__device__ __forceinline__ uint32_t f2key(float f) {
  if (f != f) return 0xffffffffu;
  const uint32_t u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float key2f(uint32_t k) {
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

// exclusive scan of one int per lane over the whole workgroup; `tot` receives the sum.  Two LDS arrays of
// (blockDim / 64) ints; every lane must call it.
__device__ __forceinline__ int block_exscan(int v, int* wsum, int& tot) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, nw = blockDim.x >> 6;
  int x = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int y = __shfl_up(x, o, 64);
    if (lane >= o) x += y;
  }
  if (lane == 63) wsum[wid] = x;
  __syncthreads();
  if (wid == 0) {
    int w = lane < nw ? wsum[lane] : 0;
#pragma unroll
    for (int o = 1; o < 16; o <<= 1) {
      const int y = __shfl_up(w, o, 64);
      if (lane >= o) w += y;
    }
    if (lane < nw) wsum[kSelBlock / 64 + lane] = w;
  }
  __syncthreads();
  const int base = wid ? wsum[kSelBlock / 64 + wid - 1] : 0;
  tot = wsum[kSelBlock / 64 + nw - 1];
  __syncthreads();
  return base + x - v;
}

// LDS histogram add; a wave whose live lanes all fall into one bin (constant heatmap regions, the top digit of
// scores that share an exponent) adds the ballot's popcount once
__device__ __forceinline__ void hist_add(int* hist, bool live, int bin) {
  const uint64_t m = __ballot(live);
  if (!m) return;
  const int first = __ffsll((unsigned long long) m) - 1;
  const int b0 = __shfl(bin, first, 64);
  const uint64_t same = __ballot(live && bin == b0);
  if (same == m) {
    if ((int) (threadIdx.x & 63) == first) atomicAdd(&hist[b0], __popcll(m));
  } else if (live) {
    atomicAdd(&hist[bin], 1);
  }
}

// ---------------------------------------------------------------------------------------------------------
// (a) select + decode
// ---------------------------------------------------------------------------------------------------------
template <int DT>
__global__ void __launch_bounds__(kSelBlock) det_select_kernel(DetParams p) {
  __shared__ int hist[2048];
  __shared__ uint64_t cand[kDetMaxK];
  __shared__ int wsum[2 * kSelBlock / 64];
  __shared__ int sel[2];
  const int bt = blockIdx.x, b = bt / p.T, t = bt % p.T, tid = threadIdx.x;
  const int HW = p.H * p.W, ncls = p.ncls[t], N = ncls * HW, K = p.K[t];
  const VampDetTask& tk = p.task[t];
  const long hoff = (long) b * N;
  uint32_t* keys = p.keys + (long) bt * p.nstride;

  // radix select of the K-th largest key: digits [31:21], [20:10], [9:0]
  uint32_t prefix = 0, pmask = 0;
  int krem = K, gt = 0;
  for (int pass = 0; pass < 3; ++pass) {
    const int sh = pass == 0 ? 21 : (pass == 1 ? 10 : 0), nb = pass == 2 ? 1024 : 2048;
    for (int i = tid; i < nb; i += kSelBlock) hist[i] = 0;
    __syncthreads();
    for (int base = 0; base < N; base += kSelBlock) {
      const int i = base + tid;
      uint32_t k = 0;
      bool live = i < N;
      if (live) {
        if (pass == 0) {
          k = f2key(score_of<DT>(ld<DT>(tk.heatmap, hoff + i)));
          keys[i] = k;
        } else {
          k = keys[i];
        }
        live = (k & pmask) == prefix;
      }
      hist_add(hist, live, (int) ((k >> sh) & (uint32_t) (nb - 1)));
    }
    __syncthreads();
    // bins in descending key order: lane tid owns bins nb-1-2tid and nb-2-2tid (one bin when nb = 1024)
    const int per = nb / kSelBlock;
    const int b0 = nb - 1 - per * tid;
    const int c0 = hist[b0], c1 = per == 2 ? hist[b0 - 1] : 0;
    int tot;
    const int ex = block_exscan(c0 + c1, wsum, tot);
    if (ex < krem && ex + c0 >= krem) {
      sel[0] = b0;
      sel[1] = ex;
    } else if (per == 2 && ex + c0 < krem && ex + c0 + c1 >= krem) {
      sel[0] = b0 - 1;
      sel[1] = ex + c0;
    }
    __syncthreads();
    prefix |= (uint32_t) sel[0] << sh;
    pmask |= (uint32_t) (nb - 1) << sh;
    krem -= sel[1];
    gt += sel[1];
    __syncthreads();
  }
  const uint32_t kth = prefix;     // keys > kth: gt of them; the first krem keys == kth by index complete K

  // gather: contiguous chunks per lane, so that equal keys are taken by lowest index
  const int chunk = (N + kSelBlock - 1) / kSelBlock;
  const int lo = min(N, tid * chunk), hi = min(N, lo + chunk);
  int ngt = 0, neq = 0;
  for (int i = lo; i < hi; ++i) {
    const uint32_t k = keys[i];
    ngt += k > kth;
    neq += k == kth;
  }
  int tot;
  int pg = block_exscan(ngt, wsum, tot);
  int pe = block_exscan(neq, wsum, tot);
  int KS = 1;
  while (KS < K) KS <<= 1;
  for (int i = tid; i < KS; i += kSelBlock) cand[i] = 0;     // padding sorts last (real keys are >= 2^31)
  __syncthreads();
  for (int i = lo; i < hi; ++i) {
    const uint32_t k = keys[i];
    const uint64_t e = ((uint64_t) k << 32) | (uint32_t) ~(uint32_t) i;
    if (k > kth) {
      if (pg < K) cand[pg] = e;
      ++pg;
    } else if (k == kth) {
      if (pe < krem && gt + pe < K) cand[gt + pe] = e;
      ++pe;
    }
  }
  __syncthreads();
  // bitonic sort, descending: score descending, then index ascending
  for (int k = 2; k <= KS; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = tid; i < KS; i += kSelBlock) {
        const int ij = i ^ j;
        if (ij > i) {
          const uint64_t a = cand[i], c = cand[ij];
          if (((i & k) == 0) ? (a < c) : (a > c)) {
            cand[i] = c;
            cand[ij] = a;
          }
        }
      }
      __syncthreads();
    }
  }

  // decode (CenterPointBBoxCoder.decode's order of operations), filter, compact
  float row[kRow];
  bool keep = false;
  if (tid < K) {
    const uint64_t e = cand[tid];
    const uint32_t idx = ~(uint32_t) e;
    const float score = key2f((uint32_t) (e >> 32));
    const int cls = (int) (idx / (uint32_t) HW), cell = (int) (idx % (uint32_t) HW);
    const int ys = cell / p.W, xs = cell % p.W;
    const long c1 = (long) b * 2 * HW + cell, c3 = (long) b * 3 * HW + cell, c0 = (long) b * HW + cell;
    float x = (float) xs + ld<DT>(tk.reg, c1);
    float y = (float) ys + ld<DT>(tk.reg, c1 + HW);
    x = x * p.osf;
    x = x * p.vs0;
    x = x + p.pc0;
    y = y * p.osf;
    y = y * p.vs1;
    y = y + p.pc1;
    row[0] = x;
    row[1] = y;
    row[2] = ld<DT>(tk.height, c0);
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      const float v = ld<DT>(tk.dim, c3 + (long) d * HW);
      row[3 + d] = p.norm_bbox ? rnd<DT>(expf(v)) : v;
    }
    row[6] = rnd<DT>(atan2f(ld<DT>(tk.rot, c1), ld<DT>(tk.rot, c1 + HW)));
    row[7] = p.has_vel ? ld<DT>(tk.vel, c1) : 0.f;
    row[8] = p.has_vel ? ld<DT>(tk.vel, c1 + HW) : 0.f;
    row[9] = score;
    row[10] = __int_as_float(cls);
    row[11] = 0.f;
    keep = !p.use_thr || score > p.thr;
    if (p.use_rng)
      keep = keep && x >= p.rng[0] && y >= p.rng[1] && row[2] >= p.rng[2] && x <= p.rng[3] && y <= p.rng[4] &&
             row[2] <= p.rng[5];
  }
  int n;
  const int pos = block_exscan(keep ? 1 : 0, wsum, n);
  if (p.kind == VAMP_NMS_ROTATE) n = min(n, p.pre_max);
  if (keep && pos < n) {
    float* dst = p.cand + ((long) bt * p.KP + pos) * kRow;
#pragma unroll
    for (int c = 0; c < kRow; c += 4) *reinterpret_cast<float4*>(dst + c) = make_float4(row[c], row[c + 1], row[c + 2], row[c + 3]);
  }
  if (tid == 0) p.ncand[bt] = n;
}

// ---------------------------------------------------------------------------------------------------------
// (b) suppression masks
// ---------------------------------------------------------------------------------------------------------
struct BevBox {
  float x, y, dx, dy, yaw;
};

__device__ __forceinline__ float cross2(float ax, float ay, float bx, float by) { return ax * by - ay * bx; }

// twice the signed area contributed by the part of edge p -> q (of a counter-clockwise polygon) that lies inside
// the counter-clockwise rectangle with corners c[0..3] (Cyrus-Beck clip against its four edge lines).  An edge
// lying ON a rectangle edge counts when it runs the same way (strict = false: the first polygon's copy of a shared
// boundary) and never for the second polygon (strict = true), so a shared boundary is counted once.
__device__ __forceinline__ float clipped_edge(float px, float py, float qx, float qy, const float (&cx)[4],
                                              const float (&cy)[4], bool strict) {
  float t0 = 0.f, t1 = 1.f;
  const float dx = qx - px, dy = qy - py;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const float ex = cx[(e + 1) & 3] - cx[e], ey = cy[(e + 1) & 3] - cy[e];
    // inside: cross(edge, point - corner) >= 0
    const float num = cross2(ex, ey, px - cx[e], py - cy[e]);
    const float den = cross2(ex, ey, dx, dy);
    if (den == 0.f) {
      if (num < 0.f || (num == 0.f && (strict || ex * dx + ey * dy <= 0.f))) return 0.f;
    } else {
      const float tt = -num / den;
      if (den > 0.f) t0 = fmaxf(t0, tt);
      else t1 = fminf(t1, tt);
    }
  }
  if (!(t0 < t1)) return 0.f;
  const float ax = px + t0 * dx, ay = py + t0 * dy, bx = px + t1 * dx, by = py + t1 * dy;
  return cross2(ax, ay, bx, by);
}

__device__ __forceinline__ void corners(const BevBox& b, float ox, float oy, float (&cx)[4], float (&cy)[4]) {
  const float c = cosf(b.yaw), s = sinf(b.yaw), hx = b.dx * 0.5f, hy = b.dy * 0.5f;
  const float ux[4] = {-hx, hx, hx, -hx}, uy[4] = {-hy, -hy, hy, hy};
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    cx[k] = (b.x - ox) + (ux[k] * c - uy[k] * s);
    cy[k] = (b.y - oy) + (ux[k] * s + uy[k] * c);
  }
}

// IoU of two rotated BEV rectangles: intersection (the boundary integral of the clipped edges of both) over
// max(union, 1e-8).  Coordinates relative to the smaller box's centre, near which every intersection vertex lies.
__device__ float rotated_iou(BevBox a, BevBox b) {
  if (!(a.dx > 0.f && a.dy > 0.f && b.dx > 0.f && b.dy > 0.f)) return 0.f;
  const float ddx = a.x - b.x, ddy = a.y - b.y;
  const float ra = a.dx * a.dx + a.dy * a.dy, rb = b.dx * b.dx + b.dy * b.dy;     // (2 r)^2
  const float rs = 0.5f * (sqrtf(ra) + sqrtf(rb));
  if (ddx * ddx + ddy * ddy > rs * rs) return 0.f;                                 // circumscribed circles apart
  const float area_a = a.dx * a.dy, area_b = b.dx * b.dy;
  const BevBox& o = area_a <= area_b ? a : b;
  float ax[4], ay[4], bx[4], by[4];
  corners(a, o.x, o.y, ax, ay);
  corners(b, o.x, o.y, bx, by);
  float twice = 0.f;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    twice += clipped_edge(ax[e], ay[e], ax[(e + 1) & 3], ay[(e + 1) & 3], bx, by, false);
    twice += clipped_edge(bx[e], by[e], bx[(e + 1) & 3], by[(e + 1) & 3], ax, ay, true);
  }
  const float inter = fmaxf(0.5f * twice, 0.f);
  return inter / fmaxf(area_a + area_b - inter, 1e-8f);
}

__global__ void __launch_bounds__(64) det_mask_kernel(DetParams p) {
  __shared__ float col[64][6];
  const int nb = p.nblk, per = nb * nb;
  const int bt = blockIdx.x / per, rb = (blockIdx.x % per) / nb, cb = blockIdx.x % nb, lane = threadIdx.x;
  const int n = p.ncand[bt];
  if (cb < rb || rb * 64 >= n || cb * 64 >= n) return;
  const int t = bt % p.T, i = rb * 64 + lane, j0 = cb * 64;
  const float* base = p.cand + (long) bt * p.KP * kRow;
  {
    const float* r = base + (long) (j0 + lane) * kRow;
    col[lane][0] = r[0];
    col[lane][1] = r[1];
    col[lane][2] = r[3];
    col[lane][3] = r[4];
    col[lane][4] = r[6];
  }
  __syncthreads();
  const float* r = base + (long) i * kRow;
  const BevBox bi{r[0], r[1], r[3], r[4], r[6]};
  uint64_t word = 0;
  if (i < n) {
    const int jn = min(64, n - j0);
    if (p.kind == VAMP_NMS_CIRCLE) {
      const float thr = p.min_radius[t];
      for (int k = 0; k < jn; ++k) {
        const float dx = col[k][0] - bi.x, dy = col[k][1] - bi.y;
        const float d2 = dx * dx + dy * dy;
        if (j0 + k > i && d2 <= thr) word |= 1ull << k;
      }
    } else if (p.kind == VAMP_NMS_SIZE_AWARE) {
      const float ts = p.thresh_scale[t];
      const float ci = fabsf(cosf(bi.yaw)), si = fabsf(sinf(bi.yaw));
      const float exi = bi.dx * ci + bi.dy * si, eyi = bi.dx * si + bi.dy * ci;
      for (int k = 0; k < jn; ++k) {
        const float cj = fabsf(cosf(col[k][4])), sj = fabsf(sinf(col[k][4]));
        const float exj = col[k][2] * cj + col[k][3] * sj, eyj = col[k][2] * sj + col[k][3] * cj;
        const bool close = fabsf(col[k][0] - bi.x) <= (exj + exi) * ts / 2.0f &&
                           fabsf(col[k][1] - bi.y) <= (eyj + eyi) * ts / 2.0f;
        if (j0 + k > i && close) word |= 1ull << k;
      }
    } else {
      const float thr = p.nms_thr[t];
      for (int k = 0; k < jn; ++k) {
        if (j0 + k <= i) continue;
        const BevBox bj{col[k][0], col[k][1], col[k][2], col[k][3], col[k][4]};
        if (rotated_iou(bi, bj) > thr) word |= 1ull << k;
      }
    }
  }
  p.masks[((long) bt * p.KP + i) * kMaxWords + cb] = word;
}

// ---------------------------------------------------------------------------------------------------------
// (c) greedy scan, one wave per (sample, task)
// ---------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint64_t readlane64(uint64_t v, int l) {
  const uint32_t lo = __builtin_amdgcn_readlane((int) (uint32_t) v, l);
  const uint32_t hi = __builtin_amdgcn_readlane((int) (uint32_t) (v >> 32), l);
  return ((uint64_t) hi << 32) | lo;
}

__global__ void __launch_bounds__(64) det_scan_kernel(DetParams p) {
  __shared__ uint64_t rows[64][kMaxWords];
  const int bt = blockIdx.x, lane = threadIdx.x;
  const int n = p.ncand[bt], nw = (n + 63) >> 6, P = p.P;
  const uint64_t* m = p.masks + (long) bt * p.KP * kMaxWords;
  int* kept = p.kept + (long) bt * P;
  uint64_t rem = 0;                    // lane w < nw: removed bits of candidates 64 w .. 64 w + 63
  int c = 0;
  for (int bi = 0; bi < nw && c < P; ++bi) {
    const int r = bi * 64 + lane;
    uint64_t diag = 0;
    for (int w = bi; w < nw; ++w) {
      const uint64_t v = r < n ? m[(long) r * kMaxWords + w] : 0;
      rows[lane][w] = v;
      if (w == bi) diag = v;
    }
    uint64_t cur = readlane64(rem, bi), keepm = 0;
    const int rn = min(64, n - bi * 64);
    for (int k = 0; k < rn && c < P; ++k) {
      if ((cur >> k) & 1) continue;
      keepm |= 1ull << k;
      cur |= readlane64(diag, k);
      if (lane == 0) kept[c] = bi * 64 + k;
      ++c;
    }
    __syncthreads();
    while (keepm) {
      const int k = __ffsll((unsigned long long) keepm) - 1;
      keepm &= keepm - 1;
      if (lane > bi && lane < nw) rem |= rows[k][lane];
    }
    __syncthreads();
  }
  if (lane == 0) p.nkept[bt] = c;
}

// ---------------------------------------------------------------------------------------------------------
// (d) merge over tasks
// ---------------------------------------------------------------------------------------------------------
template <int DT>
__global__ void __launch_bounds__(256) det_merge_kernel(DetParams p, float* __restrict__ boxes, void* __restrict__ scores,
                                                        int* __restrict__ labels, int* __restrict__ counts) {
  const int b = blockIdx.x, T = p.T, P = p.P, rows = T * P, cs = p.cs;
  int total = 0;
  for (int t = 0; t < T; ++t) total += p.nkept[b * T + t];
  if (threadIdx.x == 0) counts[b] = total;
  for (int r = threadIdx.x; r < rows; r += blockDim.x) {
    float v[kRow];
#pragma unroll
    for (int c = 0; c < kRow; ++c) v[c] = 0.f;
    int label = 0;
    if (r < total) {
      int t = 0, k = r;
      for (int nk = p.nkept[b * T]; k >= nk; nk = p.nkept[b * T + t]) {
        k -= nk;
        ++t;
      }
      const int bt = b * T + t;
      const int ci = p.kept[(long) bt * P + k];
      const float* src = p.cand + ((long) bt * p.KP + ci) * kRow;
#pragma unroll
      for (int c = 0; c < kRow; ++c) v[c] = src[c];
      label = __float_as_int(v[10]) + p.flag[t];
    }
    float* dst = boxes + ((long) b * rows + r) * cs;
#pragma unroll
    for (int c = 0; c < 9; ++c)
      if (c < cs) dst[c] = v[c];
    const long si = (long) b * rows + r;
    if constexpr (DT == VAMP_F32) static_cast<float*>(scores)[si] = v[9];
    else if constexpr (DT == VAMP_BF16) static_cast<uint16_t*>(scores)[si] = f32_to_bf16_c10(v[9]);
    else static_cast<uint16_t*>(scores)[si] = f32_to_f16(v[9]);
    labels[si] = label;
  }
}

// ---------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------
static_assert(sizeof(VampDetDesc) == 58 * 4, "VampDetDesc layout: part of the ABI (the binding reads it from include/vampire_hip.h)");

int det_validate(const VampDetDesc* d) {
  VAMP_REQUIRE(d, "desc is NULL");
  VAMP_REQUIRE(d->B >= 1 && d->B <= (1 << 20), "B must be in [1, 2^20]");
  VAMP_REQUIRE(d->T >= 1 && d->T <= kDetMaxT, "T must be in [1, 8]");
  VAMP_REQUIRE(d->H >= 1 && d->W >= 1, "H, W must be positive");
  VAMP_REQUIRE(d->in_dtype == VAMP_F32 || d->in_dtype == VAMP_BF16 || d->in_dtype == VAMP_F16,
               "in_dtype must be VAMP_F32, VAMP_BF16 or VAMP_F16");
  VAMP_REQUIRE(d->nms_kind == VAMP_NMS_CIRCLE || d->nms_kind == VAMP_NMS_SIZE_AWARE || d->nms_kind == VAMP_NMS_ROTATE,
               "unknown nms_kind");
  VAMP_REQUIRE(d->max_num >= 1, "max_num must be positive");
  VAMP_REQUIRE(d->post_max_size >= 1 && d->post_max_size <= d->max_num, "post_max_size must be in [1, max_num]");
  VAMP_REQUIRE(d->nms_kind != VAMP_NMS_ROTATE || d->pre_max_size >= 1, "pre_max_size must be positive");
  VAMP_REQUIRE(d->has_vel == 0 || d->has_vel == 1, "has_vel must be 0 or 1");
  VAMP_REQUIRE(d->reserved == 0, "reserved must be 0");
  for (int t = 0; t < d->T; ++t) {
    VAMP_REQUIRE(d->ncls[t] >= 1 && d->ncls[t] <= kDetMaxNcls, "ncls must be in [1, 4]");
    const long N = (long) d->ncls[t] * d->H * d->W;
    VAMP_REQUIRE(N < 0x7fffffffL, "ncls * H * W must be below 2^31");
    VAMP_REQUIRE(std::min<long>(d->max_num, N) <= kDetMaxK, "K = min(max_num, ncls * H * W) must be <= 1024");
  }
  return VAMP_OK;
}

// the padded counts of *q and its regions carved from `workspace` (NULL: only the size, which is returned, is of use)
size_t det_workspace(const VampDetDesc* d, DetParams* q, void* workspace) {
  long nmax = 0, kmax = 0;
  for (int t = 0; t < d->T; ++t) {
    const long N = (long) d->ncls[t] * d->H * d->W;
    nmax = std::max(nmax, N);
    kmax = std::max(kmax, std::min<long>(d->max_num, N));
  }
  const size_t BT = (size_t) d->B * d->T;
  q->nstride = (long) align_up(nmax, 64);
  q->KP = (int) align_up(kmax, 64);
  q->nblk = q->KP / 64;
  Carve c(workspace);
  q->keys = c.take<uint32_t>(BT * q->nstride);
  q->cand = c.take<float>(BT * q->KP * kRow);
  q->ncand = c.take<int>(BT);
  q->masks = c.take<uint64_t>(BT * q->KP * kMaxWords);
  q->kept = c.take<int>(BT * d->post_max_size);
  q->nkept = c.take<int>(BT);
  return c.off;
}

template <int DT>
void det_launch(const DetParams& q, float* boxes, void* scores, int* labels, int* counts, hipStream_t s) {
  const int BT = q.B * q.T;
  VAMP_TIMED(kProfAux, s, (det_select_kernel<DT><<<BT, kSelBlock, 0, s>>>(q)));
  VAMP_TIMED(kProfAux, s, (det_mask_kernel<<<BT * q.nblk * q.nblk, 64, 0, s>>>(q)));
  VAMP_TIMED(kProfAux, s, (det_scan_kernel<<<BT, 64, 0, s>>>(q)));
  VAMP_TIMED(kProfAux, s, (det_merge_kernel<DT><<<q.B, 256, 0, s>>>(q, boxes, scores, labels, counts)));
}

}  // namespace
}  // namespace vamp

using namespace vamp;

extern "C" {

size_t vamp_det_workspace_bytes(const VampDetDesc* d) {
  if (det_validate(d)) return 0;
  DetParams q{};
  return det_workspace(d, &q, nullptr);
}

int vamp_det_postprocess(const VampDetDesc* d, const VampDetTask* tasks, float* boxes, void* scores, int32_t* labels,
                         int32_t* counts, void* workspace, size_t workspace_bytes, void* stream) {
  if (int e = det_validate(d)) return e;
  VAMP_REQUIRE(tasks, "tasks is NULL");
  for (int t = 0; t < d->T; ++t) {
    const VampDetTask& k = tasks[t];
    VAMP_REQUIRE(k.heatmap && k.reg && k.height && k.dim && k.rot, "a task's head pointer is NULL");
    VAMP_REQUIRE(!d->has_vel || k.vel, "has_vel is set but a task's vel is NULL");
  }
  VAMP_REQUIRE(boxes && scores && labels && counts, "an output pointer is NULL");
  DetParams q{};
  if (int e = workspace_fits(__func__, workspace, workspace_bytes, det_workspace(d, &q, workspace))) return e;
  int flag = 0;
  for (int t = 0; t < d->T; ++t) {
    q.task[t] = tasks[t];
    q.ncls[t] = d->ncls[t];
    q.K[t] = (int) std::min<long>(d->max_num, (long) d->ncls[t] * d->H * d->W);
    q.flag[t] = flag;
    flag += d->ncls[t];
    q.min_radius[t] = d->min_radius[t];
    q.thresh_scale[t] = d->thresh_scale[t];
    q.nms_thr[t] = d->nms_thr[t];
  }
  q.B = d->B; q.T = d->T; q.H = d->H; q.W = d->W;
  q.P = d->post_max_size; q.pre_max = d->pre_max_size; q.kind = d->nms_kind;
  q.has_vel = d->has_vel; q.norm_bbox = d->norm_bbox != 0;
  q.use_thr = d->use_score_threshold != 0; q.use_rng = d->use_center_range != 0;
  q.cs = d->has_vel ? 9 : 7;
  q.thr = d->score_threshold; q.osf = d->out_size_factor;
  q.vs0 = d->voxel_size[0]; q.vs1 = d->voxel_size[1]; q.pc0 = d->pc_range[0]; q.pc1 = d->pc_range[1];
  for (int i = 0; i < 6; ++i) q.rng[i] = d->post_center_range[i];
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (d->in_dtype == VAMP_F32) det_launch<VAMP_F32>(q, boxes, scores, labels, counts, s);
  else if (d->in_dtype == VAMP_BF16) det_launch<VAMP_BF16>(q, boxes, scores, labels, counts, s);
  else det_launch<VAMP_F16>(q, boxes, scores, labels, counts, s);
  return check_launch("det_postprocess");
}

}  // extern "C"
