// Segmentation loss on the device: w_ce * cross-entropy + w_lv * Lovasz-softmax ('present' classes) of logits [P, C]
// against integer labels under an optional mask (base_exp.py:519-575 -- the four `_ce_lovasz(x[mask], y[mask])` of the
// training step; lovasz_losses.py:171-199 `lovasz_softmax_flat`, restated in multitask.lovasz_softmax), forward and
// gradient with respect to the logits, without compaction, without a host synchronisation, without float atomics and
// with bitwise repeatable results.  An element is VALID when its mask byte is set (or there is no mask) and its label
// lies in [0, C); n = number of valid elements, P = B * S all elements, T = ceil(P / 2048) tiles.
//
//  rows      seg_row_kernel, one lane per element.  Softmax in fp32 (max, sum of expf, e / sum; three passes over the
//            row, no register array), err[c] = |[label == c] - p[c]|, and per class the sort record of the element:
//            key = kInvalid - (bits(err) + 1) for a valid element, kInvalid for the others, payload = element index
//            with the foreground flag in bit 31.  bits(err) is monotonic on [0, 1], so an ascending stable sort of the
//            key is err descending with equal errors by ascending element index, and every invalid element behind
//            every valid one (a valid err of exactly 0 has key kInvalid - 1).  Records are class-major [C, P].  The
//            workgroup stores its float64 partial of -log p[label] and its count of valid elements.
//  sort      per class a least-significant-digit radix sort of the (key, payload) records, four passes of 8 bits, three
//            launches each: seg_hist_kernel (LDS histogram of a 2048-record tile, stored digit-major [C, 256, T]),
//            seg_scan_kernel (one workgroup per class, exclusive scan of the 256 T counters in place) and
//            seg_scatter_kernel (a tile again; a wave takes 64 consecutive records per round, equal digits found with
//            eight ballots, rank = earlier records of the wave's earlier rounds + lower lanes with the digit; the four
//            waves' counts are stacked in wave order behind the tile's offset: stable).
//  jaccard   seg_fg_kernel counts the foreground records of every tile of the sorted order, seg_scan_kernel turns the
//            counts of a class into exclusive prefixes and the total G, and seg_jaccard_kernel walks a tile: cum = the
//            inclusive foreground count at the 1-based position k, I = G - cum, U = G + k - cum, and the Jaccard step
//            in float64 from the integers, without a difference of quotients:
//                foreground  delta = 1 / U          background  delta = I / ((U - 1) U)        (U_{k-1} = U_k - 1 there)
//            The tile's float64 partial of err * delta is stored, and the element's UNIT gradient d LV_c / d p[i, c] =
//            -sign(d) delta (sign(d) = +1 foreground, -1 background, 0 where err is exactly 0; 0 for a class without
//            foreground) goes to ug[c, i].  That array (4 bytes per element and class) is all the backward keeps; the
//            sort's double buffers are forward scratch.  The optional sorted_err / perm rows are written here.
//  finish    seg_finish_kernel, one workgroup: n, the CE partials and every class's tile partials in index order,
//            n_present = classes with G > 0, terms = (CE, LV), loss = w_ce CE + w_lv LV; n = 0 gives exactly 0 for all.
//  backward  seg_bwd_kernel, one lane per element: softmax again, dot = sum_k p[k] ug[k], and in float64
//                g[c] = grad_loss (w_ce (p[c] - fg[c]) / n + w_lv p[c] (ug[c] - dot) / n_present),
//            written once; invalid elements get exactly 0.
// Every grid depends on the shapes only; sixteen launches forward, one backward.  Nothing needs initialisation.
#include <cmath>

#include "common.hpp"
#include "wave_reduce.hpp"

namespace vamp {
namespace {

constexpr int kSegBlock = 256;
constexpr int kSegWaves = kSegBlock / 64;
constexpr int kSegItems = 8;
constexpr int kSegTile = kSegBlock * kSegItems;      // 2048 records of one class
constexpr int kSegRadix = 256;
constexpr int kSegPasses = 4;                        // 4 x 8 bits: the whole key
constexpr int kSegScanBlock = 1024;
constexpr int kSegScanItems = 16;
constexpr uint32_t kSegInvalid = 0x3F800001u;        // bits(1.0f) + 1: the largest key of a valid element, reversed to 0
constexpr int kSegMaxC = 32;
constexpr int kSegHdrInts = 64;                      // kept header: n, n_present, G[32]

struct SegParams {
  const float* logits;
  const void* labels;
  const uint8_t* mask;
  const float* grad_loss;
  float* grad;
  float* loss;
  float* terms;
  int* counts;
  float* sorted_err;
  int* perm;
  uint32_t* key[2];
  uint32_t* pay[2];
  int* hist;                                         // [C, 256, T]
  int* tilefg;                                       // [C, T]
  int* rowcnt;                                       // [nrow]
  double* cepart;                                    // [nrow]
  double* lvpart;                                    // [C, T]
  int* hdr;                                          // kept: n, n_present, G[c]
  float* ug;                                         // kept: [C, P]
  long P, S;
  int C, T, nrow, layout, label_dtype;
  float w_ce, w_lv;
};

__device__ __forceinline__ long seg_label(const void* l, int dt, long i) {
  if (dt == VAMP_I64) return static_cast<const int64_t*>(l)[i];
  if (dt == VAMP_I32) return static_cast<const int32_t*>(l)[i];
  return static_cast<const uint8_t*>(l)[i];
}

__device__ __forceinline__ bool seg_valid(const SegParams& p, long i, long* lab) {
  *lab = seg_label(p.labels, p.label_dtype, i);
  return (!p.mask || p.mask[i] != 0) && *lab >= 0 && *lab < p.C;
}

// logit c of element i is x[c * stride]
__device__ __forceinline__ long seg_row(const SegParams& p, long i, long* stride) {
  if (p.layout == VAMP_SEG_ROWS) {
    *stride = 1;
    return i * p.C;
  }
  *stride = p.S;
  return (i / p.S) * p.C * p.S + i % p.S;
}

// the row's maximum and the fp32 sum of expf(x - m) in class order; p[c] = expf(x[c] - m) / sum
__device__ __forceinline__ void seg_softmax_stats(const float* x, long stride, int C, float* m, float* sum) {
  float mx = x[0];
  for (int c = 1; c < C; ++c) mx = fmaxf(mx, x[c * stride]);
  float s = 0.0f;
  for (int c = 0; c < C; ++c) s += expf(x[c * stride] - mx);
  *m = mx;
  *sum = s;
}

// ---------------------------------------------------------------------------------------------------------
// rows
// ---------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kSegBlock) seg_row_kernel(SegParams p) {
  __shared__ double red[kSegWaves];
  __shared__ int redi[kSegWaves];
  const long i = (long) blockIdx.x * kSegBlock + threadIdx.x;
  double ce = 0.0;
  int nv = 0;
  if (i < p.P) {
    long lab;
    if (seg_valid(p, i, &lab)) {
      long stride;
      const float* x = p.logits + seg_row(p, i, &stride);
      float m, sum;
      seg_softmax_stats(x, stride, p.C, &m, &sum);
      double sumd = 0.0;
      for (int c = 0; c < p.C; ++c) {
        const float e = expf(x[c * stride] - m);
        const float pc = e / sum;
        const bool fg = c == lab;
        const float err = fabsf((fg ? 1.0f : 0.0f) - pc);
        p.key[0][c * p.P + i] = kSegInvalid - (__float_as_uint(err) + 1u);
        p.pay[0][c * p.P + i] = (uint32_t) i | (fg ? 0x80000000u : 0u);
        sumd += (double) e;
      }
      ce = log(sumd) - ((double) x[lab * stride] - (double) m);
      nv = 1;
    } else {
      for (int c = 0; c < p.C; ++c) {
        p.key[0][c * p.P + i] = kSegInvalid;
        p.pay[0][c * p.P + i] = (uint32_t) i;
      }
    }
  }
  const double tot = block_sum<kSegWaves>(ce, red);
  const int cnt = block_sum<kSegWaves>(nv, redi);
  if (threadIdx.x == 0) {
    p.cepart[blockIdx.x] = tot;
    p.rowcnt[blockIdx.x] = cnt;
  }
}

// ---------------------------------------------------------------------------------------------------------
// sort
// ---------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kSegBlock) seg_hist_kernel(SegParams p, int src, int shift) {
  __shared__ int bins[kSegRadix];
  const int t = blockIdx.x, c = blockIdx.y, tid = threadIdx.x;
  bins[tid] = 0;
  __syncthreads();
  const uint32_t* k = p.key[src] + c * p.P;
  const long base = (long) t * kSegTile;
#pragma unroll
  for (int r = 0; r < kSegItems; ++r) {
    const long pos = base + r * kSegBlock + tid;
    if (pos < p.P) atomicAdd(&bins[(k[pos] >> shift) & (kSegRadix - 1)], 1);
  }
  __syncthreads();
  p.hist[((long) c * kSegRadix + tid) * p.T + t] = bins[tid];
}

// exclusive scan in place of h[blockIdx.x * M .. + M); total[blockIdx.x] (when given) receives the sum
__global__ void __launch_bounds__(kSegScanBlock) seg_scan_kernel(int* hist, long M, int* total) {
  __shared__ int wsum[kSegScanBlock / 64];
  int* h = hist + blockIdx.x * M;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int carry = 0;
  for (long base = 0; base < M; base += (long) kSegScanBlock * kSegScanItems) {
    const long j0 = base + (long) tid * kSegScanItems;
    int v[kSegScanItems], s = 0;
#pragma unroll
    for (int q = 0; q < kSegScanItems; ++q) {
      v[q] = j0 + q < M ? h[j0 + q] : 0;
      s += v[q];
    }
    int inc = s;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int u = __shfl_up(inc, o, 64);
      if (lane >= o) inc += u;
    }
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    int wb = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < kSegScanBlock / 64; ++w) {
      wb += w < wave ? wsum[w] : 0;
      tot += wsum[w];
    }
    int ex = carry + wb + inc - s;
#pragma unroll
    for (int q = 0; q < kSegScanItems; ++q) {
      if (j0 + q < M) h[j0 + q] = ex;
      ex += v[q];
    }
    carry += tot;
    __syncthreads();
  }
  if (total && tid == 0) total[blockIdx.x] = carry;
}

__global__ void __launch_bounds__(kSegBlock) seg_scatter_kernel(SegParams p, int src, int shift) {
  __shared__ int wcnt[kSegWaves][kSegRadix];
  __shared__ int wbase[kSegWaves][kSegRadix];
  const int t = blockIdx.x, c = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
#pragma unroll
  for (int w = 0; w < kSegWaves; ++w) wcnt[w][tid] = 0;
  __syncthreads();
  const uint32_t* ks = p.key[src] + c * p.P;
  const uint32_t* vs = p.pay[src] + c * p.P;
  uint32_t* kd = p.key[src ^ 1] + c * p.P;
  uint32_t* vd = p.pay[src ^ 1] + c * p.P;
  const long base = (long) t * kSegTile + wave * (kSegItems * 64);
  const unsigned long long below = (1ull << lane) - 1ull;
  uint32_t k[kSegItems], v[kSegItems];
  int rk[kSegItems];
#pragma unroll
  for (int r = 0; r < kSegItems; ++r) {
    const long pos = base + r * 64 + lane;
    const bool in = pos < p.P;
    k[r] = in ? ks[pos] : 0u;
    v[r] = in ? vs[pos] : 0u;
    const int d = (k[r] >> shift) & (kSegRadix - 1);
    unsigned long long same = __ballot(in);
#pragma unroll
    for (int b = 0; b < 8; ++b) {
      const bool bit = (d >> b) & 1;
      const unsigned long long bal = __ballot(bit);
      same &= bit ? bal : ~bal;
    }
    // the wave's own row of counters: its lanes read before the digit's first lane adds the round's count
    int prior = 0;
    if (in) prior = wcnt[wave][d];
    rk[r] = prior + __popcll(same & below);
    __builtin_amdgcn_wave_barrier();
    if (in && (same & below) == 0ull) wcnt[wave][d] = prior + __popcll(same);
    __builtin_amdgcn_wave_barrier();
  }
  __syncthreads();
  {
    int run = p.hist[((long) c * kSegRadix + tid) * p.T + t];
#pragma unroll
    for (int w = 0; w < kSegWaves; ++w) {
      wbase[w][tid] = run;
      run += wcnt[w][tid];
    }
  }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < kSegItems; ++r) {
    const long pos = base + r * 64 + lane;
    if (pos >= p.P) continue;
    const int d = (k[r] >> shift) & (kSegRadix - 1);
    const long dst = (long) wbase[wave][d] + rk[r];
    if (dst >= 0 && dst < p.P) {                     // (always: the offsets come from the same records)
      kd[dst] = k[r];
      vd[dst] = v[r];
    }
  }
}

// ---------------------------------------------------------------------------------------------------------
// Jaccard steps over the sorted order
// ---------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kSegBlock) seg_fg_kernel(SegParams p) {
  __shared__ int redi[kSegWaves];
  const int t = blockIdx.x, c = blockIdx.y, tid = threadIdx.x;
  const uint32_t* vs = p.pay[0] + c * p.P;
  const long base = (long) t * kSegTile;
  int n = 0;
#pragma unroll
  for (int r = 0; r < kSegItems; ++r) {
    const long pos = base + r * kSegBlock + tid;
    if (pos < p.P) n += (int) (vs[pos] >> 31);
  }
  const int tot = block_sum<kSegWaves>(n, redi);
  if (tid == 0) p.tilefg[(long) c * p.T + t] = tot;
}

__global__ void __launch_bounds__(kSegBlock) seg_jaccard_kernel(SegParams p) {
  __shared__ double red[kSegWaves];
  __shared__ int wsum[kSegWaves];
  const int t = blockIdx.x, c = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint32_t* ks = p.key[0] + c * p.P;
  const uint32_t* vs = p.pay[0] + c * p.P;
  const long base = (long) t * kSegTile + (long) tid * kSegItems;
  const int G = p.hdr[2 + c];
  uint32_t k[kSegItems], v[kSegItems];
  int s = 0;
#pragma unroll
  for (int q = 0; q < kSegItems; ++q) {
    const bool in = base + q < p.P;
    k[q] = in ? ks[base + q] : kSegInvalid;
    v[q] = in ? vs[base + q] : 0u;
    s += (int) (v[q] >> 31);
  }
  int inc = s;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int u = __shfl_up(inc, o, 64);
    if (lane >= o) inc += u;
  }
  if (lane == 63) wsum[wave] = inc;
  __syncthreads();
  int cum = p.tilefg[(long) c * p.T + t] + inc - s;  // foreground records before this lane's first
  for (int w = 0; w < wave; ++w) cum += wsum[w];
  double acc = 0.0;
  float* ug = p.ug + c * p.P;
#pragma unroll
  for (int q = 0; q < kSegItems; ++q) {
    const long pos = base + q;
    if (pos >= p.P || k[q] == kSegInvalid) continue; // past the class's n valid records
    const bool fg = (v[q] >> 31) != 0;
    const long idx = v[q] & 0x7FFFFFFFu;
    cum += fg ? 1 : 0;
    const float err = __uint_as_float(kSegInvalid - k[q] - 1u);
    float u = 0.0f;
    if (G > 0) {
      const double U = (double) G + (double) (pos + 1) - (double) cum;
      const double delta = fg ? 1.0 / U : (double) (G - cum) / ((U - 1.0) * U);
      acc += (double) err * delta;
      if (err != 0.0f) u = fg ? -(float) delta : (float) delta;
    }
    if (idx < p.P) ug[idx] = u;
    if (p.sorted_err) p.sorted_err[c * p.P + pos] = err;
    if (p.perm) p.perm[c * p.P + pos] = (int) idx;
  }
  const double tot = block_sum<kSegWaves>(acc, red);
  if (tid == 0) p.lvpart[(long) c * p.T + t] = tot;
}

__global__ void __launch_bounds__(kSegBlock) seg_finish_kernel(SegParams p) {
  __shared__ double red[kSegWaves];
  __shared__ int redi[kSegWaves];
  __shared__ double cls[kSegMaxC];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  int nv = 0;
  double ce = 0.0;
  for (int j = tid; j < p.nrow; j += kSegBlock) {
    nv += p.rowcnt[j];
    ce += p.cepart[j];
  }
  const int n = block_sum<kSegWaves>(nv, redi);
  const double ces = block_sum<kSegWaves>(ce, red);
  for (int c = wave; c < p.C; c += kSegWaves) {
    const double* q = p.lvpart + (long) c * p.T;
    double a = 0.0;
    for (int j = lane; j < p.T; j += 64) a += q[j];
    a = wave_sum(a);
    if (lane == 0) cls[c] = a;
  }
  __syncthreads();
  if (tid == 0) {
    int present = 0;
    double lv = 0.0;
    for (int c = 0; c < p.C; ++c)
      if (p.hdr[2 + c] > 0) {
        ++present;
        lv += cls[c];
      }
    const double cem = n > 0 ? ces / (double) n : 0.0;
    const double lvm = n > 0 && present > 0 ? lv / (double) present : 0.0;
    p.terms[0] = (float) cem;
    p.terms[1] = (float) lvm;
    p.loss[0] = (float) ((double) p.w_ce * cem + (double) p.w_lv * lvm);
    p.counts[0] = n;
    p.counts[1] = n > 0 ? present : 0;
    p.hdr[0] = n;
    p.hdr[1] = n > 0 ? present : 0;
  }
}

// ---------------------------------------------------------------------------------------------------------
// backward
// ---------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kSegBlock) seg_bwd_kernel(SegParams p) {
  const long i = (long) blockIdx.x * kSegBlock + threadIdx.x;
  if (i >= p.P) return;
  long stride;
  const long off = seg_row(p, i, &stride);
  float* g = p.grad + off;
  long lab;
  const int n = p.hdr[0], present = p.hdr[1];
  if (n <= 0 || present <= 0 || !seg_valid(p, i, &lab)) {
    for (int c = 0; c < p.C; ++c) g[c * stride] = 0.0f;
    return;
  }
  const float* x = p.logits + off;
  const float* ug = p.ug + i;
  float m, sum;
  seg_softmax_stats(x, stride, p.C, &m, &sum);
  double dot = 0.0;
  for (int c = 0; c < p.C; ++c) dot += (double) (expf(x[c * stride] - m) / sum) * (double) ug[c * p.P];
  const double gl = (double) p.grad_loss[0];
  const double a = (double) p.w_ce / (double) n, b = (double) p.w_lv / (double) present;
  for (int c = 0; c < p.C; ++c) {
    const double pc = (double) (expf(x[c * stride] - m) / sum);
    const double v = a * (pc - (c == lab ? 1.0 : 0.0)) + b * (pc * ((double) ug[c * p.P] - dot));
    g[c * stride] = (float) (gl * v);
  }
}

// ---------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------
static_assert(sizeof(VampSegLossDesc) == 40, "VampSegLossDesc layout: part of the ABI (the binding reads it from include/vampire_hip.h)");

int seg_validate(const VampSegLossDesc* d) {
  VAMP_REQUIRE(d, "desc is NULL");
  VAMP_REQUIRE(d->layout == VAMP_SEG_ROWS || d->layout == VAMP_SEG_PLANES, "layout must be VAMP_SEG_ROWS or VAMP_SEG_PLANES");
  VAMP_REQUIRE(d->C >= 2 && d->C <= kSegMaxC, "C must be in [2, 32]");
  VAMP_REQUIRE(d->B >= 1 && d->S >= 1, "B * S must be at least 1");
  VAMP_REQUIRE(d->B < (1L << 31) && d->S < (1L << 31) && d->B * d->S < (1L << 31) && d->B * d->S * d->C < (1L << 31),
               "B * S * C must be below 2^31");
  VAMP_REQUIRE(d->label_dtype == VAMP_I64 || d->label_dtype == VAMP_I32 || d->label_dtype == VAMP_U8,
               "label_dtype must be VAMP_I64, VAMP_I32 or VAMP_U8");
  VAMP_REQUIRE(std::isfinite(d->w_ce) && std::isfinite(d->w_lv), "w_ce, w_lv must be finite");
  VAMP_REQUIRE(d->reserved == 0, "reserved must be 0");
  return VAMP_OK;
}

void seg_params(const VampSegLossDesc* d, SegParams* q) {
  q->P = d->B * d->S; q->S = d->S; q->C = d->C;
  q->T = (int) ((q->P + kSegTile - 1) / kSegTile);
  q->nrow = (int) ((q->P + kSegBlock - 1) / kSegBlock);
  q->layout = d->layout; q->label_dtype = d->label_dtype;
  q->w_ce = d->w_ce; q->w_lv = d->w_lv;
}

// The two buffers of seg_params' shapes, each with its own carve (NULL: only the size, which is returned, is of use):
// the forward's workspace ...
size_t seg_workspace(SegParams* q, void* workspace) {
  const size_t rec = (size_t) q->C * q->P, tiles = (size_t) q->C * q->T;
  Carve c(workspace);
  for (int j = 0; j < 2; ++j) {
    q->key[j] = c.take<uint32_t>(rec);
    q->pay[j] = c.take<uint32_t>(rec);
  }
  q->hist = c.take<int>(tiles * kSegRadix);
  q->tilefg = c.take<int>(tiles);
  q->rowcnt = c.take<int>((size_t) q->nrow);
  q->cepart = c.take<double>((size_t) q->nrow);
  q->lvpart = c.take<double>(tiles);
  return c.off;
}
// ... and what the forward keeps for the backward: the header at offset 0, the gradient rows behind it
size_t seg_kept(SegParams* q, void* kept) {
  Carve c(kept);
  q->hdr = c.take<int>(kSegHdrInts);
  q->ug = c.take<float>((size_t) q->C * q->P);
  return c.off;
}

}  // namespace
}  // namespace vamp

using namespace vamp;

extern "C" {

size_t vamp_seg_loss_workspace_bytes(const VampSegLossDesc* d) {
  if (seg_validate(d)) return 0;
  SegParams q{};
  seg_params(d, &q);
  return seg_workspace(&q, nullptr);
}

size_t vamp_seg_loss_kept_bytes(const VampSegLossDesc* d) {
  if (seg_validate(d)) return 0;
  SegParams q{};
  seg_params(d, &q);
  return seg_kept(&q, nullptr);
}

int vamp_seg_loss_forward(const VampSegLossDesc* d, const float* logits, const void* labels, const uint8_t* mask,
                          float* loss, float* terms, int32_t* counts, float* sorted_err, int32_t* perm, void* kept,
                          size_t kept_bytes, void* workspace, size_t workspace_bytes, void* stream) {
  if (int e = seg_validate(d)) return e;
  if (!logits || !labels || !loss || !terms || !counts)
    return fail(VAMP_ENOSPC, "%s: an input or output pointer is NULL", __func__);
  SegParams q{};
  seg_params(d, &q);
  const size_t need = seg_workspace(&q, workspace), keep = seg_kept(&q, kept);
  if (!kept || kept_bytes < keep)
    return fail(VAMP_ENOSPC, "%s: kept %ld < %ld bytes", __func__, (long) kept_bytes, (long) keep);
  if (int e = workspace_fits(__func__, workspace, workspace_bytes, need)) return e;
  if (!aligned(workspace, 8) || !aligned(kept, 8))
    return fail(VAMP_ENOSPC, "%s: the workspace and the kept buffer must be 8-byte aligned", __func__);
  q.logits = logits; q.labels = labels; q.mask = mask;
  q.loss = loss; q.terms = terms; q.counts = counts; q.sorted_err = sorted_err; q.perm = perm;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const dim3 tiles(q.T, q.C);
  VAMP_TIMED(kProfAux, st, (seg_row_kernel<<<q.nrow, kSegBlock, 0, st>>>(q)));
  for (int pass = 0; pass < kSegPasses; ++pass) {
    const int src = pass & 1, shift = 8 * pass;
    VAMP_TIMED(kProfAux, st, (seg_hist_kernel<<<tiles, kSegBlock, 0, st>>>(q, src, shift)));
    VAMP_TIMED(kProfAux, st, (seg_scan_kernel<<<q.C, kSegScanBlock, 0, st>>>(q.hist, (long) kSegRadix * q.T, nullptr)));
    VAMP_TIMED(kProfAux, st, (seg_scatter_kernel<<<tiles, kSegBlock, 0, st>>>(q, src, shift)));
  }
  static_assert(kSegPasses % 2 == 0, "the sorted records end in buffer 0");
  VAMP_TIMED(kProfAux, st, (seg_fg_kernel<<<tiles, kSegBlock, 0, st>>>(q)));
  VAMP_TIMED(kProfAux, st, (seg_scan_kernel<<<q.C, kSegScanBlock, 0, st>>>(q.tilefg, (long) q.T, q.hdr + 2)));
  VAMP_TIMED(kProfAux, st, (seg_jaccard_kernel<<<tiles, kSegBlock, 0, st>>>(q)));
  VAMP_TIMED(kProfAux, st, (seg_finish_kernel<<<1, kSegBlock, 0, st>>>(q)));
  return check_launch("seg_loss_forward");
}

int vamp_seg_loss_backward(const VampSegLossDesc* d, const float* logits, const void* labels, const uint8_t* mask,
                           const float* grad_loss, float* grad_logits, const void* kept, size_t kept_bytes,
                           void* stream) {
  if (int e = seg_validate(d)) return e;
  if (!logits || !labels || !grad_loss || !grad_logits)
    return fail(VAMP_ENOSPC, "%s: an input or output pointer is NULL", __func__);
  SegParams q{};
  seg_params(d, &q);
  const size_t keep = seg_kept(&q, const_cast<void*>(kept));
  if (!kept || kept_bytes < keep)
    return fail(VAMP_ENOSPC, "%s: kept %ld < %ld bytes", __func__, (long) kept_bytes, (long) keep);
  if (!aligned(kept, 8))
    return fail(VAMP_ENOSPC, "%s: the kept buffer must be 8-byte aligned", __func__);
  q.logits = logits; q.labels = labels; q.mask = mask; q.grad_loss = grad_loss; q.grad = grad_logits;
  hipStream_t st = static_cast<hipStream_t>(stream);
  VAMP_TIMED(kProfAux, st, (seg_bwd_kernel<<<q.nrow, kSegBlock, 0, st>>>(q)));
  return check_launch("seg_loss_backward");
}

}  // extern "C"
