// Detection loss on the device: the reference head's loss (bev_depth_head.py:321-379: clip_sigmoid +
// GaussianFocalLoss on the heatmaps, weighted L1 on the gathered box rows) for every task of a head, forward and
// gradient, without a host synchronisation, without float atomics and with bitwise repeatable results.
//
//  counts    loss_counts_kernel, one 1024-lane workgroup per task: the number of heatmap targets equal to 1 and the
//            sum of the masks, as integers, stored as fp32 (counts[t] = (n_pos, n_mask), unclamped: the caller may
//            average them over ranks).  The clamps max(., 1) and max(., 1e-4) are applied where the factors are used.
//  forward   (a) loss_partial_kernel: the tasks' heatmaps are cut into chunks of 2048 elements, one 256-lane
//            workgroup each; every element runs the reference's fp32 chain (sigmoid, clamp, the two focal terms, one
//            fp32 operation per step) and the workgroup's sum is taken in float64 in a fixed order.  Behind the heat
//            chunks, one workgroup per (task, sample) sums code_weights[c] * |pred[b, c, ind] - anno| over the live
//            slots and columns, again in float64.  Every workgroup stores one partial in the workspace.
//            (b) loss_finish_kernel, one workgroup, one wave per task: the task's partials in a fixed order (lane-
//            strided in index order, then a butterfly), divided by the clamped factors: terms[t] = (L_heat, L_box),
//            loss = the sum of the 2 T terms in task order.
//  backward  (a) grad_dense_kernel over the same heat chunks: d loss / d logit from the recomputed sigmoid, every
//            element of the heatmap gradients written; behind them, chunks that zero the regression gradient maps.
//            1 - s is taken as e / (1 + e), e = exp(-x), which keeps its relative accuracy where 1 - s would round.
//            (b) grad_box_kernel, one workgroup per (task, sample): the live slots are compacted in slot order into
//            LDS (cell, slot); a live slot that is the first of its cell adds the contributions of the later live
//            slots of the same cell in ascending slot order and stores the sums over launch (a)'s zeros.  One writer
//            per cell: no atomics.  The search is quadratic in the live slots only.
// A slot is live when its mask is non-zero and 0 <= ind < H * W: a masked slot whose index is out of range is
// skipped and never dereferenced (torch's gather would assert there).  A column is live when its target is not NaN.
// The workspace needs no initialisation; all launches can be captured in a graph.
#include <cmath>

#include "common.hpp"
#include "wave_reduce.hpp"

namespace vamp {
namespace {

constexpr int kLossMaxT = 8;
constexpr int kLossMaxNcls = 4;
constexpr int kLossBlock = 256;
constexpr int kLossWaves = kLossBlock / 64;
constexpr int kLossPer = 8;                         // elements per lane of a heat chunk
constexpr int kLossChunk = kLossBlock * kLossPer;   // 2048
constexpr int kCountBlock = 1024;
constexpr int kLossMaxB = 4096;
constexpr int kLossMaxObjs = 4096;                  // 32 KiB of LDS cells and slots in grad_box_kernel
constexpr int kLossMaxSide = 8192;
constexpr long kLossMaxChunks = 1L << 22;
constexpr int kFinishBlock = kLossMaxT * 64;        // one wave per task

struct LossTaskPtrs {
  float* p[6];                                      // heatmap, reg, height, dim, rot, vel
};

struct LossParams {
  LossTaskPtrs pred[kLossMaxT];                     // forward / backward: the predictions (read)
  LossTaskPtrs grad[kLossMaxT];                     // backward: the gradients (written; nullptr: not wanted)
  const float* heat;
  const float* anno;
  const int64_t* inds;
  const uint8_t* masks;
  const float* counts;
  const float* grad_loss;
  float* loss;
  float* terms;
  double* part;                                     // [nchunk + T * B] partial sums
  long heat_off[kLossMaxT];                         // element offset of task t's [B, ncls, H, W] block
  long heat_n[kLossMaxT];                           // its element count
  int chunk_off[kLossMaxT + 1];                     // first heat chunk of task t; [T]: their number
  int zchunks;                                      // chunks per task of the regression gradient maps
  int B, T, HW, code, K;
  float cw[10], w_bbox;
};

// column c of the code lives in tensor col_tensor(c) (1 reg, 2 height, 3 dim, 4 rot, 5 vel) at channel col_chan(c)
__device__ __forceinline__ int col_tensor(int c) { return c < 2 ? 1 : c < 3 ? 2 : c < 6 ? 3 : c < 8 ? 4 : 5; }
__device__ __forceinline__ int col_chan(int c) { return c < 2 ? c : c < 3 ? 0 : c < 6 ? c - 3 : c < 8 ? c - 6 : c - 8; }
__device__ __forceinline__ int tensor_chans(int j) { return j == 2 ? 1 : j == 3 ? 3 : 2; }

__device__ __forceinline__ int task_of_chunk(const LossParams& p, int chunk) {
  int t = 0;
#pragma unroll
  for (int i = 1; i < kLossMaxT; ++i) t += (i < p.T && chunk >= p.chunk_off[i]) ? 1 : 0;
  return t;
}

// ---------------------------------------------------------------------------------------------------------
// counts
// ---------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int ones4(const float4 v) {
  return (v.x == 1.0f ? 1 : 0) + (v.y == 1.0f ? 1 : 0) + (v.z == 1.0f ? 1 : 0) + (v.w == 1.0f ? 1 : 0);
}

// One workgroup has to read a whole task (the entry point has no workspace to combine several through), so it keeps
// many bytes in flight: 16-byte loads, four per lane and round (64 KiB per round), scalar loads up to the first
// 16-byte boundary and behind the last whole vector.
__global__ void __launch_bounds__(kCountBlock) loss_counts_kernel(LossParams p, float* counts) {
  __shared__ long red[2][kCountBlock / 64];
  const int t = blockIdx.x, tid = threadIdx.x;
  const float* h = p.heat + p.heat_off[t];
  const long n = p.heat_n[t];
  long npos = 0, nmask = 0;
  const long head = min(n, (long) ((16 - (reinterpret_cast<uintptr_t>(h) & 15)) & 15) / 4);
  const long nvec = (n - head) / 4;
  const float4* hv = reinterpret_cast<const float4*>(h + head);
  if (tid < head) npos += h[tid] == 1.0f ? 1 : 0;
  long i = tid;
  for (; i + 3 * kCountBlock < nvec; i += 4 * kCountBlock) {
    const float4 a = hv[i], b = hv[i + kCountBlock], c = hv[i + 2 * kCountBlock], d = hv[i + 3 * kCountBlock];
    npos += ones4(a) + ones4(b) + ones4(c) + ones4(d);
  }
  for (; i < nvec; i += kCountBlock) npos += ones4(hv[i]);
  for (long e = head + 4 * nvec + tid; e < n; e += kCountBlock) npos += h[e] == 1.0f ? 1 : 0;
  const uint8_t* m = p.masks + (long) t * p.B * p.K;
  for (long e = tid; e < (long) p.B * p.K; e += kCountBlock) nmask += m[e];
  npos = wave_sum(npos);
  nmask = wave_sum(nmask);
  if ((tid & 63) == 0) { red[0][tid >> 6] = npos; red[1][tid >> 6] = nmask; }
  __syncthreads();
  if (tid == 0) {
    long a = 0, b = 0;
    for (int w = 0; w < kCountBlock / 64; ++w) { a += red[0][w]; b += red[1][w]; }
    counts[2 * t] = (float) a;
    counts[2 * t + 1] = (float) b;
  }
}

// ---------------------------------------------------------------------------------------------------------
// forward
// ---------------------------------------------------------------------------------------------------------
// clip_sigmoid + gaussian_focal_loss of one element, one fp32 operation per step as torch evaluates them
__device__ __forceinline__ float focal_term(float x, float h) {
  const float s = 1.0f / (1.0f + expf(-x));
  const float p = fminf(fmaxf(s, 1e-4f), 0.9999f);
  const float om = 1.0f - p;
  const float pos = h == 1.0f ? (-logf(p + 1e-12f)) * (om * om) : 0.0f;
  const float q = 1.0f - h, q2 = q * q;
  const float neg = ((-logf(om + 1e-12f)) * (p * p)) * (q2 * q2);
  return pos + neg;
}

__device__ __forceinline__ bool slot_live(const LossParams& p, long row) {
  if (p.masks[row] == 0) return false;
  const int64_t ind = p.inds[row];
  return ind >= 0 && ind < p.HW;
}

__global__ void __launch_bounds__(kLossBlock) loss_partial_kernel(LossParams p) {
  __shared__ double red[kLossWaves];
  const int wg = blockIdx.x, tid = threadIdx.x;
  const int nchunk = p.chunk_off[p.T];
  double acc = 0.0;
  if (wg < nchunk) {
    const int t = task_of_chunk(p, wg);
    const long base = (long) (wg - p.chunk_off[t]) * kLossChunk, n = p.heat_n[t];
    const float* x = p.pred[t].p[0];
    const float* h = p.heat + p.heat_off[t];
#pragma unroll
    for (int i = 0; i < kLossPer; ++i) {
      const long e = base + i * kLossBlock + tid;
      if (e < n) acc += (double) focal_term(x[e], h[e]);
    }
  } else {
    const int tb = wg - nchunk, t = tb / p.B, b = tb % p.B;
    const long row0 = (long) tb * p.K;                 // anno / inds / masks are [T, B, K]
    for (int k = tid; k < p.K; k += kLossBlock) {
      if (!slot_live(p, row0 + k)) continue;
      const long ind = p.inds[row0 + k];
      const float* a = p.anno + (row0 + k) * p.code;
      for (int c = 0; c < p.code; ++c) {
        const float tgt = a[c];
        if (tgt != tgt) continue;
        const int j = col_tensor(c);
        const float v = p.pred[t].p[j][((long) b * tensor_chans(j) + col_chan(c)) * p.HW + ind];
        acc += (double) (fabsf(v - tgt) * p.cw[c]);
      }
    }
  }
  const double tot = block_sum<kLossWaves>(acc, red);
  if (tid == 0) p.part[wg] = tot;
}

__global__ void __launch_bounds__(kFinishBlock) loss_finish_kernel(LossParams p) {
  __shared__ double sterm[kLossMaxT][2];
  const int t = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if (t < p.T) {
    double hs = 0.0, bs = 0.0;
    for (int i = p.chunk_off[t] + lane; i < p.chunk_off[t + 1]; i += 64) hs += p.part[i];
    const double* bp = p.part + p.chunk_off[p.T] + (long) t * p.B;
    for (int i = lane; i < p.B; i += 64) bs += bp[i];
    hs = wave_sum(hs);
    bs = wave_sum(bs);
    if (lane == 0) {
      const float f_pos = fmaxf(p.counts[2 * t], 1.0f), f_num = fmaxf(p.counts[2 * t + 1], 1e-4f);
      sterm[t][0] = hs / (double) f_pos;
      sterm[t][1] = (double) p.w_bbox * bs / (double) f_num;
      p.terms[2 * t] = (float) sterm[t][0];
      p.terms[2 * t + 1] = (float) sterm[t][1];
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double tot = 0.0;
    for (int i = 0; i < p.T; ++i) tot += sterm[i][0] + sterm[i][1];
    p.loss[0] = (float) tot;
  }
}

// ---------------------------------------------------------------------------------------------------------
// backward
// ---------------------------------------------------------------------------------------------------------
// (the upstream gradient is the last factor: a scaled loss scales every element with one rounding)
__device__ __forceinline__ float focal_grad(float x, float h, float inv_pos, float gl) {
  const float e = expf(-x);
  const float s = 1.0f / (1.0f + e);
  if (!(s >= 1e-4f && s <= 0.9999f)) return 0.0f;       // the clamp passes no gradient outside (a NaN logit: 0)
  const float om = e / (1.0f + e);                      // 1 - s without the cancellation; inside the clamp p = s
  const float lp = logf(s + 1e-12f), lq = logf(om + 1e-12f);
  const float q = 1.0f - h, q2 = q * q;
  float g = (q2 * q2) * ((s * s) / (om + 1e-12f) - (2.0f * s) * lq);
  if (h == 1.0f) g += (2.0f * om) * lp - (om * om) / (s + 1e-12f);
  return gl * ((inv_pos * (s * om)) * g);
}

__global__ void __launch_bounds__(kLossBlock) grad_dense_kernel(LossParams p) {
  const int wg = blockIdx.x, tid = threadIdx.x;
  const int nchunk = p.chunk_off[p.T];
  if (wg < nchunk) {
    const int t = task_of_chunk(p, wg);
    float* g = p.grad[t].p[0];
    if (!g) return;
    const long base = (long) (wg - p.chunk_off[t]) * kLossChunk, n = p.heat_n[t];
    const float* x = p.pred[t].p[0];
    const float* h = p.heat + p.heat_off[t];
    const float gl = p.grad_loss[0], inv_pos = 1.0f / fmaxf(p.counts[2 * t], 1.0f);
#pragma unroll
    for (int i = 0; i < kLossPer; ++i) {
      const long e = base + i * kLossBlock + tid;
      if (e < n) g[e] = focal_grad(x[e], h[e], inv_pos, gl);
    }
    return;
  }
  // zeros of the regression gradient maps: task t's maps as one run of B * code * HW elements, tensor by tensor
  const int z = wg - nchunk, t = z / p.zchunks;
  const long bhw = (long) p.B * p.HW, n = bhw * p.code;
  const long base = (long) (z % p.zchunks) * kLossChunk;
#pragma unroll
  for (int i = 0; i < kLossPer; ++i) {
    const long e = base + i * kLossBlock + tid;
    if (e >= n) break;
    const int c = (int) (e / bhw);                      // first column of the tensor the element lies in, by column
    const int j = col_tensor(c);
    const long first = j == 1 ? 0 : j == 2 ? 2 : j == 3 ? 3 : j == 4 ? 6 : 8;
    float* g = p.grad[t].p[j];
    if (g) g[e - first * bhw] = 0.0f;
  }
}

__global__ void __launch_bounds__(kLossBlock) grad_box_kernel(LossParams p) {
  extern __shared__ int lds[];                          // [K] cells and [K] slots of the live slots, in slot order
  __shared__ int wcnt[kLossWaves];
  int* cell = lds;
  int* slot = lds + p.K;
  const int tb = blockIdx.x, t = tb / p.B, b = tb % p.B, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const long row0 = (long) tb * p.K;
  // compact the live slots, keeping their order (ballot scan over chunks of 256 slots)
  const uint64_t lt = (1ull << lane) - 1ull;
  int nlive = 0;
  for (int k0 = 0; k0 < p.K; k0 += kLossBlock) {
    const int k = k0 + tid;
    const bool live = k < p.K && slot_live(p, row0 + k);
    const uint64_t m = __ballot(live);
    if (lane == 0) wcnt[wid] = __popcll(m);
    __syncthreads();
    int off = nlive, tot = 0;
#pragma unroll
    for (int w = 0; w < kLossWaves; ++w) {
      off += w < wid ? wcnt[w] : 0;
      tot += wcnt[w];
    }
    if (live) {
      const int o = off + __popcll(m & lt);
      cell[o] = (int) p.inds[row0 + k];
      slot[o] = k;
    }
    nlive += tot;
    __syncthreads();
  }
  const float gl = p.grad_loss[0], base = p.w_bbox / fmaxf(p.counts[2 * t + 1], 1e-4f);
  for (int i = tid; i < nlive; i += kLossBlock) {
    const int ind = cell[i];
    bool first = true;
    for (int j = 0; j < i; ++j)
      if (cell[j] == ind) { first = false; break; }
    if (!first) continue;
    float v[10], g[10];
    for (int c = 0; c < p.code; ++c) {
      const int j = col_tensor(c);
      v[c] = p.pred[t].p[j][((long) b * tensor_chans(j) + col_chan(c)) * p.HW + ind];
      g[c] = 0.0f;
    }
    // this slot, then the later live slots of the cell, in ascending slot order
    for (int j = i; j < nlive; ++j) {
      if (cell[j] != ind) continue;
      const float* a = p.anno + (row0 + slot[j]) * p.code;
      for (int c = 0; c < p.code; ++c) {
        const float tgt = a[c];
        if (tgt != tgt) continue;
        const float d = v[c] - tgt;
        g[c] += (d > 0.0f ? 1.0f : d < 0.0f ? -1.0f : 0.0f) * (base * p.cw[c]);
      }
    }
    for (int c = 0; c < p.code; ++c) {
      const int j = col_tensor(c);
      float* gp = p.grad[t].p[j];
      if (gp) gp[((long) b * tensor_chans(j) + col_chan(c)) * p.HW + ind] = gl * g[c];
    }
  }
}

// ---------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------
static_assert(sizeof(VampDetLossDesc) == 112, "VampDetLossDesc layout: part of the ABI (the binding reads it from include/vampire_hip.h)");
static_assert(sizeof(LossParams) <= 4096, "kernel arguments");

int loss_validate(const VampDetLossDesc* d) {
  VAMP_REQUIRE(d, "desc is NULL");
  VAMP_REQUIRE(d->B >= 1 && d->B <= kLossMaxB, "B must be in [1, 4096]");
  VAMP_REQUIRE(d->T >= 1 && d->T <= kLossMaxT, "T must be in [1, 8]");
  VAMP_REQUIRE(d->H >= 1 && d->H <= kLossMaxSide && d->W >= 1 && d->W <= kLossMaxSide, "H, W must be in [1, 8192]");
  for (int t = 0; t < d->T; ++t) VAMP_REQUIRE(d->ncls[t] >= 1 && d->ncls[t] <= kLossMaxNcls, "ncls must be in [1, 4]");
  VAMP_REQUIRE(d->code == 8 || d->code == 10, "code must be 8 or 10");
  VAMP_REQUIRE(d->has_vel == 0 || d->has_vel == 1, "has_vel must be 0 or 1");
  VAMP_REQUIRE(d->code == (d->has_vel ? 10 : 8), "code must agree with has_vel (10 with velocity, 8 without)");
  VAMP_REQUIRE(d->max_objs >= 1 && d->max_objs <= kLossMaxObjs, "max_objs must be in [1, 4096]");
  for (int c = 0; c < d->code; ++c) VAMP_REQUIRE(std::isfinite(d->code_weights[c]), "code_weights must be finite");
  VAMP_REQUIRE(std::isfinite(d->loss_bbox_weight), "loss_bbox_weight must be finite");
  VAMP_REQUIRE(d->reserved[0] == 0 && d->reserved[1] == 0, "reserved must be 0");
  long chunks = 0;
  for (int t = 0; t < d->T; ++t)
    chunks += ((long) d->B * d->ncls[t] * d->H * d->W + kLossChunk - 1) / kLossChunk;
  chunks += (long) d->T * (((long) d->B * d->code * d->H * d->W + kLossChunk - 1) / kLossChunk);
  VAMP_REQUIRE(chunks <= kLossMaxChunks, "B * H * W is too large (2^22 chunks of 2048 elements at most)");
  return VAMP_OK;
}

void loss_params(const VampDetLossDesc* d, LossParams* q) {
  long off = 0;
  int chunk = 0;
  for (int t = 0; t < d->T; ++t) {
    q->heat_off[t] = off;
    q->heat_n[t] = (long) d->B * d->ncls[t] * d->H * d->W;
    q->chunk_off[t] = chunk;
    off += q->heat_n[t];
    chunk += (int) ((q->heat_n[t] + kLossChunk - 1) / kLossChunk);
  }
  for (int t = d->T; t <= kLossMaxT; ++t) q->chunk_off[t] = chunk;
  q->zchunks = (int) (((long) d->B * d->code * d->H * d->W + kLossChunk - 1) / kLossChunk);
  q->B = d->B; q->T = d->T; q->HW = d->H * d->W; q->code = d->code; q->K = d->max_objs;
  for (int c = 0; c < 10; ++c) q->cw[c] = c < d->code ? d->code_weights[c] : 0.0f;
  q->w_bbox = d->loss_bbox_weight;
}

size_t loss_workspace(const VampDetLossDesc* d) {
  LossParams q{};
  loss_params(d, &q);
  return align_up(((size_t) q.chunk_off[d->T] + (size_t) d->T * d->B) * sizeof(double), 256);
}

int loss_tasks(const VampDetLossDesc* d, const VampDetTask* tasks, LossTaskPtrs* out, bool all) {
  for (int t = 0; t < d->T; ++t) {
    const void* src[6] = {tasks[t].heatmap, tasks[t].reg, tasks[t].height, tasks[t].dim, tasks[t].rot,
                          d->has_vel ? tasks[t].vel : nullptr};
    for (int j = 0; j < 6; ++j) {
      if (all && (j < 5 || d->has_vel) && !src[j])
        return fail(VAMP_ENOSPC, "%s: a prediction pointer of task %ld is NULL", __func__, t);
      out[t].p[j] = const_cast<float*>(static_cast<const float*>(src[j]));
    }
  }
  return VAMP_OK;
}

}  // namespace
}  // namespace vamp

using namespace vamp;

extern "C" {

size_t vamp_det_loss_workspace_bytes(const VampDetLossDesc* d) {
  if (loss_validate(d)) return 0;
  return loss_workspace(d);
}

int vamp_det_loss_counts(const VampDetLossDesc* d, const float* heat, const uint8_t* masks, float* counts,
                         void* stream) {
  if (int e = loss_validate(d)) return e;
  if (!heat || !masks || !counts) return fail(VAMP_ENOSPC, "%s: heat, masks or counts is NULL", __func__);
  LossParams q{};
  loss_params(d, &q);
  q.heat = heat; q.masks = masks;
  hipStream_t s = static_cast<hipStream_t>(stream);
  VAMP_TIMED(kProfAux, s, (loss_counts_kernel<<<d->T, kCountBlock, 0, s>>>(q, counts)));
  return check_launch("det_loss_counts");
}

int vamp_det_loss_forward(const VampDetLossDesc* d, const VampDetTask* preds, const float* heat, const float* anno,
                          const int64_t* inds, const uint8_t* masks, const float* counts, float* loss, float* terms,
                          void* workspace, size_t workspace_bytes, void* stream) {
  if (int e = loss_validate(d)) return e;
  if (!preds || !heat || !anno || !inds || !masks || !counts || !loss || !terms)
    return fail(VAMP_ENOSPC, "%s: an input or output pointer is NULL", __func__);
  LossParams q{};
  loss_params(d, &q);
  if (int e = loss_tasks(d, preds, q.pred, true)) return e;
  const size_t need = loss_workspace(d);
  if (int e = workspace_fits(__func__, workspace, workspace_bytes, need)) return e;
  q.heat = heat; q.anno = anno; q.inds = inds; q.masks = masks; q.counts = counts; q.loss = loss; q.terms = terms;
  q.part = static_cast<double*>(workspace);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int grid = q.chunk_off[d->T] + d->T * d->B;
  VAMP_TIMED(kProfAux, s, (loss_partial_kernel<<<grid, kLossBlock, 0, s>>>(q)));
  VAMP_TIMED(kProfAux, s, (loss_finish_kernel<<<1, kFinishBlock, 0, s>>>(q)));
  return check_launch("det_loss_forward");
}

int vamp_det_loss_backward(const VampDetLossDesc* d, const VampDetTask* preds, const float* heat, const float* anno,
                           const int64_t* inds, const uint8_t* masks, const float* counts, const float* grad_loss,
                           const VampDetTask* grads, void* workspace, size_t workspace_bytes, void* stream) {
  if (int e = loss_validate(d)) return e;
  if (!preds || !heat || !anno || !inds || !masks || !counts || !grad_loss || !grads)
    return fail(VAMP_ENOSPC, "%s: an input or output pointer is NULL", __func__);
  LossParams q{};
  loss_params(d, &q);
  if (int e = loss_tasks(d, preds, q.pred, true)) return e;
  loss_tasks(d, grads, q.grad, false);
  const size_t need = loss_workspace(d);              // (the backward stores nothing there: one size for both)
  if (int e = workspace_fits(__func__, workspace, workspace_bytes, need)) return e;
  q.heat = heat; q.anno = anno; q.inds = inds; q.masks = masks; q.counts = counts; q.grad_loss = grad_loss;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int grid = q.chunk_off[d->T] + d->T * q.zchunks;
  VAMP_TIMED(kProfAux, s, (grad_dense_kernel<<<grid, kLossBlock, 0, s>>>(q)));
  VAMP_TIMED(kProfAux, s, (grad_box_kernel<<<d->T * d->B, kLossBlock, 2 * (size_t) d->max_objs * sizeof(int), s>>>(q)));
  return check_launch("det_loss_backward");
}

}  // extern "C"
