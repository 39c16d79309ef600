// The parameter update that ends a training step, on the device: gradient-norm clipping, AdamW, the averaged (EMA)
// weights and the loss-scale bookkeeping of fp16 training in three launches, for any number of tensors
// (base_cli.py:61-90 Trainer(gradient_clip_val=35, precision=16); base_exp.py:931-943 AdamW; callbacks/ema.py:23-117
// ModelEMA / EMACallback) -- without a host synchronisation, without atomics, bitwise repeatable, capturable in a graph.
//
// The work is described by a CHUNK TABLE in device memory that the host builds once (vampire_amd/optim.py plan_update):
// every tensor is cut into chunks of at most VAMP_UPDATE_CHUNK elements, a chunk never crosses a tensor, one workgroup
// takes one chunk, so the grids depend on the shapes only.  The table's first n_param_chunks entries are the chunks of
// the parameters, the n_buffer_chunks behind them those of the floating-point buffers (EMA only).  exp_avg, exp_avg_sq
// and ema are flat fp32 arrays of the updater's own in which every tensor starts at a multiple of 4 elements: the
// state side of a chunk is always 16-byte aligned.
//
// VAMP_UPDATE_CHUNK = 4096 = 256 lanes x 4 elements (one 16-byte access) x 4 rounds.  The kernel is a pure stream: a
// round of the apply pass has five 16-byte loads per lane in flight (p, g, m, v, ema: 20 KiB per workgroup) and needs
// 36 registers, so eight workgroups fit a CU and keep about 160 KiB of loads in flight there, several times what
// hides an HBM miss; latency is hidden by occupancy, and more rounds per lane add nothing but code.  A chunk moves
// 144 KiB, which dwarfs a workgroup's start-up; a larger chunk would not serve the model's many small tensors (306 of
// the 435 parameter tensors of the cfg-A network have at most 4096 elements and take one workgroup whatever the chunk
// size), and the table (32 bytes per chunk) and the partial sums (8 bytes per parameter chunk) stay under half a
// megabyte for 52 M parameters.  Measured on the MI355X on that network's tensor list: the apply pass runs at the
// rate of a float4 copy (6.0 TB/s), and a build with 8192 elements per chunk gave the same step time within the
// run-to-run spread (0.405 - 0.418 against 0.411 - 0.415 ms replayed), so the smaller chunk stays.
//
//  norm     upd_norm_kernel, one workgroup per parameter chunk: the float64 sum of g g over the chunk, element
//           i0 = 1024 r + 4 lane + q of round r added by its lane in the order (r, q), then the butterfly of
//           wave_reduce.hpp and the waves in index order, into the chunk's own slot.  A square of an fp32 value cannot
//           overflow float64, so a sum that is not finite means exactly "some element is inf or NaN".  A chunk whose
//           parameter has no gradient stores 0.
//  finish   upd_finish_kernel, one workgroup of 1024: the slots lane-strided in index order, the same block sum, thread
//           0 writes the scalar block (VampUpdateScalars) in float64, each value rounded to fp32 once: total_norm =
//           sqrt(sum) / S, found_inf, clip_coef = min(1, max_norm / (total_norm + 1e-6)), mult = clip_coef / S, the
//           AdamW scalars of step t (t advances unless found_inf): 1 - lr wd, lr / (1 - beta1^t), sqrt(1 - beta2^t),
//           the EMA decay d = ema_decay (1 - exp(-n / 2000)) of update n (n always advances) and 1 - d, and the next
//           loss scale (torch's GradScaler rule: x 0.5 on found_inf, x 2 after 2000 clean steps).
//  apply    upd_apply_kernel, one workgroup per chunk, parameters and buffers in one launch.  A parameter element,
//           in fp32 and in THIS ORDER, every operation rounded by itself (the library is built with
//           -ffp-contract=off):
//               g' = g mult
//               p  = p (1 - lr wd)
//               m  = m + (g' - m) (1 - beta1)
//               v  = v beta2 + ((1 - beta2) g') g'
//               p  = p - (lr / bc1) (m / (sqrt(v) / sqrt(bc2) + eps))
//               e  = e d + (1 - d) p
//           which is the order of torch's single-tensor AdamW (mul_, lerp_, mul_ + addcmul_, addcdiv_) and of the
//           reference's EMA loop.  With found_inf set p, m and v are not stored (they keep their bits) and the EMA
//           line runs on the unchanged p.  A buffer element, and an element of a parameter without a gradient, takes
//           the EMA line only.  Every element is written once.  A group of four elements is one 16-byte access per
//           stream where param and grad are aligned for it and the group lies inside the chunk, else element accesses;
//           the arithmetic of an element is the same on both paths, so a parameter that is a slice at any element
//           offset gets the bits of an aligned copy.  All loads of a round are issued before their first use.
#include <cmath>

#include "common.hpp"
#include "wave_reduce.hpp"

namespace vamp {
namespace {

constexpr int kUpdBlock = 256;
constexpr int kUpdWaves = kUpdBlock / 64;
constexpr int kUpdVec = 4;
constexpr int kUpdRoundElems = kUpdBlock * kUpdVec;
constexpr int kUpdRounds = VAMP_UPDATE_CHUNK / kUpdRoundElems;
constexpr int kUpdChunk = kUpdRoundElems * kUpdRounds;
constexpr int kUpdFinishBlock = 1024;                           // one workgroup over 8 bytes per parameter chunk
static_assert(kUpdChunk == VAMP_UPDATE_CHUNK, "VAMP_UPDATE_CHUNK is the workgroup's chunk");
static_assert(sizeof(VampUpdateChunk) == 32, "VampUpdateChunk layout: part of the ABI (the binding reads it from include/vampire_hip.h)");
static_assert(sizeof(VampUpdateScalars) == 128, "VampUpdateScalars layout: part of the ABI (the binding reads it from include/vampire_hip.h)");
static_assert(sizeof(VampParamUpdateDesc) == 64, "VampParamUpdateDesc layout: part of the ABI (the binding reads it from include/vampire_hip.h)");

__device__ __forceinline__ bool upd_aligned16(const void* a, const void* b) {
  return ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b)) & 15u) == 0;
}

// up to four elements of `src` from i0 on into x (the others 0); `full`: one 16-byte load
__device__ __forceinline__ void upd_load(const float* src, int i0, int len, bool full, float (&x)[kUpdVec]) {
  if (full) {
    const float4 w = *reinterpret_cast<const float4*>(src + i0);
    x[0] = w.x; x[1] = w.y; x[2] = w.z; x[3] = w.w;
  } else {
#pragma unroll
    for (int q = 0; q < kUpdVec; ++q) x[q] = i0 + q < len ? src[i0 + q] : 0.0f;
  }
}

__device__ __forceinline__ void upd_store(float* dst, int i0, int len, bool full, const float (&x)[kUpdVec]) {
  if (full) {
    *reinterpret_cast<float4*>(dst + i0) = make_float4(x[0], x[1], x[2], x[3]);
  } else {
#pragma unroll
    for (int q = 0; q < kUpdVec; ++q)
      if (i0 + q < len) dst[i0 + q] = x[q];
  }
}

__global__ void __launch_bounds__(kUpdBlock) upd_norm_kernel(const VampUpdateChunk* __restrict__ table,
                                                             double* __restrict__ slots) {
  __shared__ double red[kUpdWaves];
  const VampUpdateChunk c = table[blockIdx.x];
  double s = 0.0;
  if (c.kind == VAMP_UPDATE_PARAM && c.grad) {                  // (uniform per workgroup)
    const float* g = static_cast<const float*>(c.grad);
    const int len = c.len < kUpdChunk ? c.len : kUpdChunk;
    const bool vec = upd_aligned16(g, nullptr);
    float x[kUpdRounds][kUpdVec];
#pragma unroll
    for (int r = 0; r < kUpdRounds; ++r) {
      const int i0 = r * kUpdRoundElems + (int) threadIdx.x * kUpdVec;
      upd_load(g, i0, len, vec && i0 + kUpdVec <= len, x[r]);
    }
#pragma unroll
    for (int r = 0; r < kUpdRounds; ++r)
#pragma unroll
      for (int q = 0; q < kUpdVec; ++q) s += (double) x[r][q] * (double) x[r][q];   // (an element past len adds +0)
  }
  const double t = block_sum<kUpdWaves>(s, red);
  if (threadIdx.x == 0) slots[blockIdx.x] = t;
}

struct UpdFinish {
  const double* slots;
  VampUpdateScalars* sc;
  double beta1, beta2, weight_decay, max_norm, ema_decay;
  int n_param, scale_mode;
};

__global__ void __launch_bounds__(kUpdFinishBlock) upd_finish_kernel(UpdFinish f) {
  __shared__ double red[kUpdFinishBlock / 64];
  double s = 0.0;
#pragma unroll 4
  for (int j = threadIdx.x; j < f.n_param; j += kUpdFinishBlock) s += f.slots[j];
  const double tot = block_sum<kUpdFinishBlock / 64>(s, red);
  if (threadIdx.x != 0) return;
  VampUpdateScalars* sc = f.sc;
  const double S = (double) sc->scale;
  const bool inf = !(tot < (double) INFINITY);                  // a sum of squares: inf or NaN, never negative
  const double norm = sqrt(tot) / S;
  double clip = 1.0;
  if (f.max_norm > 0.0) {
    const double c = f.max_norm / (norm + 1e-6);
    clip = c < 1.0 ? c : 1.0;                                   // (NaN: 1, the step is skipped anyway)
  }
  const long t = sc->step + (inf ? 0 : 1), n = sc->updates + 1;
  const double lr = sc->lr;
  const double bc1 = 1.0 - pow(f.beta1, (double) t), bc2 = 1.0 - pow(f.beta2, (double) t);
  const double d = f.ema_decay > 0.0 ? f.ema_decay * (1.0 - exp(-(double) n / 2000.0)) : 0.0;
  sc->step = t;
  sc->updates = n;
  sc->found_inf = inf ? 1 : 0;
  sc->total_norm = (float) norm;
  sc->clip_coef = (float) clip;
  sc->mult = (float) (clip / S);
  sc->decay_mul = (float) (1.0 - lr * f.weight_decay);
  sc->step_size = (float) (lr / bc1);
  sc->bc2_sqrt = (float) sqrt(bc2);
  sc->ema_d = (float) d;
  sc->ema_1md = (float) (1.0 - d);
  if (f.scale_mode == VAMP_UPDATE_SCALE_DYNAMIC) {
    if (inf) {
      sc->scale = (float) (S * 0.5);
      sc->growth = 0;
    } else if (sc->growth + 1 >= VAMP_UPDATE_GROWTH_INTERVAL) {
      sc->scale = (float) (S * 2.0);
      sc->growth = 0;
    } else {
      sc->growth = sc->growth + 1;
    }
  }
}

struct UpdApply {
  const VampUpdateChunk* table;
  float *m, *v, *ema;                                           // ema == nullptr: no averaged weights
  const VampUpdateScalars* sc;
  float omb1, beta2, omb2, eps;
  int n_param;
};

__global__ void __launch_bounds__(kUpdBlock) upd_apply_kernel(UpdApply a) {
  const VampUpdateChunk c = a.table[blockIdx.x];
  const bool is_param = (int) blockIdx.x < a.n_param && c.kind == VAMP_UPDATE_PARAM && c.grad;
  const bool use_ema = a.ema != nullptr;
  if (!is_param && !use_ema) return;                            // (uniform per workgroup, as every branch on them)
  const bool skip = a.sc->found_inf != 0;
  const float mult = a.sc->mult, dm = a.sc->decay_mul, ss = a.sc->step_size, b2s = a.sc->bc2_sqrt;
  const float d = a.sc->ema_d, omd = a.sc->ema_1md;
  float* p = static_cast<float*>(c.param);
  const float* g = static_cast<const float*>(c.grad);
  const int len = c.len < kUpdChunk ? c.len : kUpdChunk;
  const bool vec = upd_aligned16(p, is_param ? g : nullptr);
  float* m = is_param ? a.m + c.state_off : nullptr;
  float* v = is_param ? a.v + c.state_off : nullptr;
  float* e = use_ema ? a.ema + c.state_off : nullptr;
#pragma unroll
  for (int r = 0; r < kUpdRounds; ++r) {
    const int i0 = r * kUpdRoundElems + (int) threadIdx.x * kUpdVec;
    if (i0 >= len) continue;
    const bool full = vec && i0 + kUpdVec <= len;
    float pv[kUpdVec], gv[kUpdVec], mv[kUpdVec], vv[kUpdVec], ev[kUpdVec];
    upd_load(p, i0, len, full, pv);
    if (is_param) {
      upd_load(g, i0, len, full, gv);
      upd_load(m, i0, len, full, mv);
      upd_load(v, i0, len, full, vv);
    }
    if (use_ema) upd_load(e, i0, len, full, ev);
    if (is_param && !skip) {
#pragma unroll
      for (int q = 0; q < kUpdVec; ++q) {
        const float gp = gv[q] * mult;
        const float pd = pv[q] * dm;
        const float mn = mv[q] + (gp - mv[q]) * a.omb1;
        const float vn = vv[q] * a.beta2 + (a.omb2 * gp) * gp;
        const float den = sqrtf(vn) / b2s + a.eps;
        pv[q] = pd - ss * (mn / den);
        mv[q] = mn;
        vv[q] = vn;
      }
      upd_store(p, i0, len, full, pv);
      upd_store(m, i0, len, full, mv);
      upd_store(v, i0, len, full, vv);
    }
    if (use_ema) {
#pragma unroll
      for (int q = 0; q < kUpdVec; ++q) ev[q] = ev[q] * d + omd * pv[q];
      upd_store(e, i0, len, full, ev);
    }
  }
}

// ---------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------
int upd_validate(const VampParamUpdateDesc* d) {
  VAMP_REQUIRE(d, "desc is NULL");
  VAMP_REQUIRE(d->n_param_chunks >= 0 && d->n_buffer_chunks >= 0, "chunk counts must not be negative");
  VAMP_REQUIRE((long) d->n_param_chunks + (long) d->n_buffer_chunks >= 1, "no chunks");
  VAMP_REQUIRE((long) d->n_param_chunks + (long) d->n_buffer_chunks < (1L << 31), "too many chunks");
  VAMP_REQUIRE(d->beta1 >= 0.0 && d->beta1 < 1.0, "beta1 must be in [0, 1)");
  VAMP_REQUIRE(d->beta2 >= 0.0 && d->beta2 < 1.0, "beta2 must be in [0, 1)");
  VAMP_REQUIRE(d->eps >= 0.0, "eps must not be negative");
  VAMP_REQUIRE(d->weight_decay >= 0.0, "weight_decay must not be negative");
  VAMP_REQUIRE(d->max_norm == d->max_norm, "max_norm is NaN");
  VAMP_REQUIRE(d->ema_decay < 1.0, "ema_decay must be below 1");
  VAMP_REQUIRE(d->scale_mode == VAMP_UPDATE_SCALE_NONE || d->scale_mode == VAMP_UPDATE_SCALE_STATIC ||
               d->scale_mode == VAMP_UPDATE_SCALE_DYNAMIC, "scale_mode must be a VAMP_UPDATE_SCALE_* value");
  VAMP_REQUIRE(d->reserved == 0, "reserved must be 0");
  return VAMP_OK;
}

}  // namespace
}  // namespace vamp

using namespace vamp;

extern "C" {

size_t vamp_param_update_workspace_bytes(const VampParamUpdateDesc* d) {
  if (upd_validate(d)) return 0;
  const size_t slots = d->n_param_chunks > 0 ? (size_t) d->n_param_chunks : 1;
  return align_up(slots * sizeof(double), 256);
}

int vamp_param_update_step(const VampParamUpdateDesc* d, const void* table, float* exp_avg, float* exp_avg_sq,
                           float* ema, void* scalars, void* workspace, size_t workspace_bytes, void* stream) {
  if (int e = upd_validate(d)) return e;
  VAMP_REQUIRE(table, "the chunk table is NULL");
  VAMP_REQUIRE(scalars, "the scalar block is NULL");
  VAMP_REQUIRE(d->n_param_chunks == 0 || (exp_avg && exp_avg_sq), "exp_avg or exp_avg_sq is NULL");
  VAMP_REQUIRE(d->ema_decay <= 0.0 || ema, "ema_decay > 0 needs the ema array");
  VAMP_REQUIRE(aligned(table, 8) && aligned(scalars, 8), "table and scalars must be 8-byte aligned");
  VAMP_REQUIRE(aligned(exp_avg, 16) && aligned(exp_avg_sq, 16) && aligned(ema, 16),
               "the state arrays must be 16-byte aligned");
  const size_t need = vamp_param_update_workspace_bytes(d);
  if (int e = workspace_fits(__func__, workspace, workspace_bytes, need)) return e;
  VAMP_REQUIRE(aligned(workspace, 8), "the workspace must be 8-byte aligned");
  hipStream_t st = static_cast<hipStream_t>(stream);
  const VampUpdateChunk* tb = static_cast<const VampUpdateChunk*>(table);
  double* slots = static_cast<double*>(workspace);
  VampUpdateScalars* sc = static_cast<VampUpdateScalars*>(scalars);
  if (d->n_param_chunks > 0)
    VAMP_TIMED(kProfAux, st, (upd_norm_kernel<<<(unsigned) d->n_param_chunks, kUpdBlock, 0, st>>>(tb, slots)));
  UpdFinish f{slots, sc, d->beta1, d->beta2, d->weight_decay, d->max_norm, d->ema_decay, d->n_param_chunks,
              d->scale_mode};
  VAMP_TIMED(kProfAux, st, (upd_finish_kernel<<<1, kUpdFinishBlock, 0, st>>>(f)));
  UpdApply a{tb, exp_avg, exp_avg_sq, d->ema_decay > 0.0 ? ema : nullptr, sc, (float) (1.0 - d->beta1),
             (float) d->beta2, (float) (1.0 - d->beta2), (float) d->eps, d->n_param_chunks};
  const unsigned grid = (unsigned) (d->n_param_chunks + (d->ema_decay > 0.0 ? d->n_buffer_chunks : 0));
  if (grid > 0) VAMP_TIMED(kProfAux, st, (upd_apply_kernel<<<grid, kUpdBlock, 0, st>>>(a)));
  return check_launch("param_update_step");
}

}  // extern "C"
