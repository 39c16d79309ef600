// Masked regression losses on the device: a PACK of up to 8 terms, each the mean smooth-L1 (beta 1) or squared error
// of `pred` against `target` (an array or one constant) over the elements a bool mask sets, clears, or both -- the
// camera depth, BEV height, sdf and occupancy density terms of the training step (base_exp.py:588-594 get_depth_loss,
// :581-586 get_height_loss_bev, :533-537 get_sdf_loss, :523-531 get_occ_density_loss), forward and gradient with respect
// to pred, without the boolean-mask compaction, without a host synchronisation, without atomics and with bitwise
// repeatable results.  For term t with n elements: d = float(pred) - target and the element loss in fp32 as aten
// computes them, S1 = the elements whose mask byte is set (all without a mask), S0 the others, mean_k = the float64
// sum over S_k divided by |S_k| in float64, exactly 0 when S_k is empty.
//
//  partial   reg_partial_kernel.  Term t owns ceil(n_t / 4096) consecutive workgroups (the prefix table `first` in the
//            kernel arguments maps a block to its term and tile).  A lane takes four groups of four consecutive elements,
//            group g of round r at tile + 1024 r + 4 lane: with pred, target and mask aligned for it a group is one
//            16-byte load of pred (8 bytes of bf16), one of target and one 4-byte load of the mask, otherwise -- and for
//            the group that crosses n -- element loads; the element a lane adds and the order it adds in are the same
//            on both paths, so a slice at any offset gives the bits of an aligned copy.  An element is SELECTED into a
//            sum, never multiplied by 0: what a side leaves out cannot reach the loss.  The workgroup's (sum_1, sum_0)
//            in float64 and (|S_1|, |S_0|) go to its own slot of the workspace.
//  finish    reg_finish_kernel, one workgroup: wave w takes terms w, w + 4; lane-strided over the term's slots in
//            index order, then a butterfly -- a term's result does not depend on the rest of the pack.  Writes
//            losses[t] (mean_1, mean_0 or their float64 sum, rounded to fp32 once) and counts[t] = (|S_1|, |S_0|).
//  backward  reg_bwd_kernel, the same grid: g = grad_losses[t] l'(d) / |S_k| in float64 for an element of a selected
//            side k (l' = d inside |d| < 1, else sign(d), a NaN d kept; 2 d for the squared error), rounded once to
//            fp32 and from there to nearest-even bf16 for a bf16 pred; exactly 0 elsewhere; every element written
//            once.  A term whose grad pointer is NULL is skipped.
// Grids depend on the shapes only; two launches forward, one backward.  Nothing needs initialisation.
#include <cmath>

#include "common.hpp"
#include "elem16.hpp"
#include "wave_reduce.hpp"

namespace vamp {
namespace {

constexpr int kRegBlock = 256;
constexpr int kRegWaves = kRegBlock / 64;
constexpr int kRegVec = 4;                           // elements of a group: one mask word
constexpr int kRegRounds = 4;
constexpr int kRegTile = kRegBlock * kRegVec * kRegRounds;
static_assert(kRegTile == VAMP_REG_TILE, "VAMP_REG_TILE is the workgroup's tile");

struct RegPack {
  const void* pred[VAMP_REG_MAX_TERMS];
  const float* target[VAMP_REG_MAX_TERMS];
  const uint8_t* mask[VAMP_REG_MAX_TERMS];
  void* grad[VAMP_REG_MAX_TERMS];
  long n[VAMP_REG_MAX_TERMS];
  int first[VAMP_REG_MAX_TERMS + 1];                 // first workgroup of a term; first[T] = the grid
  float cval[VAMP_REG_MAX_TERMS];
  uint8_t kind[VAMP_REG_MAX_TERMS], side[VAMP_REG_MAX_TERMS], bf16[VAMP_REG_MAX_TERMS], cst[VAMP_REG_MAX_TERMS];
  uint8_t vec[VAMP_REG_MAX_TERMS];                   // every operand of the launch aligned for group loads
  int T;
  double* psum;                                      // [grid, 2]
  int* pcnt;                                         // [grid, 2]
  float* losses;                                     // [T]
  int64_t* counts;                                   // [T, 2]
  const float* grad_losses;                          // [T]
};

__device__ __forceinline__ int reg_term_of(const RegPack& p, int b) {
  int t = 0;
  for (int k = 1; k < p.T; ++k) t = b >= p.first[k] ? k : t;
  return t;
}

// One group: up to four elements from i0 on, `live` = the bits of those below n, `set` = the bits whose mask byte is
// set (all live bits without a mask).  tv of a constant target is the constant.
struct RegGroup {
  float pv[kRegVec], tv[kRegVec];
  unsigned live, set;
};

__device__ __forceinline__ RegGroup reg_load(const RegPack& p, int t, long i0, long n) {
  RegGroup g;
  const bool cst = p.cst[t] != 0, bf = p.bf16[t] != 0;
  const uint8_t* mk = p.mask[t];
  if (p.vec[t] && i0 + kRegVec <= n) {
    g.live = 0xFu;
    if (bf) {
      const uint2 w = *reinterpret_cast<const uint2*>(static_cast<const uint16_t*>(p.pred[t]) + i0);
      const float4 v = bf16x4_to_f32(w);
      g.pv[0] = v.x; g.pv[1] = v.y; g.pv[2] = v.z; g.pv[3] = v.w;
    } else {
      const float4 w = *reinterpret_cast<const float4*>(static_cast<const float*>(p.pred[t]) + i0);
      g.pv[0] = w.x; g.pv[1] = w.y; g.pv[2] = w.z; g.pv[3] = w.w;
    }
    if (cst) {
#pragma unroll
      for (int q = 0; q < kRegVec; ++q) g.tv[q] = p.cval[t];
    } else {
      const float4 w = *reinterpret_cast<const float4*>(p.target[t] + i0);
      g.tv[0] = w.x; g.tv[1] = w.y; g.tv[2] = w.z; g.tv[3] = w.w;
    }
    g.set = 0xFu;
    if (mk) {
      const uint32_t w = *reinterpret_cast<const uint32_t*>(mk + i0);
      g.set = ((w & 0xFFu) ? 1u : 0u) | ((w & 0xFF00u) ? 2u : 0u) | ((w & 0xFF0000u) ? 4u : 0u) |
              ((w & 0xFF000000u) ? 8u : 0u);
    }
    return g;
  }
  g.live = g.set = 0u;
#pragma unroll
  for (int q = 0; q < kRegVec; ++q) {
    g.pv[q] = g.tv[q] = 0.0f;
    if (i0 + q < n) {
      g.live |= 1u << q;
      g.pv[q] = bf ? bf16_to_f32(static_cast<const uint16_t*>(p.pred[t])[i0 + q]) : static_cast<const float*>(p.pred[t])[i0 + q];
      g.tv[q] = cst ? p.cval[t] : p.target[t][i0 + q];
      if (!mk || mk[i0 + q] != 0) g.set |= 1u << q;
    }
  }
  return g;
}

__device__ __forceinline__ float reg_elem(int kind, float d) {
  if (kind == VAMP_REG_MSE) return d * d;
  const float z = fabsf(d);
  return z < 1.0f ? (0.5f * z) * z : z - 0.5f;
}

__global__ void __launch_bounds__(kRegBlock) reg_partial_kernel(RegPack p) {
  __shared__ double red[kRegWaves];
  __shared__ int redi[kRegWaves];
  const int b = blockIdx.x, t = reg_term_of(p, b);
  const long n = p.n[t], base = (long) (b - p.first[t]) * kRegTile;
  const int kind = p.kind[t];
  const bool want1 = p.side[t] != VAMP_REG_CLEAR, want0 = p.side[t] != VAMP_REG_SET;
  double s1 = 0.0, s0 = 0.0;
  int c1 = 0, c0 = 0;
#pragma unroll
  for (int r = 0; r < kRegRounds; ++r) {
    const long i0 = base + (long) r * (kRegBlock * kRegVec) + (long) threadIdx.x * kRegVec;
    if (i0 >= n) continue;
    const RegGroup g = reg_load(p, t, i0, n);
#pragma unroll
    for (int q = 0; q < kRegVec; ++q) {
      if (!((g.live >> q) & 1u)) continue;
      const bool m = (g.set >> q) & 1u;
      c1 += m ? 1 : 0;
      c0 += m ? 0 : 1;
      if (m ? want1 : want0) {                       // selected: a NaN outside the side never meets a sum
        const double l = (double) reg_elem(kind, g.pv[q] - g.tv[q]);
        if (m) s1 += l;
        else s0 += l;
      }
    }
  }
  const double t1 = block_sum<kRegWaves>(s1, red), t0 = block_sum<kRegWaves>(s0, red);
  const int n1 = block_sum<kRegWaves>(c1, redi), n0 = block_sum<kRegWaves>(c0, redi);
  if (threadIdx.x == 0) {
    p.psum[2 * (long) b] = t1;
    p.psum[2 * (long) b + 1] = t0;
    p.pcnt[2 * (long) b] = n1;
    p.pcnt[2 * (long) b + 1] = n0;
  }
}

__global__ void __launch_bounds__(kRegBlock) reg_finish_kernel(RegPack p) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int t = wave; t < p.T; t += kRegWaves) {
    double s1 = 0.0, s0 = 0.0;
    long c1 = 0, c0 = 0;
    for (long j = p.first[t] + lane; j < p.first[t + 1]; j += 64) {
      s1 += p.psum[2 * j];
      s0 += p.psum[2 * j + 1];
      c1 += p.pcnt[2 * j];
      c0 += p.pcnt[2 * j + 1];
    }
    s1 = wave_sum(s1);
    s0 = wave_sum(s0);
    const int i1 = wave_sum((int) c1), i0 = wave_sum((int) c0);                // (n < 2^31)
    if (lane == 0) {
      const double m1 = i1 > 0 ? s1 / (double) i1 : 0.0, m0 = i0 > 0 ? s0 / (double) i0 : 0.0;
      const int side = p.side[t];
      p.losses[t] = (float) (side == VAMP_REG_SET ? m1 : (side == VAMP_REG_CLEAR ? m0 : m1 + m0));
      p.counts[2 * t] = i1;
      p.counts[2 * t + 1] = i0;
    }
  }
}

__global__ void __launch_bounds__(kRegBlock) reg_bwd_kernel(RegPack p) {
  const int b = blockIdx.x, t = reg_term_of(p, b);
  if (!p.grad[t]) return;
  const long n = p.n[t], base = (long) (b - p.first[t]) * kRegTile;
  const int kind = p.kind[t];
  const bool bf = p.bf16[t] != 0;
  const bool want1 = p.side[t] != VAMP_REG_CLEAR, want0 = p.side[t] != VAMP_REG_SET;
  const double gl = (double) p.grad_losses[t];
  const double cnt1 = (double) p.counts[2 * t], cnt0 = (double) p.counts[2 * t + 1];
#pragma unroll
  for (int r = 0; r < kRegRounds; ++r) {
    const long i0 = base + (long) r * (kRegBlock * kRegVec) + (long) threadIdx.x * kRegVec;
    if (i0 >= n) continue;
    const RegGroup g = reg_load(p, t, i0, n);
    float out[kRegVec];
#pragma unroll
    for (int q = 0; q < kRegVec; ++q) {
      const bool m = (g.set >> q) & 1u;
      out[q] = 0.0f;
      if (((g.live >> q) & 1u) && (m ? want1 : want0)) {
        const float d = g.pv[q] - g.tv[q];
        double lp;
        if (kind == VAMP_REG_MSE) lp = 2.0 * (double) d;
        else lp = fabsf(d) < 1.0f ? (double) d : (d > 0.0f ? 1.0 : (d < 0.0f ? -1.0 : (double) d));  // (NaN)
        out[q] = (float) (gl * lp / (m ? cnt1 : cnt0));
      }
    }
    if (g.live == 0xFu && p.vec[t]) {
      if (bf) {
        uint2 w;
        w.x = f32_to_bf16(out[0]) | ((uint32_t) f32_to_bf16(out[1]) << 16);
        w.y = f32_to_bf16(out[2]) | ((uint32_t) f32_to_bf16(out[3]) << 16);
        *reinterpret_cast<uint2*>(static_cast<uint16_t*>(p.grad[t]) + i0) = w;
      } else {
        *reinterpret_cast<float4*>(static_cast<float*>(p.grad[t]) + i0) = make_float4(out[0], out[1], out[2], out[3]);
      }
    } else {
#pragma unroll
      for (int q = 0; q < kRegVec; ++q) {
        if (!((g.live >> q) & 1u)) continue;
        if (bf) static_cast<uint16_t*>(p.grad[t])[i0 + q] = f32_to_bf16(out[q]);
        else static_cast<float*>(p.grad[t])[i0 + q] = out[q];
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------
static_assert(sizeof(VampRegTerm) == 32, "VampRegTerm layout: part of the ABI (the binding reads it from include/vampire_hip.h)");
static_assert(sizeof(VampRegLossDesc) == 8 + 32 * VAMP_REG_MAX_TERMS, "VampRegLossDesc layout");

int reg_validate(const VampRegLossDesc* d) {
  VAMP_REQUIRE(d, "desc is NULL");
  VAMP_REQUIRE(d->T >= 1 && d->T <= VAMP_REG_MAX_TERMS, "T must be in [1, 8]");
  VAMP_REQUIRE(d->reserved == 0, "reserved must be 0");
  for (int t = 0; t < d->T; ++t) {
    const VampRegTerm& m = d->terms[t];
    VAMP_REQUIRE(m.n >= 1 && m.n < (1L << 31), "n must be in [1, 2^31)");
    VAMP_REQUIRE(m.kind == VAMP_REG_SMOOTH_L1 || m.kind == VAMP_REG_MSE, "kind must be VAMP_REG_SMOOTH_L1 or VAMP_REG_MSE");
    VAMP_REQUIRE(m.side == VAMP_REG_SET || m.side == VAMP_REG_CLEAR || m.side == VAMP_REG_BOTH,
                 "side must be VAMP_REG_SET, VAMP_REG_CLEAR or VAMP_REG_BOTH");
    VAMP_REQUIRE(m.pred_dtype == VAMP_F32 || m.pred_dtype == VAMP_BF16, "pred_dtype must be VAMP_F32 or VAMP_BF16");
    VAMP_REQUIRE(m.target_is_const == 0 || m.target_is_const == 1, "target_is_const must be 0 or 1");
    VAMP_REQUIRE(m.reserved == 0, "reserved must be 0");
  }
  return VAMP_OK;
}

// the descriptor and the operands into the kernels' argument; grad_host == nullptr: the forward
int reg_pack(const VampRegLossDesc* d, const void* const* pred, const float* const* target, const uint8_t* const* mask,
             void* const* grad, RegPack* q) {
  VAMP_REQUIRE(pred && target && mask, "a pointer array is NULL");
  q->T = d->T;
  long blocks = 0;
  for (int t = 0; t < d->T; ++t) {
    const VampRegTerm& m = d->terms[t];
    VAMP_REQUIRE(pred[t], "a pred pointer is NULL");
    VAMP_REQUIRE(m.target_is_const || target[t], "a target pointer is NULL and the term has no constant");
    VAMP_REQUIRE(mask[t] || m.side == VAMP_REG_SET, "side CLEAR or BOTH needs a mask");
    const bool bf = m.pred_dtype == VAMP_BF16;
    q->pred[t] = pred[t];
    q->target[t] = m.target_is_const ? nullptr : target[t];
    q->mask[t] = mask[t];
    q->grad[t] = grad ? grad[t] : nullptr;
    q->n[t] = m.n;
    q->first[t] = (int) blocks;
    q->cval[t] = m.target_value;
    q->kind[t] = (uint8_t) m.kind; q->side[t] = (uint8_t) m.side; q->bf16[t] = bf; q->cst[t] = (uint8_t) m.target_is_const;
    const uintptr_t ea = bf ? 8 : 16;
    q->vec[t] = aligned(pred[t], ea) && (m.target_is_const || aligned(target[t], 16)) &&
                (!mask[t] || aligned(mask[t], 4)) && (!q->grad[t] || aligned(q->grad[t], ea));
    blocks += (m.n + kRegTile - 1) / kRegTile;
  }
  q->first[d->T] = (int) blocks;
  for (int t = d->T + 1; t <= VAMP_REG_MAX_TERMS; ++t) q->first[t] = (int) blocks;
  return VAMP_OK;
}

size_t reg_blocks(const VampRegLossDesc* d) {
  size_t blocks = 0;
  for (int t = 0; t < d->T; ++t) blocks += (size_t) ((d->terms[t].n + kRegTile - 1) / kRegTile);
  return blocks;
}

// the forward's two tables of per-workgroup partials carved from `workspace` (NULL: only the returned size is of use)
size_t reg_workspace(const VampRegLossDesc* d, RegPack* q, void* workspace) {
  const size_t blocks = reg_blocks(d);
  Carve c(workspace);
  q->psum = c.take<double>(blocks * 2);
  q->pcnt = c.take<int>(blocks * 2);
  return c.off;
}

}  // namespace
}  // namespace vamp

using namespace vamp;

extern "C" {

size_t vamp_reg_loss_workspace_bytes(const VampRegLossDesc* d) {
  if (reg_validate(d)) return 0;
  RegPack q{};
  return reg_workspace(d, &q, nullptr);
}

int vamp_reg_loss_forward(const VampRegLossDesc* d, const void* const* pred_host, const float* const* target_host,
                          const uint8_t* const* mask_host, float* losses, int64_t* counts, void* workspace,
                          size_t workspace_bytes, void* stream) {
  if (int e = reg_validate(d)) return e;
  RegPack q{};
  if (int e = reg_pack(d, pred_host, target_host, mask_host, nullptr, &q)) return e;
  VAMP_REQUIRE(losses && counts, "an output pointer is NULL");
  if (int e = workspace_fits(__func__, workspace, workspace_bytes, reg_workspace(d, &q, workspace), VAMP_EINVAL)) return e;
  VAMP_REQUIRE(aligned(workspace, 8), "the workspace must be 8-byte aligned");
  q.losses = losses;
  q.counts = counts;
  hipStream_t st = static_cast<hipStream_t>(stream);
  VAMP_TIMED(kProfAux, st, (reg_partial_kernel<<<(unsigned) reg_blocks(d), kRegBlock, 0, st>>>(q)));
  VAMP_TIMED(kProfAux, st, (reg_finish_kernel<<<1, kRegBlock, 0, st>>>(q)));
  return check_launch("reg_loss_forward");
}

int vamp_reg_loss_backward(const VampRegLossDesc* d, const void* const* pred_host, const float* const* target_host,
                           const uint8_t* const* mask_host, const int64_t* counts, const float* grad_losses,
                           void* const* grad_pred_host, void* stream) {
  if (int e = reg_validate(d)) return e;
  VAMP_REQUIRE(grad_pred_host, "a pointer array is NULL");
  RegPack q{};
  if (int e = reg_pack(d, pred_host, target_host, mask_host, grad_pred_host, &q)) return e;
  VAMP_REQUIRE(counts && grad_losses, "an input pointer is NULL");
  q.counts = const_cast<int64_t*>(counts);
  q.grad_losses = grad_losses;
  hipStream_t st = static_cast<hipStream_t>(stream);
  VAMP_TIMED(kProfAux, st, (reg_bwd_kernel<<<(unsigned) reg_blocks(d), kRegBlock, 0, st>>>(q)));
  return check_launch("reg_loss_backward");
}

}  // extern "C"
