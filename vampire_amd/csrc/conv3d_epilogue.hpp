// The epilogue of the 3x3x3 convolutions (conv3d.hip, conv3d_bf16.hip, conv3d_bf16_s2.hip): what a kernel does to an
// accumulator at the point where it stores it -- y = act(acc + bias + residual), per segment of output channels, each
// segment into a tensor of its own -- and the host-side check of the descriptor that all entry points share.
// The arithmetic is fp32, in that order, one rounding per step (the library is built without contraction), and the
// result is rounded once to the segment's output type.
#pragma once
#include "common.hpp"
#include "elem16.hpp"

#include <math.h>

namespace vamp {
namespace {

// compute type of a kernel: what its operands are and what a segment stores unless it asks for fp32
enum { kEpiF32 = 0, kEpiBF16 = 1, kEpiF16 = 2 };

// The segment that holds output channel c, as values: the descriptor lives in the kernel arguments, and a lane-varying
// index into it would be copied to scratch -- four constant-index reads and selects are not.
struct EpiSel {
  const float* bias;
  const void* residual;
  void* out;
  const void* grad_out;
  int cc, nch, act, f32;       // cc: the channel inside its segment
  float slope;
  bool hit;                    // false: no segment holds the channel, nothing is stored for it
};

__device__ __forceinline__ EpiSel epi_select(const VampConvEpilogue& ep, int c) {
  EpiSel s{nullptr, nullptr, nullptr, nullptr, 0, 1, VAMP_ACT_NONE, 0, 0.f, false};
#pragma unroll
  for (int i = 0; i < VAMP_CONV_EPI_MAX_SEGS; ++i) {
    const VampConvEpiSeg& g = ep.seg[i];
    if (i < ep.nseg && c >= g.c0 && c < g.c0 + g.nch) {
      s.bias = g.bias; s.residual = g.residual; s.out = g.out; s.grad_out = g.grad_out;
      s.cc = c - g.c0; s.nch = g.nch; s.act = g.act; s.f32 = g.out_f32; s.slope = g.slope;
      s.hit = true;
    }
  }
  return s;
}

typedef float epi_f32x4 __attribute__((ext_vector_type(4)));

// element i of a tensor of the segment's output type
template <int KIND>
__device__ __forceinline__ float epi_load(const void* p, long i, int f32) {
  if (KIND == kEpiF32 || f32) return static_cast<const float*>(p)[i];
  const uint16_t u = static_cast<const uint16_t*>(p)[i];
  return KIND == kEpiF16 ? f16_to_f32(u) : bf16_to_f32(u);
}
template <int KIND>
__device__ __forceinline__ void epi_put(void* p, long i, int f32, float v) {
  if (KIND == kEpiF32 || f32) static_cast<float*>(p)[i] = v;
  else static_cast<uint16_t*>(p)[i] = f32_to_e16<KIND == kEpiF16>(v);
}

__device__ __forceinline__ float epi_act(int act, float slope, float v) {
  if (act == VAMP_ACT_LEAKY_RELU) return v > 0.f ? v : v * slope;
  if (act == VAMP_ACT_SIGMOID) return 1.f / (1.f + expf(-v));
  return v;
}

// acc -> the stored value of (sample b, the selected channel, voxel `vox` of a `plane`-voxel output volume);
// bv = the channel's bias (read once by the caller), has_bias = the segment has one
template <int KIND>
__device__ __forceinline__ void epi_store(const EpiSel& s, bool has_bias, float bv, long b, long plane, long vox,
                                          float acc) {
  const long i = (b * s.nch + s.cc) * plane + vox;
  float v = acc;
  if (has_bias) v = v + bv;
  if (s.residual) v = v + epi_load<KIND>(s.residual, i, s.f32);
  epi_put<KIND>(s.out, i, s.f32, epi_act(s.act, s.slope, v));
}

// The store of a 16-bit kernel's accumulator tile: this lane's rows are the channels m * 16 + 4 kg + rg, its columns
// the voxels rowoff + x0 + 16 n + li (x0 + 16 n + li < X) of sample b.  OF32: the segments store fp32 (one call's
// segments share the type, so that it is a compile-time property of the store).  Two phases: every bias and residual
// load of the tile first, each into a register of its own; then the arithmetic and the stores with no load between
// them -- a load between two stores makes the wave wait for the earlier store to complete (one vmcnt counter), a
// memory round trip per element.  What varies per lane (a channel's segment: bias, residual, activation) is
// selected, not branched on; only the sigmoid is a branch.  The loads are unconditional for the same reason (a
// load inside a branch is waited for inside it): a lane without a bias or residual, or outside the volume, reads
// `safe` instead -- any readable 4 bytes, the kernel's weights -- and drops the value.
template <int KIND, bool OF32, int MT, int NN>
__device__ __forceinline__ void epi_store_tile(const VampConvEpilogue& ep, const epi_f32x4 (&acc)[MT][NN], int kg, int li,
                                               long b, long plane, long rowoff, int x0, int X, const void* safe) {
  unsigned rv[MT][4][NN];        // the residuals as loaded (widened in the second phase: a use here would wait here)
  float bv[MT][4];
  if (ep.nseg == 1) {
    // an ordinary layer: the segment's fields are the same for every lane (scalar registers, scalar branches); only
    // whether a lane's channel lies in the segment varies
    const VampConvEpiSeg& g = ep.seg[0];
    const bool has_b = g.bias != nullptr, has_r = g.residual != nullptr;
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
      for (int rg = 0; rg < 4; ++rg) {
        const int cc = m * 16 + 4 * kg + rg - g.c0;
        const bool hit = cc >= 0 && cc < g.nch;
        bv[m][rg] = has_b ? *(hit ? g.bias + cc : static_cast<const float*>(safe)) : 0.f;
        const long cb = (b * g.nch + cc) * plane + rowoff;
        if (has_r) {
#pragma unroll
          for (int n = 0; n < NN; ++n) {
            const int x = x0 + n * 16 + li;
            const bool use = hit && x < X;
            if (OF32) rv[m][rg][n] = *(use ? static_cast<const unsigned*>(g.residual) + (cb + x) : static_cast<const unsigned*>(safe));
            else rv[m][rg][n] = *(use ? static_cast<const uint16_t*>(g.residual) + (cb + x) : static_cast<const uint16_t*>(safe));
          }
        }
      }
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
      for (int rg = 0; rg < 4; ++rg) {
        const int cc = m * 16 + 4 * kg + rg - g.c0;
        const bool hit = cc >= 0 && cc < g.nch;
        const long cb = (b * g.nch + cc) * plane + rowoff;
#pragma unroll
        for (int n = 0; n < NN; ++n) {
          const int x = x0 + n * 16 + li;
          float v = acc[m][n][rg];
          if (has_b) v = v + bv[m][rg];
          if (has_r)
            v = v + (OF32 ? __uint_as_float(rv[m][rg][n])
                          : (KIND == kEpiF16 ? f16_to_f32((uint16_t) rv[m][rg][n]) : bf16_to_f32((uint16_t) rv[m][rg][n])));
          v = epi_act(g.act, g.slope, v);
          if (hit && x < X) epi_put<KIND>(g.out, cb + x, OF32, v);
        }
      }
    return;
  }
#pragma unroll
  for (int m = 0; m < MT; ++m)
#pragma unroll
    for (int rg = 0; rg < 4; ++rg) {
      const EpiSel sel = epi_select(ep, m * 16 + 4 * kg + rg);       // (channels >= cout lie in no segment)
      bv[m][rg] = *((sel.hit && sel.bias) ? sel.bias + sel.cc : static_cast<const float*>(safe));
      const long cb = (b * sel.nch + sel.cc) * plane + rowoff;
#pragma unroll
      for (int n = 0; n < NN; ++n) {
        const int x = x0 + n * 16 + li;
        const bool use = sel.hit && sel.residual && x < X;
        if (OF32) rv[m][rg][n] = *(use ? static_cast<const unsigned*>(sel.residual) + (cb + x) : static_cast<const unsigned*>(safe));
        else rv[m][rg][n] = *(use ? static_cast<const uint16_t*>(sel.residual) + (cb + x) : static_cast<const uint16_t*>(safe));
      }
    }
#pragma unroll
  for (int m = 0; m < MT; ++m)
#pragma unroll
    for (int rg = 0; rg < 4; ++rg) {
      const EpiSel sel = epi_select(ep, m * 16 + 4 * kg + rg);
      const long cb = (b * sel.nch + sel.cc) * plane + rowoff;
#pragma unroll
      for (int n = 0; n < NN; ++n) {
        const int x = x0 + n * 16 + li;
        float v = acc[m][n][rg];
        v = sel.bias ? v + bv[m][rg] : v;
        const float r = OF32 ? __uint_as_float(rv[m][rg][n])
                             : (KIND == kEpiF16 ? f16_to_f32((uint16_t) rv[m][rg][n]) : bf16_to_f32((uint16_t) rv[m][rg][n]));
        v = sel.residual ? v + r : v;
        const float lk = v > 0.f ? v : v * sel.slope;
        v = sel.act == VAMP_ACT_LEAKY_RELU ? lk : v;
        if (sel.act == VAMP_ACT_SIGMOID) v = 1.f / (1.f + expf(-v));
        if (sel.hit && x < X) epi_put<KIND>(sel.out, cb + x, OF32, v);
      }
    }
}

// ---------------------------------------------------------------------------
// host: the descriptor's rules, before any launch.  `half`: a 16-bit kind (only those may store fp32 from the "other
// dtype" slot); `mode`: 0 = structure only (the *_supported answer), 1 = forward pointers, 2 = backward pointers.
// ---------------------------------------------------------------------------
inline int epi_check(const char* who, const VampConvDesc* d, const VampConvEpilogue* e, bool half, int mode) {
#define VAMP_EPI_REQ(cond, msg)                                                                       \
  do {                                                                                                \
    if (!(cond)) return ::vamp::fail(VAMP_EINVAL, "%s: requirement failed: " msg, who);               \
  } while (0)
  VAMP_EPI_REQ(d != nullptr && e != nullptr, "descriptor or epilogue is NULL");
  VAMP_EPI_REQ(e->nseg >= 1 && e->nseg <= VAMP_CONV_EPI_MAX_SEGS, "1 <= nseg <= 4");
  for (int i = 0; i < e->nseg; ++i) {
    const VampConvEpiSeg& g = e->seg[i];
    VAMP_EPI_REQ(g.c0 >= 0 && g.nch >= 1 && g.c0 <= d->cout - g.nch, "segment outside [0, cout)");
    VAMP_EPI_REQ(g.act == VAMP_ACT_NONE || g.act == VAMP_ACT_LEAKY_RELU || g.act == VAMP_ACT_SIGMOID,
                 "unknown activation");
    VAMP_EPI_REQ(g.out_f32 == 0 || g.out_f32 == 1, "out_f32 must be 0 or 1");
    VAMP_EPI_REQ(half || g.out_f32 == 0, "out_f32 is for the 16-bit kinds: the fp32 kind stores fp32 already");
    VAMP_EPI_REQ(g.out_f32 == e->seg[0].out_f32, "the segments of one call share out_f32");
    VAMP_EPI_REQ(g.slope == g.slope, "slope is NaN");
    for (int j = 0; j < i; ++j)
      VAMP_EPI_REQ(g.c0 >= e->seg[j].c0 + e->seg[j].nch || e->seg[j].c0 >= g.c0 + g.nch, "segments overlap");
    if (mode == 1) {
      VAMP_EPI_REQ(g.out != nullptr, "NULL segment output");
      VAMP_EPI_REQ(aligned(g.out, 16) && aligned(g.residual, 16) && aligned(g.bias, 16),
                   "segment tensors must start on a 16-byte boundary");
    } else if (mode == 2) {
      VAMP_EPI_REQ(g.grad_out != nullptr, "NULL segment gradient");
      VAMP_EPI_REQ(g.act == VAMP_ACT_NONE || g.out != nullptr, "an activation's backward needs the segment's output");
    }
  }
#undef VAMP_EPI_REQ
  return VAMP_OK;
}

}  // namespace
}  // namespace vamp
