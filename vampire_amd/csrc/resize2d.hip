// 2-D bilinear resize of the rendered maps between render and losses, gfx950:
// `F.interpolate(x, size, mode='bilinear', align_corners=True)` on [planes, ih, iw] -> [planes, oh, ow], fp32 --
// the x4 `upsample2d` of the three camera maps (base_vampire2.py:616-626) and the 0.5x resize behind
// `voxel_output`'s 1x1 convolution on a 256-cell grid (base_vampire2.py:203-209), forward and backward.
//
// One call takes up to VAMP_RESIZE2D_MAX_SEGS tensors that share ih, iw, oh, ow (rgb, seg logits and depth are one
// launch each way); the segment pointers travel by value in the kernel arguments, so a call is one kernel launch on
// the caller's stream and nothing else: no table upload, no host memory the device reads later.
//
// Index / weight arithmetic follows aten (area_pixel_compute_source_index with align_corners=True), in fp32:
// scale = (in - 1) / (out - 1) (0 when out == 1), src = scale * o, i0 = (int) src, i1 = i0 + (i0 < in - 1),
// l1 = src - i0, l0 = 1 - l1; blend h0 * (w0 * a + w1 * b) + h1 * (w0 * c + w1 * d).
//
// Forward: store-bound.  A thread computes the taps of four neighbouring outputs of one row once, walks a group of
// planes with them and writes 16 bytes per plane; the low-resolution input is re-read from L1 / L2.
//
// Backward: aten scatters with float atomics.  Here it is a separable gather in one fixed order.  Along one axis
// the outputs whose taps include source index i are the contiguous run [F(i - 1), F(i + 1)), F(v) = first output
// with i0 >= v (i0 is monotone in o).  A workgroup owns (plane, band of kBandRows source rows, kBlock source
// columns); it streams the gradient rows [F(y0 - 1), F(y1)) that touch the band, kStageRows at a time with 16-byte
// loads into an LDS strip, a thread reduces each row along x over the run of its source column (weights in
// registers), and folds the row sums along y into two running accumulators (rows i0 and i0 + 1 of the walk); a
// source row is stored when the walk leaves it, rows and columns nothing touches as 0.  Each gradient element is
// read once, but for the rows two neighbouring bands share.  No atomics, no zero fill, bitwise repeatable; the same
// kernel serves out > in, the identity and out < in (runs of one or two outputs).
#include "common.hpp"

namespace vamp {
namespace {

constexpr int kBlock = VAMP_RESIZE2D_COL_CHUNK;            // threads: one per source column of the backward
constexpr int kMaxSegs = VAMP_RESIZE2D_MAX_SEGS;
constexpr int kFwdPlanes = VAMP_RESIZE2D_PLANE_GROUP;   // planes a forward thread walks with one set of taps
constexpr int kBandRows = VAMP_RESIZE2D_BAND_ROWS;      // source rows per backward workgroup
constexpr int kStripChunk = VAMP_RESIZE2D_STRIP_CHUNK;  // gradient columns one wave-wide 16-byte load covers
constexpr int kStripMax = VAMP_RESIZE2D_STRIP_MAX;      // gradient columns of the LDS strip (per row)
constexpr int kStageRows = 4;                           // gradient rows staged per step: one per wave
constexpr int kMaxRun = VAMP_RESIZE2D_MAX_RUN;          // outputs per source column the weight registers hold
// strip element a lives at a + (a >> 5): a thread's run starts about `ratio` elements after its neighbour's, and at
// the x4 of the camera maps 32 lanes would meet on 8 banks without the skew
constexpr int kStripStride = kStripMax + kStripMax / 32;
static_assert(kBlock == 64 * kStageRows && kStripChunk == 4 * kWave && kStripMax % 4 == 0, "staging shape");

struct Seg {
  const float* src;     // forward: in, backward: grad_out
  float* dst;           // forward: out, backward: grad_in
  int planes;
};
struct Args {
  Seg seg[kMaxSegs];
  int nseg, ih, iw, oh, ow;
  float sy, sx;         // (in - 1) / (out - 1) per axis, divided on the host
};

float axis_scale(int in, int out) { return out > 1 ? (float) (in - 1) / (float) (out - 1) : 0.f; }

struct Tap {
  int i0, i1;
  float l0, l1;
};
__host__ __device__ __forceinline__ Tap axis_tap(float scale, int o, int in) {
  const float src = scale * (float) o;
  Tap t;
  t.i0 = (int) src;
  t.i1 = t.i0 + ((t.i0 < in - 1) ? 1 : 0);
  t.l1 = src - (float) t.i0;
  t.l0 = 1.0f - t.l1;
  return t;
}

// F(v): the first output o in [0, out] whose i0 is >= v.  The estimate only places the start of the search; the two
// loops make the answer exact whatever the division rounds to.
__host__ __device__ __forceinline__ int first_at_least(float scale, int out, int v) {
  if (v <= 0) return 0;
  int o = 0;
  if (scale > 0.f) {
    const float e = (float) v / scale - 2.f;
    o = e > 0.f ? (e < (float) out ? (int) e : out) : 0;
  }
  while (o > 0 && (int) (scale * (float) (o - 1)) >= v) --o;
  while (o < out && (int) (scale * (float) o) < v) ++o;
  return o;
}

// the segment that holds unit `u` when every segment contributes ceil(planes / per) units; u becomes the index
// inside the segment.  Selects over the unrolled loop: the kernel arguments are never indexed dynamically.
__device__ __forceinline__ Seg find_segment(const Args& a, int per, int& u) {
  Seg s = a.seg[0];
  bool found = false;
#pragma unroll
  for (int k = 0; k < kMaxSegs; ++k) {
    if (k < a.nseg && !found) {
      const int units = (a.seg[k].planes + per - 1) / per;
      if (u < units) {
        s = a.seg[k];
        found = true;
      } else {
        u -= units;
      }
    }
  }
  return s;
}

// thread per VEC neighbouring outputs of one row, kFwdPlanes planes per thread
template <int VEC>
__global__ void __launch_bounds__(kBlock)
resize2d_fwd_kernel(const Args a) {
  const int owv = a.ow / VEC;
  const unsigned idx = blockIdx.x * (unsigned) kBlock + threadIdx.x;
  if (idx >= (unsigned) a.oh * (unsigned) owv) return;
  const int oy = (int) (idx / (unsigned) owv), ox = (int) (idx % (unsigned) owv) * VEC;
  int group = blockIdx.y;
  const Seg s = find_segment(a, kFwdPlanes, group);
  const Tap ty = axis_tap(a.sy, oy, a.ih);
  Tap tx[VEC];
#pragma unroll
  for (int v = 0; v < VEC; ++v) tx[v] = axis_tap(a.sx, ox + v, a.iw);
  const int r0 = ty.i0 * a.iw, r1 = ty.i1 * a.iw;
  const long ipix = (long) a.ih * a.iw, opix = (long) a.oh * a.ow;
  const int p0 = group * kFwdPlanes, p1 = min(s.planes, p0 + kFwdPlanes);
  // where all taps of the VEC outputs lie in the three source columns c0 .. c0 + 2 (ratios from about 1.5 up):
  // 6 loads per plane instead of 16, every tap picks its column by its distance 0, 1 or 2 from c0 -- i0 too, which is
  // c0 + 2 where the last output of a row sits on the last source column (i0 == i1 == iw - 1); same values, same
  // arithmetic as the general path
  const int c0 = tx[0].i0, c1 = min(c0 + 1, a.iw - 1), c2 = min(c0 + 2, a.iw - 1);
  const bool narrow = VEC > 1 && tx[VEC - 1].i1 - c0 <= 2;
  float* const q0 = s.dst + (long) oy * a.ow + ox;
  auto store = [&](int pl, const float (&r)[VEC]) {
    float* q = q0 + pl * opix;
    if constexpr (VEC == 4) {
      *reinterpret_cast<float4*>(q) = make_float4(r[0], r[1], r[2], r[3]);
    } else {
      q[0] = r[0];
    }
  };
  // the loads of a batch of planes are issued before its first store (the compiler may not move a load over a store
  // to memory it cannot tell apart): kBatch planes' latencies overlap
  if (narrow) {
    constexpr int kBatch = 4;
    for (int pb = p0; pb < p1; pb += kBatch) {
      float t[kBatch][6];
#pragma unroll
      for (int j = 0; j < kBatch; ++j) {
        const float* p = s.src + min(pb + j, p1 - 1) * ipix;
        t[j][0] = p[r0 + c0], t[j][1] = p[r0 + c1], t[j][2] = p[r0 + c2];
        t[j][3] = p[r1 + c0], t[j][4] = p[r1 + c1], t[j][5] = p[r1 + c2];
      }
#pragma unroll
      for (int j = 0; j < kBatch; ++j) {
        if (pb + j < p1) {
          float r[VEC];
#pragma unroll
          for (int v = 0; v < VEC; ++v) {
            const int d0 = tx[v].i0 - c0, d1 = tx[v].i1 - c0;
            const float va = d0 == 0 ? t[j][0] : (d0 == 1 ? t[j][1] : t[j][2]);
            const float vb = d1 == 0 ? t[j][0] : (d1 == 1 ? t[j][1] : t[j][2]);
            const float vc = d0 == 0 ? t[j][3] : (d0 == 1 ? t[j][4] : t[j][5]);
            const float vd = d1 == 0 ? t[j][3] : (d1 == 1 ? t[j][4] : t[j][5]);
            r[v] = ty.l0 * (tx[v].l0 * va + tx[v].l1 * vb) + ty.l1 * (tx[v].l0 * vc + tx[v].l1 * vd);
          }
          store(pb + j, r);
        }
      }
    }
  } else {
    constexpr int kBatch = 2;
    for (int pb = p0; pb < p1; pb += kBatch) {
      float t[kBatch][VEC][4];
#pragma unroll
      for (int j = 0; j < kBatch; ++j) {
        const float* p = s.src + min(pb + j, p1 - 1) * ipix;
#pragma unroll
        for (int v = 0; v < VEC; ++v)
          t[j][v][0] = p[r0 + tx[v].i0], t[j][v][1] = p[r0 + tx[v].i1], t[j][v][2] = p[r1 + tx[v].i0], t[j][v][3] = p[r1 + tx[v].i1];
      }
#pragma unroll
      for (int j = 0; j < kBatch; ++j) {
        if (pb + j < p1) {
          float r[VEC];
#pragma unroll
          for (int v = 0; v < VEC; ++v)   // aten's nesting (UpSampleBilinear2d.cu)
            r[v] = ty.l0 * (tx[v].l0 * t[j][v][0] + tx[v].l1 * t[j][v][1]) + ty.l1 * (tx[v].l0 * t[j][v][2] + tx[v].l1 * t[j][v][3]);
          store(pb + j, r);
        }
      }
    }
  }
}

__device__ __forceinline__ int strip_at(int a) { return a + (a >> 5); }

// workgroup per (plane, band of source rows, kBlock source columns); MH = outputs per source column the x loop is
// unrolled for; VEC: the gradient rows are read with 16-byte loads (ow % 4 == 0, 16-byte aligned base)
template <int MH, bool VEC>
__global__ void __launch_bounds__(kBlock)
resize2d_bwd_kernel(const Args a) {
  __shared__ float strip[kStageRows * kStripStride];
  const int nchunk = (a.iw + kBlock - 1) / kBlock, nband = (a.ih + kBandRows - 1) / kBandRows;
  const int chunk = (int) (blockIdx.x % (unsigned) nchunk);
  const int band = (int) ((blockIdx.x / (unsigned) nchunk) % (unsigned) nband);
  int pl = (int) (blockIdx.x / ((unsigned) nchunk * (unsigned) nband));
  const Seg s = find_segment(a, 1, pl);
  const int x0 = chunk * kBlock, x1 = min(a.iw, x0 + kBlock);
  const int y0 = band * kBandRows, y1 = min(a.ih, y0 + kBandRows);
  // gradient columns the chunk's runs cover, from a multiple of 4 (the host has checked that they fit the strip)
  const int ob = first_at_least(a.sx, a.ow, x0 - 1) & ~3;
  const int oe = min(first_at_least(a.sx, a.ow, x1), ob + kStripMax);
  const int rb = first_at_least(a.sy, a.oh, y0 - 1), re = first_at_least(a.sy, a.oh, y1);

  // this thread's source column: its run of outputs and their weights
  const int x = x0 + threadIdx.x;
  const bool live = x < x1;
  int rel = 0, n = 0;
  float w[MH];
#pragma unroll
  for (int k = 0; k < MH; ++k) w[k] = 0.f;
  if (live) {
    const int begin = first_at_least(a.sx, a.ow, x - 1);
    n = min(first_at_least(a.sx, a.ow, x + 1) - begin, MH);
    rel = begin - ob;
#pragma unroll
    for (int k = 0; k < MH; ++k) {
      if (k < n) {
        const Tap t = axis_tap(a.sx, begin + k, a.iw);
        w[k] = (t.i0 == x ? t.l0 : 0.f) + (t.i1 == x ? t.l1 : 0.f);
      }
    }
  }

  const float* g = s.src + (long) pl * a.oh * a.ow;
  float* gin = s.dst + (long) pl * a.ih * a.iw;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  int cur = y0 - 1;                    // the walk: acc_lo belongs to source row cur, acc_hi to cur + 1
  float acc_lo = 0.f, acc_hi = 0.f;
  for (int r = rb; r < re; r += kStageRows) {
    __syncthreads();                   // the previous step's readers are done with the strip
    if (r + wave < re) {               // wave w stages gradient row r + w
      const float* row = g + (long) (r + wave) * a.ow;
      float* dst = strip + wave * kStripStride;
      if constexpr (VEC) {
        for (int c = ob + 4 * lane; c < oe; c += kStripChunk) {
          const float4 v = *reinterpret_cast<const float4*>(row + c);
          const int e = c - ob;
          dst[strip_at(e)] = v.x;
          dst[strip_at(e + 1)] = v.y;
          dst[strip_at(e + 2)] = v.z;
          dst[strip_at(e + 3)] = v.w;
        }
      } else {
        for (int c = ob + lane; c < oe; c += kWave) dst[strip_at(c - ob)] = row[c];
      }
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < kStageRows; ++q) {
      if (r + q < re) {                // uniform
        const Tap t = axis_tap(a.sy, r + q, a.ih);
        while (cur < t.i0) {           // the walk leaves row cur: it is complete
          if (live && cur >= y0) gin[(long) cur * a.iw + x] = acc_lo;
          acc_lo = acc_hi;
          acc_hi = 0.f;
          ++cur;
        }
        const float* src = strip + q * kStripStride;
        float sum = 0.f;
#pragma unroll
        for (int k = 0; k < MH; ++k)
          if (k < n) sum += w[k] * src[strip_at(rel + k)];
        acc_lo += t.l0 * sum;
        if (t.i1 == t.i0) acc_lo += t.l1 * sum;
        else acc_hi += t.l1 * sum;
      }
    }
  }
  for (; cur < y1; ++cur) {
    if (live && cur >= y0) gin[(long) cur * a.iw + x] = acc_lo;
    acc_lo = acc_hi;
    acc_hi = 0.f;
  }
}

bool run_fits(int in, int out, int hits) {
  if (in == 1) return out <= hits;
  return 2L * (out - 1) / (in - 1) + 2 <= hits;
}

// every chunk of kBlock source columns finds the gradient columns of its runs inside the LDS strip
bool strip_fits(int iw, int ow) {
  const float sx = axis_scale(iw, ow);
  for (int x0 = 0; x0 < iw; x0 += kBlock) {
    const int x1 = x0 + kBlock < iw ? x0 + kBlock : iw;
    const int ob = first_at_least(sx, ow, x0 - 1) & ~3, oe = first_at_least(sx, ow, x1);
    if ((oe - ob + 3) / 4 * 4 > kStripMax) return false;
  }
  return true;
}

bool supported(int ih, int iw, int oh, int ow) {
  if (ih <= 0 || iw <= 0 || oh <= 0 || ow <= 0) return false;
  if ((long) ih * iw >= 0x7fffffffL || (long) oh * ow >= 0x7fffffffL) return false;
  return run_fits(iw, ow, kMaxRun) && strip_fits(iw, ow);
}

int check_desc(const VampResize2dDesc* d, Args* a, long* planes) {
  VAMP_REQUIRE(d != nullptr, "desc is NULL");
  VAMP_REQUIRE(d->ih > 0 && d->iw > 0 && d->oh > 0 && d->ow > 0, "sizes must be positive");
  VAMP_REQUIRE((long) d->ih * d->iw < 0x7fffffffL && (long) d->oh * d->ow < 0x7fffffffL, "plane too large");
  VAMP_REQUIRE(d->nseg >= 1 && d->nseg <= kMaxSegs, "1 <= nseg <= 4");
  *planes = 0;
  for (int k = 0; k < d->nseg; ++k) {
    VAMP_REQUIRE(d->seg[k].planes > 0 && d->seg[k].planes < 65536, "0 < planes (batch * channels) < 65536 per segment");
    VAMP_REQUIRE(d->seg[k].src && d->seg[k].dst, "NULL tensor");
    a->seg[k].src = static_cast<const float*>(d->seg[k].src);
    a->seg[k].dst = static_cast<float*>(d->seg[k].dst);
    a->seg[k].planes = (int) d->seg[k].planes;
    *planes += d->seg[k].planes;
  }
  for (int k = d->nseg; k < kMaxSegs; ++k) a->seg[k] = Seg{nullptr, nullptr, 0};
  a->nseg = d->nseg;
  a->ih = d->ih, a->iw = d->iw, a->oh = d->oh, a->ow = d->ow;
  a->sy = axis_scale(d->ih, d->oh), a->sx = axis_scale(d->iw, d->ow);
  VAMP_REQUIRE(supported(d->ih, d->iw, d->oh, d->ow),
               "resize ratio outside the backward's run registers or LDS strip (about out / in <= 4.1 along x)");
  return VAMP_OK;
}

// every segment's hi-resolution tensor (forward: dst, backward: src) takes 16-byte accesses
bool wide_ok(const VampResize2dDesc* d, bool hi_is_dst) {
  if (d->ow % 4 != 0) return false;
  for (int k = 0; k < d->nseg; ++k) {
    const void* p = hi_is_dst ? d->seg[k].dst : d->seg[k].src;
    if (!aligned(p, 16)) return false;
  }
  return true;
}

template <int MH>
void launch_backward(const Args& a, bool vec, unsigned grid, hipStream_t s) {
  if (vec) {
    VAMP_TIMED(kProfResize2d, s, (resize2d_bwd_kernel<MH, true><<<grid, kBlock, 0, s>>>(a)));
  } else {
    VAMP_TIMED(kProfResize2d, s, (resize2d_bwd_kernel<MH, false><<<grid, kBlock, 0, s>>>(a)));
  }
}

}  // namespace
}  // namespace vamp

using namespace vamp;

extern "C" {

int vamp_resize2d_supported(int32_t ih, int32_t iw, int32_t oh, int32_t ow) {
  return supported(ih, iw, oh, ow) ? 1 : 0;
}

size_t vamp_resize2d_workspace_bytes(int32_t ih, int32_t iw, int32_t oh, int32_t ow) {
  return 0;   // the backward's run tables live in registers and LDS
}

int vamp_resize2d_forward(const VampResize2dDesc* d, void* stream) {
  Args a;
  long planes;
  if (int e = check_desc(d, &a, &planes)) return e;
  hipStream_t s = static_cast<hipStream_t>(stream);
  unsigned groups = 0;
  for (int k = 0; k < a.nseg; ++k) groups += (unsigned) ((a.seg[k].planes + kFwdPlanes - 1) / kFwdPlanes);
  const bool vec = wide_ok(d, true);
  const long threads = (long) a.oh * (vec ? a.ow / 4 : a.ow);
  const dim3 grid((unsigned) ((threads + kBlock - 1) / kBlock), groups);
  if (vec) {
    VAMP_TIMED(kProfResize2d, s, (resize2d_fwd_kernel<4><<<grid, kBlock, 0, s>>>(a)));
  } else {
    VAMP_TIMED(kProfResize2d, s, (resize2d_fwd_kernel<1><<<grid, kBlock, 0, s>>>(a)));
  }
  return check_launch("resize2d_fwd_kernel");
}

int vamp_resize2d_backward(const VampResize2dDesc* d, void* workspace, size_t workspace_bytes, void* stream) {
  Args a;
  long planes;
  if (int e = check_desc(d, &a, &planes)) return e;
  VAMP_REQUIRE(workspace_bytes >= vamp_resize2d_workspace_bytes(d->ih, d->iw, d->oh, d->ow), "workspace too small");
  hipStream_t s = static_cast<hipStream_t>(stream);
  const long nchunk = (a.iw + kBlock - 1) / kBlock, nband = (a.ih + kBandRows - 1) / kBandRows;
  VAMP_REQUIRE(planes * nchunk * nband < 0x7fffffffL, "too many workgroups");
  const unsigned grid = (unsigned) (planes * nchunk * nband);
  const bool vec = wide_ok(d, false);
  if (run_fits(a.iw, a.ow, 4)) launch_backward<4>(a, vec, grid, s);
  else if (run_fits(a.iw, a.ow, 10)) launch_backward<10>(a, vec, grid, s);
  else launch_backward<kMaxRun>(a, vec, grid, s);
  return check_launch("resize2d_bwd_kernel");
}

}  // extern "C"
