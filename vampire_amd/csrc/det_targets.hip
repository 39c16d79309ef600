// Detection training targets on the device: the reference head's get_targets (bev_depth_head.py:168-319, with
// mmdet3d's gaussian_radius / gaussian_2d / draw_heatmap_gaussian) for every task and every sample in two
// launches that never synchronise with the host:
//
//  (a) tgt_assign_kernel, one 256-lane workgroup per (sample, task): the task's boxes in slot order -- class by
//      class in the task's class order, ascending box index within a class -- from per-class counts and a
//      ballot scan over the sample's labels.  The box of slot k < max_objs runs the reference's fp32 chain
//      (size check, Gaussian radius, centre, range check) and writes its anno / ind / mask row, zeros when it is
//      skipped; the slots from the task's box count to max_objs are zeroed too, so the outputs need no memset.
//      Drawn boxes leave a draw record (class, x, y, radius) in slot order in the workspace, skipped ones a
//      record of class -1.
//  (b) tgt_heatmap_kernel, one workgroup per (sample, task, 32 x 8 pixel tile): the (sample, task)'s records are
//      staged in LDS in chunks of 256, those whose square misses the tile are dropped, and every pixel takes,
//      per class, the smallest exponent q / (2 sigma^2) of the records that cover it.  The stamp value is
//      exp(-q / (2 sigma^2)) in float64 (mmdet3d builds the stamp with numpy), zeroed below DBL_EPSILON, rounded
//      to fp32; exp and the rounding are monotone, so this is the max-merge of the stamps.  Every pixel of the
//      map is written, zeros included.
// The workspace needs no initialisation.  No atomics, no host synchronisation: the output is a pure function of
// the inputs and the launches can be captured in a graph.
#include <float.h>

#include <algorithm>
#include <cmath>

#include "common.hpp"
#include "wave_reduce.hpp"

namespace vamp {
namespace {

constexpr int kTgtMaxT = 8;
constexpr int kTgtMaxNcls = 4;
constexpr int kTgtBlock = 256;
constexpr int kTgtWaves = kTgtBlock / 64;
constexpr int kTileW = 32, kTileH = 8;             // heatmap tile: 32-pixel (128-byte) rows, 8 rows
constexpr int kTgtMaxB = 4096;
constexpr int kTgtMaxM = 1 << 20;
constexpr int kTgtMaxObjs = 8192;
constexpr int kTgtMaxSide = 8192;
constexpr float kTgtMaxRadius = 1073741824.0f;    // 2^30: a radius at or above it is skipped like a non-finite one

struct TgtParams {
  const float* boxes;
  const void* labels;
  float* heat;
  float* anno;
  int64_t* inds;
  uint8_t* masks;
  int4* rec;                         // [B, T, max_objs] draw records (cls, x, y, r); cls -1: nothing to draw
  int* nrec;                         // [B, T] min(boxes of the task, max_objs)
  long heat_off[kTgtMaxT];           // element offset of task t's [B, ncls, fh, fw] block
  int ncls[kTgtMaxT], flag[kTgtMaxT];
  int B, T, M, cols, code, max_objs, fh, fw, min_radius, norm_bbox, lab64, ntx;
  // the reference divides 0-dim device tensors by CPU scalars, which aten computes as a product with the scalar's
  // reciprocal, taken on the host: 1.0f / b in fp32 for a 0-dim fp32 tensor (voxel_size[i]), (float) (1.0 / b)
  // for a Python number (out_size_factor, 1 + o); the other overlap terms are Python floats rounded to fp32
  float inv_vs0, inv_vs1, inv_osf, pc0, pc1;
  float k_1mo, k_inv_1po, k_m2o, k_om1, k_4a3;
};

__device__ __forceinline__ int pick4(int c, int a0, int a1, int a2, int a3) {
  return c == 0 ? a0 : c == 1 ? a1 : c == 2 ? a2 : a3;
}

// aten's float -> int32 cast on this device (v_cvt_i32_f32): truncation, saturation, NaN -> 0
__device__ __forceinline__ int cvt_i32(float f) {
  if (f != f) return 0;
  if (f >= 2147483648.0f) return 0x7fffffff;
  if (f <= -2147483648.0f) return (int) 0x80000000u;
  return (int) f;
}

// mmdet3d's gaussian_radius((length, width), o) as the reference evaluates it: every step an fp32 op on 0-dim
// device tensors, Python scalars rounded to fp32, x**2 as x * x, Python's min (a NaN first operand stays).
__device__ __forceinline__ float gaussian_radius_f32(const TgtParams& p, float h, float w) {
  const float b1 = h + w;
  const float c1 = ((w * h) * p.k_1mo) * p.k_inv_1po;
  const float r1 = (b1 + sqrtf(b1 * b1 - c1 * 4.0f)) * 0.5f;
  const float b2 = (h + w) * 2.0f;
  const float c2 = (w * p.k_1mo) * h;
  const float r2 = (b2 + sqrtf(b2 * b2 - c2 * 16.0f)) * 0.5f;
  const float b3 = (h + w) * p.k_m2o;
  const float c3 = (w * p.k_om1) * h;
  const float r3 = (b3 + sqrtf(b3 * b3 - c3 * p.k_4a3)) * 0.5f;
  float r = r1;
  if (r2 < r) r = r2;
  if (r3 < r) r = r3;
  return r;
}

__device__ __forceinline__ int load_class(const TgtParams& p, int b, int i, int t) {
  const long k = (long) b * p.M + i;
  const long lab = p.lab64 ? static_cast<const int64_t*>(p.labels)[k] : (long) static_cast<const int32_t*>(p.labels)[k];
  const long c = lab - p.flag[t];
  return (c >= 0 && c < p.ncls[t]) ? (int) c : -1;
}

// ---------------------------------------------------------------------------------------------------------
// (a) slot assignment + per-box chain
// ---------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kTgtBlock) tgt_assign_kernel(TgtParams p) {
  __shared__ int wc[kTgtWaves][kTgtMaxNcls];
  const int bt = blockIdx.x, b = bt / p.T, t = bt % p.T;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;

  // per-class box counts of this task
  int n0 = 0, n1 = 0, n2 = 0, n3 = 0;
  for (int i = tid; i < p.M; i += kTgtBlock) {
    const int c = load_class(p, b, i, t);
    n0 += c == 0; n1 += c == 1; n2 += c == 2; n3 += c == 3;
  }
  n0 = wave_sum(n0); n1 = wave_sum(n1); n2 = wave_sum(n2); n3 = wave_sum(n3);
  if (lane == 0) { wc[wid][0] = n0; wc[wid][1] = n1; wc[wid][2] = n2; wc[wid][3] = n3; }
  __syncthreads();
  int cnt[kTgtMaxNcls];
#pragma unroll
  for (int c = 0; c < kTgtMaxNcls; ++c) {
    cnt[c] = 0;
#pragma unroll
    for (int w = 0; w < kTgtWaves; ++w) cnt[c] += wc[w][c];
  }
  __syncthreads();
  // running slot of each class's next box: the task's boxes are the classes' runs, one after the other
  int run0 = 0, run1 = cnt[0], run2 = run1 + cnt[1], run3 = run2 + cnt[2];
  const int ntask = run3 + cnt[3];
  const int nslots = min(ntask, p.max_objs);
  const long row0 = ((long) t * p.B + b) * p.max_objs;
  int4* rec = p.rec + ((long) b * p.T + t) * p.max_objs;
  if (tid == 0) p.nrec[bt] = nslots;

  const uint64_t lt = (1ull << lane) - 1ull;
  int seen = 0;
  for (int s = 0; s < p.M && seen < ntask; s += kTgtBlock) {
    const int i = s + tid;
    const int c = i < p.M ? load_class(p, b, i, t) : -1;
    int rank = 0;
#pragma unroll
    for (int cc = 0; cc < kTgtMaxNcls; ++cc) {
      const uint64_t m = __ballot(c == cc);
      if (c == cc) rank = __popcll(m & lt);
      if (lane == 0) wc[wid][cc] = __popcll(m);
    }
    __syncthreads();
    int below = 0;                     // boxes of class c in the lower waves of this chunk
    for (int w = 0; w < wid; ++w) below += c >= 0 ? wc[w][c] : 0;
    const int slot = c >= 0 ? pick4(c, run0, run1, run2, run3) + below + rank : -1;
    int add[kTgtMaxNcls];
#pragma unroll
    for (int cc = 0; cc < kTgtMaxNcls; ++cc) {
      add[cc] = 0;
#pragma unroll
      for (int w = 0; w < kTgtWaves; ++w) add[cc] += wc[w][cc];
    }
    run0 += add[0]; run1 += add[1]; run2 += add[2]; run3 += add[3];
    seen += add[0] + add[1] + add[2] + add[3];
    __syncthreads();
    if (slot < 0 || slot >= p.max_objs) continue;

    // the reference's per-box chain (bev_depth_head.py:258-314)
    const float* bx = p.boxes + ((long) b * p.M + i) * p.cols;
    float row[10];
#pragma unroll
    for (int k = 0; k < 10; ++k) row[k] = 0.0f;
    int4 rc = make_int4(-1, 0, 0, 0);
    long ind = 0;
    const float w = (bx[3] * p.inv_vs0) * p.inv_osf;
    const float l = (bx[4] * p.inv_vs1) * p.inv_osf;
    if (w > 0.0f && l > 0.0f) {
      const float rad = gaussian_radius_f32(p, l, w);
      // a non-finite radius makes the reference raise (int(nan)); such a box is skipped here
      if (rad > -1.0f && rad < kTgtMaxRadius) {
        const int r = max(p.min_radius, (int) rad);
        const float cx = ((bx[0] - p.pc0) * p.inv_vs0) * p.inv_osf;
        const float cy = ((bx[1] - p.pc1) * p.inv_vs1) * p.inv_osf;
        const int ix = cvt_i32(cx), iy = cvt_i32(cy);
        if (ix >= 0 && ix < p.fw && iy >= 0 && iy < p.fh) {
          rc = make_int4(c, ix, iy, r);
          ind = (long) iy * p.fw + ix;
          row[0] = cx - (float) ix;
          row[1] = cy - (float) iy;
          row[2] = bx[2];
#pragma unroll
          for (int k = 0; k < 3; ++k) row[3 + k] = p.norm_bbox ? logf(bx[3 + k]) : bx[3 + k];
          row[6] = sinf(bx[6]);
          row[7] = cosf(bx[6]);
          if (p.cols == 9) { row[8] = bx[7]; row[9] = bx[8]; }
        }
      }
    }
    float* dst = p.anno + (row0 + slot) * p.code;
#pragma unroll
    for (int k = 0; k < 10; ++k)
      if (k < p.code) dst[k] = row[k];
    p.inds[row0 + slot] = ind;
    p.masks[row0 + slot] = rc.x >= 0 ? 1 : 0;
    rec[slot] = rc;
  }

  // the slots no box reached
  const int nz = p.max_objs - nslots;
  for (int k = tid; k < nz * p.code; k += kTgtBlock) p.anno[(row0 + nslots) * p.code + k] = 0.0f;
  for (int k = tid; k < nz; k += kTgtBlock) {
    p.inds[row0 + nslots + k] = 0;
    p.masks[row0 + nslots + k] = 0;
  }
}

// ---------------------------------------------------------------------------------------------------------
// (b) heatmaps: gather over the draw records
// ---------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kTgtBlock) tgt_heatmap_kernel(TgtParams p) {
  __shared__ int4 srec[kTgtBlock];
  __shared__ double sden[kTgtBlock];
  __shared__ int wcnt[kTgtWaves];
  const int bt = blockIdx.y, b = bt / p.T, t = bt % p.T;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int x0 = (blockIdx.x % p.ntx) * kTileW, y0 = (blockIdx.x / p.ntx) * kTileH;
  const int px = x0 + (tid % kTileW), py = y0 + (tid / kTileW);
  const int n = p.nrec[bt];
  const int4* rec = p.rec + (long) bt * p.max_objs;
  const uint64_t lt = (1ull << lane) - 1ull;

  // per class: the smallest exponent q / (2 sigma^2) of the records covering the pixel (+inf: none)
  double v0 = INFINITY, v1 = INFINITY, v2 = INFINITY, v3 = INFINITY;
  for (int base = 0; base < n; base += kTgtBlock) {
    const int k = base + tid;
    int4 rc = make_int4(-1, 0, 0, 0);
    if (k < n) rc = rec[k];
    // the stamp covers |x - rc.y| <= r, |y - rc.z| <= r (draw_heatmap_gaussian clips it to the map)
    const bool keep = rc.x >= 0 && rc.y - rc.w < x0 + kTileW && rc.y + rc.w >= x0 && rc.z - rc.w < y0 + kTileH &&
                      rc.z + rc.w >= y0;
    const uint64_t m = __ballot(keep);
    if (lane == 0) wcnt[wid] = __popcll(m);
    __syncthreads();
    int off = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < kTgtWaves; ++w) {
      off += w < wid ? wcnt[w] : 0;
      tot += wcnt[w];
    }
    if (keep) {
      const int j = off + __popcll(m & lt);
      srec[j] = rc;
      // gaussian_2d: sigma = diameter / 6 in float64, exponent -(x*x + y*y) / (2 * sigma * sigma)
      const double sigma = (2.0 * rc.w + 1.0) / 6.0;
      sden[j] = (2.0 * sigma) * sigma;
    }
    __syncthreads();
    for (int j = 0; j < tot; ++j) {
      const int4 q = srec[j];
      const int dx = px - q.y, dy = py - q.z;
      if (abs(dx) <= q.w && abs(dy) <= q.w) {
        const double v = (double) (dx * dx + dy * dy) / sden[j];
        if (q.x == 0) v0 = v < v0 ? v : v0;
        else if (q.x == 1) v1 = v < v1 ? v : v1;
        else if (q.x == 2) v2 = v < v2 ? v : v2;
        else v3 = v < v3 ? v : v3;
      }
    }
    __syncthreads();
  }
  if (px >= p.fw || py >= p.fh) return;
  const int ncls = p.ncls[t];
  const long plane = (long) p.fh * p.fw;
  float* dst = p.heat + p.heat_off[t] + (long) b * ncls * plane + (long) py * p.fw + px;
#pragma unroll
  for (int c = 0; c < kTgtMaxNcls; ++c) {
    if (c >= ncls) break;
    const double v = c == 0 ? v0 : c == 1 ? v1 : c == 2 ? v2 : v3;
    double g = v < INFINITY ? exp(-v) : 0.0;  // most pixels lie under no stamp: no exp for them
    if (g < DBL_EPSILON) g = 0.0;             // h[h < eps * h.max()] = 0, h.max() = 1
    dst[c * plane] = (float) g;
  }
}

// ---------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------
static_assert(sizeof(VampDetTargetDesc) == 112, "VampDetTargetDesc layout: part of the ABI (the binding reads it from include/vampire_hip.h)");

int tgt_validate(const VampDetTargetDesc* d) {
  VAMP_REQUIRE(d, "desc is NULL");
  VAMP_REQUIRE(d->B >= 1 && d->B <= kTgtMaxB, "B must be in [1, 4096]");
  VAMP_REQUIRE(d->T >= 1 && d->T <= kTgtMaxT, "T must be in [1, 8]");
  VAMP_REQUIRE(d->M >= 0 && d->M <= kTgtMaxM, "M must be in [0, 2^20]");
  for (int t = 0; t < d->T; ++t) VAMP_REQUIRE(d->ncls[t] >= 1 && d->ncls[t] <= kTgtMaxNcls, "ncls must be in [1, 4]");
  VAMP_REQUIRE(d->box_cols == 7 || d->box_cols == 9, "box_cols must be 7 or 9");
  VAMP_REQUIRE(d->code == 8 || d->code == 10, "code must be 8 or 10");
  VAMP_REQUIRE(d->code == d->box_cols + 1, "code must be box_cols + 1 (10 with velocity, 8 without)");
  VAMP_REQUIRE(d->max_objs >= 1 && d->max_objs <= kTgtMaxObjs, "max_objs must be in [1, 8192]");
  VAMP_REQUIRE(d->fh >= 1 && d->fh <= kTgtMaxSide && d->fw >= 1 && d->fw <= kTgtMaxSide, "fh, fw must be in [1, 8192]");
  VAMP_REQUIRE(d->out_size_factor >= 1, "out_size_factor must be positive");
  VAMP_REQUIRE(d->min_radius >= 0 && d->min_radius < (1 << 30), "min_radius must be in [0, 2^30)");
  VAMP_REQUIRE(d->voxel_size[0] > 0.0f && d->voxel_size[1] > 0.0f && std::isfinite(d->voxel_size[0]) &&
               std::isfinite(d->voxel_size[1]), "voxel_size must be positive and finite");
  VAMP_REQUIRE(std::isfinite(d->pc_range[0]) && std::isfinite(d->pc_range[1]), "pc_range must be finite");
  VAMP_REQUIRE(std::isfinite(d->gaussian_overlap), "gaussian_overlap must be finite");
  VAMP_REQUIRE(d->label_dtype == VAMP_I32 || d->label_dtype == VAMP_I64, "label_dtype must be VAMP_I32 or VAMP_I64");
  VAMP_REQUIRE(d->norm_bbox == 0 || d->norm_bbox == 1, "norm_bbox must be 0 or 1");
  VAMP_REQUIRE(d->reserved[0] == 0 && d->reserved[1] == 0, "reserved must be 0");
  return VAMP_OK;
}

// the regions of *q carved from `workspace` (NULL: only the size, which is returned, is of use)
size_t tgt_workspace(const VampDetTargetDesc* d, TgtParams* q, void* workspace) {
  const size_t BT = (size_t) d->B * d->T;
  Carve c(workspace);
  q->rec = c.take<int4>(BT * d->max_objs);
  q->nrec = c.take<int>(BT);
  return c.off;
}

}  // namespace
}  // namespace vamp

using namespace vamp;

extern "C" {

size_t vamp_det_targets_workspace_bytes(const VampDetTargetDesc* d) {
  if (tgt_validate(d)) return 0;
  TgtParams q{};
  return tgt_workspace(d, &q, nullptr);
}

int vamp_det_targets(const VampDetTargetDesc* d, const float* boxes, const void* labels, float* heatmaps, float* anno,
                     int64_t* inds, uint8_t* masks, void* workspace, size_t workspace_bytes, void* stream) {
  if (int e = tgt_validate(d)) return e;
  VAMP_REQUIRE(d->M == 0 || (boxes && labels), "boxes or labels is NULL");
  VAMP_REQUIRE(heatmaps && anno && inds && masks, "an output pointer is NULL");
  TgtParams q{};
  if (int e = workspace_fits(__func__, workspace, workspace_bytes, tgt_workspace(d, &q, workspace))) return e;
  q.boxes = boxes; q.labels = labels; q.heat = heatmaps; q.anno = anno; q.inds = inds; q.masks = masks;
  long off = 0;
  int flag = 0;
  for (int t = 0; t < d->T; ++t) {
    q.ncls[t] = d->ncls[t];
    q.flag[t] = flag;
    q.heat_off[t] = off;
    flag += d->ncls[t];
    off += (long) d->B * d->ncls[t] * d->fh * d->fw;
  }
  q.B = d->B; q.T = d->T; q.M = d->M; q.cols = d->box_cols; q.code = d->code; q.max_objs = d->max_objs;
  q.fh = d->fh; q.fw = d->fw; q.min_radius = d->min_radius; q.norm_bbox = d->norm_bbox;
  q.lab64 = d->label_dtype == VAMP_I64;
  q.ntx = (d->fw + kTileW - 1) / kTileW;
  // aten's reciprocals of CPU scalars, computed on the host as here (see TgtParams)
  q.inv_vs0 = 1.0f / d->voxel_size[0];
  q.inv_vs1 = 1.0f / d->voxel_size[1];
  q.inv_osf = (float) (1.0 / d->out_size_factor);
  q.pc0 = d->pc_range[0]; q.pc1 = d->pc_range[1];
  // gaussian_radius's Python-float terms: (1 - o), (1 + o), -2 * o, (o - 1), 4 * (4 * o), each rounded to fp32
  const double o = d->gaussian_overlap;
  q.k_1mo = (float) (1.0 - o);
  q.k_inv_1po = (float) (1.0 / (1.0 + o));
  q.k_m2o = (float) (-2.0 * o);
  q.k_om1 = (float) (o - 1.0);
  q.k_4a3 = (float) (4.0 * (4.0 * o));
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int nty = (d->fh + kTileH - 1) / kTileH;
  VAMP_TIMED(kProfAux, s, (tgt_assign_kernel<<<d->B * d->T, kTgtBlock, 0, s>>>(q)));
  VAMP_TIMED(kProfAux, s, (tgt_heatmap_kernel<<<dim3(q.ntx * nty, d->B * d->T), kTgtBlock, 0, s>>>(q)));
  return check_launch("det_targets");
}

}  // extern "C"
