// Camera and BEV training labels rasterised from the lidar points on the device: the reference loader's
// depth_transform (nusc_det_seg_dataset.py:178-231, behind the margins of map_pointcloud_to_image, :362-367),
// get_bev_seg_map (:233-265) and the every-s-th-pixel pick of get_downsampled_gt (base_exp.py:596-632), for every
// sample and camera in three launches that never synchronise with the host:
//
//  (a) ll_fill_kernel: the camera key planes [B, N, h, w] of the workspace are set to all-ones, the BEV key plane
//      [B, ny, nx] to 0, with 16-byte stores.  The workspace needs no initialisation.
//  (b) ll_scatter_kernel, grid (ceil(M / 256), B), one thread per point: the sample's camera table (three rows of
//      lidar2cam, the 3 x 3 of the intrinsics, the augmentation row) is staged in LDS once per workgroup; the thread
//      loads its point once, walks the N cameras and then takes its BEV cell.  A point that lands in a cell offers
//      the cell a 64-bit key with one no-return integer atomic: (depth bits << 32) | index under an unsigned MIN for
//      the cameras (the nearest point wins, equal depths go to the lowest index), (ordered height << 32) |
//      (0xFFFFFFFF - index) under an unsigned MAX for the BEV map (the highest point wins, equal heights go to the
//      lowest index).  The reference's order among equal depths / heights is that of an unstable argsort, i.e.
//      undefined: the lowest-index rule is this library's own.
//  (c) ll_resolve_kernel, one thread per cell: the winner's depth / height bits, its label & 0xFF and the fg / mask
//      byte, zeros for a cell no point reached.  Every output element is written.
//
// Integer min / max do not depend on the arrival order, so the result is a pure function of the inputs and bitwise
// repeatable; no float atomics, no host synchronisation, capturable in a graph (the augmentation table lives in
// device memory and may change between replays).  The camera chain is fp32, one rounding per operation in the
// reference's order (the file is built with -ffp-contract=off), except the rotation, which numpy computes in
// float64 and rounds to fp32; the BEV coordinates are float64 as numpy makes them.
//
// The BEV map is [ny, nx], rows along y and columns along x.  That equals the reference for its square grids; its
// own indexing (a map shaped (nx, ny) written at [y, x]) is inconsistent when nx != ny.
#include <cmath>

#include "common.hpp"

namespace vamp {
namespace {

constexpr int kLLBlock = 256;
constexpr int kLLMaxB = 4096;
constexpr int kLLMaxN = 16;
constexpr int kLLMaxM = 1 << 24;
constexpr int kLLMaxSide = 8192;
constexpr int kLLMaxRaw = 65536;
constexpr long kLLMaxCells = 1l << 33;
constexpr int kAugCols = 8;                       // resize, crop_x, crop_y, flip, cos, sin, 0, 0

struct LLParams {
  const float* points;                            // [B, M, cols]
  const void* labels;                             // [B, M] uint8 | int64
  const int32_t* counts;                          // [B] or nullptr: every row counts
  const float* lidar2cam;                         // [B, N, 4, 4]
  const float* intrin;                            // [B, N, 4, 4]
  const double* aug;                              // [B, N, 8]
  float* cam_depth; int64_t* cam_seg; uint8_t* cam_fg;
  int64_t* bev_seg; float* bev_height; uint8_t* bev_mask;
  unsigned long long* cam_keys;                   // [B, N, h, w]
  unsigned long long* bev_keys;                   // [B, ny, nx]
  long cam_units, bev_units;                      // 16-byte units of the two key regions (0: part skipped)
  long cam_cells, bev_cells;
  double origin_x, origin_y, size, cx_hi, cy_hi;
  float z_lo, z_hi, fW, fH, half_w, half_h, raw_u_hi, raw_v_hi;
  int B, N, M, cols, lab64, H, W, stride, h, w, ny, nx;
};

// the usual monotone map of fp32 bits to uint32 (-0.0 ranks just below +0.0), and back
__device__ __forceinline__ uint32_t ordered_bits(float f) {
  const uint32_t b = __float_as_uint(f);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float ordered_float(uint32_t o) {
  return __uint_as_float((o & 0x80000000u) ? (o ^ 0x80000000u) : ~o);
}

__device__ __forceinline__ long load_label(const LLParams& p, long k) {
  return p.lab64 ? (long) static_cast<const int64_t*>(p.labels)[k] : (long) static_cast<const uint8_t*>(p.labels)[k];
}

// ---------------------------------------------------------------------------------------------------------
// (a) fill
// ---------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kLLBlock) ll_fill_kernel(LLParams p) {
  const long i = (long) blockIdx.x * kLLBlock + threadIdx.x;
  if (i < p.cam_units) {
    reinterpret_cast<uint4*>(p.cam_keys)[i] = make_uint4(0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu);
  } else if (i - p.cam_units < p.bev_units) {
    reinterpret_cast<uint4*>(p.bev_keys)[i - p.cam_units] = make_uint4(0u, 0u, 0u, 0u);
  }
}

// ---------------------------------------------------------------------------------------------------------
// (b) scatter
// ---------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kLLBlock) ll_scatter_kernel(LLParams p) {
  __shared__ float s_m[kLLMaxN][12];              // lidar2cam rows 0 .. 2
  __shared__ float s_k[kLLMaxN][9];               // intrinsics rows 0 .. 2, columns 0 .. 2
  __shared__ double s_a[kLLMaxN][kAugCols];
  const int b = blockIdx.y, tid = threadIdx.x;
  const bool cam = p.cam_keys != nullptr;
  if (cam) {
    for (int i = tid; i < p.N * 12; i += kLLBlock) s_m[i / 12][i % 12] = p.lidar2cam[((long) b * p.N + i / 12) * 16 + i % 12];
    for (int i = tid; i < p.N * 9; i += kLLBlock) {
      const int n = i / 9, r = (i % 9) / 3, c = i % 3;
      s_k[n][i % 9] = p.intrin[((long) b * p.N + n) * 16 + r * 4 + c];
    }
    for (int i = tid; i < p.N * kAugCols; i += kLLBlock) s_a[i / kAugCols][i % kAugCols] = p.aug[(long) b * p.N * kAugCols + i];
    __syncthreads();
  }
  const int i = blockIdx.x * kLLBlock + tid;
  int cnt = p.M;
  if (p.counts) cnt = min(max(p.counts[b], 0), p.M);
  if (i >= cnt) return;
  const float* pt = p.points + ((long) b * p.M + i) * p.cols;
  const float x = pt[0], y = pt[1], z = pt[2];

  if (cam) {
    const long plane = (long) p.h * p.w;
    for (int n = 0; n < p.N; ++n) {
      const float* m = s_m[n];
      const float* k = s_k[n];
      // lidar -> camera -> raw pixel: fp32, left to right
      const float xc = ((m[0] * x + m[1] * y) + m[2] * z) + m[3];
      const float yc = ((m[4] * x + m[5] * y) + m[6] * z) + m[7];
      const float zc = ((m[8] * x + m[9] * y) + m[10] * z) + m[11];
      const float depth = zc;
      const float den = (k[6] * xc + k[7] * yc) + k[8] * zc;
      float u = ((k[0] * xc + k[1] * yc) + k[2] * zc) / den;
      float v = ((k[3] * xc + k[4] * yc) + k[5] * zc) / den;
      // map_pointcloud_to_image's margins (a NaN fails every comparison)
      if (!(depth > 0.0f && u > 1.0f && u < p.raw_u_hi && v > 1.0f && v < p.raw_v_hi)) continue;
      // depth_transform
      const double* a = s_a[n];
      const float resize = (float) a[0];
      u = u * resize;
      v = v * resize;
      u = u - (float) a[1];
      v = v - (float) a[2];
      if (a[3] != 0.0) u = p.fW - u;
      u = u - p.half_w;
      v = v - p.half_h;
      const double ud = (double) u, vd = (double) v;
      u = (float) (a[4] * ud + a[5] * vd);
      v = (float) (-a[5] * ud + a[4] * vd);
      u = u + p.half_w;
      v = v + p.half_h;
      // on the floats, before any conversion: NaN, +-Inf, 1e30 and -0.5 fall out here
      if (!(u >= 0.0f && u < p.fW && v >= 0.0f && v < p.fH)) continue;
      const int iu = (int) u, iv = (int) v;
      if (iu % p.stride != 0 || iv % p.stride != 0) continue;      // map[::s, ::s] of the full-resolution map
      const long cell = ((long) b * p.N + n) * plane + (long) (iv / p.stride) * p.w + iu / p.stride;
      const unsigned long long key = ((unsigned long long) __float_as_uint(depth) << 32) | (unsigned) i;
      (void) __hip_atomic_fetch_min(p.cam_keys + cell, key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }

  if (p.bev_keys) {
    const double cx = ((double) x - p.origin_x) / p.size;
    const double cy = ((double) y - p.origin_y) / p.size;
    if (cx > 1.0 && cx < p.cx_hi && cy > 1.0 && cy < p.cy_hi && z > p.z_lo && z < p.z_hi) {
      const long cell = ((long) b * p.ny + (int) cy) * p.nx + (int) cx;
      const unsigned long long key = ((unsigned long long) ordered_bits(z) << 32) | (0xFFFFFFFFu - (unsigned) i);
      (void) __hip_atomic_fetch_max(p.bev_keys + cell, key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

// ---------------------------------------------------------------------------------------------------------
// (c) resolve
// ---------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kLLBlock) ll_resolve_kernel(LLParams p) {
  const long i = (long) blockIdx.x * kLLBlock + threadIdx.x;
  if (i < p.cam_cells) {
    const unsigned long long key = p.cam_keys[i];
    float depth = 0.0f;
    long lab = 0;
    if (key != ~0ull) {
      const long b = i / ((long) p.N * p.h * p.w);
      depth = __uint_as_float((uint32_t) (key >> 32));
      lab = load_label(p, b * p.M + (long) (uint32_t) key) & 0xFF;
    }
    p.cam_depth[i] = depth;
    p.cam_seg[i] = lab;
    p.cam_fg[i] = depth > 0.0f ? 1 : 0;
    return;
  }
  const long j = i - p.cam_cells;
  if (j >= p.bev_cells) return;
  const unsigned long long key = p.bev_keys[j];
  float height = 0.0f;
  long lab = 0;
  if (key != 0ull) {
    const long b = j / ((long) p.ny * p.nx);
    height = ordered_float((uint32_t) (key >> 32));
    lab = load_label(p, b * p.M + (long) (0xFFFFFFFFu - (uint32_t) key)) & 0xFF;
  }
  p.bev_seg[j] = lab;
  p.bev_height[j] = height;
  p.bev_mask[j] = key != 0ull ? 1 : 0;
}

// ---------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------
static_assert(sizeof(VampLidarLabelDesc) == 88, "VampLidarLabelDesc layout: part of the ABI (the binding reads it from include/vampire_hip.h)");

int ll_validate(const VampLidarLabelDesc* d) {
  VAMP_REQUIRE(d, "desc is NULL");
  VAMP_REQUIRE(d->B >= 1 && d->B <= kLLMaxB, "B must be in [1, 4096]");
  VAMP_REQUIRE(d->N >= 1 && d->N <= kLLMaxN, "N must be in [1, 16]");
  VAMP_REQUIRE(d->M >= 0 && d->M <= kLLMaxM, "M must be in [0, 2^24]");
  VAMP_REQUIRE(d->point_cols == 3 || d->point_cols == 4, "point_cols must be 3 or 4");
  VAMP_REQUIRE(d->label_dtype == VAMP_U8 || d->label_dtype == VAMP_I64, "label_dtype must be VAMP_U8 or VAMP_I64");
  VAMP_REQUIRE(d->H >= 1 && d->H <= kLLMaxSide && d->W >= 1 && d->W <= kLLMaxSide, "H, W must be in [1, 8192]");
  VAMP_REQUIRE(d->ny >= 1 && d->ny <= kLLMaxSide && d->nx >= 1 && d->nx <= kLLMaxSide, "ny, nx must be in [1, 8192]");
  VAMP_REQUIRE(d->stride >= 1 && d->H % d->stride == 0 && d->W % d->stride == 0, "stride must be positive and divide H and W");
  VAMP_REQUIRE(d->raw_w >= 1 && d->raw_w <= kLLMaxRaw && d->raw_h >= 1 && d->raw_h <= kLLMaxRaw,
               "raw_w, raw_h must be in [1, 65536]");
  VAMP_REQUIRE(d->size > 0.0 && std::isfinite(d->size), "size must be positive and finite");
  VAMP_REQUIRE(std::isfinite(d->origin_x) && std::isfinite(d->origin_y), "origin must be finite");
  VAMP_REQUIRE(d->z_lo < d->z_hi, "z_lo must be below z_hi");
  VAMP_REQUIRE((long) d->B * d->N * (d->H / d->stride) * (d->W / d->stride) <= kLLMaxCells &&
               (long) d->B * d->ny * d->nx <= kLLMaxCells, "B N h w and B ny nx must not exceed 2^33 cells");
  VAMP_REQUIRE(d->reserved[0] == 0 && d->reserved[1] == 0, "reserved must be 0");
  return VAMP_OK;
}

// The two key tables, the camera maps' then the BEV maps', carved from `workspace` (NULL: only `bytes` is of use), each
// with the count of 16-byte units the fill kernel writes: its whole padded region.
struct LLWs {
  unsigned long long *cam_keys, *bev_keys;
  long cam_units, bev_units;
  size_t bytes;
};
LLWs ll_workspace(const VampLidarLabelDesc* d, void* workspace) {
  Carve c(workspace);
  LLWs w;
  w.cam_keys = c.take<unsigned long long>((size_t) d->B * d->N * (d->H / d->stride) * (d->W / d->stride));
  w.cam_units = (long) (c.off / 16);
  w.bev_keys = c.take<unsigned long long>((size_t) d->B * d->ny * d->nx);
  w.bev_units = (long) (c.off / 16) - w.cam_units;
  w.bytes = c.off;
  return w;
}

}  // namespace
}  // namespace vamp

using namespace vamp;

extern "C" {

size_t vamp_lidar_labels_workspace_bytes(const VampLidarLabelDesc* d) {
  if (ll_validate(d)) return 0;
  return ll_workspace(d, nullptr).bytes;
}

int vamp_lidar_labels(const VampLidarLabelDesc* d, const float* points, const void* labels, const int32_t* counts,
                      const float* lidar2cam, const float* intrin, const double* aug, float* cam_depth,
                      int64_t* cam_seg, uint8_t* cam_fg, int64_t* bev_seg, float* bev_height, uint8_t* bev_mask,
                      void* workspace, size_t workspace_bytes, void* stream) {
  if (int e = ll_validate(d)) return e;
  const bool cam = cam_depth || cam_seg || cam_fg, bev = bev_seg || bev_height || bev_mask;
  VAMP_REQUIRE(cam || bev, "the camera outputs and the BEV outputs are all NULL: nothing to do");
  VAMP_REQUIRE(!cam || (cam_depth && cam_seg && cam_fg), "cam_depth, cam_seg, cam_fg must be NULL together or not at all");
  VAMP_REQUIRE(!bev || (bev_seg && bev_height && bev_mask), "bev_seg, bev_height, bev_mask must be NULL together or not at all");
  VAMP_REQUIRE(d->M == 0 || (points && labels), "points or labels is NULL");
  VAMP_REQUIRE(!cam || (lidar2cam && intrin && aug), "lidar2cam, intrin or aug is NULL");
  VAMP_REQUIRE(!cam || aligned(aug, 8), "aug must be 8-byte aligned");
  const LLWs w = ll_workspace(d, workspace);
  if (int e = workspace_fits(__func__, workspace, workspace_bytes, w.bytes)) return e;
  VAMP_REQUIRE(aligned(workspace, 16), "workspace must be 16-byte aligned");

  LLParams q{};
  q.points = points; q.labels = labels; q.counts = counts;
  q.lidar2cam = lidar2cam; q.intrin = intrin; q.aug = aug;
  q.cam_depth = cam_depth; q.cam_seg = cam_seg; q.cam_fg = cam_fg;
  q.bev_seg = bev_seg; q.bev_height = bev_height; q.bev_mask = bev_mask;
  q.B = d->B; q.N = d->N; q.M = d->M; q.cols = d->point_cols; q.lab64 = d->label_dtype == VAMP_I64;
  q.H = d->H; q.W = d->W; q.stride = d->stride; q.h = d->H / d->stride; q.w = d->W / d->stride;
  q.ny = d->ny; q.nx = d->nx;
  if (cam) {
    q.cam_keys = w.cam_keys;
    q.cam_units = w.cam_units;
    q.cam_cells = (long) d->B * d->N * q.h * q.w;
  }
  if (bev) {
    q.bev_keys = w.bev_keys;
    q.bev_units = w.bev_units;
    q.bev_cells = (long) d->B * d->ny * d->nx;
  }
  q.origin_x = d->origin_x; q.origin_y = d->origin_y; q.size = d->size;
  q.cx_hi = (double) (d->nx - 1); q.cy_hi = (double) (d->ny - 1);
  q.z_lo = d->z_lo; q.z_hi = d->z_hi;
  q.fW = (float) d->W; q.fH = (float) d->H;
  q.half_w = (float) (d->W / 2.0); q.half_h = (float) (d->H / 2.0);
  q.raw_u_hi = (float) (d->raw_w - 1); q.raw_v_hi = (float) (d->raw_h - 1);

  hipStream_t s = static_cast<hipStream_t>(stream);
  const long units = q.cam_units + q.bev_units, cells = q.cam_cells + q.bev_cells;
  VAMP_TIMED(kProfAux, s, (ll_fill_kernel<<<(unsigned) ((units + kLLBlock - 1) / kLLBlock), kLLBlock, 0, s>>>(q)));
  if (d->M > 0)
    VAMP_TIMED(kProfAux, s, (ll_scatter_kernel<<<dim3((d->M + kLLBlock - 1) / kLLBlock, d->B), kLLBlock, 0, s>>>(q)));
  VAMP_TIMED(kProfAux, s, (ll_resolve_kernel<<<(unsigned) ((cells + kLLBlock - 1) / kLLBlock), kLLBlock, 0, s>>>(q)));
  return check_launch("lidar_labels");
}

}  // extern "C"
