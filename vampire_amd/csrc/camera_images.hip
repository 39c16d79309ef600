// The image half of the reference loader's camera path on the device: img_transform (nusc_det_seg_dataset.py:118-146:
// Pillow's resize, crop, horizontal flip and rotate) followed by mmcv.imnormalize (:679-681), for every sample and
// camera in two launches that never synchronise with the host.  include/vampire_hip.h states the arithmetic (rules
// 1 - 5); all float64 work (the bicubic taps, the rotation constants) is done by the caller, the kernels see int32
// tables in device memory, so the augmentation may change under a replayed graph.
//
//  (a) img_resample_kernel, grid (ceil(W / 64), ceil(H / 8), B N), 256 threads: one workgroup per 8 x 64 tile of one
//      camera's crop window in the resized image.  The first two waves read the tile's column and row windows and
//      reduce them to the raw footprint [fy0, fy0 + fh) x [fx0, fx0 + fw); every window is clamped to the raw image
//      and to the footprint here, once, so that nothing a table holds can make a later index leave the LDS tile or
//      the raw image.  The footprint's rows go to LDS, a wave per row: whole aligned dwords where all four bytes
//      belong to the row, single bytes at the row's head and tail (3-byte pixels, any row alignment; the LDS row
//      keeps the address's phase, so a dword is stored as a dword).  Horizontal pass: one lane per (footprint row,
//      column) -- a wave walks one row, the taps sit tap-major in LDS -- into a uint8 LDS tile [fh][64][3]; the
//      rounding to uint8 between the passes is part of the definition.  Vertical pass: one lane per four bytes of an
//      output row, read as one dword per tap, stored as one dword into the staging image [B N][H][pitch] of the
//      workspace.  A column or row of the crop window outside the resized image has no taps and comes out 0.
//      Every staging byte the second kernel can read is written: the workspace needs no initialisation.
//  (b) img_finish_kernel, grid (ceil(H ceil(W / 4) / 256), B N): one lane per four output pixels: fixed-point rotate
//      index, bounds, flip, staging fetch or 0, channel swap, normalise; 16-byte planar stores (8-byte for bf16)
//      and 12 bytes of out_u8 when W is a multiple of 4, element stores otherwise.
//
// No atomics; the result is a pure function of the inputs.  The file is built with -ffp-contract=off: the
// normalisation is a subtraction and a multiplication, each rounded to fp32.
#include <climits>
#include <cmath>

#include "common.hpp"
#include "elem16.hpp"

namespace vamp {
namespace {

constexpr int kImgBlock = 256;
constexpr int kTileW = VAMP_IMG_TILE_W, kTileH = VAMP_IMG_TILE_H, kMaxTaps = VAMP_IMG_MAX_TAPS;
constexpr int kHRow = kTileW * 3;                 // bytes of one row of the horizontal pass's tile
constexpr int kImgMaxB = 4096, kImgMaxN = 16, kImgMaxRaw = 65536, kImgMaxSide = 4096;
static_assert(kTileW == 64 && kTileH <= 64 && kHRow % 16 == 0 && kImgBlock >= 128, "the tile the kernels are written for");

struct ImgParams {
  const uint8_t* raw;
  const int32_t *col_first, *col_count, *col_taps, *row_first, *row_count, *row_taps, *consts;
  void* out;
  uint8_t* out_u8;
  uint8_t* stage;
  long raw_b_stride, raw_n_stride, raw_row_stride;
  int N, raw_h, raw_w, H, W, taps_x, taps_y, foot_w, foot_h, raw_pitch, stage_pitch, out_bf16, to_rgb;
  float mean[3], std_inv[3];
};

__device__ __forceinline__ int wave_min(int v) {
  for (int m = 32; m >= 1; m >>= 1) v = min(v, __shfl_xor(v, m));
  return v;
}
__device__ __forceinline__ int wave_max(int v) {
  for (int m = 32; m >= 1; m >>= 1) v = max(v, __shfl_xor(v, m));
  return v;
}
// clip(0, 255, v >> 22), clamped BEFORE the shift.  Written as min(max(v >> 22, 0), 255), two of these packed into one
// word compile to v_ashr_pk_u8_i32 on gfx950, and the vertical pass's words came back from the MI355X with bytes 0 and
// 1 right and bytes 2 and 3 wrong in the rows where the resize overshoots; this form keeps the clamp a v_med3_i32 and
// the shift an unsigned one, and the words are right.
__device__ __forceinline__ int clip8(int v) { return (int) ((uint32_t) min(max(v, 0), (256 << 22) - 1) >> 22); }

// One axis of a tile, one lane per output index: the window [first, first + count) clamped to [0, in) and to `taps`,
// the tile's footprint [f0, f0 + fn) (fn <= foot), then the window relative to and inside the footprint.
__device__ __forceinline__ void tile_axis(bool valid, int first, int count, int in, int taps, int foot, int lane,
                                          int* rel_out, int* cnt_out, int* foot_out) {
  int lo = valid ? min(max(first, 0), in) : 0;
  int cnt = valid ? min(max(count, 0), taps) : 0;
  cnt = min(lo + cnt, in) - lo;
  const int f0 = wave_min(cnt > 0 ? lo : INT_MAX);
  const int f1 = wave_max(cnt > 0 ? lo + cnt : 0);
  const int fn = f1 > f0 ? min(f1 - f0, foot) : 0;
  int rel = 0;
  if (cnt > 0) {
    rel = lo - f0;
    cnt = rel < fn ? min(cnt, fn - rel) : 0;
    if (cnt == 0) rel = 0;
  }
  rel_out[lane] = rel;
  cnt_out[lane] = cnt;
  if (lane == 0) {
    foot_out[0] = fn > 0 ? f0 : 0;
    foot_out[1] = fn;
  }
}

// ---------------------------------------------------------------------------------------------------------
// (a) resample: raw footprint -> LDS, horizontal pass -> uint8 LDS tile, vertical pass -> staging image
// ---------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kImgBlock) img_resample_kernel(ImgParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char s_dyn[];   // hbuf [foot_h][192] | raw [foot_h][raw_pitch]
  __shared__ int s_ctap[kMaxTaps * kTileW];       // [tap][column]: a wave's lanes read consecutive banks
  __shared__ int s_rtap[kTileH * kMaxTaps];       // [row][tap]
  __shared__ int s_crel[kTileW], s_ccnt[kTileW], s_rrel[64], s_rcnt[64];
  __shared__ int s_foot[4];                       // fx0, fw, fy0, fh
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int bn = blockIdx.z, j0 = blockIdx.x * kTileW, i0 = blockIdx.y * kTileH;
  const int tw = min(kTileW, p.W - j0), th = min(kTileH, p.H - i0);

  if (wave == 0) {
    const bool valid = lane < tw;
    const long at = (long) bn * p.W + j0 + lane;
    tile_axis(valid, valid ? p.col_first[at] : 0, valid ? p.col_count[at] : 0, p.raw_w, p.taps_x, p.foot_w, lane,
              s_crel, s_ccnt, s_foot);
  } else if (wave == 1) {
    const bool valid = lane < th;
    const long at = (long) bn * p.H + i0 + lane;
    tile_axis(valid, valid ? p.row_first[at] : 0, valid ? p.row_count[at] : 0, p.raw_h, p.taps_y, p.foot_h, lane,
              s_rrel, s_rcnt, s_foot + 2);
  }
  for (int i = tid; i < p.taps_x * kTileW; i += kImgBlock) {
    const int k = i >> 6, j = i & 63;
    s_ctap[i] = j < tw ? p.col_taps[((long) bn * p.taps_x + k) * p.W + j0 + j] : 0;
  }
  for (int i = tid; i < p.taps_y * kTileH; i += kImgBlock) {
    const int k = i / kTileH, r = i % kTileH;
    s_rtap[r * kMaxTaps + k] = r < th ? p.row_taps[((long) bn * p.taps_y + k) * p.H + i0 + r] : 0;
  }
  __syncthreads();

  const int fx0 = s_foot[0], fw = s_foot[1], fy0 = s_foot[2], fh = s_foot[3];
  unsigned char* s_h = s_dyn;
  unsigned char* s_raw = s_dyn + p.foot_h * kHRow;
  const uint8_t* img = p.raw + (long) (bn / p.N) * p.raw_b_stride + (long) (bn % p.N) * p.raw_n_stride + (long) fx0 * 3;
  const int nb = fw * 3;

  // the footprint's rows, a wave per row; byte i of the row lives at s_raw[r * raw_pitch + phase + i]
  if (nb > 0) {
    for (int r = wave; r < fh; r += kImgBlock / 64) {
      const uint8_t* g = img + (long) (fy0 + r) * p.raw_row_stride;
      const int phase = (int) (reinterpret_cast<uintptr_t>(g) & 3);
      const uint8_t* ga = g - phase;
      unsigned char* row = s_raw + r * p.raw_pitch;
      const int end = phase + nb;                 // the row's bytes are [phase, end) from ga
      for (int d = lane; d * 4 < end; d += 64) {
        const int o = d * 4;
        if (o >= phase && o + 4 <= end) {
          *reinterpret_cast<uint32_t*>(row + o) = *reinterpret_cast<const uint32_t*>(ga + o);
        } else {
          for (int e = max(o, phase); e < min(o + 4, end); ++e) row[e] = ga[e];
        }
      }
    }
  }
  __syncthreads();

  // horizontal pass: lane = column, a wave per footprint row
  {
    const int cnt = s_ccnt[lane];
    const int rel3 = s_crel[lane] * 3;
    for (int r = wave; r < fh; r += kImgBlock / 64) {
      const int phase = (int) (reinterpret_cast<uintptr_t>(img + (long) (fy0 + r) * p.raw_row_stride) & 3);
      const unsigned char* src = s_raw + r * p.raw_pitch + phase + rel3;
      int a0 = 1 << 21, a1 = 1 << 21, a2 = 1 << 21;
      for (int k = 0; k < cnt; ++k) {
        const int t = s_ctap[k * kTileW + lane];
        a0 += t * (int) src[3 * k];
        a1 += t * (int) src[3 * k + 1];
        a2 += t * (int) src[3 * k + 2];
      }
      unsigned char* dst = s_h + r * kHRow + lane * 3;
      dst[0] = (unsigned char) clip8(a0);
      dst[1] = (unsigned char) clip8(a1);
      dst[2] = (unsigned char) clip8(a2);
    }
  }
  __syncthreads();

  // vertical pass: four bytes of an output row per lane
  constexpr int kQ = kHRow / 4;
  uint8_t* stage = p.stage + ((long) bn * p.H + i0) * p.stage_pitch + (long) j0 * 3;
  const int room = p.stage_pitch - j0 * 3;        // bytes of the staging row from this tile's first column on
  for (int i = tid; i < th * kQ; i += kImgBlock) {
    const int r = i / kQ, q = i % kQ;
    if (q * 4 + 4 > room) continue;
    const int cnt = s_rcnt[r];
    const uint32_t* src = reinterpret_cast<const uint32_t*>(s_h + s_rrel[r] * kHRow) + q;
    int a0 = 1 << 21, a1 = 1 << 21, a2 = 1 << 21, a3 = 1 << 21;
    for (int k = 0; k < cnt; ++k) {
      const int t = s_rtap[r * kMaxTaps + k];
      const uint32_t w = src[k * kQ];
      a0 += t * (int) (w & 255u);
      a1 += t * (int) ((w >> 8) & 255u);
      a2 += t * (int) ((w >> 16) & 255u);
      a3 += t * (int) (w >> 24);
    }
    const uint32_t v = (uint32_t) clip8(a0) | ((uint32_t) clip8(a1) << 8) | ((uint32_t) clip8(a2) << 16) |
                       ((uint32_t) clip8(a3) << 24);
    *reinterpret_cast<uint32_t*>(stage + (long) r * p.stage_pitch + q * 4) = v;
  }
}

// ---------------------------------------------------------------------------------------------------------
// (b) finish: rotate index, flip, fetch, channel swap, normalise
// ---------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kImgBlock) img_finish_kernel(ImgParams p) {
  const int bn = blockIdx.y;
  const int quads = (p.W + 3) / 4;
  const int i = blockIdx.x * kImgBlock + threadIdx.x;
  if (i >= p.H * quads) return;
  const int y = i / quads, x0 = (i % quads) * 4;
  const int32_t* c = p.consts + (long) bn * VAMP_IMG_CONST_COLS;
  const int a0 = c[0], a1 = c[1], a2 = c[2], a3 = c[3], a4 = c[4], a5 = c[5], flip = c[10];
  const uint8_t* stage = p.stage + (long) bn * p.H * p.stage_pitch;

  uint8_t px[4][3];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int x = x0 + e;
    const int sx = (a2 + y * a1 + x * a0) >> 16, sy = (a5 + y * a4 + x * a3) >> 16;
    px[e][0] = px[e][1] = px[e][2] = 0;
    if (x < p.W && sx >= 0 && sx < p.W && sy >= 0 && sy < p.H) {
      const uint8_t* s = stage + (long) sy * p.stage_pitch + (flip ? p.W - 1 - sx : sx) * 3;
      px[e][0] = s[0];
      px[e][1] = s[1];
      px[e][2] = s[2];
    }
  }
  const bool vec = p.W % 4 == 0;
  const long pix = ((long) bn * p.H + y) * p.W + x0;
  if (p.out_u8) {
    uint8_t* o = p.out_u8 + pix * 3;
    if (vec) {
      uint32_t w[3];
#pragma unroll
      for (int d = 0; d < 3; ++d) {
        w[d] = 0;
#pragma unroll
        for (int e = 0; e < 4; ++e) w[d] |= (uint32_t) px[(d * 4 + e) / 3][(d * 4 + e) % 3] << (8 * e);
        reinterpret_cast<uint32_t*>(o)[d] = w[d];
      }
    } else {
      for (int e = 0; e < 4 && x0 + e < p.W; ++e)
        for (int ch = 0; ch < 3; ++ch) o[e * 3 + ch] = px[e][ch];
    }
  }
  if (!p.out) return;
  const long plane = (long) p.H * p.W;
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {
    const int from = p.to_rgb ? 2 - ch : ch;
    float v[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = ((float) px[e][from] - p.mean[ch]) * p.std_inv[ch];
    const long at = ((long) bn * 3 + ch) * plane + (long) y * p.W + x0;
    if (p.out_bf16) {
      uint16_t* o = static_cast<uint16_t*>(p.out) + at;
      if (vec) {
        *reinterpret_cast<uint2*>(o) = make_uint2((uint32_t) f32_to_bf16(v[0]) | ((uint32_t) f32_to_bf16(v[1]) << 16),
                                                  (uint32_t) f32_to_bf16(v[2]) | ((uint32_t) f32_to_bf16(v[3]) << 16));
      } else {
        for (int e = 0; e < 4 && x0 + e < p.W; ++e) o[e] = f32_to_bf16(v[e]);
      }
    } else {
      float* o = static_cast<float*>(p.out) + at;
      if (vec) {
        *reinterpret_cast<float4*>(o) = make_float4(v[0], v[1], v[2], v[3]);
      } else {
        for (int e = 0; e < 4 && x0 + e < p.W; ++e) o[e] = v[e];
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------
static_assert(sizeof(VampImageDesc) == 104, "VampImageDesc layout: part of the ABI (the binding reads it from include/vampire_hip.h)");

int img_validate(const VampImageDesc* d) {
  VAMP_REQUIRE(d, "desc is NULL");
  VAMP_REQUIRE(d->B >= 1 && d->B <= kImgMaxB, "B must be in [1, 4096]");
  VAMP_REQUIRE(d->N >= 1 && d->N <= kImgMaxN, "N must be in [1, 16]");
  VAMP_REQUIRE(d->raw_h >= 1 && d->raw_h <= kImgMaxRaw && d->raw_w >= 1 && d->raw_w <= kImgMaxRaw,
               "raw_h, raw_w must be in [1, 65536]");
  VAMP_REQUIRE(d->H >= 1 && d->H <= kImgMaxSide && d->W >= 1 && d->W <= kImgMaxSide, "H, W must be in [1, 4096]");
  VAMP_REQUIRE(d->taps_x >= 1 && d->taps_x <= kMaxTaps && d->taps_y >= 1 && d->taps_y <= kMaxTaps,
               "taps_x, taps_y must be in [1, 16] (VAMP_IMG_MAX_TAPS): the resize is outside the library's range");
  VAMP_REQUIRE(d->foot_w >= 1 && d->foot_w <= VAMP_IMG_FOOT_W && d->foot_h >= 1 && d->foot_h <= VAMP_IMG_FOOT_H,
               "foot_w, foot_h must be in [1, 272] and [1, 48]: the resize is outside the library's range");
  VAMP_REQUIRE(d->out_dtype == VAMP_F32 || d->out_dtype == VAMP_BF16 || d->out_dtype == VAMP_IMG_OUT_NONE,
               "out_dtype must be VAMP_F32, VAMP_BF16 or VAMP_IMG_OUT_NONE");
  VAMP_REQUIRE(d->to_rgb == 0 || d->to_rgb == 1, "to_rgb must be 0 or 1");
  for (int c = 0; c < 3; ++c)
    VAMP_REQUIRE(std::isfinite(d->mean[c]) && std::isfinite(d->std_inv[c]), "mean and std_inv must be finite");
  VAMP_REQUIRE(d->raw_row_stride >= (int64_t) d->raw_w * 3, "raw_row_stride must be at least 3 raw_w bytes");
  VAMP_REQUIRE(d->raw_n_stride >= 0 && d->raw_b_stride >= 0, "raw_n_stride, raw_b_stride must not be negative");
  VAMP_REQUIRE((long) d->B * d->N <= 65535, "B N must not exceed 65535");
  VAMP_REQUIRE(d->reserved[0] == 0 && d->reserved[1] == 0, "reserved must be 0");
  return VAMP_OK;
}

size_t img_stage_pitch(const VampImageDesc* d) { return align_up((size_t) d->W * 3, 16); }

}  // namespace
}  // namespace vamp

using namespace vamp;

extern "C" {

size_t vamp_camera_images_workspace_bytes(const VampImageDesc* d) {
  if (img_validate(d)) return 0;
  return align_up((size_t) d->B * d->N * d->H * img_stage_pitch(d), 256);
}

int vamp_camera_images(const VampImageDesc* d, const uint8_t* raw, const int32_t* col_first, const int32_t* col_count,
                       const int32_t* col_taps, const int32_t* row_first, const int32_t* row_count,
                       const int32_t* row_taps, const int32_t* consts, void* out, uint8_t* out_u8, void* workspace,
                       size_t workspace_bytes, void* stream) {
  if (int e = img_validate(d)) return e;
  VAMP_REQUIRE(out || out_u8, "out and out_u8 are both NULL: nothing to do");
  VAMP_REQUIRE((out != nullptr) == (d->out_dtype != VAMP_IMG_OUT_NONE),
               "out must be given exactly when out_dtype is not VAMP_IMG_OUT_NONE");
  VAMP_REQUIRE(raw && col_first && col_count && col_taps && row_first && row_count && row_taps && consts,
               "raw or a plan table is NULL");
  VAMP_REQUIRE(aligned(out, 16), "out must be 16-byte aligned");
  VAMP_REQUIRE(aligned(out_u8, 4), "out_u8 must be 4-byte aligned");
  const size_t need = vamp_camera_images_workspace_bytes(d);
  if (int e = workspace_fits(__func__, workspace, workspace_bytes, need)) return e;
  VAMP_REQUIRE(aligned(workspace, 16), "workspace must be 16-byte aligned");

  ImgParams q{};
  q.raw = raw;
  q.col_first = col_first; q.col_count = col_count; q.col_taps = col_taps;
  q.row_first = row_first; q.row_count = row_count; q.row_taps = row_taps; q.consts = consts;
  q.out = out; q.out_u8 = out_u8; q.stage = static_cast<uint8_t*>(workspace);
  q.raw_b_stride = (long) d->raw_b_stride; q.raw_n_stride = (long) d->raw_n_stride;
  q.raw_row_stride = (long) d->raw_row_stride;
  q.N = d->N; q.raw_h = d->raw_h; q.raw_w = d->raw_w; q.H = d->H; q.W = d->W;
  q.taps_x = d->taps_x; q.taps_y = d->taps_y; q.foot_w = d->foot_w; q.foot_h = d->foot_h;
  // a row of the LDS footprint: 3 foot_w bytes behind a phase of up to 3, in an odd number of dwords
  q.raw_pitch = (int) align_up((size_t) d->foot_w * 3 + 3, 4);
  if ((q.raw_pitch / 4) % 2 == 0) q.raw_pitch += 4;
  q.stage_pitch = (int) img_stage_pitch(d);
  q.out_bf16 = d->out_dtype == VAMP_BF16; q.to_rgb = d->to_rgb;
  for (int c = 0; c < 3; ++c) { q.mean[c] = d->mean[c]; q.std_inv[c] = d->std_inv[c]; }

  hipStream_t s = static_cast<hipStream_t>(stream);
  const int BN = d->B * d->N;
  const size_t lds = (size_t) d->foot_h * (kHRow + q.raw_pitch);
  const dim3 tiles((d->W + kTileW - 1) / kTileW, (d->H + kTileH - 1) / kTileH, BN);
  VAMP_TIMED(kProfAux, s, (img_resample_kernel<<<tiles, kImgBlock, lds, s>>>(q)));
  const int quads = d->H * ((d->W + 3) / 4);
  VAMP_TIMED(kProfAux, s, (img_finish_kernel<<<dim3((quads + kImgBlock - 1) / kImgBlock, BN), kImgBlock, 0, s>>>(q)));
  return check_launch("camera_images");
}

}  // extern "C"
