// Shared by the lift kernels: parameters and the bit-exact voxel -> pixel projection.
#pragma once
#include "common.hpp"
#include "cell_list.hpp"

#include <algorithm>

namespace vamp {

struct LiftParams {
  int B, N, C, D, fH, fW, Z, Y, X;
  float u_max, v_max, u_div, v_div, d_lo, d_hi, d_span;
  int use_depth;
};

inline LiftParams to_params(const VampLiftDesc* d) {
  LiftParams p;
  p.B = d->B; p.N = d->N; p.C = d->C; p.D = d->D; p.fH = d->fH; p.fW = d->fW;
  p.Z = d->Z; p.Y = d->Y; p.X = d->X;
  p.u_max = d->u_max; p.v_max = d->v_max; p.u_div = d->u_div; p.v_div = d->v_div;
  p.d_lo = d->d_lo; p.d_hi = d->d_hi; p.d_span = d->d_span; p.use_depth = d->use_depth;
  return p;
}

// Result of projecting one voxel centre into one camera.
struct LiftTap {
  bool valid;
  int ix0, iy0, iz0;
  float wx0, wx1, wy0, wy1, wz0, wz1;
  float zz;              // projected depth (camera z), used to bin voxels into depth slabs
  float fx, fy, fz;      // continuous tap coordinates
};

// get_pixel (bv2:365-388) + validity / normalisation (bv2:493-505) + aten's
// grid_sampler_unnormalize for align_corners=False.  Evaluation order is part of
// the contract (bit-exact tap indices): do not reassociate, do not fuse.
// WAVE_CULL (callers in wave-uniform control flow only): when the third row of `ida` is exactly
// (0, 0, 1, 0) -- image-plane augmentations never touch depth -- the projected depth zz equals the
// camera-space z bit for bit (or is NaN), so a camera that no lane of the wave has in front of it
// (z > d_lo, resp. z > 0) is invalid for all 64 voxels and the divisions, the third matrix and
// the normalisation are skipped: the same masks as the full chain, about half of the projections
// (the cameras facing away) at a third of the instructions.
// lift_project_from: the chain behind its first product.  `p` = inv(bda) . (x, y, z, 1), which is the same
// vector for every camera of a sample whose cameras share inv(bda) bit for bit (they do: bda is one matrix
// per sample, bv2:370-372), so callers that know it (the cull word's kLiftCullSharedBda bit) form it once.
template <bool WAVE_CULL = false>
__device__ __forceinline__ LiftTap lift_project_from(const LiftParams& P, const float* __restrict__ m, Vec4 p) {
  p = matvec(m + 16, p);   // intrin @ inv(sensor2ego)
  if (WAVE_CULL) {
    const bool e3 = m[40] == 0.0f && m[41] == 0.0f && m[42] == 1.0f && m[43] == 0.0f;   // uniform
    if (e3 && !__any(p.z > (P.use_depth ? P.d_lo : 0.0f))) {
      LiftTap t;
      t.valid = false;
      t.ix0 = t.iy0 = t.iz0 = 0;
      t.wx0 = t.wx1 = t.wy0 = t.wy1 = t.wz0 = t.wz1 = 0.f;
      t.zz = p.z;
      t.fx = t.fy = t.fz = 0.f;
      return t;
    }
  }
  float zc = (p.z < 1e-6f) ? 1e-6f : p.z;   // clamp(min=eps); NaN stays NaN
  p.x = p.x / zc;
  p.y = p.y / zc;
  p = matvec(m + 32, p);   // ida
  const float u = p.x, v = p.y, zz = p.z;
  LiftTap t;
  bool ok = (u > -0.5f) && (u < P.u_max) && (v > -0.5f) && (v < P.v_max);
  if (P.use_depth) ok = ok && (zz > P.d_lo) && (zz < P.d_hi);
  else ok = ok && (zz > 0.0f);
  t.valid = ok;
  t.zz = zz;
  float nx = 2.0f * (u / P.u_div) - 1.0f;
  float ny = 2.0f * (v / P.v_div) - 1.0f;
  float nz = P.use_depth ? (2.0f * ((zz - P.d_lo) / P.d_span) - 1.0f) : 0.0f;
  nx = fminf(fmaxf(nx, -2.0f), 2.0f);
  ny = fminf(fmaxf(ny, -2.0f), 2.0f);
  nz = fminf(fmaxf(nz, -2.0f), 2.0f);
  const float fx = ((nx + 1.0f) * (float) P.fW - 1.0f) / 2.0f;
  const float fy = ((ny + 1.0f) * (float) P.fH - 1.0f) / 2.0f;
  const float fz = ((nz + 1.0f) * (float) P.D - 1.0f) / 2.0f;
  const float flx = floorf(fx), fly = floorf(fy), flz = floorf(fz);
  t.ix0 = (int) flx; t.iy0 = (int) fly; t.iz0 = (int) flz;
  t.wx1 = fx - flx; t.wx0 = (flx + 1.0f) - fx;
  t.wy1 = fy - fly; t.wy0 = (fly + 1.0f) - fy;
  t.wz1 = fz - flz; t.wz0 = (flz + 1.0f) - fz;
  t.fx = fx; t.fy = fy; t.fz = fz;
  return t;
}

template <bool WAVE_CULL = false>
__device__ __forceinline__ LiftTap lift_project(const LiftParams& P, const float* __restrict__ m,
                                                float x, float y, float z) {
  return lift_project_from<WAVE_CULL>(P, m, matvec(m, Vec4{x, y, z, 1.0f}));   // inv(bda) first
}


// ---------------------------------------------------------------------------
// The tile of the projecting kernels (lift.hip) and the patch of voxels one camera cull word stands for (the workspace
// below holds a word per patch).
// ---------------------------------------------------------------------------
// tile shape: lanes along x for coalesced stores
// A wave is a 16 x 4 patch of voxels, not a 64 x 1 row: the exact wave-level camera cull of
// lift_project<true> skips a camera only when none of the wave's voxels has it in front, and a
// 6.4 m x 1.6 m patch is on one side of most cameras where a 25.6 m row is not (cfg-B: 47 -> 36 us;
// 8 x 32 / 16 x 16 / 32 x 8 / 64 x 4 workgroup tiles: 36.5 / 35.7 / 38.2 / 47.1).
#ifndef VAMP_LIFT_TX
#define VAMP_LIFT_TX 16
#define VAMP_LIFT_TY 16
#endif
#ifndef VAMP_CULL_WPW
#define VAMP_CULL_WPW 4      // (1 / 2 / 4: first launch 9.9 / 9.0 / 9.0 us, forward kernel 28.3 / 28.4 / 28.4 at cfg-B)
#endif
constexpr int kCullWpw = VAMP_CULL_WPW;     // waves of lift_fwd_kernel (stacked along y) that share a word: 1, 2 or 4
constexpr int kCullPX = VAMP_LIFT_TX, kCullPY = 64 / VAMP_LIFT_TX * kCullWpw;

struct LiftCull {
  unsigned* words;      // [B][Z][nyp][nxp]
  int nxp, nyp;         // patches per row / column of one z plane
  int px, py;           // patch shape in voxels
  int group;            // lanes per patch in a cull workgroup: the power of two >= N
  int bps;              // stand-alone cull: workgroups (256 / group patches each) per sample
  int ppt;              // forward's first launch: patches per feature tile (N * ptiles tiles per sample)
};

// ---------------------------------------------------------------------------
// The lift workspace (vamp_lift_workspace_bytes; region by region: vamp_lift_workspace_layout), in this order, every
// region 256-byte aligned and back to back:
//   feat_cl | gfeat_cl | cnt | off | bsum | boff | aux | amask | ptaps | pcell | recs | rowq | cull words
// cnt .. rowq are the cell lists of the lift backward (lift_bwd_cell.hip); they lie behind the copies: a forward must
// not disturb prepared offsets.  Cell = (image, floor tap row + 1, floor tap column + 1): (fH + 1) x (fW + 1) cells per
// camera image.  The FORWARD kernel (grad mode) or the stand-alone prepare kernel counts the valid (voxel, camera)
// pairs per cell and leaves every pair's taps and its four depth samples in `ptaps` (and `pcell`), indexed by
// (image, voxel); the backward's fill pass only re-lays them in cell order, each with its voxel's gradient row --
// nothing on the backward projects a voxel or reads a depth plane again.
// ---------------------------------------------------------------------------
struct LiftWorkspace {
  float* feat_cl;                    // [B * N, HW, C] channel-last fp32 copy of the features
  float* gfeat_cl;                   // [B * N, HW, C] the splat backward's gradient in that layout
  int *cnt, *off, *bsum, *boff, *aux;   // counters (+ the scan's ticket word) and the scan's levels, as launch_cell_scan takes them
  unsigned* amask;                   // [B * V] cameras each voxel has a pair with (N <= 32)
  float4* ptaps;                     // [B * N * V][2] of the pair, voxel order (sparse): {wx1, wy1, wz1, (iz0 + 1) | (ix0 + 1) << 16} |
                                     // its depth samples sum_d w_d depth[d, pixel] at its four pixel taps (32 bytes side by side:
                                     // as two arrays the second store cost the training forward 8 us)
  int* pcell;                        // [B * N * V] (floor row + 1) << 16 | (floor column + 1)
  float4* recs;                      // [cap][2 + C / 4] every pair in cell order: its taps | its depth samples | its voxel's
                                     // row grad_out / (hits + 1e-6) -- everything the gather needs of a pair, one run
  int* rowq;                         // [B * N * fH] image rows, those with the most pairs first
  LiftCull cull;                     // camera cull words of the forward's waves (cull.words: the last region) and their geometry
  long ncull;
  size_t offset[VAMP_LIFTWS_REGIONS], region_bytes[VAMP_LIFTWS_REGIONS];   // of the regions above, in that order
  int cw, ch;                        // cells per row / column of one camera
  long ncell;                        // padded to the scan tile, + 2 for the range ends
  size_t bytes;
};

// `workspace` may be nullptr (only the sizes and the geometry are of use then)
inline LiftWorkspace lift_workspace(const VampLiftDesc* d, void* workspace) {
  LiftWorkspace w;
  w.cw = d->fW + 1;
  w.ch = d->fH + 1;
  const long nc = (long) d->B * d->N * w.cw * w.ch + 2;
  w.ncell = (nc + kScanTile - 1) / kScanTile * kScanTile;
  const size_t ncell = (size_t) w.ncell;
  // every (voxel, camera) pair can be valid
  const size_t V = (size_t) d->Z * d->Y * d->X;
  const size_t cap = (size_t) d->B * d->N * V;
  w.cull.px = VAMP_LIFT_TX;
  w.cull.py = kCullPY;
  w.cull.nxp = (d->X + VAMP_LIFT_TX - 1) / VAMP_LIFT_TX;
  w.cull.nyp = (d->Y + VAMP_LIFT_TY - 1) / VAMP_LIFT_TY * (4 / kCullWpw);
  w.ncull = (long) d->B * d->Z * w.cull.nyp * w.cull.nxp;
  w.cull.group = 1;
  while (w.cull.group < d->N) w.cull.group *= 2;
  const int ppb = std::min(256 / w.cull.group, 64);
  const long per_sample = (long) d->Z * w.cull.nyp * w.cull.nxp;
  w.cull.bps = (int) ((per_sample + ppb - 1) / ppb);
  const long tiles = (long) d->N * (((long) d->fH * d->fW + 63) / 64);
  w.cull.ppt = (int) ((per_sample + tiles - 1) / tiles);
  Carve c(workspace);
  int region = 0;
  auto take = [&](auto*& p, size_t count) {      // the next region of the table: `count` elements for p
    w.offset[region] = c.off;
    p = c.take<std::remove_reference_t<decltype(*p)>>(count);
    w.region_bytes[region] = c.off - w.offset[region];
    ++region;
  };
  const size_t feat = (size_t) d->B * d->N * d->fH * d->fW * d->C;
  take(w.feat_cl, feat);
  take(w.gfeat_cl, feat);
  take_scan(take, ncell, w.cnt, w.off, w.bsum, w.boff, w.aux);
  take(w.amask, (size_t) d->B * V);
  take(w.ptaps, cap * 2);
  take(w.pcell, cap);
  take(w.recs, cap * (size_t) (2 + (d->C + 3) / 4));
  take(w.rowq, (size_t) d->B * d->N * d->fH);
  take(w.cull.words, (size_t) w.ncull);
  w.bytes = c.off;
  return w;
}

// VAMP_REQUIRE in a function that refuses in the name of its caller `who` (the plans)
#define VAMP_REQUIRE_AS(who, cond, msg)                                                             \
  do {                                                                                              \
    if (!(cond)) return ::vamp::fail(VAMP_EINVAL, "%s: requirement failed: " msg, who);             \
  } while (0)

// What the projecting kernels hand to lift_emit_pair.
struct LiftEmit {
  int* cnt;
  unsigned* amask;
  float4* ptaps;                     // [.][2]: taps | depth samples
  int* pcell;
  int cw, ch;
};

inline LiftEmit lift_emit_of(const LiftWorkspace& w) { return LiftEmit{w.cnt, w.amask, w.ptaps, w.pcell, w.cw, w.ch}; }

// One camera of one voxel, called in WAVE-UNIFORM control flow (exited lanes are fine): counts the
// pair in its cell -- one atomic per run of lanes with equal cells, x-neighbouring voxels share a
// cell in the far field -- and stores its taps and its depth samples `dep` (depth_taps: the planes around
// the projected depth interpolated at the four pixel taps, zero padding) at (image, voxel).  Returns whether
// the voxel has a pair with this camera (at least one of the four pixel taps exists).
// (The depth samples are stored by lift_emit_dep, which callers place BEHIND their other loads: the store has to
// wait for the depth planes, and issued here -- in front of the feature gather -- it held that gather's loads
// back by a round trip per camera: 37 -> 45 us for the training forward.)
__device__ __forceinline__ bool lift_emit_pair(const LiftParams& P, const LiftEmit& E, const LiftTap& t,
                                               bool live, long bn, long V, long vox, int lane) {
  const bool act = live && t.valid && t.ix0 >= -1 && t.ix0 < P.fW && t.iy0 >= -1 && t.iy0 < P.fH;
  if (!__any(act)) return false;
  const long cell = (bn * E.ch + (t.iy0 + 1)) * E.cw + (t.ix0 + 1);
  const LaneRun r = lane_run(act, cell, lane);
  if (r.head) atomicAdd(E.cnt + cell, r.len);
  if (act) {
    // (iz0 >= -1 for a valid pair; the cell column rides in the upper half of the same word)
    E.ptaps[(bn * V + vox) * 2] = make_float4(t.wx1, t.wy1, t.wz1, __int_as_float((t.iz0 + 1) | ((t.ix0 + 1) << 16)));
    E.pcell[bn * V + vox] = ((t.iy0 + 1) << 16) | (t.ix0 + 1);
  }
  return act;
}
__device__ __forceinline__ void lift_emit_dep(const LiftEmit& E, bool act, long bn, long V, long vox, const float (&dep)[4]) {
  if (act) E.ptaps[(bn * V + vox) * 2 + 1] = make_float4(dep[0], dep[1], dep[2], dep[3]);
}

// ---- the lift's host functions that cross files, each declared here once ----
// lift_bwd_cell.hip
// The shapes the cell lists cannot hold: asked (by the plans, by vamp_lift_prepare) before anything is launched, wherever
// pairs are emitted or the prepare pass runs (`who`: the entry point whose name a refusal carries)
int lift_cells_fit(const char* who, const VampLiftDesc* d);
// the counters in front of a kernel that emits pairs: zeroed, or -- `clean` -- promised zero (verified under vamp_debug_checks)
int launch_lift_cells_begin(const LiftWorkspace& w, bool clean, hipStream_t s);
// ... and their scan behind it
int launch_lift_cells_end(const LiftWorkspace& w, hipStream_t s);
int lift_cells_scan_job(const LiftWorkspace& w, ScanJob* job);
// The backward's plan for `who`: vamp_lift_backward_plan.
int lift_backward_plan(const char* who, const VampLiftDesc* d, int flags, size_t workspace_bytes, VampLiftBackwardPlan* out);
// the cell-list backward as the plan says (path VAMP_LIFTPLAN_BWD_CELL)
int launch_lift_bwd_cell(const VampLiftDesc* d, const LiftParams& P, const VampLiftBackwardPlan& plan, const LiftWorkspace& w,
                         const float* mats, const float* xs, const float* ys, const float* zs, const void* depth,
                         const void* feat, const float* gout, const uint64_t* hits, float* gdepth, float* gfeat,
                         hipStream_t s);
// lift.hip
// (the caller has asked lift_cells_fit)
int launch_lift_cell_prepare(const VampLiftDesc* d, const LiftParams& P, const LiftWorkspace& w, const float* mats,
                             const float* xs, const float* ys, const float* zs, const void* depth, hipStream_t s);
// the channel counts the fused kernels are compiled for
inline bool lift_channels_ok(int C) { return C == 4 || C == 8 || (C % 16 == 0 && C <= 64); }
int lift_validate(const VampLiftDesc* d);

}  // namespace vamp

// lift.hip: the pair cells' scan as a job for a launch shared with another cell list (vamp_render_camera_prepare_with_lift)
extern "C" int lift_scan_job(const VampLiftDesc* d, void* workspace, size_t workspace_bytes, vamp::ScanJob* job);
