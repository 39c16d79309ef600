// The four point queries of a step in one operator: the lidar points' semantic logits and sdf and the Occ3D grid's
// logits and density of base_vampire2.py:576-609, from packed points with per-sample counts.
//
//   pts_logits  = grid_sample(semantic_logits[b], lidar points of b, padding_mode='border')   bv2:590
//   pts_sdf     = grid_sample(density_feature[b], lidar points of b) * inside-mask            bv2:594-595
//   occ_logits  = grid_sample(semantic_logits, bda-rotated occ grid, padding_mode='border')   bv2:603
//   occ_density = grid_sample(density(density_feature), same grid)                            bv2:604
//
// Forward: one launch per point set, thread per point.  A point's tap coordinates are computed once (point_sample.hpp,
// the chain of sample_points.hip: same bits).  Inside the bounds the border clip is the identity, so one set of taps
// serves all K + 1 channels; a lidar point outside adds nothing to the sdf (the mask); an occupancy point outside takes
// the clipped taps for the K semantic channels and the unclipped ones, non-voxel taps skipped, for the density.
//
// Backward: ONE cell list (cell_list.hpp) over the union of both point sets and all samples, and one per-voxel gather
// that writes grad_semantic and grad_density once each.  Record sources are numbered
//   [0, B M)                     lidar point (b, i)                         clipped taps
//   [B M, B M + B P)             occupancy point (b, p)                     clipped taps
//   [B M + B P, B M + 2 B P)     the same occupancy point when it is outside: unclipped taps, density entry only
// and a source's gradient row is K + 1 floats, padded to a multiple of 4: entry 0 the density channel, then the K
// semantic channels.  The lidar sdf reaches grad_density raw, the occupancy density through the activation's
// derivative, which is applied once per voxel: the gather keeps entry 0 of the lidar sources and of the occupancy
// sources in two accumulators (record_accumulate<.., SPLIT>).  A voxel whose records from BOTH sets together exceed
// kPtsHeavy goes to the heavy kernel.  d beta: one partial per workgroup, summed in a fixed order.
#include "point_sample.hpp"

#include <algorithm>

namespace vamp {

// the gather's shape, the same three as sample_points.hip
constexpr int kPtsHeavy = 256;
constexpr int PGL = 8;                 // lanes per voxel in the gather
constexpr int PVPB = 256 / PGL;
constexpr int kHeavyGrid = 4096;       // workgroups of the heavy kernel, at most

struct QueryParams {
  SampleParams S;          // the volume's geometry; C = K, border = 0 (clip_tap is applied where it belongs)
  int M, want_sdf, P, occ_shared;
  long nL, nO;             // B * M, B * P
};

static int validate(const VampQueryDesc* d) {
  VAMP_REQUIRE(d != nullptr, "descriptor is NULL");
  VAMP_REQUIRE(d->B > 0 && d->K > 0 && d->K + 1 <= 32, "B > 0, 0 < K, K + 1 <= 32 (the gather's widest row)");
  VAMP_REQUIRE(d->Z > 0 && d->Y > 0 && d->X > 0 && d->X < 2047 && d->Y < 2047 && d->Z < 511,
               "volume extents (X, Y < 2047, Z < 511: packed tap keys)");
  VAMP_REQUIRE(d->span[0] != 0.f && d->span[1] != 0.f && d->span[2] != 0.f, "zero span");
  VAMP_REQUIRE(d->density_mode == VAMP_DENSITY_SIGMOID || d->density_mode == VAMP_DENSITY_SDF_LAPLACE, "density_mode");
  VAMP_REQUIRE(d->sem_dtype == VAMP_F32 || d->sem_dtype == VAMP_BF16, "sem_dtype");
  VAMP_REQUIRE(d->den_dtype == VAMP_F32 || d->den_dtype == VAMP_BF16, "den_dtype");
  VAMP_REQUIRE(d->M >= 0 && d->P_occ >= 0, "M >= 0, P_occ >= 0");
  VAMP_REQUIRE((long) d->B * ((long) d->M + 2L * d->P_occ) < 0x7fffffffL, "too many points");
  const size_t voxels = (size_t) d->B * d->Z * d->Y * d->X;
  VAMP_REQUIRE(voxels < 0x7fffffffu && cell_count_padded(d->B, d->Z, d->Y, d->X) < 0x7fffffffL,
               "voxel / cell count exceeds 2^31");
  return VAMP_OK;
}

static QueryParams to_params(const VampQueryDesc* d) {
  QueryParams q;
  SampleParams& p = q.S;
  p.B = d->B; p.C = d->K; p.Z = d->Z; p.Y = d->Y; p.X = d->X; p.Pb = d->P_occ;
  for (int i = 0; i < 3; ++i) { p.lo[i] = d->lo[i]; p.span[i] = d->span[i]; }
  p.border = 0; p.mask_outside = 0; p.activation = 1; p.channel_last = 0;
  p.density_mode = d->density_mode; p.sdf_bias = d->sdf_bias; p.beta_min = d->beta_min;
  const long n12 = (long) d->lattice[1] * d->lattice[2];
  const bool lat = d->lattice[0] > 0 && n12 > 0 && (long) d->lattice[0] * n12 == d->P_occ;
  p.n0 = lat ? d->lattice[0] : 0;
  p.n12 = lat ? (int) n12 : 0;
  q.M = d->M; q.want_sdf = d->want_sdf; q.P = d->P_occ; q.occ_shared = d->occ_shared;
  q.nL = (long) d->B * d->M; q.nO = (long) d->B * d->P_occ;
  return q;
}

// rows of sample b that count: counts[b] clamped to [0, M]
__device__ __forceinline__ int live_rows(const int* __restrict__ counts, int b, int M) {
  return counts ? min(max(counts[b], 0), M) : M;
}

// ---------------------------------------------------------------------------
// forward
// ---------------------------------------------------------------------------
template <typename TS, typename TD>
__global__ void __launch_bounds__(256)
point_queries_lidar_fwd_kernel(QueryParams Q, const TS* __restrict__ sem, const TD* __restrict__ den,
                               const float* __restrict__ pts, const int* __restrict__ counts,
                               float* __restrict__ pts_logits, float* __restrict__ pts_sdf) {
  const SampleParams& P = Q.S;
  const int p = blockIdx.x * 256 + threadIdx.x;
  const int b = blockIdx.y;
  if (p >= Q.M) return;
  const long row = (long) b * Q.M + p;
  if (p >= live_rows(counts, b, Q.M)) {          // padding: never read, written as exact 0
    for (int c = 0; c < P.C; ++c) pts_logits[row * P.C + c] = 0.f;
    if (Q.want_sdf) pts_sdf[row] = 0.f;
    return;
  }
  PointTap t = point_tap(P, pts + row * 3);
  clip_tap(P, t);                                 // (the identity for a point inside)
  const Taps8 q = point_taps8(P, t);
  const long V = (long) P.Z * P.Y * P.X;
  DensityParams none;
  none.mode = VAMP_DENSITY_SIGMOID; none.beta = 1.f; none.ib = 1.f; none.bias = 0.f;
  for (int c = 0; c < P.C; ++c)
    pts_logits[row * P.C + c] = taps8_sample(q, sem, ((long) b * P.C + c) * V, false, none);
  if (Q.want_sdf) pts_sdf[row] = t.inside ? taps8_sample(q, den, (long) b * V, false, none) : 0.f;
}

template <typename TS, typename TD>
__global__ void __launch_bounds__(256)
point_queries_occ_fwd_kernel(QueryParams Q, const TS* __restrict__ sem, const TD* __restrict__ den,
                             const float* __restrict__ beta_raw, const float* __restrict__ occ,
                             float* __restrict__ occ_logits, float* __restrict__ occ_density) {
  const SampleParams& P = Q.S;
  int p = blockIdx.x * 256 + threadIdx.x;
  const int b = blockIdx.y;
  if (p >= Q.P) return;
  // lattice hint, as sample_points_fwd_kernel: consecutive lanes walk the lattice axis that runs along the volume's x
  if (P.n0 > 0) p = (p % P.n0) * P.n12 + p / P.n0;
  const PointTap t = point_tap(P, occ + ((long) (Q.occ_shared ? 0 : b) * Q.P + p) * 3);
  PointTap tc = t;
  clip_tap(P, tc);
  const Taps8 qc = point_taps8(P, tc);
  const long V = (long) P.Z * P.Y * P.X;
  const DensityParams dp = load_density(P.density_mode, beta_raw, P.beta_min, P.sdf_bias);
  for (int c = 0; c < P.C; ++c)
    occ_logits[((long) b * P.C + c) * Q.P + p] = taps8_sample(qc, sem, ((long) b * P.C + c) * V, false, dp);
  float s;
  if (t.inside) {
    s = taps8_sample(qc, den, (long) b * V, true, dp);
  } else {
    const Taps8 qz = point_taps8(P, t);
    s = taps8_sample(qz, den, (long) b * V, true, dp);
  }
  occ_density[(long) b * Q.P + p] = s;
}

// ---------------------------------------------------------------------------
// backward: rank, fill + gradient rows, gather
// ---------------------------------------------------------------------------
struct Source {
  int b, p;          // sample, point index inside its set
  int kind;          // 0 lidar, 1 occupancy (clipped taps), 2 occupancy (unclipped taps, density only)
};
__device__ __forceinline__ Source source_of(const QueryParams& Q, long g) {
  Source s;
  if (g < Q.nL) {
    s.kind = 0; s.b = (int) (g / Q.M); s.p = (int) (g % Q.M);
    return s;
  }
  long o = g - Q.nL;
  s.kind = 1;
  if (o >= Q.nO) { o -= Q.nO; s.kind = 2; }
  s.b = (int) (o / Q.P); s.p = (int) (o % Q.P);
  return s;
}

__global__ void __launch_bounds__(256)
point_queries_rank_kernel(QueryParams Q, const float* __restrict__ pts, const int* __restrict__ counts,
                          const float* __restrict__ occ, int* __restrict__ cnt, int* __restrict__ KEY,
                          int* __restrict__ RANK, float4* __restrict__ F, long ncell_b) {
  const SampleParams& P = Q.S;
  const long gid = (long) blockIdx.x * 256 + threadIdx.x;
  const long total = Q.nL + 2 * Q.nO;
  const int lane = threadIdx.x & 63;
  const long g = min(gid, total - 1);
  const Source src = source_of(Q, g);
  bool live = gid < total;
  float c[3] = {0.f, 0.f, 0.f};
  if (src.kind == 0) {
    live = live && src.p < live_rows(counts, src.b, Q.M);
    if (live) { const float* q = pts + g * 3; c[0] = q[0]; c[1] = q[1]; c[2] = q[2]; }
  } else {
    const float* q = occ + ((long) (Q.occ_shared ? 0 : src.b) * Q.P + src.p) * 3;
    c[0] = q[0]; c[1] = q[1]; c[2] = q[2];
  }
  PointTap t = point_tap(P, c);
  const bool inside = t.inside;
  if (src.kind != 2) clip_tap(P, t);
  const float flx = floorf(t.fx), fly = floorf(t.fy), flz = floorf(t.fz);
  // a source contributes iff at least one tap per axis is a voxel: floor in [-1, size - 1]
  bool act = live && flx >= -1.f && flx <= (float) (P.X - 1) && fly >= -1.f &&
             fly <= (float) (P.Y - 1) && flz >= -1.f && flz <= (float) (P.Z - 1);
  if (src.kind == 2 && inside) act = false;       // inside, the clipped record carries the density entry
  const int key = act ? pack_cell_key((int) flx, (int) fly, (int) flz) : 0;
  const long cell = key_to_cell(key, P.Y, P.X, (unsigned) src.b, ncell_b);
  const LaneRun r = lane_run(act, cell, lane);
  int base = 0;
  if (r.head) base = atomicAdd(cnt + cell, r.len);
  base = __shfl(base, act ? r.start : lane, 64);
  if (gid < total) {
    KEY[gid] = act ? key : -1;                    // -1, not pack_cell_key's 0: floors (-1, -1, -1) pack to 0 as well
    if (act) {
      RANK[gid] = base + (lane - r.start);
      F[gid] = make_float4(t.fx, t.fy, t.fz, inside ? 1.f : 0.f);
    }
  }
}

// the record of a source into its slot, and the source's gradient row [CP]: density entry, K semantic entries, zeros
__global__ void __launch_bounds__(256)
point_queries_fill_kernel(QueryParams Q, const int* __restrict__ KEY, const int* __restrict__ RANK,
                          const float4* __restrict__ F, const int* __restrict__ off,
                          const int* __restrict__ boff, const float* __restrict__ g_pts_logits,
                          const float* __restrict__ g_pts_sdf, const float* __restrict__ g_occ_logits,
                          const float* __restrict__ g_occ_density, float4* __restrict__ R,
                          float* __restrict__ G, int CP, long ncell_b) {
  const SampleParams& P = Q.S;
  const long gid = (long) blockIdx.x * 256 + threadIdx.x;
  if (gid >= Q.nL + 2 * Q.nO) return;
  const int key = KEY[gid];
  if (key < 0) return;                // no record (point_queries_rank_kernel): its upstream rows are never read
  const Source src = source_of(Q, gid);
  const long cell = key_to_cell(key, P.Y, P.X, (unsigned) src.b, ncell_b);
  const long slot = (long) boff[cell / kScanTile] + off[cell] + RANK[gid];
  const float4 f = F[gid];
  R[slot] = make_float4(f.x, f.y, f.z, __int_as_float((int) gid));
  const bool inside = f.w != 0.f;
  float* row = G + gid * CP;
  const int K = P.C;
  if (src.kind == 0) {
    const long i = (long) src.b * Q.M + src.p;
    row[0] = (Q.want_sdf && g_pts_sdf && inside) ? g_pts_sdf[i] : 0.f;
    for (int c = 0; c < K; ++c) row[1 + c] = g_pts_logits ? g_pts_logits[i * K + c] : 0.f;
  } else {
    const long i = (long) src.b * Q.P + src.p;
    row[0] = (g_occ_density && (inside || src.kind == 2)) ? g_occ_density[i] : 0.f;
    for (int c = 0; c < K; ++c)
      row[1 + c] = (g_occ_logits && src.kind == 1) ? g_occ_logits[((long) src.b * K + c) * Q.P + src.p] : 0.f;
  }
  for (int c = K + 1; c < CP; ++c) row[c] = 0.f;
}

// grad_density of one voxel from the two density sums: raw (lidar sdf) + act * d sigma / d s; returns the d beta term
template <typename TD>
__device__ __forceinline__ float finish_density(const DensityParams& dp, bool has_occ, const TD* __restrict__ den,
                                                long idx, float raw, float act, float& out) {
  if (!has_occ) { out = raw; return 0.f; }
  float sigma, dsig_ds, dsig_db;
  density_all(dp, ldf(den, idx), sigma, dsig_ds, dsig_db);
  out = raw + act * dsig_ds;
  return act * dsig_db;
}

template <typename TD, int CP4>
__global__ void __launch_bounds__(256)
point_queries_gather_kernel(QueryParams Q, const TD* __restrict__ den, const float* __restrict__ beta_raw,
                            const int* __restrict__ off, const int* __restrict__ boff,
                            const float4* __restrict__ R, const float* __restrict__ G,
                            float* __restrict__ gsem, float* __restrict__ gden,
                            float* __restrict__ beta_part, int* __restrict__ heavy,
                            int* __restrict__ nheavy, long ncell_b, int runs_x) {
  constexpr int CP = CP4 * 4;
  const SampleParams& P = Q.S;
  __shared__ float outs[CP][PVPB + 1];
  __shared__ float outb[PVPB];
  __shared__ float red[4];
  const int tid = threadIdx.x;
  const int g = tid / PGL, l = tid % PGL;
  const unsigned lin = blockIdx.x;
  const int bx = lin % (unsigned) runs_x;
  const unsigned rest = lin / (unsigned) runs_x;
  const int ix = bx * PVPB + g, iy = rest % (unsigned) P.Y;
  const int zb = rest / (unsigned) P.Y;
  const int iz = zb % P.Z, b = zb / P.Z;
  const bool vox_ok = ix < P.X;
  const CellRanges cr = cell_ranges<PGL>(P.Y, P.X, off, boff, ncell_b, b, min(ix, P.X - 1), iy, iz, l);
  float acc[CP];
  float accb = 0.f;
#pragma unroll
  for (int c = 0; c < CP; ++c) acc[c] = 0.f;
  if (vox_ok && cr.tot > kPtsHeavy) {
    if (l == 0) heavy[atomicAdd(nheavy, 1)] = ((b * P.Z + iz) * P.Y + iy) * P.X + ix;
  } else if (vox_ok) {
    const float fix = (float) ix, fiy = (float) iy, fiz = (float) iz;
    for (int k = l; k < cr.tot; k += PGL)
      record_accumulate<CP4, true>(cr, k, R, G, fix, fiy, fiz, acc, (int) Q.nL, accb);
  }
  accb += lane_partner<4>(accb);
  accb += lane_partner<2>(accb);
  accb += lane_partner<1>(accb);
  if (l == 0) outb[g] = accb;
  {
    int cbase = 0;
    reduce_halving<CP, PGL / 2, PGL, CP>(acc, l, cbase);
    constexpr int NL = reduce_left<CP, PGL / 2>();
    constexpr int DUP = reduce_dups<CP, PGL / 2>();
    if ((l & DUP) == 0) {
#pragma unroll
      for (int c = 0; c < NL; ++c) outs[cbase + c][g] = acc[c];
    }
  }
  __syncthreads();
  const long V = (long) P.Z * P.Y * P.X;
  const long vox0 = ((long) iz * P.Y + iy) * P.X + (long) bx * PVPB;
  const bool has_occ = Q.P > 0;
  const DensityParams dp = has_occ ? load_density(P.density_mode, beta_raw, P.beta_min, P.sdf_bias) : DensityParams();
  float dbeta = 0.f;
  for (int e = tid; e < (P.C + 1) * PVPB; e += 256) {
    const int c = e / PVPB, gx = e % PVPB;
    if (bx * PVPB + gx >= P.X) continue;
    if (c == 0) {
      if (!gden) continue;
      const long idx = (long) b * V + vox0 + gx;
      float o;
      dbeta += finish_density(dp, has_occ, den, idx, outs[0][gx], outb[gx], o);
      gden[idx] = o;
    } else {
      gsem[((long) b * P.C + (c - 1)) * V + vox0 + gx] = outs[c][gx];
    }
  }
  if (beta_part) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) dbeta += __shfl_down(dbeta, o, 64);
    if ((tid & 63) == 0) red[tid >> 6] = dbeta;
    __syncthreads();
    if (tid == 0) beta_part[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
  }
}

template <typename TD, int CP4>
__global__ void __launch_bounds__(256)
point_queries_heavy_kernel(QueryParams Q, const TD* __restrict__ den, const float* __restrict__ beta_raw,
                           const int* __restrict__ off, const int* __restrict__ boff,
                           const float4* __restrict__ R, const float* __restrict__ G,
                           float* __restrict__ gsem, float* __restrict__ gden,
                           float* __restrict__ beta_part, const int* __restrict__ heavy,
                           const int* __restrict__ nheavy, long ncell_b) {
  constexpr int CP = CP4 * 4;
  const SampleParams& P = Q.S;
  __shared__ float part[4][CP];
  __shared__ float partb[4];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const long V = (long) P.Z * P.Y * P.X;
  const bool has_occ = Q.P > 0;
  const DensityParams dp = has_occ ? load_density(P.density_mode, beta_raw, P.beta_min, P.sdf_bias) : DensityParams();
  const int n = *nheavy;
  float dbeta = 0.f;                  // thread 0: this workgroup's heavy voxels
  for (int item = blockIdx.x; item < n; item += gridDim.x) {
    int vid = heavy[item];
    const int ix = vid % P.X; vid /= P.X;
    const int iy = vid % P.Y; vid /= P.Y;
    const int iz = vid % P.Z, b = vid / P.Z;
    const CellRanges cr = cell_ranges<64>(P.Y, P.X, off, boff, ncell_b, b, ix, iy, iz, lane);
    float acc[CP];
    float accb = 0.f;
#pragma unroll
    for (int c = 0; c < CP; ++c) acc[c] = 0.f;
    const float fix = (float) ix, fiy = (float) iy, fiz = (float) iz;
    for (int k = tid; k < cr.tot; k += 256)
      record_accumulate<CP4, true>(cr, k, R, G, fix, fiy, fiz, acc, (int) Q.nL, accb);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) accb += __shfl_down(accb, o, 64);
    if (lane == 0) partb[wv] = accb;
    {
      int cbase = 0;
      reduce_halving<CP, 32, 64, CP>(acc, lane, cbase);
      constexpr int NL = reduce_left<CP, 32>();
      constexpr int DUP = reduce_dups<CP, 32>();
      if ((lane & DUP) == 0) {
#pragma unroll
        for (int c = 0; c < NL; ++c) part[wv][cbase + c] = acc[c];
      }
    }
    __syncthreads();
    if (tid < P.C + 1) {
      const float v = (part[0][tid] + part[1][tid]) + (part[2][tid] + part[3][tid]);
      const long vox = ((long) iz * P.Y + iy) * P.X + ix;
      if (tid == 0) {
        if (gden) {
          const float vb = (partb[0] + partb[1]) + (partb[2] + partb[3]);
          float o;
          dbeta += finish_density(dp, has_occ, den, (long) b * V + vox, v, vb, o);
          gden[(long) b * V + vox] = o;
        }
      } else {
        gsem[((long) b * P.C + (tid - 1)) * V + vox] = v;
      }
    }
    __syncthreads();
  }
  if (beta_part && tid == 0) beta_part[blockIdx.x] = dbeta;
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
static PointWs qry_ws(const VampQueryDesc* d, void* workspace) {
  const size_t nblk = (size_t) ((d->X + PVPB - 1) / PVPB) * d->Y * d->Z * d->B;     // one partial per gather workgroup, + the heavy kernel's
  return point_ws(d->B, d->Z, d->Y, d->X, (size_t) d->B * ((size_t) d->M + 2 * (size_t) d->P_occ), (d->K + 1 + 3) / 4 * 4,
                  nblk + kHeavyGrid, workspace);
}

template <typename TD>
static int backward_t(const VampQueryDesc* d, const QueryParams& Q, const void* density, const float* beta,
                      const float* points, const int* counts, const float* occ_points,
                      const float* g_pts_logits, const float* g_pts_sdf, const float* g_occ_logits,
                      const float* g_occ_density, float* grad_semantic, float* grad_density, float* grad_beta,
                      void* workspace, hipStream_t s) {
  const PointWs w = qry_ws(d, workspace);
  const long ncell = cell_count_padded(d->B, d->Z, d->Y, d->X);
  const long ntile = ncell / kScanTile;
  const long ncell_b = (long) (d->Z + 1) * (d->Y + 1) * (d->X + 1);
  const long src = Q.nL + 2 * Q.nO;
  const size_t voxels = (size_t) d->B * d->Z * d->Y * d->X;
  const int CP = (d->K + 1 + 3) / 4 * 4, CP4 = CP / 4;
  const TD* den = static_cast<const TD*>(density);
  if (int ze = launch_zero(w.cnt, (size_t) (ncell + kScanPad) * sizeof(int), s)) return ze;
  int* nheavy = w.aux + ntile + 1;
  const unsigned pgrid = (unsigned) std::max<long>(1, (src + 255) / 256);
  if (src > 0) {
    point_queries_rank_kernel<<<pgrid, 256, 0, s>>>(Q, points, counts, occ_points, w.cnt, w.key, w.rank, w.F, ncell_b);
    if (int e = check_launch("point_queries_rank_kernel")) return e;
  }
  if (int e = launch_cell_scan(w.cnt, w.off, w.bsum, w.boff, w.aux, ncell, s)) return e;
  if (int ze = launch_zero(nheavy, sizeof(int), s)) return ze;
  if (src > 0) {
    point_queries_fill_kernel<<<pgrid, 256, 0, s>>>(Q, w.key, w.rank, w.F, w.off, w.boff, g_pts_logits, g_pts_sdf,
                                                    g_occ_logits, g_occ_density, w.R, w.G, CP, ncell_b);
    if (int e = check_launch("point_queries_fill_kernel")) return e;
  }
  const int runs_x = (d->X + PVPB - 1) / PVPB;
  const long nblk = (long) runs_x * d->Y * d->Z * d->B;
  VAMP_REQUIRE(nblk < 0x7fffffffL - kHeavyGrid, "too many x-runs");
  const unsigned hgrid = (unsigned) std::min<size_t>(voxels, kHeavyGrid);
  const bool want_beta = Q.P > 0 && grad_density && grad_beta && d->density_mode == VAMP_DENSITY_SDF_LAPLACE;
  float* bp = want_beta ? w.beta_part : nullptr;
#define VAMP_QRY(CP4V)                                                                                 \
  do {                                                                                                 \
    point_queries_gather_kernel<TD, CP4V><<<(unsigned) nblk, 256, 0, s>>>(                             \
        Q, den, beta, w.off, w.boff, w.R, w.G, grad_semantic, grad_density, bp, w.heavy, nheavy,       \
        ncell_b, runs_x);                                                                              \
    point_queries_heavy_kernel<TD, CP4V><<<hgrid, 256, 0, s>>>(                                        \
        Q, den, beta, w.off, w.boff, w.R, w.G, grad_semantic, grad_density, bp ? bp + nblk : nullptr,  \
        w.heavy, nheavy, ncell_b);                                                                     \
  } while (0)
  switch (CP4) {
    case 1: VAMP_QRY(1); break;
    case 2: VAMP_QRY(2); break;
    case 3: VAMP_QRY(3); break;
    case 4: VAMP_QRY(4); break;
    case 5: VAMP_QRY(5); break;
    case 6: VAMP_QRY(6); break;
    case 7: VAMP_QRY(7); break;
    default: VAMP_QRY(8); break;
  }
#undef VAMP_QRY
  if (int e = check_launch("point_queries_gather_kernel")) return e;
  // grad_beta += sign(beta) * (the workgroups' partials, light then heavy, in a fixed order)
  if (want_beta) return launch_beta_reduce(w.beta_part, (int) (nblk + hgrid), beta, grad_beta, s);
  return VAMP_OK;
}

template <typename TS, typename TD>
static int forward_t(const VampQueryDesc* d, const QueryParams& Q, const void* semantic, const void* density,
                     const float* beta, const float* points, const int* counts, const float* occ_points,
                     float* pts_logits, float* pts_sdf, float* occ_logits, float* occ_density, hipStream_t s) {
  const TS* sem = static_cast<const TS*>(semantic);
  const TD* den = static_cast<const TD*>(density);
  if (d->M > 0) {
    dim3 grid((unsigned) ((d->M + 255) / 256), d->B);
    point_queries_lidar_fwd_kernel<TS, TD><<<grid, 256, 0, s>>>(Q, sem, den, points, counts, pts_logits, pts_sdf);
    if (int e = check_launch("point_queries_lidar_fwd_kernel")) return e;
  }
  if (d->P_occ > 0) {
    dim3 grid((unsigned) ((d->P_occ + 255) / 256), d->B);
    point_queries_occ_fwd_kernel<TS, TD><<<grid, 256, 0, s>>>(Q, sem, den, beta, occ_points, occ_logits, occ_density);
    if (int e = check_launch("point_queries_occ_fwd_kernel")) return e;
  }
  return VAMP_OK;
}

}  // namespace vamp

using namespace vamp;

extern "C" {

int vamp_point_queries_supported(const VampQueryDesc* d) { return (d && validate(d) == VAMP_OK) ? 1 : 0; }

size_t vamp_point_queries_workspace_bytes(const VampQueryDesc* d) {
  if (!d || validate(d)) return 0;
  return qry_ws(d, nullptr).bytes;
}

int vamp_point_queries_forward(const VampQueryDesc* d, const void* semantic, const void* density,
                               const float* beta, const float* points, const int32_t* counts,
                               const float* occ_points, float* pts_logits, float* pts_sdf,
                               float* occ_logits, float* occ_density, void* stream) {
  if (int e = validate(d)) return e;
  const bool need_den = (d->M > 0 && d->want_sdf) || d->P_occ > 0;
  VAMP_REQUIRE(semantic && (density || !need_den), "null pointer");
  VAMP_REQUIRE(d->M == 0 || (points && pts_logits && (pts_sdf || !d->want_sdf)), "null pointer");
  VAMP_REQUIRE(d->P_occ == 0 || (occ_points && occ_logits && occ_density), "null pointer");
  VAMP_REQUIRE(beta || d->P_occ == 0 || d->density_mode == VAMP_DENSITY_SIGMOID, "beta is NULL");
  const QueryParams Q = to_params(d);
  hipStream_t s = static_cast<hipStream_t>(stream);
#define VAMP_QRY_FWD(TS, TD)                                                                            \
  return forward_t<TS, TD>(d, Q, semantic, density, beta, points, counts, occ_points, pts_logits, pts_sdf, \
                           occ_logits, occ_density, s)
  if (d->sem_dtype == VAMP_F32) {
    if (d->den_dtype == VAMP_F32) VAMP_QRY_FWD(float, float);
    VAMP_QRY_FWD(float, __hip_bfloat16);
  }
  if (d->den_dtype == VAMP_F32) VAMP_QRY_FWD(__hip_bfloat16, float);
  VAMP_QRY_FWD(__hip_bfloat16, __hip_bfloat16);
#undef VAMP_QRY_FWD
}

int vamp_point_queries_backward(const VampQueryDesc* d, const void* density, const float* beta,
                                const float* points, const int32_t* counts, const float* occ_points,
                                const float* g_pts_logits, const float* g_pts_sdf,
                                const float* g_occ_logits, const float* g_occ_density,
                                float* grad_semantic, float* grad_density, float* grad_beta,
                                void* workspace, size_t workspace_bytes, void* stream) {
  if (int e = validate(d)) return e;
  const bool need_den = (d->M > 0 && d->want_sdf) || d->P_occ > 0;
  VAMP_REQUIRE(grad_semantic && (grad_density || !need_den) && (density || !grad_density || d->P_occ == 0),
               "null pointer");
  VAMP_REQUIRE((d->M == 0 || points) && (d->P_occ == 0 || occ_points), "null pointer");
  VAMP_REQUIRE(beta || d->P_occ == 0 || d->density_mode == VAMP_DENSITY_SIGMOID, "beta is NULL");
  const size_t need = vamp_point_queries_workspace_bytes(d);
  if (int e = workspace_fits(__func__, workspace, workspace_bytes, need)) return e;
  const QueryParams Q = to_params(d);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (d->den_dtype == VAMP_F32)
    return backward_t<float>(d, Q, density, beta, points, counts, occ_points, g_pts_logits, g_pts_sdf, g_occ_logits,
                             g_occ_density, grad_semantic, grad_density, grad_beta, workspace, s);
  return backward_t<__hip_bfloat16>(d, Q, density, beta, points, counts, occ_points, g_pts_logits, g_pts_sdf,
                                    g_occ_logits, g_occ_density, grad_semantic, grad_density, grad_beta, workspace, s);
}

}  // extern "C"
