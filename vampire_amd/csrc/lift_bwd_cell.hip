// LIFT backward as a cell list ("sort, then own").  Autograd of base_vampire2.py:507-514
// (grid_sampler_3d backward + the camera mean):
//
//   count   done by the FORWARD kernel in grad mode (lift.hip, lift_emit_pair; lift_pairs_kernel for a
//           backward whose forward did not): every valid (voxel, camera) pair increments the counter of
//           its cell = (camera, floor tap row + 1, floor tap column + 1), (fH + 1) x (fW + 1) cells per
//           camera, and leaves its taps {wx1, wy1, wz1, iz0} at (image, voxel)
//   scan    exclusive prefix sum of the counters -> cell start offsets (runtime.hip)
//   fill    thread per voxel, NO projection: every pair of the voxel (camera mask + taps + depth samples from the
//           forward) goes to the next slot of its cell (slots handed out by atomics on the cell cursor) as ONE
//           record [taps | depth samples | the voxel's row grad_out / (hits + 1e-6)], 32 + 4 C bytes: everything
//           the gather needs of a pair, contiguous, in the order it will read it
//   gather  one workgroup per STRIP of 16 consecutive pixels of a feature-map row.  The pairs that touch
//           the strip are those of the cell rows iy, iy + 1, columns x0 .. x0 + 16: two contiguous ranges
//           of the cell-ordered records.  The workgroup stages them in LDS (lane = pair for the taps, four lanes
//           per pair for the gradient row: plain streaming reads, every load of a chunk in flight at once and
//           none of them dependent on another, none in a branch), then consumes them dealt by PAIR, whatever
//           pixels the pairs fall on: the depth terms lane = (pair, role) -- the pair's channels dotted with the
//           features of the role's pixel -- into the strip's LDS tile of 64-bit fixed-point sums, the feature
//           gradient as [16 pixels x 4 pairs] x [4 pairs x 16 channels] products of the fp32 matrix cores, blocks of
//           four pairs dealt round-robin to the waves.  No float atomics, no cross-lane folds; depth-gradient planes
//           leave as 64-byte runs.
//
// Round 6 changed what a pair carries (review item 2: "change the tile, not the order").  Through round 5 the fill
// wrote a 41 MB channel-last TABLE of normalised gradient rows, one per voxel, and 20-byte pair records beside it;
// the gather loaded a pair's voxel index, then -- a second, dependent round trip, a random 64-byte line per pair --
// its table row, and interpolated the pair's depth sample from a [D][16] tile of depth columns it had loaded at the
// head of every strip.  Now the forward keeps the four depth samples it computes anyway (16 bytes per pair), the
// fill writes the row INTO the record, and the gather's staging is one round trip of sequential reads: no table,
// no voxel indices, no depth tile (the depth columns are only loaded, late, by the fused softmax backward of the
// logits entry).
//
// (Round 3 ran one WAVE per pixel with lane = pair: 67 584 waves at cfg-B of which half held fewer
// than ten pairs, each paying the column staging, the range loads, a 64-lane fold of 16 channels and
// 16-byte pieces of 86 depth planes -- 5.85 M L2 requests and 92 us for 2.4 M pair visits; every pair
// was read by four pixels.  A strip reads a pair 2.1 times and has 16x fewer, 16x fuller units of work.)
//
// No float atomics on global memory, no memset of the outputs, no layout transposes.
#include "lift_common.hpp"

#include <algorithm>
#include <type_traits>

namespace vamp {

// ---------------------------------------------------------------------------
// fill: thread per voxel, the 64 lanes of a wave are 64 consecutive voxels of one sample's flattened (z, y, x) index
// ---------------------------------------------------------------------------
#ifndef VAMP_FILL_NB
#define VAMP_FILL_NB 3        // cameras per batch: their loads, then their atomics, are in flight together (4: scratch at C = 16)
#endif
#ifdef VAMP_LIFT_STAMPS
// diagnostic build only (tools/debug/fill_stamps.py; -DVAMP_LIFT_STAMPS): per-wave phase stamps of the fill
__device__ long long g_fill_stamps[16384 * 8];
#define FSTAMP(i) fst[i] = __builtin_amdgcn_s_memtime()
#else
#define FSTAMP(i)
#endif

template <int CH>
__global__ void __launch_bounds__(256, 6)
lift_bwd_fill_kernel(LiftParams P, int cw, int ch, const float* __restrict__ gout,
                     const uint64_t* __restrict__ hits, const unsigned* __restrict__ amask,
                     const float4* __restrict__ ptaps, const int* __restrict__ pcell,
                     int* __restrict__ cnt, const int* __restrict__ off, const int* __restrict__ boff,
                     float4* __restrict__ recs, int* __restrict__ rowq, int bn_lo, int bn_hi, int wps) {
  const int tid = threadIdx.x, lane = tid & 63;
  // A duty of the first workgroup, beside its voxels: the order in which the gather takes the image
  // rows -- those with the most pairs first (counting sort by the bit length of a row's pair count), so
  // that its long-running workgroups start early and the light ones fill the tail.
  if (blockIdx.x == 0) {
    __shared__ int cls[34];
    if (tid < 34) cls[tid] = 0;
    __syncthreads();
    const int nrow = (bn_hi - bn_lo) * P.fH;
    auto row_class = [&](int r) {
      const long c0 = ((long) bn_lo * ch + (long) (r / P.fH) * ch + r % P.fH) * cw, c1 = c0 + 2 * cw;
      const int w = (off[c1] + boff[c1 / kScanTile]) - (off[c0] + boff[c0 / kScanTile]);
      return 32 - __clz(max(w, 0));                  // 0 .. 32, heavy rows get high classes
    };
    for (int r = tid; r < nrow; r += 256) atomicAdd(cls + row_class(r), 1);
    __syncthreads();
    if (tid == 0) {
      int run = 0;
      for (int k = 32; k >= 0; --k) { const int n = cls[k]; cls[k] = run; run += n; }
    }
    __syncthreads();
    for (int r = tid; r < nrow; r += 256) rowq[(long) bn_lo * P.fH + atomicAdd(cls + row_class(r), 1)] = bn_lo * P.fH + r;
  }
#ifdef VAMP_LIFT_STAMPS
  long long fst[6];
  FSTAMP(0);
#endif
  // wave w of the launch: sample w / wps, voxels 64 (w % wps) .. + 63 of its V.  A run of lanes that share a cell
  // breaks at a row end at most (once per X voxels); with tiles of 64 x 4 voxels the last wave of a row of X = 200
  // had 8 live lanes of 64 and paid every round trip of a full one.
  const long V = (long) P.Z * P.Y * P.X;
  // (wave and sample are uniform: every plane and image base below is a scalar, the lane adds its 32-bit voxel)
  const int wave = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (tid >> 6));
  const int b = wave / wps;
  const int vox = (wave - b * wps) * 64 + lane;
  const bool live = b < P.B && vox < V;

  // images [bn_lo, bn_hi) of the flattened (sample, camera) index
  const int n_lo = max(0, bn_lo - b * P.N), n_hi = min(P.N, bn_hi - b * P.N);
  const unsigned range = n_hi > n_lo ? (((1u << (n_hi - n_lo)) - 1u) << n_lo) : 0u;
  const unsigned vmask = live ? ((amask + (long) b * V)[vox] & range) : 0u;
  // the cameras present in the wave (9 % of the voxels are seen by no camera: whole waves of them leave here)
  unsigned um = 0;
  for (int n = n_lo; n < n_hi; ++n)
    if (__any((vmask >> n) & 1u)) um |= 1u << n;
  if (um == 0u) return;
  FSTAMP(1);

  const int C = P.C;
  const int nchunk = C / CH;
  const int RS = 2 + C / 4;                          // float4 pieces per record
  // The records of a wave's pairs leave through LDS: a lane's 32 + 4 C bytes are one record, but stored by the lane
  // itself they are RS separate 16-byte pieces 16 RS bytes apart (the first build of this kernel: 62 us).  Staged
  // [lane][piece] and written piece by piece with consecutive lanes on consecutive pieces, a record is one run, and
  // the records of a run of lanes that share a cell -- consecutive slots -- are one longer run.
  extern __shared__ float4 fstage[];                 // [4 waves][64 lanes][RS]
  __shared__ int fslot[4][64];
  float4* my = fstage + (size_t) (tid >> 6) * 64 * RS;
  int* myslot = fslot[tid >> 6];

  // the voxel's row grad_out / (hit count + 1e-6), the camera-mean factor of bv2:512-514 -- the same for every
  // camera of the voxel -- into the lane's LDS row behind the two tap pieces
  float v[CH];
  uint64_t hw = 0;
  auto row_load = [&](int chunk) {
    if (vmask != 0u) {
      hw = (hits + (long) b * V * nchunk)[(long) vox * nchunk + chunk];
#pragma unroll
      for (int k = 0; k < CH; ++k) v[k] = (gout + ((long) b * C + chunk * CH + k) * V)[vox];
    }
  };
  auto row_stage = [&](int chunk) {
    if (vmask != 0u) {
#pragma unroll
      for (int k = 0; k < CH; ++k)
        v[k] *= __builtin_amdgcn_rcpf((float) ((hw >> (4 * k)) & 15) + 1e-6f);   // 1 ulp: gradients are held to 1e-4
#pragma unroll
      for (int c4 = 0; c4 < CH; c4 += 4)
        my[lane * RS + 2 + (chunk * CH + c4) / 4] = make_float4(v[c4], v[c4 + 1], v[c4 + 2], v[c4 + 3]);
    }
  };
  // Three dependent round trips per wave: the mask; everything that needs only the mask -- the row and the taps and
  // cells of the first batch of cameras, in flight together (the row's registers are free again before the atomics);
  // the cursor atomics with the cells' start offsets beside them.
  for (int chunk = 0; chunk < nchunk - 1; ++chunk) { row_load(chunk); row_stage(chunk); }
  row_load(nchunk - 1);

  constexpr int NB = VAMP_FILL_NB;
  auto batch = [&](auto first) {
    int nk[NB], base[NB], start[NB], len[NB], cellk[NB], offk[NB], boffk[NB];
    float4 tapk[NB], depk[NB];
    int pck[NB];
#pragma unroll
    for (int k = 0; k < NB; ++k) {                   // the next NB cameras present (uniform)
      nk[k] = um ? __ffs(um) - 1 : -1;
      um &= um - 1u;
    }
    // No load of the batch sits in a branch of its own (the wait counters are exact only in straight-line code: a
    // wait behind a skipped load waits for everything): a lane without the pair reads what the wave's first lane
    // with it reads.
#pragma unroll
    for (int k = 0; k < NB; ++k) {
      tapk[k] = make_float4(0.f, 0.f, 0.f, 0.f);
      depk[k] = tapk[k];
      pck[k] = 0;
      if (nk[k] < 0) continue;                       // uniform
      const bool act = (vmask >> nk[k]) & 1u;
      const int lv = act ? vox : vox - lane + (__ffsll((long long) __ballot(act)) - 1);
      const long iv = ((long) b * P.N + nk[k]) * V;     // uniform
      tapk[k] = (ptaps + iv * 2)[(long) lv * 2];
      depk[k] = (ptaps + iv * 2)[(long) lv * 2 + 1];
      pck[k] = (pcell + iv)[lv];
    }
    if (decltype(first)::value) row_stage(nchunk - 1);
    if (decltype(first)::value) FSTAMP(2);
#pragma unroll
    for (int k = 0; k < NB; ++k) {                   // cells and runs of the whole batch, then its atomics back to back
      base[k] = 0;
      start[k] = lane;
      len[k] = 0;
      cellk[k] = 0;
      offk[k] = 0;
      boffk[k] = 0;
      if (nk[k] < 0) continue;                       // uniform
      const bool act = (vmask >> nk[k]) & 1u;
      // (launch_lift_cells_begin: fewer than 2^31 cells)
      const int cell = act ? (int) ((((long) b * P.N + nk[k]) * ch + (pck[k] >> 16)) * cw + (pck[k] & 0xffff)) : 0;
      cellk[k] = cell;
      const LaneRun r = lane_run(act, cell, lane);
      if (act) start[k] = r.start;
      if (r.head) len[k] = r.len;
    }
#pragma unroll
    for (int k = 0; k < NB; ++k) {
      if (nk[k] < 0) continue;                       // uniform
#ifndef VAMP_FILL_NOATOMIC         // (measurement build: wrong slots)
      if (len[k] > 0) base[k] = atomicAdd(cnt + cellk[k], len[k]);
#endif
      // (the cell is known before the atomic returns: its start offset is asked for beside it)
      offk[k] = off[cellk[k]];
      boffk[k] = boff[cellk[k] / kScanTile];
    }
    if (decltype(first)::value) FSTAMP(3);
    // every slot of the batch in front of the first store (a wait for an atomic behind stores waits for the stores)
    int slotk[NB];
#pragma unroll
    for (int k = 0; k < NB; ++k) {
      slotk[k] = -1;
      if (nk[k] < 0) continue;                       // uniform
      const bool act = (vmask >> nk[k]) & 1u;
      const int rb = __shfl(base[k], start[k], 64);
      if (act) slotk[k] = offk[k] + boffk[k] + rb + (lane - start[k]);
    }
    if (decltype(first)::value) FSTAMP(4);
#pragma unroll
    for (int k = 0; k < NB; ++k) {
      if (nk[k] < 0) continue;                       // uniform
      const int slot = slotk[k];
      // (a wave writes and reads its own slab: fence + wave barrier, no instruction on gfx9)
      my[lane * RS] = tapk[k];
      my[lane * RS + 1] = depk[k];
      myslot[lane] = slot;
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      for (int i = lane; i < 64 * RS; i += 64) {
        const int r = i / RS, q = i - r * RS;
        const int sl = myslot[r];
#ifdef VAMP_FILL_NOSTORE           // (measurement build: no records)
        if (sl == -12345) recs[(long) sl * RS + q] = my[i];
#else
        if (sl >= 0) recs[(long) sl * RS + q] = my[i];
#endif
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
    }
  };
  batch(std::true_type{});
  while (um) batch(std::false_type{});               // (more than NB cameras in one wave: none at six cameras)
#ifdef VAMP_LIFT_STAMPS
  FSTAMP(5);
  const int npair_lanes = __popcll(__ballot(vmask != 0u));
  if (lane == 0 && wave < 16384) {
    long long* o = g_fill_stamps + (long) wave * 8;
    for (int i = 0; i < 6; ++i) o[i] = fst[i];
    o[6] = npair_lanes;
    o[7] = 1;
  }
#endif
}

// ---------------------------------------------------------------------------
// gather: one workgroup per strip of kS pixels of one feature-map row
// ---------------------------------------------------------------------------
constexpr int kS = 16;               // pixels per strip: depth planes move as 64-byte runs
constexpr int kW = 4;                // waves per workgroup
constexpr int kRow = 24;             // floats per staged pair: 16 channels + {w dep A, w dep B, column << 16 | iz0 + 1, -} + 2 x {w wz0, w wz1}
constexpr int kFix = 44;             // fixed-point depth sums: |term| < 2^41, 2^10 .. 2^20 terms fit

typedef float f32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}
// exponent e with |v| < 2^e (v = 0 -> a very small exponent)
__device__ __forceinline__ int exp_above(float v) {
  int e;
  frexpf(fmaxf(fabsf(v), 1e-30f), &e);
  return e;
}
// round(w * 2^sc) as a 64-bit integer, |result| < 2^51: the integer sits in the mantissa of
// w * 2^sc + 1.5 * 2^52 (five instructions; a float -> int64 cast is a dozen)
__device__ __forceinline__ unsigned long long fixed_of(float w, int sc) {
  const double x = ldexp((double) w, sc) + 6755399441055744.0;
  return (unsigned long long) (__double_as_longlong(x) - 0x4338000000000000LL);
}

#ifdef VAMP_LIFT_STAMPS
// diagnostic build only (tools/debug/lift_stamps.py; -DVAMP_LIFT_STAMPS): per-workgroup phase stamps of the strip gather
__device__ long long g_stamps[16384 * 8];
#define STAMP() __builtin_amdgcn_s_memtime()
#endif

static size_t strip_lds_floats(int D, int cap) {
  // 64-bit gtile + stage (staged pairs | the waves' grad_feat tiles | the softmax backward's depth columns)
  // + cell starts + per-pixel scale exponents + softmax partials (in the consume phase: the feature tile) + chunk maxima
  return (size_t) D * kS * 2 + (size_t) std::max(std::max(cap * kRow, kW * kS * 16), D * kS) + 2 * (kS + 2) + kS + 17 * kS + 8;
}

// The depth gradient of the strip is summed in 64-bit fixed point in LDS (ds_add_u64 is served at
// 11-19 cycles per wave instruction on gfx950, ds_add_f32 at 100-190, and a read-add-write per pair
// costs two LDS round trips in a loop that is nothing but latency): a term w * dot is bounded by
// max|g| * sum_c |feat_c| of its pixel, so with the power-of-two scale 2^(kFix - e_g - e_f[pixel]) every
// term is below 2^41 and keeps >= 20 bits under a typical term; integer adds are associative, so
// the sums have the same bits every run.  e_g follows the largest table row staged so far (+3 bits
// of headroom); when a later chunk exceeds it the tile is shifted down once.
template <typename T, bool VEC>
__global__ void __launch_bounds__(kW * 64, 4)
lift_bwd_strip_kernel(LiftParams P, int cw, int ch, int spr, int xgroup, int bn_lo, int cap,
                      const T* __restrict__ depth, const T* __restrict__ feat,
                      const int* __restrict__ off, const int* __restrict__ boff,
                      const float4* __restrict__ recs, const int* __restrict__ rowq, int* __restrict__ cnt,
                      float* __restrict__ gdepth, float* __restrict__ gfeat, int softmax_bwd, int fcl) {
  extern __shared__ float smem[];
  constexpr int NT = kW * 64;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int C = P.C, D = P.use_depth ? P.D : 0;
  const int DS = D * kS;
  long long* gtile = reinterpret_cast<long long*>(smem);            // [D][kS] the depth columns' gradients, fixed point
  float* stage = smem + 2 * DS;                                     // [cap][kRow] staged pairs
  float* dtile = stage;                                             // [D][kS] the depth columns (softmax backward only, at the end)
  int* offs = reinterpret_cast<int*>(stage + max(max(cap * kRow, kW * kS * 16), DS));   // [2][kS + 2] cell starts
  int* efp = offs + 2 * (kS + 2);                                   // [kS] exponent of sum_c |feat_c|
  float* red = reinterpret_cast<float*>(efp + kS);                  // [16 + 1][kS]
  float* cmax = red + 17 * kS;                                      // [kW] chunk maxima

  // the strips of one image row run on one XCD: vertical and horizontal neighbours share cells
  const unsigned lin = xcd_grouped(blockIdx.x, gridDim.x, xgroup);
  const int sx = lin % spr;
  const int row = rowq[(long) bn_lo * P.fH + lin / spr];            // heavy rows first (fill kernel)
  const int iy = row % P.fH;
  const long bn = row / P.fH;
  const int b = (int) (bn / P.N);
  const int x0 = sx * kS;
  const int np = min(kS, P.fW - x0);                 // pixels of a ragged last strip
  const long HW = (long) P.fH * P.fW;
  const long V = (long) P.Z * P.Y * P.X;
  const long pix0 = (long) iy * P.fW + x0;
  float* ftile = red;                                               // [kS][16] the strip's features of a channel chunk (consume phase)

#ifdef VAMP_LIFT_STAMPS
  long long st0 = STAMP(), st_stage = 0, st_cons = 0, st2 = 0;
  const long long rt0 = wall_clock64();
#endif
  // start offsets of the cells (row iy + h, column x0 + j), j = 0 .. kS + 1.  A pair of cell (row,
  // column) has iy0 = row - 1, ix0 = column - 1; the cells are linear in (row, column), so the end of a
  // row is the start of the next.
  if (tid < 2 * (kS + 2)) {
    const int h = tid / (kS + 2), j = tid % (kS + 2);
    const long c = (bn * ch + iy + h) * cw + min(x0 + j, cw);
    offs[tid] = off[c] + boff[c / kScanTile];
    // the fill's cursors (= the counters the next forward counts into) go back to zero: this strip owns
    // the cells of its row and columns, the last strip of a row also column fW, the last row also row fH
    if ((h == 0 || iy == P.fH - 1) && (j < np || (j == np && x0 + np == P.fW))) cnt[c] = 0;
  }
  for (int e = tid; e < DS / 2; e += NT) reinterpret_cast<float4*>(gtile)[e] = make_float4(0.f, 0.f, 0.f, 0.f);
  // one feature of the strip: channel-first planes [C][HW], or (fcl: VAMP_LIFTBWD_FEAT_CHANNEL_LAST, uniform) the
  // caller's channel-last rows [HW][C] -- a strip's 16 channels x kS pixels are then one contiguous run
  auto feat_at = [&](int c, int pp) -> float {
    return fcl ? ldf(feat, (bn * HW + pix0 + pp) * C + c) : ldf(feat, (bn * C + c) * HW + pix0 + pp);
  };
  {
    // sum_c |feat_c| of every pixel over ALL channels: the bound of the depth terms
    const int pp = tid % kS;
    float sa = 0.f;
    for (int c = tid / kS; c < C; c += NT / kS) sa += fabsf(pp < np ? feat_at(c, pp) : 0.f);
    red[tid] = sa;
  }
  __syncthreads();
  if (tid < kS) {
    float t = 0.f;
    for (int k = 0; k < NT / kS; ++k) t += red[k * kS + tid];
    efp[tid] = exp_above(t);
  }
  __syncthreads();
#ifdef VAMP_LIFT_STAMPS
  long long st1 = STAMP();
#endif

  const int n0 = offs[np + 1] - offs[0];             // pairs of cell row iy
  const int NP = n0 + offs[kS + 2 + np + 1] - offs[kS + 2];   // pairs of both cell rows
  int eg = -1000;                                    // uniform: current exponent of the table rows

  for (int c0 = 0; c0 < C; c0 += 16) {               // channel chunk
    const int nq = min(4, (C - c0) / 4);             // float4 pieces of this chunk
    // the strip's 16 x 16 features of this chunk, in the reduction buffer (idle until the softmax epilogue) as
    // [pixel][channel] with the 16-byte piece index xor-ed by pixel / 4: the depth lanes below read the rows of
    // arbitrary pixels, and the same piece of all 16 rows then sits in 16 different bank quads.  (No barrier here:
    // the buffer's last readers are two barriers back, the next ones behind the two barriers of the first chunk.)
    {
      // (consecutive threads = consecutive pixels of a channel plane, or consecutive channels of a channel-last row)
      const int cc = fcl ? tid % 16 : tid / kS, pp = fcl ? tid / 16 : tid % kS;
      ftile[pp * 16 + ((((cc >> 2) ^ (pp >> 2)) & 3) << 2) + (cc & 3)] = (c0 + cc < C && pp < np) ? feat_at(c0 + cc, pp) : 0.f;
    }
    // grad_feat of the chunk: four 16 x 16 accumulator tiles of the matrix cores per wave (column = channel = lane & 15,
    // row = pixel = 4 (lane >> 4) + register): sixteen partial sums per element over the workgroup, as many as the
    // lane-per-(pixel, slot) loop before it kept, so the fp32 sums are as short
    f32x4 acc[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) acc[k] = f32x4{0.f, 0.f, 0.f, 0.f};
    // The loads of the stage phase run one chunk ahead, and none depends on another: a pair's record sits at its
    // POSITION in the cell-ordered list (round 6: the gradient row travels in the record; through round 5 a pair's
    // voxel index had to arrive before its table row could be asked for).
    // stage phase A: lanes 0..31 of a wave = pair 32 wv + lane of the chunk (taps and depth samples; the lane works
    // out the pair's terms for its two pixels); phase B: four lanes per pair, each one 16-byte piece of the row
    const int jA = 32 * wv + lane;
    const bool laneA = lane < 32 && jA < cap;
    const int RS = 2 + C / 4;                        // float4 pieces per record
    // (No load sits in a branch: a lane without a pair of its own reads the strip's last record, and what it read is
    // dropped when the chunk is staged.  Behind a skipped load the wait counters cannot be exact, and a wait for this
    // chunk's registers would also wait for everything asked for since.)
    const int o0 = offs[0], o1 = offs[kS + 2];
    auto rec_at = [&](int t) -> long {
      const int tt = min(t, NP - 1);
      return (long) (tt >= n0 ? o1 + (tt - n0) : o0 + tt) * RS;
    };
    auto load_taps = [&](int tc, float4& rc, float4& dp) {
      const long pos = rec_at(tc + 32 * wv + (lane & 31));
      rc = recs[pos];
      dp = recs[pos + 1];
    };
    auto load_rows = [&](int tc, float4 (&g)[2]) {
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2)                   // the voxel's row of grad_out / (hits + 1e-6), this chunk of channels
        g[s2] = recs[rec_at(tc + 32 * wv + 16 * s2 + (lane >> 2)) + 2 + c0 / 4 + min(lane & 3, nq - 1)];
    };
    // one chunk: staged from the registers it was loaded into, which then take the next chunk
    auto chunk = [&](int t0, float4& rcA, float4& dpA, float4 (&gA)[2]) {
      const int nst = min(cap, NP - t0);
      __syncthreads();                               // the previous chunk (or the last channel chunk's tile sum) is consumed
#ifdef VAMP_LIFT_STAMPS
      long long sa = STAMP();
#endif
      // ---- stage chunk [t0, t0 + nst) from the registers
      float gm = 0.f;
      if (laneA && jA < nst) {
        const int h = t0 + jA >= n0;
        const float4 rc = rcA;
        // the pair's taps: fractional coordinates (w1 of each axis), the lower depth plane and the
        // cell column; the weights of the lower taps are taken as 1 - w1 (the forward's
        // (floor + 1) - f up to an ulp: gradients are held to 1e-4)
        const int pk = __float_as_int(rc.w);
        const int iz0 = (pk & 0xffff) - 1, col = pk >> 16;
        const float wz1v = rc.z, wz0v = 1.0f - rc.z;
        const float wy = h ? 1.0f - rc.y : rc.y;
        const bool z0in = iz0 >= 0 && iz0 < D, z1in = iz0 + 1 >= 0 && iz0 + 1 < D;
        // the forward's depth samples at the pair's four pixel taps, [y tap][x tap]: this strip's row is the pair's
        // y1 tap when the pair comes from cell row iy (h = 0), its y0 tap from cell row iy + 1
        const float dpy[2] = {h ? dpA.x : dpA.z, h ? dpA.y : dpA.w};     // [x tap] of this row
        float* st = stage + jA * kRow;
        // the pair's cell column in the strip, 0 .. np, travels with both roles beside iz0 + 1 (an integer in a float's
        // bits: never an operand of arithmetic): the consume phase no longer knows a pair's pixels from its position
        const float tag = __int_as_float(((col - x0) << 16) | (pk & 0xffff));
        float wd[2], w0[2], w1[2];
#pragma unroll
        for (int role = 0; role < 2; ++role) {       // role A: the pixel is the x1 tap, role B: the x0 tap
          const int pr = col - role - x0;
          const bool pin = pr >= 0 && pr < np;
          const float wj = wy * (role ? 1.0f - rc.x : rc.x);
          const float dep = dpy[1 - role];
          wd[role] = pin ? wj * dep : 0.f;
          w0[role] = (pin && z0in) ? wj * wz0v : 0.f;
          w1[role] = (pin && z1in) ? wj * wz1v : 0.f;
        }
        // {w dep A, w dep B, tag, -} is what the grad_feat lanes read, {w wz0, w wz1} of a role what its depth lane reads
        reinterpret_cast<float4*>(st)[4] = make_float4(wd[0], wd[1], tag, 0.f);
        reinterpret_cast<float4*>(st)[5] = make_float4(w0[0], w1[0], w0[1], w1[1]);
      }
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2) {
        const int j = 32 * wv + 16 * s2 + (lane >> 2);
        const float4 g4 = (j < nst && (lane & 3) < nq) ? gA[s2] : make_float4(0.f, 0.f, 0.f, 0.f);
        gm = fmaxf(gm, fmaxf(fmaxf(fabsf(g4.x), fabsf(g4.y)), fmaxf(fabsf(g4.z), fabsf(g4.w))));
        if (j < nst) reinterpret_cast<float4*>(stage + j * kRow)[lane & 3] = g4;
      }
      // ---- the next chunk's loads
      load_taps(t0 + cap, rcA, dpA);
      load_rows(t0 + cap, gA);
      gm = wave_max(gm);
      if (lane == 0) cmax[wv] = gm;
      __syncthreads();
      if (D > 0) {
        const int ec = exp_above(fmaxf(fmaxf(cmax[0], cmax[1]), fmaxf(cmax[2], cmax[3])));
        if (ec > eg) {                               // uniform; the first chunk, rarely a later one
          const int en = ec + 3;
          if (eg > -1000) {
            const int sh = min(en - eg, 63);
            for (int e = tid; e < DS; e += NT) gtile[e] >>= sh;
            __syncthreads();
          }
          eg = en;
        }
      }
#ifdef VAMP_LIFT_STAMPS
      long long sb = STAMP(); st_stage += sb - sa;
#endif
      // ---- consume.  The work of a chunk is dealt by pair, not by pixel: its cost does not depend on how the pairs
      // spread over the strip's pixels (the records are in cell order: a dense chunk is the pairs of one or two cells,
      // two or four pixels).
      // Depth terms: lane = (pair, role).  The pair's channels dotted with the features of the role's pixel, a chain of
      // sixteen fmaf in channel order from zero, then the two fixed-point adds.
      if (D > 0) {
        for (int j = tid >> 1; j < nst; j += NT / 2) {
          const float4* sr = reinterpret_cast<const float4*>(stage + j * kRow);
          const float2 wz = *reinterpret_cast<const float2*>(stage + j * kRow + 20 + 2 * (tid & 1));
          const int tag = __float_as_int(stage[j * kRow + 18]);
          const int pr = min(max((tag >> 16) - (tid & 1), 0), kS - 1);   // (outside the strip: both weights are zero)
          const float4* fr = reinterpret_cast<const float4*>(ftile + pr * 16);
          float dot = 0.f;
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            const float4 g = sr[k], f = fr[(k ^ (pr >> 2)) & 3];
            dot = __builtin_fmaf(f.x, g.x, dot);
            dot = __builtin_fmaf(f.y, g.y, dot);
            dot = __builtin_fmaf(f.z, g.z, dot);
            dot = __builtin_fmaf(f.w, g.w, dot);
          }
          const float w0 = wz.x * dot, w1 = wz.y * dot;
          const int sce = kFix - eg - efp[pr];
          unsigned long long* gp = reinterpret_cast<unsigned long long*>(gtile + ((tag & 0xffff) - 1) * kS + pr);
          if (w0 != 0.f) atomicAdd(gp, fixed_of(w0, sce));
          if (w1 != 0.f) atomicAdd(gp + kS, fixed_of(w1, sce));
        }
      }
      // grad_feat[pixel][channel] += W[pixel][pair] G[pair][channel] on the fp32 matrix cores (v_mfma_f32_16x16x4_f32:
      // per element a chain of fmaf over the four pairs in order), a block of four pairs per instruction, the blocks
      // dealt round-robin to the waves and to each wave's four accumulators.  A: lane = (pixel = lane & 15, pair =
      // lane >> 4), the pair's w dep of the role whose pixel this is, or zero; B: lane = (pair, channel = lane & 15).
      // Behind the chunk's end BOTH are selected zero: what lies there is stale, 0 x NaN is NaN.
      // Four blocks a turn, one per accumulator: their operands are asked for together.
      auto operands = [&](int bi, float& a, float& b) {
        const int j = 4 * bi + (lane >> 4);
        const float* sr = stage + min(j, cap - 1) * kRow;
        const float2 wd = *reinterpret_cast<const float2*>(sr + 16);
        const int dx = (__float_as_int(sr[18]) >> 16) - (lane & 15);  // 0: the pixel is the pair's x1 tap, 1: its x0 tap
        const float g = sr[lane & 15];
        const bool in = j < nst;
        a = in ? (dx == 0 ? wd.x : (dx == 1 ? wd.y : 0.f)) : 0.f;
        b = in ? g : 0.f;
      };
      for (int bi = wv; 4 * bi < nst; bi += 4 * kW) {      // (uniform)
        float a[4], b[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) operands(bi + k * kW, a[k], b[k]);
#pragma unroll
        for (int k = 0; k < 4; ++k) acc[k] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[k], b[k], acc[k], 0, 0, 0);
      }
#ifdef VAMP_LIFT_STAMPS
      __syncthreads();
      st_cons += STAMP() - sb;
#endif
    };
    if (NP > 0) {                                    // (uniform)
      float4 rcA, dpA, gA[2];
      load_taps(0, rcA, dpA);
      load_rows(0, gA);
      for (int t0 = 0; t0 < NP; t0 += cap) chunk(t0, rcA, dpA, gA);
    }
    // grad_feat: the wave's four tiles added, the four waves through LDS
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 4; ++r) stage[(wv * kS + 4 * (lane >> 4) + r) * 16 + (lane & 15)] = (acc[0][r] + acc[1][r]) + (acc[2][r] + acc[3][r]);
    __syncthreads();
#ifdef VAMP_LIFT_STAMPS
    st2 = STAMP();
#endif
    {
      // consecutive threads = consecutive pixels of one channel (or, channel-last, consecutive channels of a pixel)
      const int cc = fcl ? tid % 16 : tid / kS, pp = fcl ? tid / 16 : tid % kS;
      float v = 0.f;
#pragma unroll
      for (int w2 = 0; w2 < kW; ++w2) v += stage[(w2 * kS + pp) * 16 + cc];
      if (pp < np && c0 + cc < C) gfeat[fcl ? (bn * HW + pix0 + pp) * C + c0 + cc : (bn * C + c0 + cc) * HW + pix0 + pp] = v;
    }
  }
  if (D > 0 && gdepth) {
    __syncthreads();
    // fixed point -> float, in place (the floats of a pass land below everything still unread)
    float* gf = reinterpret_cast<float*>(gtile);
    for (int e0 = 0; e0 < DS; e0 += 6 * NT) {
      float v[6];
#pragma unroll
      for (int k = 0; k < 6; ++k) {
        const int e = e0 + k * NT + tid;
        v[k] = e < DS ? (float) ldexp((double) gtile[e], -(kFix - eg - efp[e % kS])) : 0.f;
      }
      __syncthreads();
#pragma unroll
      for (int k = 0; k < 6; ++k) {
        const int e = e0 + k * NT + tid;
        if (e < DS) gf[e] = v[k];
      }
      __syncthreads();
    }
    if (softmax_bwd) {
      // VAMP_LIFTBWD_LOGITS: the depth column is softmax(logits) (base_vampire2.py:550) and the caller
      // wants the gradient of the logits, p * (g - sum_d p g): the gradient tile sits in LDS and the strip's
      // depth columns join it here (the stage region is free by now), so the softmax backward costs one
      // small reduction per strip and no pass of its own over HBM
      // the depth columns: 16-byte pieces of the planes' 64-byte runs (fW % 4 == 0), else single values
      if (VEC) {
        for (int e0 = 0; e0 < DS / 4; e0 += 2 * NT) {
          float4 v[2];
    #pragma unroll
          for (int k = 0; k < 2; ++k) {
            const int e = min(e0 + k * NT + tid, DS / 4 - 1);
            const int dz = e / (kS / 4), p4 = min((e % (kS / 4)) * 4, np - 4);
            v[k] = *reinterpret_cast<const float4*>(reinterpret_cast<const float*>(depth) + (bn * P.D + dz) * HW + pix0 + p4);
          }
    #pragma unroll
          for (int k = 0; k < 2; ++k) {
            const int e = e0 + k * NT + tid;
            if (e < DS / 4) reinterpret_cast<float4*>(dtile)[e] = v[k];
          }
        }
      } else {
        for (int e0 = 0; e0 < DS; e0 += 6 * NT) {
          float v[6];
    #pragma unroll
          for (int k = 0; k < 6; ++k) {
            const int ec = min(e0 + k * NT + tid, DS - 1);
            v[k] = ldf(depth, (bn * P.D + ec / kS) * HW + pix0 + min(ec % kS, np - 1));
          }
    #pragma unroll
          for (int k = 0; k < 6; ++k) {
            const int e = e0 + k * NT + tid;
            if (e < DS) dtile[e] = v[k];
          }
        }
      }
      __syncthreads();
      const int pp = tid % kS, gq = tid / kS;        // 16 partial sums per pixel
      float s = 0.f;
      for (int dz = gq; dz < D; dz += NT / kS) s = __builtin_fmaf(dtile[dz * kS + pp], gf[dz * kS + pp], s);
      red[gq * kS + pp] = s;
      __syncthreads();
      if (tid < kS) {
        float t = 0.f;
        for (int k = 0; k < NT / kS; ++k) t += red[k * kS + tid];
        red[16 * kS + tid] = t;
      }
      __syncthreads();
    }
    if (VEC) {
      for (int e = tid; e < DS / 4; e += NT) {
        const int dz = e / (kS / 4), p4 = (e % (kS / 4)) * 4;
        if (p4 >= np) continue;
        float4 v = reinterpret_cast<const float4*>(gf)[e];
        if (softmax_bwd) {
          const float4 d = reinterpret_cast<const float4*>(dtile)[e];
          const float4 sd = *reinterpret_cast<const float4*>(red + 16 * kS + p4);
          v = make_float4(d.x * (v.x - sd.x), d.y * (v.y - sd.y), d.z * (v.z - sd.z), d.w * (v.w - sd.w));
        }
        *reinterpret_cast<float4*>(gdepth + (bn * P.D + dz) * HW + pix0 + p4) = v;
      }
    } else {
      // consecutive threads = consecutive pixels of one depth plane
      for (int e = tid; e < DS; e += NT) {
        const int dz = e / kS, pp = e % kS;
        if (pp >= np) continue;
        float v = gf[e];
        if (softmax_bwd) v = dtile[e] * (v - red[16 * kS + pp]);
        gdepth[(bn * P.D + dz) * HW + pix0 + pp] = v;
      }
    }
  }
#ifdef VAMP_LIFT_STAMPS
  __syncthreads();
  if (tid == 0 && blockIdx.x < 16384) {
    long long* o = g_stamps + (long) blockIdx.x * 8;
    o[0] = st0; o[1] = st1; o[2] = st_stage; o[3] = st_cons; o[4] = st2; o[5] = STAMP(); o[6] = rt0; o[7] = wall_clock64();
  }
#endif
}

#ifdef VAMP_LIFT_STAMPS
}  // namespace vamp
extern "C" int vamp_debug_read_stamps(long long* host, int n) {
  return (int) hipMemcpyFromSymbol(host, HIP_SYMBOL(vamp::g_stamps), (size_t) n * 8 * sizeof(long long));
}
extern "C" int vamp_debug_read_fill_stamps(long long* host, int n) {
  return (int) hipMemcpyFromSymbol(host, HIP_SYMBOL(vamp::g_fill_stamps), (size_t) n * 8 * sizeof(long long));
}
namespace vamp {
#endif

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
int lift_cells_fit(const char* who, const VampLiftDesc* d) {
  const size_t cap = (size_t) d->B * d->N * d->Z * d->Y * d->X;
  VAMP_REQUIRE_AS(who, cap < 0x7fffffffu && lift_workspace(d, nullptr).ncell < 0x7fffffffL, "pair / cell count exceeds 2^31");
  VAMP_REQUIRE_AS(who, d->C % 4 == 0, "C must be a multiple of 4");
  VAMP_REQUIRE_AS(who, d->fW < 32767 && d->fH < 32767 && d->D < 65535, "feature map too large for the packed cell coordinates");
  return VAMP_OK;
}

// zero the counters in front of a kernel that emits pairs / scan them behind it
int launch_lift_cells_begin(const LiftWorkspace& w, bool clean, hipStream_t s) {
  if (clean)                        // (VAMP_LIFTFWD_CELLS_CLEAN: the caller vouches for zeroed counters)
    return debug_expect_range(w.cnt, (size_t) (w.ncell + kScanPad), 0, 0, s, "VAMP_LIFTFWD_CELLS_CLEAN: the lift workspace's cell counters are zero");
  return launch_zero(w.cnt, (size_t) (w.ncell + kScanPad) * sizeof(int), s);
}

int launch_lift_cells_end(const LiftWorkspace& w, hipStream_t s) {
  return launch_cell_scan(w.cnt, w.off, w.bsum, w.boff, w.aux, w.ncell, s);
}
int lift_cells_scan_job(const LiftWorkspace& w, ScanJob* job) {
  return make_scan_job(w.cnt, w.off, w.bsum, w.boff, w.aux, w.ncell, job);
}

// The backward's plan: every choice vamp_lift_backward_ex makes, from the descriptor, the flags and the workspace size.
// No HIP call.
int lift_backward_plan(const char* who, const VampLiftDesc* d, int flags, size_t workspace_bytes, VampLiftBackwardPlan* out) {
  if (!out) return fail(VAMP_EINVAL, "%s: requirement failed: plan is NULL", who);
  memset(out, 0, sizeof(*out));
  if (int e = lift_validate(d)) return e;
  VampLiftBackwardPlan& p = *out;
  VAMP_REQUIRE_AS(who, lift_channels_ok(d->C), "C must be 4, 8 or a multiple of 16 (<= 64)");
  // VAMP_LIFTBWD_FEAT_CHANNEL_LAST: feat is read, and grad_feat written, as [B, N, fH, fW, C] fp32
  p.feat_cl = (flags & VAMP_LIFTBWD_FEAT_CHANNEL_LAST) != 0;
  VAMP_REQUIRE_AS(who, !p.feat_cl || d->in_dtype == VAMP_F32, "VAMP_LIFTBWD_FEAT_CHANNEL_LAST takes fp32 features (and depth)");
  const LiftWorkspace w = lift_workspace(d, nullptr);
  p.bytes_needed = (int64_t) w.bytes;
  const long BN = (long) d->B * d->N, HW = (long) d->fH * d->fW;
  const int ch = d->C == 4 ? 4 : (d->C == 8 ? 8 : 16);
  if (flags & VAMP_LIFTBWD_SPLAT) {
    VAMP_REQUIRE_AS(who, !(flags & VAMP_LIFTBWD_LOGITS), "VAMP_LIFTBWD_LOGITS is a feature of the default (cell-list) backward");
    p.path = VAMP_LIFTPLAN_BWD_SPLAT;
    p.to_cl = p.to_cf = !p.feat_cl;
    p.zero_feat_bytes = BN * HW * d->C * (int64_t) sizeof(float);
    p.zero_depth_bytes = d->use_depth ? BN * d->D * HW * (int64_t) sizeof(float) : 0;
    p.splat_ch = ch;
    p.splat_grid[0] = (d->X + VAMP_LIFT_TX - 1) / VAMP_LIFT_TX;
    p.splat_grid[1] = (d->Y + VAMP_LIFT_TY - 1) / VAMP_LIFT_TY;
    p.splat_grid[2] = d->Z * d->B;
    return workspace_fits(who, workspace_bytes, w.bytes);
  }
  p.path = VAMP_LIFTPLAN_BWD_CELL;
  p.prepare = !(flags & VAMP_LIFTBWD_CELLS_VALID);
  if (p.prepare)
    if (int e = lift_cells_fit(who, d)) return e;
  // fill: a wave per 64 voxels of a sample's flattened (z, y, x) index, four waves per workgroup
  const long wps = ((long) d->Z * d->Y * d->X + 63) / 64;
  VAMP_REQUIRE_AS(who, wps * 64 < 0x7fffffffL && wps * d->B < 0x7fffffffL, "voxel count exceeds 2^31");
  p.fill_ch = ch;
  p.fill_grid = (int32_t) ((wps * d->B + 3) / 4);
  p.fill_lds = (int64_t) 4 * 64 * (2 + d->C / 4) * sizeof(float4);      // [wave][lane][record piece]
  // gather variants (same kernel, smaller record chunks: the tests run them to cross the chunk boundaries at every
  // size): pairs staged per chunk, 128 by default
  p.cap = (flags & VAMP_LIFTBWD_WPP1) ? 128 : ((flags & VAMP_LIFTBWD_WPP4) ? 64 : ((flags & VAMP_LIFTBWD_WPP16) ? 32 : 128));
  p.strip_lds = (int64_t) (strip_lds_floats(d->use_depth ? d->D : 0, p.cap) * sizeof(float));
  if (p.strip_lds > 150 * 1024) return fail(VAMP_EINVAL, "%s: D too large for the LDS depth tiles", who);
  p.raise_lds = p.strip_lds > 64 * 1024;
  // 16-byte tile I/O needs fp32 depth planes whose strips start on 16-byte boundaries
  p.vec = d->in_dtype == VAMP_F32 && d->fW % 4 == 0;
  p.strip_grid = (int32_t) ((unsigned) BN * d->fH * ((d->fW + kS - 1) / kS));
  p.softmax_bwd = (flags & VAMP_LIFTBWD_LOGITS) != 0;
  return workspace_fits(who, workspace_bytes, w.bytes);
}

// the fill, as the plan says (the counters are the fill cursors: the scan left them at zero)
static int launch_lift_fill(const VampLiftDesc* d, const LiftParams& P, const VampLiftBackwardPlan& p, const LiftWorkspace& w,
                            const float* gout, const uint64_t* hits, hipStream_t s) {
  const int BN = d->B * d->N;
  const int wps = (int) (((long) d->Z * d->Y * d->X + 63) / 64);
#define VAMP_CELL(CH)                                                                                        \
  VAMP_TIMED(kProfLiftBwdFill, s, (lift_bwd_fill_kernel<CH><<<(unsigned) p.fill_grid, 256, (size_t) p.fill_lds, s>>>(   \
      P, w.cw, w.ch, gout, hits, w.amask, w.ptaps, w.pcell, w.cnt, w.off, w.boff, w.recs, w.rowq, 0, BN, wps)))
  if (p.fill_ch == 4) VAMP_CELL(4); else if (p.fill_ch == 8) VAMP_CELL(8); else VAMP_CELL(16);
#undef VAMP_CELL
  return check_launch("lift_bwd_fill_kernel");
}

template <typename T>
static int launch_cell_t(const VampLiftDesc* d, const LiftParams& P, const VampLiftBackwardPlan& p, const LiftWorkspace& w,
                         const float* mats, const float* xs, const float* ys, const float* zs, const void* depth,
                         const void* feat, const float* gout, const uint64_t* hits, float* gdepth, float* gfeat,
                         hipStream_t s) {
  // (the one step that can fail without being a launch: in front of the first launch)
  auto strip = p.vec ? lift_bwd_strip_kernel<T, true> : lift_bwd_strip_kernel<T, false>;
  if (p.raise_lds &&
      hipFuncSetAttribute(reinterpret_cast<const void*>(strip), hipFuncAttributeMaxDynamicSharedMemorySize,
                          (int) p.strip_lds) != hipSuccess)
    return fail(VAMP_EHIP, "%s: cannot raise dynamic LDS", __func__);
  if (p.prepare)
    if (int e = launch_lift_cell_prepare(d, P, w, mats, xs, ys, zs, depth, s)) return e;
  if (int e = launch_lift_fill(d, P, p, w, gout, hits, s)) return e;
  const int spr = (d->fW + kS - 1) / kS;
  VAMP_TIMED(kProfLiftBwd, s, (strip<<<(unsigned) p.strip_grid, kW * 64, (size_t) p.strip_lds, s>>>(
      P, w.cw, w.ch, spr, spr, 0, p.cap, static_cast<const T*>(depth), static_cast<const T*>(feat),
      w.off, w.boff, w.recs, w.rowq, w.cnt, gdepth, gfeat, p.softmax_bwd, p.feat_cl)));
  return check_launch("lift_bwd_strip_kernel");
}

int launch_lift_bwd_cell(const VampLiftDesc* d, const LiftParams& P, const VampLiftBackwardPlan& p, const LiftWorkspace& w,
                         const float* mats, const float* xs, const float* ys, const float* zs, const void* depth,
                         const void* feat, const float* gout, const uint64_t* hits, float* gdepth, float* gfeat,
                         hipStream_t s) {
  if (d->in_dtype == VAMP_F32)
    return launch_cell_t<float>(d, P, p, w, mats, xs, ys, zs, depth, feat, gout, hits, gdepth, gfeat, s);
  return launch_cell_t<__hip_bfloat16>(d, P, p, w, mats, xs, ys, zs, depth, feat, gout, hits, gdepth, gfeat, s);
}

}  // namespace vamp
