// Detection scoring on the device, the per-batch half: the matching of the nuScenes detection protocol
// `detection_cvpr_2019` -- what the reference hands to the devkit's NuScenesEval behind det_evaluators.py:61-117 --
// for every sample and class of a batch in one launch that never synchronises with the host.
//
// det_eval_kernel, one 256-lane workgroup per (sample, class):
//  (a) the class's ground truth inside the class range is compacted, in row order, into LDS (centre and row; at most
//      VAMP_DET_EVAL_GT_CAP boxes), counted into npos[class];
//  (b) the class's predictions inside the range are compacted, in row order, into LDS (the score, an integer key that
//      orders like it, centre, row); every other row the workgroup owns -- rows of its class outside the range and, for
//      class 0, rows at or beyond counts[b] and rows whose label is no class -- is written as an invalid record;
//  (c) a counting rank in LDS orders the predictions by (score descending, row descending);
//  (d) wave 0 walks them in that order.  Lane l holds the ground-truth boxes 4 l .. 4 l + 3 in registers together with
//      their taken bits, one set per distance threshold; per prediction and threshold a masked minimum over the lanes
//      that hold boxes of the float64 squared distance (compared as its bit pattern, which orders like the value for
//      x >= 0; the four thresholds' reductions run in lockstep) and a ballot give the nearest untaken box, lowest row first; the squared distance is compared with the squared threshold.  Lane 0
//      computes the five errors of the match at the true-positive threshold in float64 and stores the 32-byte record.
// Every record slot of the batch has exactly one writer; npos and the error counters are integer atomic adds.  The
// record bytes are a pure function of the inputs, whatever order the workgroups run in.
#include <cmath>

#include "common.hpp"
#include "wave_reduce.hpp"

namespace vamp {
namespace {

constexpr int kEvBlock = 256;
constexpr int kEvWaves = kEvBlock / 64;
constexpr int kEvGtCap = VAMP_DET_EVAL_GT_CAP;
constexpr int kEvGtPerLane = kEvGtCap / 64;
constexpr int kEvMaxM = VAMP_DET_EVAL_MAX_WIDTH;
constexpr int kEvMaxCls = VAMP_DET_EVAL_MAX_CLASSES;
constexpr int kEvMaxB = 4096;
constexpr int kEvMaxG = 1 << 20;
constexpr double kEvPi = 3.141592653589793;
constexpr double kEvSpeed = 0.2;                   // det_evaluators.py:254-255
constexpr unsigned long long kEvNone = ~0ull;
static_assert(kEvGtCap % 64 == 0 && kEvGtCap >= 256, "the LDS cap on ground truth per (sample, class)");
static_assert(kEvMaxM <= 65536, "prediction rows are kept as 16-bit indices");

enum { kEvStCursor = 0, kEvStBoxes = 1, kEvStGtCap = 2, kEvStLabel = 3, kEvStFull = 4, kEvStNpos = 8 };

struct EvParams {
  const float* boxes;
  const void* scores;
  const int32_t* labels;
  const int32_t* counts;
  const float* gt_boxes;
  const void* gt_labels;
  const int8_t* gt_attrs;
  uint4* rec;
  unsigned long long* state;
  double range[kEvMaxCls];
  double th2[4];                     // squared thresholds
  int flags[kEvMaxCls], attr_moving[kEvMaxCls], attr_still[kEvMaxCls];
  int B, M, G, cols, score_dtype, gt64, ncls, max_boxes, max_samples, tp_idx;
};

__device__ __forceinline__ bool ev_in_range(float x, float y, double range) {
  const double dx = (double) x, dy = (double) y;
  return sqrt(dx * dx + dy * dy) < range;           // false for a NaN centre
}

__device__ __forceinline__ float ev_score(const EvParams& p, long k) {
  if (p.score_dtype == VAMP_F32) return static_cast<const float*>(p.scores)[k];
  const uint16_t u = static_cast<const uint16_t*>(p.scores)[k];
  return p.score_dtype == VAMP_BF16 ? bf16_to_f32(u) : f16_to_f32(u);
}

// an integer that orders like the score (a total order: -0 counts as +0; a NaN of either sign and any payload gets the
// one key above +inf's, so that NaNs tie and the higher row goes first, as the host's descending sort has them)
__device__ __forceinline__ uint32_t ev_key(float s) {
  const uint32_t u = __float_as_uint(s + 0.0f);
  if ((u & 0x7fffffffu) > 0x7f800000u) return 0xffffffffu;
  return (u >> 31) ? ~u : (u | 0x80000000u);
}

// Python's float modulus (the floored one) for m > 0
__device__ __forceinline__ double ev_pymod(double x, double m) {
  double r = fmod(x, m);
  if (r != 0.0 && r < 0.0) r += m;
  return r;
}

// the five errors of a match (trans, scale, orient, vel, attr) in float64, rounded to fp32
__device__ __forceinline__ void ev_errors(const EvParams& p, int c, const float* pb, const float* gb, int gattr,
                                          double d2, float (&e)[5]) {
  const int f = p.flags[c];
  const float nanf_ = __uint_as_float(0x7fc00000u);
  e[0] = (float) sqrt(d2);
  const double g3 = gb[3], g4 = gb[4], g5 = gb[5], p3 = pb[3], p4 = pb[4], p5 = pb[5];
  const double inter = ((g3 < p3 ? g3 : p3) * (g4 < p4 ? g4 : p4)) * (g5 < p5 ? g5 : p5);
  const double vg = (g3 * g4) * g5, vp = (p3 * p4) * p5;
  e[1] = (float) (1.0 - inter / ((vg + vp) - inter));
  e[2] = nanf_;
  if (f & VAMP_DET_EVAL_HAS_ORIENT) {
    const double per = (f & VAMP_DET_EVAL_HALF_PERIOD) ? kEvPi : 2.0 * kEvPi;
    double d = ev_pymod(((double) gb[6] - (double) pb[6]) + per / 2.0, per) - per / 2.0;
    if (d > kEvPi) d -= 2.0 * kEvPi;
    e[2] = (float) fabs(d);
  }
  const bool vel = p.cols == 9;
  e[3] = nanf_;
  if (f & VAMP_DET_EVAL_HAS_VEL) {
    const double dvx = vel ? (double) gb[7] - (double) pb[7] : 0.0, dvy = vel ? (double) gb[8] - (double) pb[8] : 0.0;
    e[3] = (float) sqrt(dvx * dvx + dvy * dvy);
  }
  e[4] = nanf_;
  if ((f & VAMP_DET_EVAL_HAS_ATTR) && gattr >= 0) {
    const double vx = vel ? (double) pb[7] : 0.0, vy = vel ? (double) pb[8] : 0.0;
    const int pa = sqrt(vx * vx + vy * vy) > kEvSpeed ? p.attr_moving[c] : p.attr_still[c];
    e[4] = gattr == pa ? 0.0f : 1.0f;
  }
}

__global__ void __launch_bounds__(kEvBlock) det_eval_kernel(EvParams p) {
  __shared__ float s_gx[kEvGtCap], s_gy[kEvGtCap];
  __shared__ int s_gi[kEvGtCap];
  __shared__ uint32_t s_key[kEvMaxM], s_sc[kEvMaxM];
  __shared__ float s_px[kEvMaxM], s_py[kEvMaxM];
  __shared__ uint16_t s_row[kEvMaxM], s_ord[kEvMaxM];
  __shared__ int s_wc[kEvWaves];

  const int b = blockIdx.x / p.ncls, c = blockIdx.x % p.ncls;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const uint64_t lt = (1ull << lane) - 1ull;
  const long long cursor = (long long) p.state[kEvStCursor];
  if (cursor < 0 || cursor + p.B > p.max_samples) {           // a full buffer drops the batch and counts it
    if (blockIdx.x == 0 && tid == 0) atomicAdd(&p.state[kEvStFull], 1ull);
    return;
  }
  const double range = p.range[c];
  int n = p.counts[b];
  if (c == 0 && tid == 0 && n > p.max_boxes) atomicAdd(&p.state[kEvStBoxes], 1ull);
  n = min(max(n, 0), p.M);
  int nbad = 0;                          // labels outside the class list, counted by the sample's class-0 workgroup

  // (a) the class's ground truth inside the range, in row order
  int ng = 0;
  for (int base = 0; base < p.G; base += kEvBlock) {
    const int i = base + tid;
    bool keep = false;
    float x = 0.0f, y = 0.0f;
    if (i < p.G) {
      const long k = (long) b * p.G + i;
      const long lab = p.gt64 ? (long) static_cast<const int64_t*>(p.gt_labels)[k]
                              : (long) static_cast<const int32_t*>(p.gt_labels)[k];
      if (lab == c) {
        const float* gb = p.gt_boxes + k * p.cols;
        x = gb[0];
        y = gb[1];
        keep = ev_in_range(x, y, range);
      }
      nbad += c == 0 && lab != -1 && (lab < 0 || lab >= p.ncls);
    }
    const uint64_t m = __ballot(keep);
    if (lane == 0) s_wc[wid] = __popcll(m);
    __syncthreads();
    int off = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < kEvWaves; ++w) {
      off += w < wid ? s_wc[w] : 0;
      tot += s_wc[w];
    }
    const int j = ng + off + __popcll(m & lt);
    if (keep && j < kEvGtCap) {
      s_gx[j] = x;
      s_gy[j] = y;
      s_gi[j] = i;
    }
    ng += tot;
    __syncthreads();
  }
  if (tid == 0) {
    if (ng > 0) atomicAdd(&p.state[kEvStNpos + c], (unsigned long long) ng);
    if (ng > kEvGtCap) atomicAdd(&p.state[kEvStGtCap], 1ull);
  }
  const int ngc = min(ng, kEvGtCap);

  // (b) the class's predictions inside the range, in row order; the other rows this workgroup owns are invalid records
  uint4* rec = p.rec + ((size_t) (cursor + b) * p.M) * 2;
  const uint4 zero = make_uint4(0u, 0u, 0u, 0u);
  int np = 0;
  for (int base = 0; base < p.M; base += kEvBlock) {
    const int i = base + tid;
    bool keep = false, invalid = false;
    float x = 0.0f, y = 0.0f;
    if (i < p.M) {
      if (i >= n) {
        invalid = c == 0;
      } else {
        const long k = (long) b * p.M + i;
        const int lab = p.labels[k];
        if (lab < 0 || lab >= p.ncls) {
          invalid = c == 0;
          nbad += c == 0;
        } else if (lab == c) {
          const float* pb = p.boxes + k * p.cols;
          x = pb[0];
          y = pb[1];
          keep = ev_in_range(x, y, range);
          invalid = !keep;
        }
      }
    }
    if (invalid) {
      rec[2 * i] = zero;
      rec[2 * i + 1] = zero;
    }
    const uint64_t m = __ballot(keep);
    if (lane == 0) s_wc[wid] = __popcll(m);
    __syncthreads();
    int off = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < kEvWaves; ++w) {
      off += w < wid ? s_wc[w] : 0;
      tot += s_wc[w];
    }
    if (keep) {
      const int j = np + off + __popcll(m & lt);             // j <= i < M <= kEvMaxM
      const float sc = ev_score(p, (long) b * p.M + i);
      s_key[j] = ev_key(sc);
      s_sc[j] = __float_as_uint(sc);      // the record's score comes from LDS: no global load on the walk's chain
      s_px[j] = x;
      s_py[j] = y;
      s_row[j] = (uint16_t) i;
    }
    np += tot;
    __syncthreads();
  }
  if (c == 0) {
    nbad = wave_sum(nbad);
    if (lane == 0 && nbad > 0) atomicAdd(&p.state[kEvStLabel], (unsigned long long) nbad);
  }

  // (c) counting rank: score descending, then row descending (rows ascend with the LDS index)
  for (int j = tid; j < np; j += kEvBlock) {
    const uint32_t kj = s_key[j];
    int rank = 0;
    for (int k = 0; k < np; ++k) {
      const uint32_t kk = s_key[k];
      rank += (kk > kj) || (kk == kj && k > j);
    }
    s_ord[rank] = (uint16_t) j;
  }
  __syncthreads();
  if (wid != 0) return;

  // (d) the walk: lane l owns the ground-truth boxes 4 l .. 4 l + 3 and their taken bits
  float gx[kEvGtPerLane], gy[kEvGtPerLane];
#pragma unroll
  for (int q = 0; q < kEvGtPerLane; ++q) {
    const int k = lane * kEvGtPerLane + q;
    gx[q] = k < ngc ? s_gx[k] : 0.0f;
    gy[q] = k < ngc ? s_gy[k] : 0.0f;
  }
  uint32_t taken[4] = {0u, 0u, 0u, 0u};
  int act = 1;                           // the lanes that hold ground truth, rounded up to a power of two
  while (act * kEvGtPerLane < ngc) act <<= 1;
  for (int r = 0; r < np; ++r) {
    const int j = s_ord[r];
    const double px = (double) s_px[j], py = (double) s_py[j];
    unsigned long long d2[kEvGtPerLane];
#pragma unroll
    for (int q = 0; q < kEvGtPerLane; ++q) {
      const double dx = (double) gx[q] - px, dy = (double) gy[q] - py;
      const double v = dx * dx + dy * dy;                     // finite and >= 0: both centres passed the range filter
      d2[q] = lane * kEvGtPerLane + q < ngc ? (unsigned long long) __double_as_longlong(v) : kEvNone;
    }
    uint32_t tp = 0u;
    int match = -1;
    double match_d2 = 0.0;
    if (ngc > 0) {                                            // (uniform) without ground truth: all false positives
      // the four thresholds' nearest untaken boxes, reduced in lockstep (four independent chains per exchange)
      unsigned long long best[4];
      int bq[4];
#pragma unroll
      for (int h = 0; h < 4; ++h) {
        best[h] = kEvNone;
        bq[h] = 0;
#pragma unroll
        for (int q = 0; q < kEvGtPerLane; ++q) {
          const bool better = !((taken[h] >> q) & 1u) && d2[q] < best[h];   // strict: the lowest row wins a tie
          best[h] = better ? d2[q] : best[h];
          bq[h] = better ? q : bq[h];
        }
      }
      unsigned long long mn[4] = {best[0], best[1], best[2], best[3]};
#pragma unroll
      for (int o = 32; o >= 1; o >>= 1) {
        if (o >= act) continue;                               // (uniform) lanes from `act` on hold no ground truth
#pragma unroll
        for (int h = 0; h < 4; ++h) {
          const unsigned long long w = __shfl_xor(mn[h], o, 64);
          mn[h] = w < mn[h] ? w : mn[h];
        }
      }
#pragma unroll
      for (int h = 0; h < 4; ++h) {
        // lanes 0 .. act - 1 all hold the minimum; lane 0's copy is the wave's
        const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t) mn[h]);
        const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t) (mn[h] >> 32));
        const unsigned long long m = ((unsigned long long) hi << 32) | lo;
        if (m == kEvNone) continue;                           // (uniform) no untaken ground truth
        const uint64_t who = __ballot(best[h] == m);
        const int win = __ffsll((unsigned long long) who) - 1;
        const int wq = __builtin_amdgcn_readlane(bq[h], win);             // (win is uniform)
        const double dist2 = __longlong_as_double((long long) m);
        if (dist2 < p.th2[h]) {
          tp |= 1u << h;
          if (lane == win) taken[h] |= 1u << wq;
          if (h == p.tp_idx) {
            match = win * kEvGtPerLane + wq;
            match_d2 = dist2;
          }
        }
      }
    }
    if (lane == 0) {
      const int row = s_row[j];
      const long k = (long) b * p.M + row;
      const float nanf_ = __uint_as_float(0x7fc00000u);
      float e[5] = {nanf_, nanf_, nanf_, nanf_, nanf_};
      if (match >= 0) {
        const long gk = (long) b * p.G + s_gi[match];
        ev_errors(p, c, p.boxes + k * p.cols, p.gt_boxes + gk * p.cols, p.gt_attrs ? (int) p.gt_attrs[gk] : -1,
                  match_d2, e);
      }
      const uint32_t word = (uint32_t) c | (1u << 8) | (tp << 16);
      rec[2 * row] = make_uint4(s_sc[j], word, __float_as_uint(e[0]), __float_as_uint(e[1]));
      rec[2 * row + 1] = make_uint4(__float_as_uint(e[2]), __float_as_uint(e[3]), __float_as_uint(e[4]), 0u);
    }
  }
}

// ---------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------
static_assert(sizeof(VampDetEvalDesc) == 408, "VampDetEvalDesc layout: part of the ABI (the binding reads it from include/vampire_hip.h)");
static_assert(VAMP_DET_EVAL_RECORD_BYTES == 2 * sizeof(uint4), "a record is two 16-byte stores");
static_assert(VAMP_DET_EVAL_STATE_WORDS >= kEvStNpos + kEvMaxCls, "state holds the counters and npos");

int ev_validate(const VampDetEvalDesc* d) {
  VAMP_REQUIRE(d, "desc is NULL");
  VAMP_REQUIRE(d->B >= 1 && d->B <= kEvMaxB, "B must be in [1, 4096]");
  VAMP_REQUIRE(d->M >= 1 && d->M <= kEvMaxM, "M must be in [1, 2048]");
  VAMP_REQUIRE(d->G >= 0 && d->G <= kEvMaxG, "G must be in [0, 2^20]");
  VAMP_REQUIRE(d->box_cols == 7 || d->box_cols == 9, "box_cols must be 7 or 9");
  VAMP_REQUIRE(d->score_dtype == VAMP_F32 || d->score_dtype == VAMP_BF16 || d->score_dtype == VAMP_F16,
               "score_dtype must be VAMP_F32, VAMP_BF16 or VAMP_F16");
  VAMP_REQUIRE(d->gt_label_dtype == VAMP_I32 || d->gt_label_dtype == VAMP_I64,
               "gt_label_dtype must be VAMP_I32 or VAMP_I64");
  VAMP_REQUIRE(d->has_attrs == 0 || d->has_attrs == 1, "has_attrs must be 0 or 1");
  VAMP_REQUIRE(d->num_classes >= 1 && d->num_classes <= kEvMaxCls, "num_classes must be in [1, 16]");
  VAMP_REQUIRE(d->max_boxes_per_sample >= 1, "max_boxes_per_sample must be positive");
  VAMP_REQUIRE(d->max_samples >= 1 && (long long) d->max_samples * d->M < (1ll << 31),
               "max_samples must be positive with max_samples * M < 2^31");
  for (int c = 0; c < d->num_classes; ++c) {
    VAMP_REQUIRE(d->class_range[c] > 0.0 && std::isfinite(d->class_range[c]), "class_range must be positive and finite");
    VAMP_REQUIRE((d->class_flags[c] & ~15) == 0, "class_flags holds VAMP_DET_EVAL_* bits only");
    VAMP_REQUIRE(d->attr_moving[c] >= -1 && d->attr_moving[c] < 128 && d->attr_still[c] >= -1 && d->attr_still[c] < 128,
                 "attr_moving, attr_still must be in [-1, 127]");
  }
  bool tp = false;
  for (int h = 0; h < 4; ++h) {
    VAMP_REQUIRE(d->dist_ths[h] > 0.0 && std::isfinite(d->dist_ths[h]), "dist_ths must be positive and finite");
    VAMP_REQUIRE(h == 0 || d->dist_ths[h] > d->dist_ths[h - 1], "dist_ths must ascend");
    tp = tp || d->dist_ths[h] == d->dist_th_tp;
  }
  VAMP_REQUIRE(tp, "dist_th_tp must be one of dist_ths");
  VAMP_REQUIRE(d->reserved[0] == 0 && d->reserved[1] == 0, "reserved must be 0");
  return VAMP_OK;
}

}  // namespace
}  // namespace vamp

using namespace vamp;

extern "C" {

int vamp_det_eval_supported(const VampDetEvalDesc* d) { return ev_validate(d) == VAMP_OK ? 1 : 0; }

size_t vamp_det_eval_record_bytes(const VampDetEvalDesc* d) {
  if (ev_validate(d)) return 0;
  return (size_t) d->max_samples * d->M * VAMP_DET_EVAL_RECORD_BYTES;
}

int vamp_det_eval_update(const VampDetEvalDesc* d, const float* boxes, const void* scores, const int32_t* labels,
                         const int32_t* counts, const float* gt_boxes, const void* gt_labels, const int8_t* gt_attrs,
                         void* records, int64_t* state, void* stream) {
  if (int e = ev_validate(d)) return e;
  VAMP_REQUIRE(boxes && scores && labels && counts, "a detection pointer is NULL");
  VAMP_REQUIRE(d->G == 0 || (gt_boxes && gt_labels), "gt_boxes or gt_labels is NULL");
  VAMP_REQUIRE(d->has_attrs == 0 || d->G == 0 || gt_attrs, "has_attrs is set and gt_attrs is NULL");
  VAMP_REQUIRE(records && state, "records or state is NULL");
  VAMP_REQUIRE(aligned(records, 16), "records must be 16-byte aligned");
  EvParams q{};
  q.boxes = boxes; q.scores = scores; q.labels = labels; q.counts = counts;
  q.gt_boxes = gt_boxes; q.gt_labels = gt_labels; q.gt_attrs = d->has_attrs ? gt_attrs : nullptr;
  q.rec = static_cast<uint4*>(records);
  q.state = reinterpret_cast<unsigned long long*>(state);
  for (int c = 0; c < d->num_classes; ++c) {
    q.range[c] = d->class_range[c];
    q.flags[c] = d->class_flags[c];
    q.attr_moving[c] = d->attr_moving[c];
    q.attr_still[c] = d->attr_still[c];
  }
  for (int h = 0; h < 4; ++h) {
    q.th2[h] = d->dist_ths[h] * d->dist_ths[h];
    if (d->dist_ths[h] == d->dist_th_tp) q.tp_idx = h;
  }
  q.B = d->B; q.M = d->M; q.G = d->G; q.cols = d->box_cols; q.score_dtype = d->score_dtype;
  q.gt64 = d->gt_label_dtype == VAMP_I64;
  q.ncls = d->num_classes; q.max_boxes = d->max_boxes_per_sample; q.max_samples = d->max_samples;
  hipStream_t s = static_cast<hipStream_t>(stream);
  VAMP_TIMED(kProfAux, s, (det_eval_kernel<<<d->B * d->num_classes, kEvBlock, 0, s>>>(q)));
  return check_launch("det_eval_update");
}

}  // extern "C"
