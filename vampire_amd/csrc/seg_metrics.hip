// Segmentation metrics on the device (base_exp.py:370-382, :634-663 and :835-840 of the reference):
//
//  * vamp_confusion_update: the argmax of the logits in a class window, compared with the target, counted
//    into a Kc x Kc int64 confusion matrix (torchmetrics' confmat[target, pred] orientation) -- what the
//    reference does with a boolean index, argmax and a torchmetrics bincount, in one streaming pass that
//    never leaves the device.  Each workgroup keeps a histogram of Kc * Kc + 1 uint32 bins in LDS (the last
//    bin counts invalid elements); lanes of a wave that fall into the same bin as the wave's first live
//    lane are added with ONE LDS add of the ballot's popcount ("free" predicted "free" is most of an
//    occupancy grid), the others add 1 each.  Every workgroup stores its histogram into a slab of its
//    own; a second launch adds the slabs in a fixed order into the int64 state.  No float atomics, no
//    global atomics: the counts are exact and reproducible.
//  * vamp_lidarseg_predict: the index_add_ of point logits onto reference points followed by the argmax
//    (:645-649, :835-838).  Points are sorted by reference index (count, the cell lists' scan, fill, then a
//    rank by point id inside each run makes the runs ascending), and one wave per reference point sums its points' rows
//    in increasing point order -- the order of a sequential CPU index_add_, hence bit-exact against it.
#include "common.hpp"
#include "elem16.hpp"

namespace vamp {
namespace {

constexpr int kConfMaxKc = 32;
constexpr int kConfMaxBins = kConfMaxKc * kConfMaxKc + 1;
constexpr int kConfBlock = 256;
constexpr int kConfMaxGrid = 1024;     // slabs: at most 1024 x 1025 uint32 (4.2 MB)
constexpr int kConfBatch = 9;          // class loads in flight per lane before they are compared (18 classes: two batches)
constexpr int kReduceWaves = 16;

struct ConfParams {
  int n, S;                 // elements, elements per block (planes layout)
  int K, Kc, lo, hi;
  long ignore;
  int use_ignore;
};

// torch.argmax: a NaN beats every number, and among equals (NaNs included) the first index wins
__device__ __forceinline__ void argmax_step(float v, int c, float& best, int& bi) {
  if (!(best != best) && (v > best || v != v)) {
    best = v;
    bi = c;
  }
}

template <int V>
__device__ __forceinline__ void ld_logits(const float* p, long off, float (&v)[V]) {
  if constexpr (V == 4) {
    const float4 x = *reinterpret_cast<const float4*>(p + off);
    v[0] = x.x; v[1] = x.y; v[2] = x.z; v[3] = x.w;
  } else {
    v[0] = p[off];
  }
}
template <int V>
__device__ __forceinline__ void ld_logits(const __hip_bfloat16* p, long off, float (&v)[V]) {
  if constexpr (V == 4) {
    const float4 x = bf16x4_to_f32(*reinterpret_cast<const uint2*>(p + off));
    v[0] = x.x; v[1] = x.y; v[2] = x.z; v[3] = x.w;
  } else {
    v[0] = ldf(p, off);
  }
}

// argmax over classes [lo, hi) of V consecutive elements whose class c sits at base[c * cs].  The loads of a
// batch are unconditional -- classes past hi - 1 re-read class hi - 1, which was compared just before them and
// can no longer win (a strict > and a NaN best are both final) -- so that they are all in flight at once (loads
// under a branch each wait for the one before).
template <typename PT, int V>
__device__ __forceinline__ void argmax_window(const PT* __restrict__ base, long cs, int lo, int hi, long (&pred)[V]) {
  float best[V];
  int bi[V];
#pragma unroll
  for (int e = 0; e < V; ++e) {
    best[e] = -__builtin_inff();     // an all -inf row keeps bi = lo, like torch
    bi[e] = lo;
  }
  for (int c0 = lo; c0 < hi; c0 += kConfBatch) {
    float v[kConfBatch][V];
#pragma unroll
    for (int j = 0; j < kConfBatch; ++j) ld_logits<V>(base, (long) min(c0 + j, hi - 1) * cs, v[j]);
#pragma unroll
    for (int j = 0; j < kConfBatch; ++j) {
#pragma unroll
      for (int e = 0; e < V; ++e) argmax_step(v[j][e], c0 + j, best[e], bi[e]);
    }
  }
#pragma unroll
  for (int e = 0; e < V; ++e) pred[e] = bi[e];
}

template <typename TT, int V>
__device__ __forceinline__ void ld_targets(const TT* __restrict__ t, int i0, long (&out)[V]) {
  if constexpr (V == 4 && sizeof(TT) == 8) {
    const int4 a = *reinterpret_cast<const int4*>(t + i0), b = *reinterpret_cast<const int4*>(t + i0 + 2);
    out[0] = (long) (((unsigned long) (unsigned) a.y << 32) | (unsigned) a.x);
    out[1] = (long) (((unsigned long) (unsigned) a.w << 32) | (unsigned) a.z);
    out[2] = (long) (((unsigned long) (unsigned) b.y << 32) | (unsigned) b.x);
    out[3] = (long) (((unsigned long) (unsigned) b.w << 32) | (unsigned) b.z);
  } else if constexpr (V == 4 && sizeof(TT) == 4) {
    const int4 a = *reinterpret_cast<const int4*>(t + i0);
    out[0] = a.x; out[1] = a.y; out[2] = a.z; out[3] = a.w;
  } else if constexpr (V == 4) {
    const unsigned u = *reinterpret_cast<const unsigned*>(t + i0);
#pragma unroll
    for (int e = 0; e < 4; ++e) out[e] = (u >> (8 * e)) & 0xffu;
  } else {
    out[0] = (long) t[i0];
  }
}

template <int V>
__device__ __forceinline__ void ld_mask(const uint8_t* __restrict__ m, int i0, bool (&out)[V]) {
  if (m == nullptr) {
#pragma unroll
    for (int e = 0; e < V; ++e) out[e] = true;
  } else if constexpr (V == 4) {
    const unsigned u = *reinterpret_cast<const unsigned*>(m + i0);
#pragma unroll
    for (int e = 0; e < 4; ++e) out[e] = ((u >> (8 * e)) & 0xffu) != 0;
  } else {
    out[0] = m[i0] != 0;
  }
}

// -1: not counted (masked out or ignored); Kc * Kc: invalid (target or integer prediction out of range)
__device__ __forceinline__ int conf_bin(const ConfParams& q, long t, long p, bool m) {
  if (!m || (q.use_ignore && t == q.ignore)) return -1;
  if (t < 0 || t >= q.Kc || p < 0 || p >= q.Kc) return q.Kc * q.Kc;
  return (int) t * q.Kc + (int) p;
}

// the lanes in the bin of the wave's first live lane go in with one add, the rest one by one
__device__ __forceinline__ void hist_add(uint32_t* hist, int bin) {
  const unsigned long long live = __ballot(bin >= 0);
  if (live == 0) return;
  const int lead = __builtin_ctzll(live);
  const int b0 = __builtin_amdgcn_readlane(bin, lead);
  const unsigned long long same = __ballot(bin == b0);
  if ((int) (threadIdx.x & 63) == lead) atomicAdd(hist + b0, (uint32_t) __popcll(same));
  else if (bin >= 0 && bin != b0) atomicAdd(hist + bin, 1u);
}

enum ConfMode { kRows = 0, kPlanes = 1, kPlanes4 = 2, kPreds = 3 };

template <typename PT, typename TT, int MODE>
__global__ void __launch_bounds__(kConfBlock)
conf_hist_kernel(ConfParams q, const PT* __restrict__ pred, const TT* __restrict__ tgt,
                 const uint8_t* __restrict__ mask, uint32_t* __restrict__ slabs) {
  constexpr int V = MODE == kPlanes4 ? 4 : 1;
  __shared__ uint32_t hist[kConfMaxBins];
  const int nb = q.Kc * q.Kc + 1;
  for (int k = threadIdx.x; k < nb; k += kConfBlock) hist[k] = 0;
  __syncthreads();
  const int ngroups = q.n / V;
  // the trip count is uniform per workgroup: hist_add's ballots see every lane of the wave
  for (long g0 = (long) blockIdx.x * kConfBlock; g0 < ngroups; g0 += (long) gridDim.x * kConfBlock) {
    const long g = g0 + threadIdx.x;
    int bin[V];
#pragma unroll
    for (int e = 0; e < V; ++e) bin[e] = -1;
    if (g < ngroups) {
      const int i0 = (int) g * V;
      long t[V], p[V];
      bool m[V];
      if constexpr (MODE == kPreds) {
        p[0] = (long) pred[i0];
      } else if constexpr (MODE == kRows) {
        argmax_window<PT, V>(pred + (long) i0 * q.K, 1, q.lo, q.hi, p);
      } else {
        const unsigned b = (unsigned) i0 / (unsigned) q.S, s = (unsigned) i0 - b * (unsigned) q.S;
        argmax_window<PT, V>(pred + (long) b * q.K * q.S + s, q.S, q.lo, q.hi, p);
      }
      ld_targets<TT, V>(tgt, i0, t);
      ld_mask<V>(mask, i0, m);
#pragma unroll
      for (int e = 0; e < V; ++e) bin[e] = conf_bin(q, t[e], p[e], m[e]);
    }
#pragma unroll
    for (int e = 0; e < V; ++e) hist_add(hist, bin[e]);
  }
  __syncthreads();
  uint32_t* slab = slabs + (long) blockIdx.x * nb;
  for (int k = threadIdx.x; k < nb; k += kConfBlock) slab[k] = hist[k];
}

// bins of 64 per workgroup; wave w adds slabs w, w + 16, ...; the 16 partial sums are added in wave order
// (the element count is below 2^31, so uint32 partial sums cannot wrap)
__global__ void __launch_bounds__(64 * kReduceWaves)
conf_reduce_kernel(const uint32_t* __restrict__ slabs, int G, int nb, int64_t* __restrict__ confmat,
                   int64_t* __restrict__ invalid) {
  __shared__ uint32_t part[kReduceWaves][64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int bin = blockIdx.x * 64 + lane;
  uint32_t acc = 0;
  if (bin < nb) {
#pragma unroll 16
    for (int r = w; r < G; r += kReduceWaves) acc += slabs[(long) r * nb + bin];
  }
  part[w][lane] = acc;
  __syncthreads();
  if (w == 0 && bin < nb) {
    uint32_t tot = 0;
#pragma unroll
    for (int k = 0; k < kReduceWaves; ++k) tot += part[k][lane];
    if (bin < nb - 1) confmat[bin] += tot;
    else invalid[0] += tot;
  }
}

int conf_grid(const VampConfDesc* d, int V) {
  const long groups = d->B * d->S / V;
  return (int) std::min<long>((groups + kConfBlock - 1) / kConfBlock, kConfMaxGrid);
}

bool is_int_pred(int32_t dt) { return dt == VAMP_I64 || dt == VAMP_I32; }

int conf_validate(const VampConfDesc* d) {
  VAMP_REQUIRE(d != nullptr, "desc is NULL");
  VAMP_REQUIRE(d->B >= 0 && d->S >= 0 && d->B < 0x7fffffffL && d->S < 0x7fffffffL, "B, S must be in [0, 2^31)");
  VAMP_REQUIRE(d->B * d->S < 0x7fffffffL, "n = B * S must be below 2^31 per call");
  VAMP_REQUIRE(d->Kc >= 1 && d->Kc <= kConfMaxKc, "Kc must be in 1..32");
  VAMP_REQUIRE(d->target_dtype == VAMP_I64 || d->target_dtype == VAMP_I32 || d->target_dtype == VAMP_U8,
               "target_dtype must be VAMP_I64, VAMP_I32 or VAMP_U8");
  VAMP_REQUIRE(d->use_ignore == 0 || d->use_ignore == 1, "use_ignore must be 0 or 1");
  if (is_int_pred(d->pred_dtype)) {
    VAMP_REQUIRE(d->layout == VAMP_SEG_ROWS && d->K == 1, "integer predictions take layout ROWS and K = 1");
    return VAMP_OK;
  }
  VAMP_REQUIRE(d->pred_dtype == VAMP_F32 || d->pred_dtype == VAMP_BF16,
               "pred_dtype must be VAMP_F32, VAMP_BF16, VAMP_I64 or VAMP_I32");
  VAMP_REQUIRE(d->layout == VAMP_SEG_ROWS || d->layout == VAMP_SEG_PLANES, "layout must be ROWS or PLANES");
  VAMP_REQUIRE(d->K >= 1 && d->K < 0x10000, "K must be in 1..65535");
  VAMP_REQUIRE(d->lo >= 0 && d->lo < d->hi && d->hi <= d->K, "class window must satisfy 0 <= lo < hi <= K");
  VAMP_REQUIRE(d->hi - 1 < d->Kc, "class window: hi - 1 must be below Kc");
  return VAMP_OK;
}

template <typename PT, typename TT>
void conf_launch(int mode, unsigned grid, const ConfParams& q, const void* pred, const void* tgt, const uint8_t* mask,
                 uint32_t* slabs, hipStream_t s) {
  const PT* p = static_cast<const PT*>(pred);
  const TT* t = static_cast<const TT*>(tgt);
#define VAMP_CONF(M) VAMP_TIMED(kProfAux, s, (conf_hist_kernel<PT, TT, M><<<grid, kConfBlock, 0, s>>>(q, p, t, mask, slabs)))
  if (mode == kRows) VAMP_CONF(kRows);
  else if (mode == kPlanes) VAMP_CONF(kPlanes);
  else VAMP_CONF(kPlanes4);
#undef VAMP_CONF
}

template <typename TT>
void conf_launch_t(int32_t pdt, int mode, unsigned grid, const ConfParams& q, const void* pred, const void* tgt,
                   const uint8_t* mask, uint32_t* slabs, hipStream_t s) {
  const TT* t = static_cast<const TT*>(tgt);
  if (pdt == VAMP_I64) {
    VAMP_TIMED(kProfAux, s, (conf_hist_kernel<int64_t, TT, kPreds><<<grid, kConfBlock, 0, s>>>(
        q, static_cast<const int64_t*>(pred), t, mask, slabs)));
  } else if (pdt == VAMP_I32) {
    VAMP_TIMED(kProfAux, s, (conf_hist_kernel<int32_t, TT, kPreds><<<grid, kConfBlock, 0, s>>>(
        q, static_cast<const int32_t*>(pred), t, mask, slabs)));
  } else if (pdt == VAMP_F32) {
    conf_launch<float, TT>(mode, grid, q, pred, tgt, mask, slabs, s);
  } else {
    conf_launch<__hip_bfloat16, TT>(mode, grid, q, pred, tgt, mask, slabs, s);
  }
}

// ------------------------------------------------------------------------------------------------
// lidar-segmentation prediction
// ------------------------------------------------------------------------------------------------
// the runs of the reference points in the cell lists' layout (runtime.hip launch_cell_scan): run r starts at
// off[r] + boff[r / kScanTile]; the counters are left at zero by the scan and serve as the fill cursors
struct LsWs {
  int *cnt, *off, *bsum, *boff, *aux, *bad, *ids, *sorted;
  long ncell;            // num_ref + 1 (run r ends where r + 1 starts), rounded up to the scan tile
  size_t bytes;
};

LsWs ls_ws(long P, long R, void* ws) {
  LsWs w;
  w.ncell = (R + 1 + kScanTile - 1) / kScanTile * kScanTile;
  const size_t ncell = (size_t) w.ncell, ntile = ncell / kScanTile;
  Carve c(ws);
  // counters, the scan's ticket and pad, then the count of points with an index out of range: one zero fill (the one
  // word more than take_scan's counters is why the five regions are taken here)
  w.cnt = c.take<int>(ncell + kScanPad + 1);
  w.bad = w.cnt + ncell + kScanPad;
  w.off = c.take<int>(ncell);
  w.bsum = c.take<int>(ntile);
  w.boff = c.take<int>(ntile);
  w.aux = c.take<int>(ntile + 4);
  w.ids = c.take<int>((size_t) std::max(P, 1L));
  w.sorted = c.take<int>((size_t) std::max(P, 1L));
  w.bytes = c.off;
  return w;
}

__device__ __forceinline__ int run_start(const int* __restrict__ off, const int* __restrict__ boff, int r) {
  return off[r] + boff[r / kScanTile];
}

__global__ void __launch_bounds__(256)
ls_count_kernel(const int64_t* __restrict__ idx, int P, int R, int* __restrict__ cnt, int* __restrict__ bad) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= P) return;
  const int64_t r = idx[i];
  atomicAdd((r >= 0 && r < R) ? cnt + r : bad, 1);
}

// a point's slot in its reference point's run, in arrival order
__global__ void __launch_bounds__(256)
ls_fill_kernel(const int64_t* __restrict__ idx, int P, int R, const int* __restrict__ off, const int* __restrict__ boff,
               int* __restrict__ fill, int* __restrict__ ids) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= P) return;
  const int64_t r = idx[i];
  if (r < 0 || r >= R) return;
  ids[run_start(off, boff, (int) r) + atomicAdd(fill + r, 1)] = i;
}

// ... and its place in increasing point order: the number of points of the run with a smaller id
__global__ void __launch_bounds__(256)
ls_rank_kernel(const int64_t* __restrict__ idx, int P, int R, const int* __restrict__ off,
               const int* __restrict__ boff, const int* __restrict__ ids, int* __restrict__ sorted) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= P) return;
  const int64_t r = idx[i];
  if (r < 0 || r >= R) return;
  const int beg = run_start(off, boff, (int) r), end = run_start(off, boff, (int) r + 1);
  int rank = 0;
  for (int k = beg; k < end; ++k) rank += ids[k] < i;
  sorted[beg + rank] = i;
}

// a beats b under torch.argmax's order: NaN above every number, the lower index among equals
__device__ __forceinline__ bool argmax_beats(float a, int ai, float b, int bi) {
  const bool an = a != a, bn = b != b;
  if (an != bn) return an;
  if (!an && a != b) return a > b;
  return ai < bi;
}

// one wave per reference point, lane c sums class lo + c of the run's rows in point order
template <typename PT>
__global__ void __launch_bounds__(256)
ls_label_kernel(const PT* __restrict__ logits, int K, int lo, int hi, int R, const int* __restrict__ off,
                const int* __restrict__ boff, const int* __restrict__ bad, const int* __restrict__ sorted,
                int64_t* __restrict__ labels, int64_t* __restrict__ invalid) {
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (blockIdx.x == 0 && threadIdx.x == 0) invalid[0] = bad[0];
  if (r >= R) return;
  const int c = lo + lane;
  const bool live = c < hi;
  float acc = 0.f;
  const int beg = run_start(off, boff, r), end = run_start(off, boff, r + 1);
  for (int k = beg; k < end; ++k) {
    const long row = (long) sorted[k] * K;
    if (live) acc += ldf(logits, row + c);
  }
  float best = live ? acc : -__builtin_inff();
  int bi = live ? c : 0x7fffffff;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ob = __shfl_xor(best, o, 64);
    const int oi = __shfl_xor(bi, o, 64);
    if (argmax_beats(ob, oi, best, bi)) {
      best = ob;
      bi = oi;
    }
  }
  if (lane == 0) labels[r] = bi;
}

int ls_validate(int64_t P, int32_t K, int32_t dtype, int32_t lo, int32_t hi, int64_t R) {
  VAMP_REQUIRE(P >= 0 && P < 0x7fffffffL, "P must be in [0, 2^31)");
  VAMP_REQUIRE(R >= 0 && R < 0x7fffffffL - 2 * kScanTile, "num_ref must be in [0, 2^31 - 4096)");
  VAMP_REQUIRE(dtype == VAMP_F32 || dtype == VAMP_BF16, "dtype must be VAMP_F32 or VAMP_BF16");
  VAMP_REQUIRE(K >= 1 && lo >= 0 && lo < hi && hi <= K, "class window must satisfy 0 <= lo < hi <= K");
  VAMP_REQUIRE(hi - lo <= kWave, "class window wider than 64");
  return VAMP_OK;
}

}  // namespace
}  // namespace vamp

using namespace vamp;

extern "C" {

size_t vamp_confusion_workspace_bytes(const VampConfDesc* d) {
  if (conf_validate(d)) return 0;
  return (size_t) std::max(conf_grid(d, 1), 1) * (d->Kc * d->Kc + 1) * sizeof(uint32_t);
}

int vamp_confusion_update(const VampConfDesc* d, const void* pred, const void* target, const uint8_t* mask,
                          int64_t* confmat, int64_t* invalid, void* workspace, size_t workspace_bytes,
                          void* stream) {
  if (int e = conf_validate(d)) return e;
  VAMP_REQUIRE(confmat && invalid, "confmat / invalid is NULL");
  const long n = d->B * d->S;
  if (n == 0) return VAMP_OK;
  VAMP_REQUIRE(pred && target, "pred / target is NULL");
  const size_t need = vamp_confusion_workspace_bytes(d);
  if (int e = workspace_fits(__func__, workspace, workspace_bytes, need)) return e;
  const size_t tsize = d->target_dtype == VAMP_I64 ? 8 : (d->target_dtype == VAMP_I32 ? 4 : 1);
  int mode = kRows;
  if (!is_int_pred(d->pred_dtype) && d->layout == VAMP_SEG_PLANES) {
    // four neighbouring elements of a class plane per lane when every stream allows the vector loads
    const bool v4 = d->S % 4 == 0 && aligned(pred, d->pred_dtype == VAMP_F32 ? 16 : 8) &&
                    aligned(target, tsize == 1 ? 4 : 16) && (mask == nullptr || aligned(mask, 4));
    mode = v4 ? kPlanes4 : kPlanes;
  }
  const int grid = conf_grid(d, mode == kPlanes4 ? 4 : 1);
  const int nb = d->Kc * d->Kc + 1;
  const ConfParams q{(int) n, (int) d->S, d->K, d->Kc, d->lo, d->hi, (long) d->ignore_index, d->use_ignore};
  hipStream_t s = static_cast<hipStream_t>(stream);
  uint32_t* slabs = static_cast<uint32_t*>(workspace);
  if (d->target_dtype == VAMP_I64) conf_launch_t<int64_t>(d->pred_dtype, mode, grid, q, pred, target, mask, slabs, s);
  else if (d->target_dtype == VAMP_I32) conf_launch_t<int32_t>(d->pred_dtype, mode, grid, q, pred, target, mask, slabs, s);
  else conf_launch_t<uint8_t>(d->pred_dtype, mode, grid, q, pred, target, mask, slabs, s);
  if (int e = check_launch("conf_hist_kernel")) return e;
  VAMP_TIMED(kProfAux, s, (conf_reduce_kernel<<<(nb + 63) / 64, 64 * kReduceWaves, 0, s>>>(slabs, grid, nb, confmat, invalid)));
  return check_launch("conf_reduce_kernel");
}

size_t vamp_lidarseg_workspace_bytes(int64_t P, int64_t num_ref) {
  if (P < 0 || num_ref < 0 || P >= 0x7fffffffL || num_ref >= 0x7fffffffL - 2 * kScanTile) return 0;
  return ls_ws(P, num_ref, nullptr).bytes;
}

int vamp_lidarseg_predict(int64_t P, int32_t K, int32_t dtype, int32_t lo, int32_t hi, const void* pts_logits,
                          const int64_t* ref_index, int64_t num_ref, int64_t* labels, int64_t* invalid,
                          void* workspace, size_t workspace_bytes, void* stream) {
  if (int e = ls_validate(P, K, dtype, lo, hi, num_ref)) return e;
  VAMP_REQUIRE(invalid != nullptr, "invalid is NULL");
  VAMP_REQUIRE(P == 0 || (pts_logits && ref_index), "pts_logits / ref_index is NULL");
  VAMP_REQUIRE(num_ref == 0 || labels, "labels is NULL");
  const LsWs w = ls_ws(P, num_ref, workspace);
  if (int e = workspace_fits(__func__, workspace, workspace_bytes, w.bytes)) return e;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int np = (int) P, R = (int) num_ref;
  if (int e = launch_zero(w.cnt, (size_t) (w.ncell + kScanPad + 1) * sizeof(int), s)) return e;
  const unsigned pgrid = (unsigned) ((np + 255) / 256);
  if (np > 0) {
    VAMP_TIMED(kProfAux, s, (ls_count_kernel<<<pgrid, 256, 0, s>>>(ref_index, np, R, w.cnt, w.bad)));
    if (int e = check_launch("ls_count_kernel")) return e;
  }
  if (int e = launch_cell_scan(w.cnt, w.off, w.bsum, w.boff, w.aux, w.ncell, s)) return e;
  if (np > 0) {
    VAMP_TIMED(kProfAux, s, (ls_fill_kernel<<<pgrid, 256, 0, s>>>(ref_index, np, R, w.off, w.boff, w.cnt, w.ids)));
    if (int e = check_launch("ls_fill_kernel")) return e;
    VAMP_TIMED(kProfAux, s, (ls_rank_kernel<<<pgrid, 256, 0, s>>>(ref_index, np, R, w.off, w.boff, w.ids, w.sorted)));
    if (int e = check_launch("ls_rank_kernel")) return e;
  }
  const unsigned lgrid = (unsigned) std::max((R + 3) / 4, 1);
  if (dtype == VAMP_F32)
    VAMP_TIMED(kProfAux, s, (ls_label_kernel<float><<<lgrid, 256, 0, s>>>(
        static_cast<const float*>(pts_logits), K, lo, hi, R, w.off, w.boff, w.bad, w.sorted, labels, invalid)));
  else
    VAMP_TIMED(kProfAux, s, (ls_label_kernel<__hip_bfloat16><<<lgrid, 256, 0, s>>>(
        static_cast<const __hip_bfloat16*>(pts_logits), K, lo, hi, R, w.off, w.boff, w.bad, w.sorted, labels, invalid)));
  return check_launch("ls_label_kernel");
}

}  // extern "C"
