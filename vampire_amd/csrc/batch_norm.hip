// Batch normalisation of an [N, C, H, W] tensor with the ReLU and the residual add that follow it in the encoders,
// in four separate steps so that a collective can sit between the first and the second of each direction
// (base_cli.py:78, 91 Trainer(sync_batchnorm=True): every BatchNorm2d of the model normalises over all ranks) --
// without a host synchronisation, without atomics, bitwise repeatable, capturable in a graph.
//
// A channel's N H W elements are numbered j = n H W + p in memory order and cut into S = ceil(N H W / VAMP_BN_CHUNK)
// chunks; one workgroup of 256 takes one (channel, chunk), so the grids (C S workgroups) depend on the shape only.
// A chunk is walked in one of three ways, chosen from H W alone (V = 16 bytes of elements: 4 fp32, 8 bf16 / fp16):
//   flat       H W a multiple of V: every plane starts on a 16-byte boundary (the tensors are 16-byte aligned), a lane
//              takes vectors j = j0 + V (lane + 256 i) and finds their plane by one division.
//   small      otherwise, H W < 32: a lane takes elements j = j0 + lane + 256 i.
//   segmented  otherwise: the chunk's planes one after the other, each as a scalar head up to the next 16-byte
//              boundary (lane q takes element q), 16-byte vectors lane-strided, a scalar tail (lane q, element q).
// A lane adds its elements in the order it meets them, so every sum below has one fixed order per shape.
//
//  stats      bn_stats_kernel: the chunk's count, mean and M2 = sum (x - mean)^2 in float64.  The sums are taken of
//             x - K with K the chunk's first element (0 if that one is not finite): t1 = sum (x - K), t2 = sum (x - K)^2, each difference exact in
//             float64, lanes then the butterfly of wave_reduce.hpp then the waves in index order; mean = K + t1 / cnt,
//             M2 = max(t2 - t1^2 / cnt, 0).  A constant chunk gives mean = K and M2 = 0 exactly, and a channel with
//             |mean| >> sigma loses nothing to cancellation.  S = 1: straight into the row; else into the chunk's slot
//             of the workspace, and bn_merge_stats_kernel (a thread per channel) merges the slots in index order.
//  merge      Chan's formula in float64: n = na + nb, delta = mb - ma, mean = ma + delta (nb / n),
//             M2 = M2a + M2b + delta^2 (na nb / n); the chunks of a rank in index order, the ranks in rank order.
//  apply      bn_apply_kernel: thread 0 of every workgroup merges its channel's `world` rows, var = M2 / n,
//             invstd = 1 / sqrt(var + eps) in float64; mean is kept as two fp32 words mh + ml, scale = fp32(weight
//             invstd).  An element, in fp32: d = (x - mh) - ml; v = fma(d, scale, bias); v = v + residual; y = v <= 0 ?
//             0 : v (a NaN stays, as torch.relu keeps it), rounded once to the element type.  The chunk-0 workgroup of a
//             channel writes saved = (mh, fp32(invstd), ml) and the running statistics, the first workgroup the batch
//             counter.  Evaluation mode takes mean and 1 / sqrt(running_var + eps) from the running statistics.
//  backward   bn_bwd_stats_kernel: dz = y <= 0 ? 0 : dy under ReLU (threshold_backward on the saved output), else dy;
//             sum dz and sum dz d in float64 as above, bn_merge_bwd_kernel over the chunks; grad_bias = sum dz,
//             grad_weight = invstd sum dz d of this rank.  bn_bwd_apply_kernel: the ranks' rows added in rank order,
//             n likewise from the forward rows; k1 = sum dz / n, k2 = invstd^2 sum dz d / n, a = weight invstd;
//             dx = fma(dz, a, fma(d, -a k2, -a k1)) = a (dz - k1 - d k2), grad_residual = dz; every element written once.
#include <cmath>
#include <type_traits>

#include "common.hpp"
#include "wave_reduce.hpp"

namespace vamp {
namespace {

constexpr int kBnBlock = 256;
constexpr int kBnWaves = kBnBlock / 64;
constexpr int kBnSmallPlane = 32;
static_assert(VAMP_BN_CHUNK % (8 * kBnBlock) == 0, "a chunk is whole rounds of the workgroup's 16-byte vectors");
static_assert(sizeof(VampBatchNormDesc) == 64, "VampBatchNormDesc layout: part of the ABI (the binding reads it from include/vampire_hip.h)");

template <int DT>
struct BnElem {
  static constexpr int V = DT == VAMP_F32 ? 4 : 8;
};

template <int DT>
__device__ __forceinline__ float bn_ld(const void* p, long i) {
  if constexpr (DT == VAMP_F32) return static_cast<const float*>(p)[i];
  else if constexpr (DT == VAMP_BF16) return bf16_to_f32(static_cast<const uint16_t*>(p)[i]);
  else return f16_to_f32(static_cast<const uint16_t*>(p)[i]);
}

template <int DT>
__device__ __forceinline__ void bn_st(void* p, long i, float v) {
  if constexpr (DT == VAMP_F32) static_cast<float*>(p)[i] = v;
  else static_cast<uint16_t*>(p)[i] = f32_to_e16<DT == VAMP_F16>(v);
}

template <int DT>
__device__ __forceinline__ float bn_e16(uint32_t half) {
  if constexpr (DT == VAMP_BF16) return bf16_to_f32((uint16_t) half);
  else return f16_to_f32((uint16_t) half);
}

// CNT elements from element i on: one 16-byte access for CNT = V (i a multiple of V, p 16-byte aligned), else one element
template <int DT, int CNT>
__device__ __forceinline__ void bn_load(const void* p, long i, float (&v)[CNT]) {
  if constexpr (CNT == 1) {
    v[0] = bn_ld<DT>(p, i);
  } else if constexpr (DT == VAMP_F32) {
    const float4 w = *reinterpret_cast<const float4*>(static_cast<const float*>(p) + i);
    v[0] = w.x; v[1] = w.y; v[2] = w.z; v[3] = w.w;
  } else {
    const uint4 w = *reinterpret_cast<const uint4*>(static_cast<const uint16_t*>(p) + i);
    const uint32_t u[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      v[2 * q] = bn_e16<DT>(u[q] & 0xffffu);
      v[2 * q + 1] = bn_e16<DT>(u[q] >> 16);
    }
  }
}

template <int DT, int CNT>
__device__ __forceinline__ void bn_store(void* p, long i, const float (&v)[CNT]) {
  if constexpr (CNT == 1) {
    bn_st<DT>(p, i, v[0]);
  } else if constexpr (DT == VAMP_F32) {
    *reinterpret_cast<float4*>(static_cast<float*>(p) + i) = make_float4(v[0], v[1], v[2], v[3]);
  } else {
    uint32_t u[4];
#pragma unroll
    for (int q = 0; q < 4; ++q)
      u[q] = (uint32_t) f32_to_e16<DT == VAMP_F16>(v[2 * q]) | ((uint32_t) f32_to_e16<DT == VAMP_F16>(v[2 * q + 1]) << 16);
    *reinterpret_cast<uint4*>(static_cast<uint16_t*>(p) + i) = make_uint4(u[0], u[1], u[2], u[3]);
  }
}

struct BnShape {
  int C, HW, NHW, S;              // S chunks per channel
};

// the workgroup's channel and the range [j0, j1) of its chunk
__device__ __forceinline__ void bn_chunk(const BnShape& sh, int& c, int& s, int& j0, int& j1) {
  c = (int) (blockIdx.x / (unsigned) sh.S);
  s = (int) (blockIdx.x - (unsigned) c * (unsigned) sh.S);
  const long b = (long) s * VAMP_BN_CHUNK;
  j0 = (int) b;
  j1 = (int) (b + VAMP_BN_CHUNK < (long) sh.NHW ? b + VAMP_BN_CHUNK : (long) sh.NHW);
}

// (j < 2^31: 32-bit unsigned divisions, and j + one stride of the loops below stays under 2^32)
__device__ __forceinline__ long bn_offset(const BnShape& sh, int c, unsigned j) {
  const unsigned n = j / (unsigned) sh.HW;
  return ((long) n * sh.C + c) * (long) sh.HW + (long) (j - n * (unsigned) sh.HW);
}

// f(element offset, integral_constant<int, 1 | V>) over the chunk [j0, j1) of channel c (the file comment's three walks)
template <int V, typename F>
__device__ __forceinline__ void bn_walk(const BnShape& sh, int c, int j0, int j1, F&& f) {
  const int tid = (int) threadIdx.x;
  constexpr std::integral_constant<int, 1> one{};
  constexpr std::integral_constant<int, V> vec{};
  if (sh.HW % V == 0) {                                         // (uniform per launch, as the two branches below)
#pragma unroll 2
    for (unsigned j = (unsigned) j0 + (unsigned) tid * V; j < (unsigned) j1; j += kBnBlock * V) f(bn_offset(sh, c, j), vec);
    return;
  }
  if (sh.HW < kBnSmallPlane) {
    for (unsigned j = (unsigned) j0 + (unsigned) tid; j < (unsigned) j1; j += kBnBlock) f(bn_offset(sh, c, j), one);
    return;
  }
  for (int j = j0; j < j1;) {
    const int n = j / sh.HW, p0 = j - n * sh.HW;
    const int len = sh.HW - p0 < j1 - j ? sh.HW - p0 : j1 - j;
    const long off = ((long) n * sh.C + c) * sh.HW + p0;
    int head = (int) ((V - (off & (V - 1))) & (V - 1));
    head = head < len ? head : len;
    const int nvec = (len - head) / V, tail = len - head - nvec * V;
    if (tid < head) f(off + tid, one);
#pragma unroll 2
    for (int v = tid; v < nvec; v += kBnBlock) f(off + head + (long) v * V, vec);
    if (tid < tail) f(off + head + (long) nvec * V + tid, one);
    j += len;
  }
}

__device__ __forceinline__ void bn_chan(double& n, double& mean, double& m2, double nb, double mb, double m2b) {
  const double nt = n + nb, delta = mb - mean;
  mean = mean + delta * (nb / nt);
  m2 = m2 + m2b + delta * delta * (n * nb / nt);
  n = nt;
}

// ---------------------------------------------------------------------------------------------------------
// forward
// ---------------------------------------------------------------------------------------------------------
template <int DT>
__global__ void __launch_bounds__(kBnBlock) bn_stats_kernel(const void* __restrict__ x, double* __restrict__ slots,
                                                            double* __restrict__ row, BnShape sh) {
  constexpr int V = BnElem<DT>::V;
  __shared__ double red[kBnWaves];
  int c, s, j0, j1;
  bn_chunk(sh, c, s, j0, j1);
  // (a first element of +-inf or NaN is no pivot: x - K would be NaN for the +-inf itself and the mean NaN, where the
  // mean of a channel that holds one +-inf is that +-inf)
  const double K0 = (double) bn_ld<DT>(x, bn_offset(sh, c, (unsigned) j0));
  const double K = K0 - K0 == 0.0 ? K0 : 0.0;
  double s1 = 0.0, s2 = 0.0;
  bn_walk<V>(sh, c, j0, j1, [&](long off, auto cnt) {
    constexpr int CNT = decltype(cnt)::value;
    float v[CNT];
    bn_load<DT, CNT>(x, off, v);
#pragma unroll
    for (int q = 0; q < CNT; ++q) {
      const double d = (double) v[q] - K;
      s1 += d;
      s2 += d * d;
    }
  });
  const double t1 = block_sum<kBnWaves>(s1, red);
  const double t2 = block_sum<kBnWaves>(s2, red);
  if (threadIdx.x != 0) return;
  const double cnt = (double) (j1 - j0);
  const double mean = K + t1 / cnt;
  double m2 = t2 - t1 * t1 / cnt;
  m2 = m2 < 0.0 ? 0.0 : m2;                                     // (a NaN stays)
  if (sh.S == 1) {
    if (c == 0) row[0] = cnt;
    row[1 + 2 * c] = mean;
    row[2 + 2 * c] = m2;
  } else {
    double* o = slots + 3 * (size_t) blockIdx.x;
    o[0] = cnt;
    o[1] = mean;
    o[2] = m2;
  }
}

__global__ void __launch_bounds__(kBnBlock) bn_merge_stats_kernel(const double* __restrict__ slots,
                                                                  double* __restrict__ row, BnShape sh) {
  const int c = (int) (blockIdx.x * kBnBlock + threadIdx.x);
  if (c >= sh.C) return;
  const double* p = slots + 3 * (size_t) c * sh.S;
  double n = p[0], mean = p[1], m2 = p[2];
  for (int s = 1; s < sh.S; ++s) bn_chan(n, mean, m2, p[3 * s], p[3 * s + 1], p[3 * s + 2]);
  if (c == 0) row[0] = n;
  row[1 + 2 * c] = mean;
  row[2 + 2 * c] = m2;
}

struct BnApply {
  const void* x;
  const void* res;
  void* y;
  const double* rows;             // [world, 2 C + 1]; training only
  const float *weight, *bias;
  float *rmean, *rvar;
  long long* nbt;
  float* saved;                   // [3, C]: mean (high word), invstd, mean (low word); may be null
  double eps, momentum;
  int world, training, update;
  BnShape sh;
};

template <int DT, bool RELU, bool RES>
__global__ void __launch_bounds__(kBnBlock) bn_apply_kernel(BnApply a) {
  constexpr int V = BnElem<DT>::V;
  __shared__ float par[4];
  const BnShape sh = a.sh;
  int c, s, j0, j1;
  bn_chunk(sh, c, s, j0, j1);
  if (threadIdx.x == 0) {
    double mean, invstd;
    if (a.training) {
      const size_t K = 2 * (size_t) sh.C + 1;
      double n = a.rows[0], m2 = a.rows[2 + 2 * c];
      mean = a.rows[1 + 2 * c];
      for (int r = 1; r < a.world; ++r) bn_chan(n, mean, m2, a.rows[r * K], a.rows[r * K + 1 + 2 * c], a.rows[r * K + 2 + 2 * c]);
      const double var = m2 / n;
      invstd = 1.0 / sqrt(var + a.eps);
      if (s == 0 && a.update) {                                 // (one workgroup per channel writes them)
        const double unbiased = n > 1.0 ? var * (n / (n - 1.0)) : var;
        a.rmean[c] = (float) ((1.0 - a.momentum) * (double) a.rmean[c] + a.momentum * mean);
        a.rvar[c] = (float) ((1.0 - a.momentum) * (double) a.rvar[c] + a.momentum * unbiased);
      }
      if (blockIdx.x == 0 && a.nbt) a.nbt[0] += 1;
    } else {
      mean = (double) a.rmean[c];
      invstd = 1.0 / sqrt((double) a.rvar[c] + a.eps);
    }
    const float mh = (float) mean, ml = (float) (mean - (double) mh);
    par[0] = mh;
    par[1] = ml == ml ? ml : 0.0f;                              // (a mean of +-inf: inf - inf)
    par[2] = (float) ((double) a.weight[c] * invstd);
    par[3] = a.bias[c];
    if (s == 0 && a.saved) {
      a.saved[c] = mh;
      a.saved[sh.C + c] = (float) invstd;
      a.saved[2 * (size_t) sh.C + c] = par[1];
    }
  }
  __syncthreads();
  const float mh = par[0], ml = par[1], sc = par[2], b = par[3];
  bn_walk<V>(sh, c, j0, j1, [&](long off, auto cnt) {
    constexpr int CNT = decltype(cnt)::value;
    float v[CNT], r[CNT];
    bn_load<DT, CNT>(a.x, off, v);
    if constexpr (RES) bn_load<DT, CNT>(a.res, off, r);
#pragma unroll
    for (int q = 0; q < CNT; ++q) {
      float t = __builtin_fmaf((v[q] - mh) - ml, sc, b);
      if constexpr (RES) t = t + r[q];
      if constexpr (RELU) t = t <= 0.0f ? 0.0f : t;
      v[q] = t;
    }
    bn_store<DT, CNT>(a.y, off, v);
  });
}

// ---------------------------------------------------------------------------------------------------------
// backward
// ---------------------------------------------------------------------------------------------------------
struct BnBwdStats {
  const void *dy, *x, *y;
  const float* saved;
  double *slots, *row;            // row [2 C]
  float *gw, *gb;
  BnShape sh;
};

template <int DT, bool RELU>
__global__ void __launch_bounds__(kBnBlock) bn_bwd_stats_kernel(BnBwdStats a) {
  constexpr int V = BnElem<DT>::V;
  __shared__ double red[kBnWaves];
  const BnShape sh = a.sh;
  int c, s, j0, j1;
  bn_chunk(sh, c, s, j0, j1);
  const float mh = a.saved[c], ml = a.saved[2 * (size_t) sh.C + c];
  double s1 = 0.0, s2 = 0.0;
  bn_walk<V>(sh, c, j0, j1, [&](long off, auto cnt) {
    constexpr int CNT = decltype(cnt)::value;
    float g[CNT], v[CNT], o[CNT];
    bn_load<DT, CNT>(a.dy, off, g);
    bn_load<DT, CNT>(a.x, off, v);
    if constexpr (RELU) bn_load<DT, CNT>(a.y, off, o);
#pragma unroll
    for (int q = 0; q < CNT; ++q) {
      float dz = g[q];
      if constexpr (RELU) dz = o[q] <= 0.0f ? 0.0f : dz;
      const float d = (v[q] - mh) - ml;
      s1 += (double) dz;
      s2 += (double) dz * (double) d;
    }
  });
  const double t1 = block_sum<kBnWaves>(s1, red);
  const double t2 = block_sum<kBnWaves>(s2, red);
  if (threadIdx.x != 0) return;
  if (sh.S == 1) {
    a.row[2 * c] = t1;
    a.row[2 * c + 1] = t2;
    a.gb[c] = (float) t1;
    a.gw[c] = (float) ((double) a.saved[sh.C + c] * t2);
  } else {
    a.slots[2 * (size_t) blockIdx.x] = t1;
    a.slots[2 * (size_t) blockIdx.x + 1] = t2;
  }
}

__global__ void __launch_bounds__(kBnBlock) bn_merge_bwd_kernel(BnBwdStats a) {
  const BnShape sh = a.sh;
  const int c = (int) (blockIdx.x * kBnBlock + threadIdx.x);
  if (c >= sh.C) return;
  const double* p = a.slots + 2 * (size_t) c * sh.S;
  double t1 = 0.0, t2 = 0.0;
  for (int s = 0; s < sh.S; ++s) {
    t1 += p[2 * s];
    t2 += p[2 * s + 1];
  }
  a.row[2 * c] = t1;
  a.row[2 * c + 1] = t2;
  a.gb[c] = (float) t1;
  a.gw[c] = (float) ((double) a.saved[sh.C + c] * t2);
}

struct BnBwdApply {
  const void *dy, *x, *y;
  const float *saved, *weight;
  const double* rows;             // [world, 2 C]
  const double* stat_rows;        // [world, 2 C + 1]: the forward's rows, for the global n
  void *dx, *gres;
  int world;
  BnShape sh;
};

template <int DT, bool RELU, bool RES>
__global__ void __launch_bounds__(kBnBlock) bn_bwd_apply_kernel(BnBwdApply a) {
  constexpr int V = BnElem<DT>::V;
  __shared__ float par[5];
  const BnShape sh = a.sh;
  int c, s, j0, j1;
  bn_chunk(sh, c, s, j0, j1);
  if (threadIdx.x == 0) {
    double t1 = 0.0, t2 = 0.0, n = 0.0;
    for (int r = 0; r < a.world; ++r) {
      t1 += a.rows[(size_t) r * 2 * sh.C + 2 * c];
      t2 += a.rows[(size_t) r * 2 * sh.C + 2 * c + 1];
      n += a.stat_rows[(size_t) r * (2 * (size_t) sh.C + 1)];
    }
    const double invstd = (double) a.saved[sh.C + c];
    const double aa = (double) a.weight[c] * invstd;
    const double k1 = t1 / n, k2 = invstd * invstd * t2 / n;
    par[0] = a.saved[c];
    par[1] = a.saved[2 * (size_t) sh.C + c];
    par[2] = (float) aa;
    par[3] = (float) (-aa * k2);
    par[4] = (float) (-aa * k1);
  }
  __syncthreads();
  const float mh = par[0], ml = par[1], A = par[2], B = par[3], K0 = par[4];
  bn_walk<V>(sh, c, j0, j1, [&](long off, auto cnt) {
    constexpr int CNT = decltype(cnt)::value;
    float g[CNT], v[CNT], o[CNT];
    bn_load<DT, CNT>(a.dy, off, g);
    bn_load<DT, CNT>(a.x, off, v);
    if constexpr (RELU) bn_load<DT, CNT>(a.y, off, o);
#pragma unroll
    for (int q = 0; q < CNT; ++q) {
      if constexpr (RELU) g[q] = o[q] <= 0.0f ? 0.0f : g[q];
      v[q] = __builtin_fmaf(g[q], A, __builtin_fmaf((v[q] - mh) - ml, B, K0));
    }
    bn_store<DT, CNT>(a.dx, off, v);
    if constexpr (RES) bn_store<DT, CNT>(a.gres, off, g);
  });
}

// ---------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------
int bn_validate(const VampBatchNormDesc* d) {
  VAMP_REQUIRE(d, "desc is NULL");
  VAMP_REQUIRE(d->C >= 1, "C must be at least 1");
  VAMP_REQUIRE(d->N >= 1 && d->H >= 1 && d->W >= 1, "N, H and W must be at least 1");
  VAMP_REQUIRE((long) d->H * (long) d->W < (1L << 31) && (long) d->N * (long) d->H * (long) d->W < (1L << 31),
               "N H W must be below 2^31");
  VAMP_REQUIRE(d->world >= 1 && d->world <= VAMP_BN_MAX_WORLD, "world must be in 1 .. 64");
  VAMP_REQUIRE(d->dtype == VAMP_F32 || d->dtype == VAMP_BF16 || d->dtype == VAMP_F16,
               "dtype must be VAMP_F32, VAMP_BF16 or VAMP_F16");
  VAMP_REQUIRE(d->act == VAMP_BN_ACT_NONE || d->act == VAMP_BN_ACT_RELU, "act must be a VAMP_BN_ACT_* value");
  VAMP_REQUIRE(d->has_residual == 0 || d->has_residual == 1, "has_residual must be 0 or 1");
  VAMP_REQUIRE(d->training == 0 || d->training == 1, "training must be 0 or 1");
  VAMP_REQUIRE(d->update_running == 0 || d->update_running == 1, "update_running must be 0 or 1");
  VAMP_REQUIRE(d->eps == d->eps && d->eps >= 0.0, "eps must not be negative");
  VAMP_REQUIRE(d->momentum >= 0.0 && d->momentum <= 1.0, "momentum must be in [0, 1]");
  VAMP_REQUIRE(d->reserved[0] == 0 && d->reserved[1] == 0, "reserved must be 0");
  const long nhw = (long) d->N * d->H * d->W, chunks = (nhw + VAMP_BN_CHUNK - 1) / VAMP_BN_CHUNK;
  VAMP_REQUIRE(chunks * (long) d->C < (1L << 31), "C ceil(N H W / VAMP_BN_CHUNK) must be below 2^31");
  return VAMP_OK;
}

inline BnShape bn_shape(const VampBatchNormDesc* d) {
  const long hw = (long) d->H * d->W, nhw = hw * d->N;
  return BnShape{d->C, (int) hw, (int) nhw, (int) ((nhw + VAMP_BN_CHUNK - 1) / VAMP_BN_CHUNK)};
}

// f(integral_constant<int, DT>) for the descriptor's element type, f(true_type | false_type) for a flag
template <typename F>
inline void bn_by_dtype(int dtype, F&& f) {
  if (dtype == VAMP_F32) f(std::integral_constant<int, VAMP_F32>{});
  else if (dtype == VAMP_BF16) f(std::integral_constant<int, VAMP_BF16>{});
  else f(std::integral_constant<int, VAMP_F16>{});
}

template <typename F>
inline void bn_by_flag(bool flag, F&& f) {
  if (flag) f(std::true_type{});
  else f(std::false_type{});
}

}  // namespace
}  // namespace vamp

using namespace vamp;

extern "C" {

size_t vamp_bn_workspace_bytes(const VampBatchNormDesc* d) {
  if (bn_validate(d)) return 0;
  const BnShape sh = bn_shape(d);
  return align_up((size_t) sh.C * (size_t) sh.S * 3 * sizeof(double), 256);
}

int vamp_bn_partial_stats(const VampBatchNormDesc* d, const void* x, double* row, void* workspace,
                          size_t workspace_bytes, void* stream) {
  if (int e = bn_validate(d)) return e;
  VAMP_REQUIRE(x && row, "x or row is NULL");
  VAMP_REQUIRE(aligned(x, 16), "x must be 16-byte aligned");
  VAMP_REQUIRE(aligned(row, 8), "the float64 row must be 8-byte aligned");
  if (int e = workspace_fits(__func__, workspace, workspace_bytes, vamp_bn_workspace_bytes(d))) return e;
  VAMP_REQUIRE(aligned(workspace, 8), "the workspace must be 8-byte aligned");
  hipStream_t st = static_cast<hipStream_t>(stream);
  const BnShape sh = bn_shape(d);
  double* slots = static_cast<double*>(workspace);
  const unsigned grid = (unsigned) sh.C * (unsigned) sh.S;
  bn_by_dtype(d->dtype, [&](auto dt) {
    VAMP_TIMED(kProfAux, st, (bn_stats_kernel<decltype(dt)::value><<<grid, kBnBlock, 0, st>>>(x, slots, row, sh)));
  });
  if (sh.S > 1)
    VAMP_TIMED(kProfAux, st,
               (bn_merge_stats_kernel<<<(unsigned) ((sh.C + kBnBlock - 1) / kBnBlock), kBnBlock, 0, st>>>(slots, row, sh)));
  return check_launch("bn_partial_stats");
}

int vamp_bn_apply(const VampBatchNormDesc* d, const void* x, const void* residual, const double* rows,
                  const float* weight, const float* bias, float* running_mean, float* running_var,
                  int64_t* num_batches_tracked, void* y, float* saved, void* stream) {
  if (int e = bn_validate(d)) return e;
  VAMP_REQUIRE(!d->has_residual || residual, "has_residual is set but residual is NULL");
  VAMP_REQUIRE(x && y && weight && bias, "x, y, weight or bias is NULL");
  VAMP_REQUIRE(aligned(x, 16) && aligned(y, 16) && aligned(residual, 16),
               "x, y and residual must be 16-byte aligned");
  if (d->training) {
    VAMP_REQUIRE(rows, "training needs the float64 rows");
    VAMP_REQUIRE(aligned(rows, 8), "the float64 rows must be 8-byte aligned");
    VAMP_REQUIRE(saved, "training needs saved");
    VAMP_REQUIRE(!d->update_running || (running_mean && running_var), "update_running needs running_mean and running_var");
  } else {
    VAMP_REQUIRE(running_mean && running_var, "evaluation needs running_mean and running_var");
    VAMP_REQUIRE(!d->update_running, "update_running needs training");
  }
  VAMP_REQUIRE(aligned(num_batches_tracked, 8), "num_batches_tracked must be 8-byte aligned");
  hipStream_t st = static_cast<hipStream_t>(stream);
  const BnShape sh = bn_shape(d);
  BnApply a{x, d->has_residual ? residual : nullptr, y, rows, weight, bias, running_mean, running_var,
            d->training ? reinterpret_cast<long long*>(num_batches_tracked) : nullptr, saved, d->eps, d->momentum,
            d->world, d->training, d->update_running, sh};
  const unsigned grid = (unsigned) sh.C * (unsigned) sh.S;
  bn_by_dtype(d->dtype, [&](auto dt) {
    bn_by_flag(d->act == VAMP_BN_ACT_RELU, [&](auto relu) {
      bn_by_flag(d->has_residual != 0, [&](auto res) {
        VAMP_TIMED(kProfAux, st, (bn_apply_kernel<decltype(dt)::value, decltype(relu)::value, decltype(res)::value>
                                  <<<grid, kBnBlock, 0, st>>>(a)));
      });
    });
  });
  return check_launch("bn_apply");
}

int vamp_bn_backward_partial(const VampBatchNormDesc* d, const void* dy, const void* x, const void* y,
                             const float* saved, double* row, float* grad_weight, float* grad_bias, void* workspace,
                             size_t workspace_bytes, void* stream) {
  if (int e = bn_validate(d)) return e;
  VAMP_REQUIRE(d->training, "the backward needs training statistics (evaluation mode has no backward)");
  VAMP_REQUIRE(dy && x && saved && row && grad_weight && grad_bias, "dy, x, saved, row, grad_weight or grad_bias is NULL");
  VAMP_REQUIRE(d->act == VAMP_BN_ACT_NONE || y, "act VAMP_BN_ACT_RELU needs the saved output y");
  VAMP_REQUIRE(aligned(dy, 16) && aligned(x, 16) && aligned(y, 16), "dy, x and y must be 16-byte aligned");
  VAMP_REQUIRE(aligned(row, 8), "the float64 row must be 8-byte aligned");
  if (int e = workspace_fits(__func__, workspace, workspace_bytes, vamp_bn_workspace_bytes(d))) return e;
  VAMP_REQUIRE(aligned(workspace, 8), "the workspace must be 8-byte aligned");
  hipStream_t st = static_cast<hipStream_t>(stream);
  const BnShape sh = bn_shape(d);
  BnBwdStats a{dy, x, y, saved, static_cast<double*>(workspace), row, grad_weight, grad_bias, sh};
  const unsigned grid = (unsigned) sh.C * (unsigned) sh.S;
  bn_by_dtype(d->dtype, [&](auto dt) {
    bn_by_flag(d->act == VAMP_BN_ACT_RELU, [&](auto relu) {
      VAMP_TIMED(kProfAux, st,
                 (bn_bwd_stats_kernel<decltype(dt)::value, decltype(relu)::value><<<grid, kBnBlock, 0, st>>>(a)));
    });
  });
  if (sh.S > 1)
    VAMP_TIMED(kProfAux, st, (bn_merge_bwd_kernel<<<(unsigned) ((sh.C + kBnBlock - 1) / kBnBlock), kBnBlock, 0, st>>>(a)));
  return check_launch("bn_backward_partial");
}

int vamp_bn_backward_apply(const VampBatchNormDesc* d, const void* dy, const void* x, const void* y,
                           const float* saved, const float* weight, const double* rows, const double* stat_rows,
                           void* dx, void* grad_residual, void* stream) {
  if (int e = bn_validate(d)) return e;
  VAMP_REQUIRE(d->training, "the backward needs training statistics (evaluation mode has no backward)");
  VAMP_REQUIRE(!d->has_residual || grad_residual, "has_residual is set but grad_residual is NULL");
  VAMP_REQUIRE(dy && x && saved && weight && rows && stat_rows && dx, "dy, x, saved, weight, rows, stat_rows or dx is NULL");
  VAMP_REQUIRE(d->act == VAMP_BN_ACT_NONE || y, "act VAMP_BN_ACT_RELU needs the saved output y");
  VAMP_REQUIRE(aligned(dy, 16) && aligned(x, 16) && aligned(y, 16) && aligned(dx, 16) &&
               aligned(grad_residual, 16), "dy, x, y, dx and grad_residual must be 16-byte aligned");
  VAMP_REQUIRE(aligned(rows, 8) && aligned(stat_rows, 8), "the float64 rows must be 8-byte aligned");
  hipStream_t st = static_cast<hipStream_t>(stream);
  const BnShape sh = bn_shape(d);
  BnBwdApply a{dy, x, y, saved, weight, rows, stat_rows, dx, d->has_residual ? grad_residual : nullptr, d->world, sh};
  const unsigned grid = (unsigned) sh.C * (unsigned) sh.S;
  bn_by_dtype(d->dtype, [&](auto dt) {
    bn_by_flag(d->act == VAMP_BN_ACT_RELU, [&](auto relu) {
      bn_by_flag(d->has_residual != 0, [&](auto res) {
        VAMP_TIMED(kProfAux, st, (bn_bwd_apply_kernel<decltype(dt)::value, decltype(relu)::value, decltype(res)::value>
                                  <<<grid, kBnBlock, 0, st>>>(a)));
      });
    });
  });
  return check_launch("bn_backward_apply");
}

}  // extern "C"
