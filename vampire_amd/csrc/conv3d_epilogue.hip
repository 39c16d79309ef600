// The backward of the convolutions' epilogue (conv3d_epilogue.hpp; the contract is in vampire_hip.h), gfx950:
//     g_z = g * act'(y)        leaky: y > 0 ? 1 : slope      sigmoid: y (1 - y)
// One elementwise pass gathers the segments' gradients into ONE [B, cout, Zo, Yo, Xo] tensor of the compute type --
// the operand of the existing backward_data / backward_weight kernels and the residual's gradient -- and leaves, per
// (channel, sample, chunk of VAMP_CONV_EPI_CHUNK voxels), the float64 sum of the g_z it wrote (as rounded; for an
// fp32-output segment of a 16-bit kind the fp32 products themselves).  A finishing
// launch adds a channel's partials in a fixed order and rounds once to fp32: grad_bias, no atomics.
#include "conv3d_epilogue.hpp"

namespace vamp {
namespace {

constexpr int kChunk = VAMP_CONV_EPI_CHUNK;
constexpr int kThreads = 256;

struct OutVol {
  long plane;        // Zo * Yo * Xo
  bool ok;
};

OutVol out_volume(const VampConvDesc* d, int stride) {
  if (!d || (stride != 1 && stride != 2) || d->B <= 0 || d->Z <= 0 || d->Y <= 0 || d->X <= 0 || d->cout <= 0 ||
      d->cout > 32 || d->B > 65535)
    return OutVol{0, false};
  const long zo = (d->Z - 1) / stride + 1, yo = (d->Y - 1) / stride + 1, xo = (d->X - 1) / stride + 1;
  return OutVol{zo * yo * xo, true};
}

int nchunks_of(long plane) { return (int) ((plane + kChunk - 1) / kChunk); }

// the 256 partial sums of a workgroup, added pairwise in a fixed tree; the total is thread 0's return value
__device__ __forceinline__ double block_sum(double v, double* red) {
  red[threadIdx.x] = v;
  __syncthreads();
#pragma unroll
  for (int o = kThreads / 2; o > 0; o >>= 1) {
    if ((int) threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  return red[0];
}

// grid (chunks, cout, B).  part[(c * B + b) * nchunks + chunk], or nullptr: no segment wants a bias gradient.
template <int KIND>
__global__ void __launch_bounds__(kThreads)
conv3d_epi_bwd_kernel(VampConvEpilogue ep, int cout, long plane, void* __restrict__ gz, double* __restrict__ part,
                      int nchunks) {
  __shared__ double red[kThreads];
  const int chunk = blockIdx.x, c = blockIdx.y, b = blockIdx.z;
  const EpiSel sel = epi_select(ep, c);                 // workgroup-uniform
  const long zb = ((long) b * cout + c) * plane;
  const long sb = ((long) b * sel.nch + sel.cc) * plane;
  double sum = 0.0;
#pragma unroll 4
  for (int i = 0; i < kChunk / kThreads; ++i) {
    const long v = (long) chunk * kChunk + i * kThreads + threadIdx.x;
    if (v >= plane) break;
    float r = 0.f;
    if (sel.hit) {
      const float g = epi_load<KIND>(sel.grad_out, sb + v, sel.f32);
      if (sel.act == VAMP_ACT_LEAKY_RELU) {
        const float y = epi_load<KIND>(sel.out, sb + v, sel.f32);
        r = y > 0.f ? g : g * sel.slope;
      } else if (sel.act == VAMP_ACT_SIGMOID) {
        const float y = epi_load<KIND>(sel.out, sb + v, sel.f32);
        r = (g * (1.f - y)) * y;
      } else {
        r = g;
      }
    }
    epi_put<KIND>(gz, zb + v, 0, r);
    // the bias sees what its segment's precision holds: the rounded g_z of a compute-type segment, the fp32 product
    // of an fp32-output segment of a 16-bit kind (whose copy in grad_z is rounded for the convolution's backward only)
    if (KIND != kEpiF32 && !sel.f32) r = KIND == kEpiF16 ? f16_to_f32(f32_to_f16(r)) : bf16_to_f32(f32_to_bf16(r));
    sum += (double) r;
  }
  if (part) {                                           // uniform
    const double tot = block_sum(sum, red);
    if (threadIdx.x == 0) part[((long) c * gridDim.z + b) * nchunks + chunk] = tot;
  }
}

// grid (cout), 64 threads: lane l adds partials l, l + 64, ... of its channel, the 64 sums meet in a fixed tree
__global__ void __launch_bounds__(64)
conv3d_epi_bias_kernel(VampConvEpilogue ep, const double* __restrict__ part, int per_channel) {
  __shared__ double red[64];
  const int c = blockIdx.x;
  float* gb = nullptr;
  int cc = 0;
#pragma unroll
  for (int i = 0; i < VAMP_CONV_EPI_MAX_SEGS; ++i)
    if (i < ep.nseg && c >= ep.seg[i].c0 && c < ep.seg[i].c0 + ep.seg[i].nch) {
      gb = ep.seg[i].grad_bias;
      cc = c - ep.seg[i].c0;
    }
  if (!gb) return;                                      // uniform
  double s = 0.0;
  for (int k = threadIdx.x; k < per_channel; k += 64) s += part[(long) c * per_channel + k];
  red[threadIdx.x] = s;
  __syncthreads();
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    if ((int) threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) gb[cc] = (float) red[0];
}

}  // namespace
}  // namespace vamp

using namespace vamp;

extern "C" {

// the kind (stride, dtype) names exists and takes the descriptor
static int kind_takes(const VampConvDesc* d, int32_t stride, int32_t dtype) {
  char keep[sizeof(g_err)];
  memcpy(keep, g_err, sizeof(keep));
  const bool half = dtype == VAMP_BF16 || dtype == VAMP_F16;
  int ok = 0;
  if (stride == 1 && dtype == VAMP_F32) ok = vamp_conv3d_supported(d);
  else if (stride == 1 && half) ok = vamp_conv3d_bf16_supported(d);
  else if (stride == 2 && half) ok = vamp_conv3d_half_s2_supported(d);
  memcpy(g_err, keep, sizeof(keep));
  return ok && out_volume(d, stride).ok;
}

// a question, not a call that can fail: the answer "no" leaves vamp_last_error as it was
int vamp_conv3d_epilogue_supported(const VampConvDesc* d, int32_t stride, int32_t dtype, const VampConvEpilogue* epi) {
  char keep[sizeof(g_err)];
  memcpy(keep, g_err, sizeof(keep));
  const bool half = dtype == VAMP_BF16 || dtype == VAMP_F16;
  const int ok = kind_takes(d, stride, dtype) && epi_check(__func__, d, epi, half, 0) == VAMP_OK;
  memcpy(g_err, keep, sizeof(keep));
  return ok;
}

size_t vamp_conv3d_epilogue_workspace_bytes(const VampConvDesc* d, int32_t stride) {
  const OutVol v = out_volume(d, stride);
  if (!v.ok) return 0;
  return align_up((size_t) d->cout * d->B * nchunks_of(v.plane) * sizeof(double), 256);
}

int vamp_conv3d_epilogue_backward(const VampConvDesc* d, int32_t stride, int32_t dtype, const VampConvEpilogue* epi,
                                  void* grad_z, void* workspace, size_t workspace_bytes, void* stream) {
  const bool half = dtype == VAMP_BF16 || dtype == VAMP_F16;
  VAMP_REQUIRE(half || dtype == VAMP_F32, "dtype must be VAMP_F32, VAMP_BF16 or VAMP_F16");
  VAMP_REQUIRE(kind_takes(d, stride, dtype), "no kind takes this descriptor, stride and dtype: see vamp_conv3d_epilogue_supported");
  if (int e = epi_check(__func__, d, epi, half, 2)) return e;
  VAMP_REQUIRE(grad_z != nullptr, "NULL grad_z");
  bool want_bias = false;
  for (int i = 0; i < epi->nseg; ++i) want_bias = want_bias || epi->seg[i].grad_bias != nullptr;
  const OutVol v = out_volume(d, stride);
  const int nchunks = nchunks_of(v.plane);
  if (want_bias) {
    const size_t need = vamp_conv3d_epilogue_workspace_bytes(d, stride);
    if (int e = workspace_fits(__func__, workspace, workspace_bytes, need)) return e;
  }
  hipStream_t s = static_cast<hipStream_t>(stream);
  double* part = want_bias ? static_cast<double*>(workspace) : nullptr;
  const dim3 grid((unsigned) nchunks, (unsigned) d->cout, (unsigned) d->B);
  if (dtype == VAMP_F32) conv3d_epi_bwd_kernel<kEpiF32><<<grid, kThreads, 0, s>>>(*epi, d->cout, v.plane, grad_z, part, nchunks);
  else if (dtype == VAMP_F16) conv3d_epi_bwd_kernel<kEpiF16><<<grid, kThreads, 0, s>>>(*epi, d->cout, v.plane, grad_z, part, nchunks);
  else conv3d_epi_bwd_kernel<kEpiBF16><<<grid, kThreads, 0, s>>>(*epi, d->cout, v.plane, grad_z, part, nchunks);
  if (int e = check_launch("conv3d_epi_bwd_kernel")) return e;
  if (want_bias) {
    conv3d_epi_bias_kernel<<<d->cout, 64, 0, s>>>(*epi, part, d->B * nchunks);
    return check_launch("conv3d_epi_bias_kernel");
  }
  return VAMP_OK;
}

}  // extern "C"
