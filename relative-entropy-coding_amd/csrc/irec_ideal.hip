// irec_ideal.hip -- the ideal half of a results row on the device and on the host (include/irec.h: irec_posterior_draw_*,
// irec_loglik_*): a seeded draw from a batch's posteriors with its KL, and the discretized-logistic log-likelihood of a batch.  The
// noise, the per-element arithmetic, what a lane does and the order of every sum are csrc/irec_ideal_core.h; the kernels here run a
// tile's 256 lanes and add their sums, and the host entry points at the end of this file run the same lanes over host memory.
//
// Both kernels move little per element (the draw: 16 B in, 4 B out): one 256-lane workgroup per (image, tile of 4096 elements), every
// lane four runs of 4 consecutive elements -- one Philox block and, where the pointers and dims allow, one 16-byte access per array
// and run.  A tile's float64 partial goes to workspace[image][tile]; ideal_finish_kernel, a lane per image, adds an image's partials
// in tile order.  No atomics: every store goes to an address that only its lane owns.  Measured (profiles/ideal/bench.json): the draw
// reaches 12 % of HBM peak on 300 images of 24 tensors, so the float64 arithmetic per element binds, not memory.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <exception>
#include <vector>

#include "irec_call.h"
#include "irec_ideal_core.h"

namespace irec {
namespace {
namespace I = irec_ideal;

// core.h's tile_sum over the workgroup's lanes: the tree of a wave (partners at distance 32 .. 1), then the wave sums in order
__device__ __forceinline__ void store_tile_sum(double v, double *wave_sum, double *out) {
#pragma unroll
  for (int off = I::WAVE / 2; off >= 1; off >>= 1) v = v + __shfl_xor(v, off, I::WAVE);
  const int lane = threadIdx.x;
  if ((lane & (I::WAVE - 1)) == 0) wave_sum[lane / I::WAVE] = v;
  __syncthreads();
  if (lane == 0) {
    double s = wave_sum[0];
#pragma unroll
    for (int w = 1; w < I::NT / I::WAVE; ++w) s = s + wave_sum[w];
    *out = s;
  }
}

__global__ __launch_bounds__(I::NT) void ideal_draw_kernel(I::DrawCall c, int64_t tiles) {
  __shared__ double wave_sum[I::NT / I::WAVE];
  const int64_t block = blockIdx.x;
  store_tile_sum(I::draw_lane(c, block / tiles, block % tiles, threadIdx.x), wave_sum, c.partials + block);
}

__global__ __launch_bounds__(I::NT) void ideal_loglik_kernel(I::LoglikCall c, int64_t tiles) {
  __shared__ double wave_sum[I::NT / I::WAVE];
  const int64_t block = blockIdx.x;
  store_tile_sum(I::loglik_lane(c, block / tiles, block % tiles, threadIdx.x), wave_sum, c.partials + block);
}

__global__ __launch_bounds__(I::FINISH_NT) void ideal_finish_kernel(const double *partials, int64_t tiles, int32_t n_images, double *out) {
  const int64_t i = (int64_t)blockIdx.x * I::FINISH_NT + threadIdx.x;
  if (i < n_images) out[i] = I::ordered_sum(partials + i * tiles, tiles);
}

size_t workspace_bytes_of(int64_t n_images, int64_t dims) { return (size_t)(8 * n_images * I::tiles_of(dims)); }

template <class Kernel, class Call>
irec_status launch(Kernel kernel, const Call &call, int32_t n_images, int64_t dims, double *out, hipStream_t st) {
  const int64_t tiles = I::tiles_of(dims);
  hipLaunchKernelGGL(kernel, dim3((unsigned)(n_images * tiles)), dim3(I::NT), 0, st, call, tiles);
  IREC_HIP(hipGetLastError());
  hipLaunchKernelGGL(ideal_finish_kernel, dim3((unsigned)((n_images + I::FINISH_NT - 1) / I::FINISH_NT)), dim3(I::FINISH_NT), 0, st,
                     (const double *)call.partials, tiles, n_images, out);
  IREC_HIP(hipGetLastError());
  return IREC_OK;
}
} // namespace
} // namespace irec

extern "C" {

size_t irec_ideal_workspace_bytes(int32_t n_images, int64_t dims) {
  if (irec_ideal::shape_error(n_images, dims)) return 0;
  return irec::workspace_bytes_of(n_images, dims);
}

irec_status irec_posterior_draw_device(const float *mq, const float *sq, const float *mp, const float *sp, int32_t n_images, int64_t dims,
                                       int64_t seed, uint32_t tag, int64_t image_base, float *sample, double *kl, void *workspace,
                                       size_t workspace_bytes, void *hip_stream) {
  using namespace irec;
  const char *who = "irec_posterior_draw_device";
  if (const char *what = I::draw_error(mq, sq, mp, sp, n_images, dims, image_base, sample, kl)) return set_last_error(IREC_E_INVALID, who, what);
  if (irec_status st = check_workspace(workspace_bytes_of(n_images, dims), workspace, workspace_bytes, who, "irec_ideal_workspace_bytes")) return st;
  I::DrawCall call;
  I::bind(call, mq, sq, mp, sp, n_images, dims, seed, tag, image_base, sample, kl, workspace);
  return launch(ideal_draw_kernel, call, n_images, dims, kl, (hipStream_t)hip_stream);
}

irec_status irec_posterior_draw_host(const float *mq, const float *sq, const float *mp, const float *sp, int32_t n_images, int64_t dims,
                                     int64_t seed, uint32_t tag, int64_t image_base, float *sample, double *kl, int32_t n_threads) try {
  using namespace irec;
  if (const char *what = I::draw_error(mq, sq, mp, sp, n_images, dims, image_base, sample, kl))
    return set_last_error(IREC_E_INVALID, "irec_posterior_draw_host", what);
  std::vector<double> ws(workspace_bytes_of(n_images, dims) / 8);
  I::DrawCall call;
  I::bind(call, mq, sq, mp, sp, n_images, dims, seed, tag, image_base, sample, kl, ws.data());
  I::draw_host(call, Chunks{n_threads, 1});
  return IREC_OK;
} catch (const std::exception &e) { return irec::set_last_error(IREC_E_INVALID, "irec_posterior_draw_host", e.what()); }

irec_status irec_loglik_device(const float *x, const float *loc, const float *log_scales, int32_t n_scales, int32_t n_images,
                               int32_t channels, int64_t plane, double binsize, double *ll, void *workspace, size_t workspace_bytes,
                               void *hip_stream) {
  using namespace irec;
  const char *who = "irec_loglik_device";
  if (const char *what = I::loglik_error(x, loc, log_scales, n_scales, n_images, channels, plane, binsize, ll)) return set_last_error(IREC_E_INVALID, who, what);
  const int64_t dims = (int64_t)channels * plane;
  if (irec_status st = check_workspace(workspace_bytes_of(n_images, dims), workspace, workspace_bytes, who, "irec_ideal_workspace_bytes")) return st;
  I::LoglikCall call;
  I::bind(call, x, loc, log_scales, n_scales, n_images, channels, plane, binsize, ll, workspace);
  return launch(ideal_loglik_kernel, call, n_images, dims, ll, (hipStream_t)hip_stream);
}

irec_status irec_loglik_host(const float *x, const float *loc, const float *log_scales, int32_t n_scales, int32_t n_images, int32_t channels,
                             int64_t plane, double binsize, double *ll, int32_t n_threads) try {
  using namespace irec;
  if (const char *what = I::loglik_error(x, loc, log_scales, n_scales, n_images, channels, plane, binsize, ll))
    return set_last_error(IREC_E_INVALID, "irec_loglik_host", what);
  const int64_t dims = (int64_t)channels * plane;
  std::vector<double> ws(workspace_bytes_of(n_images, dims) / 8);
  I::LoglikCall call;
  I::bind(call, x, loc, log_scales, n_scales, n_images, channels, plane, binsize, ll, ws.data());
  I::loglik_host(call, Chunks{n_threads, 1});
  return IREC_OK;
} catch (const std::exception &e) { return irec::set_last_error(IREC_E_INVALID, "irec_loglik_host", e.what()); }

} // extern "C"
