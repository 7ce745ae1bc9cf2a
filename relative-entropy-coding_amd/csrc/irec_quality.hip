// irec_quality.hip -- PSNR and MS-SSIM of a batch on the device and on the host (include/irec.h: irec_quality_*).  The arithmetic, the
// phases of a tile and the order of every sum are csrc/irec_quality_core.h; the kernels here put the barriers between the phases, and
// the host entry point at the end of this file runs the same phases over host memory.
//
// One launch per scale, one 256-thread workgroup per 32 x 32 tile of an (image, channel) plane: the tile and its 10-pixel halo of both
// images go into LDS once (42 KB with the row sums and the reduction), the separable 11-tap filter runs there on the four quantities,
// and what leaves is the tile's partial (three doubles) and its 16 x 16 cells of the next scale's two planes.  No moment plane goes to
// memory, no atomics: every store goes to an address that only its tile owns.  quality_finish_kernel, one wave per value, adds the
// partials in tile order in float64.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <exception>
#include <vector>

#include "irec_call.h"
#include "irec_quality_core.h"

namespace irec {
namespace {
namespace Q = irec_quality;

__global__ __launch_bounds__(Q::NT) void quality_scale_kernel(Q::Call c, int32_t k) {
  __shared__ Q::TileMem m;
  const int tid = threadIdx.x;
  const Q::Tile T = Q::tile_of(c, k, blockIdx.x);
  const float sse = Q::phase_load(c, T, m, tid);
  __syncthreads();
  if (T.next_a) Q::phase_down(T, m, tid);
  Q::phase_h(c, m, tid);
  __syncthreads();
  Q::phase_v(c, T, m, tid, sse);
  __syncthreads();
  for (int d = Q::NT / 2; d > 0; d /= 2) {
    Q::phase_reduce_step(m, tid, d);
    __syncthreads();
  }
  if (tid == 0) Q::phase_store(T, m);
}

// The sums of core.h's finish_host, a wave per value: the lanes stage 64 partials at a time in LDS and lane 0 adds them in order.
template <int N_SUMS>
__device__ void staged_sums(const double *p, int64_t n, double *stage, double (&acc)[N_SUMS]) {
  const int lane = threadIdx.x;
  for (int64_t lo = 0; lo < n; lo += Q::FINISH_NT) {
    const int64_t live = n - lo < Q::FINISH_NT ? n - lo : Q::FINISH_NT;
    if (lane < live) {
#pragma unroll
      for (int j = 0; j < N_SUMS; ++j) stage[j * Q::FINISH_NT + lane] = p[(lo + lane) * Q::PART + j];
    }
    __syncthreads();
    if (lane == 0) {
#pragma unroll
      for (int j = 0; j < N_SUMS; ++j) acc[j] = Q::ordered_sum(stage + j * Q::FINISH_NT, 1, live, acc[j]);
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(Q::FINISH_NT) void quality_finish_kernel(Q::Call c) {
  __shared__ double stage[2 * Q::FINISH_NT];
  const int64_t planes = (int64_t)c.N * c.C, v = blockIdx.x;
  if (v < planes * c.n_scales) {
    const int64_t plane = v / c.n_scales;
    const int32_t k = (int32_t)(v % c.n_scales);
    const Q::Level L = Q::level_of(planes, c.H, c.W, k);
    double acc[2] = {0.0, 0.0};
    staged_sums(c.partials + L.part_at + plane * L.tiles() * Q::PART, L.tiles(), stage, acc);
    if (threadIdx.x == 0) Q::finish_plane_store(c, plane, k, L, acc[0], acc[1]);
  } else {
    const int64_t n = v - planes * c.n_scales;
    const Q::Level L0 = Q::level_of(planes, c.H, c.W, 0);
    double acc[1] = {0.0};
    staged_sums(c.partials + L0.part_at + n * c.C * L0.tiles() * Q::PART + 2, c.C * L0.tiles(), stage, acc);
    if (threadIdx.x == 0) c.sse[n] = (float)acc[0];
  }
}

size_t workspace_bytes_of(int32_t n, int32_t c, int32_t h, int32_t w, int32_t n_scales) {
  int64_t doubles = 0, floats = 0;
  Q::workspace_sizes((int64_t)n * c, h, w, n_scales, &doubles, &floats);
  return (size_t)(8 * doubles + 4 * floats);
}

// IREC_OK, or the argument error of both entries
irec_status check_args(const char *who, const float *a, const float *b, int32_t n, int32_t c, int32_t h, int32_t w, int32_t n_scales,
                       const irec_quality_params *p, const float *per_scale, const float *sse) {
  if (!a || !b || !p || !per_scale || !sse) return set_last_error(IREC_E_INVALID, who, "null pointer");
  if (const char *what = Q::shape_error(n, c, h, w, n_scales, p)) return set_last_error(IREC_E_INVALID, who, what);
  return IREC_OK;
}
} // namespace
} // namespace irec

extern "C" {

size_t irec_quality_workspace_bytes(int32_t n, int32_t c, int32_t h, int32_t w, int32_t n_scales) {
  const irec_quality_params unit = {1.0f, 0.0f, 1.0f, 0.0f, 0, 0, 1.0f, 0.01f, 0.03f};
  if (irec_quality::shape_error(n, c, h, w, n_scales, &unit)) return 0;
  return irec::workspace_bytes_of(n, c, h, w, n_scales);
}

irec_status irec_quality_device(const float *a, const float *b, int32_t n, int32_t c, int32_t h, int32_t w, int32_t n_scales,
                                const irec_quality_params *params, float *per_scale, float *sse, void *workspace,
                                size_t workspace_bytes, void *hip_stream) {
  using namespace irec;
  if (irec_status st = check_args("irec_quality_device", a, b, n, c, h, w, n_scales, params, per_scale, sse)) return st;
  if (irec_status st = check_workspace(workspace_bytes_of(n, c, h, w, n_scales), workspace, workspace_bytes, "irec_quality_device", "irec_quality_workspace_bytes")) return st;
  Q::Call call;
  Q::bind(call, a, b, n, c, h, w, n_scales, params, per_scale, sse, workspace);
  hipStream_t st = (hipStream_t)hip_stream;
  const int64_t planes = (int64_t)n * c;
  for (int32_t k = 0; k < n_scales; ++k) {
    const Q::Level L = Q::level_of(planes, h, w, k);
    hipLaunchKernelGGL(quality_scale_kernel, dim3((unsigned)(planes * L.tiles())), dim3(Q::NT), 0, st, call, k);
    IREC_HIP(hipGetLastError());
  }
  hipLaunchKernelGGL(quality_finish_kernel, dim3((unsigned)Q::n_values(call)), dim3(Q::FINISH_NT), 0, st, call);
  IREC_HIP(hipGetLastError());
  return IREC_OK;
}

irec_status irec_quality_host(const float *a, const float *b, int32_t n, int32_t c, int32_t h, int32_t w, int32_t n_scales,
                              const irec_quality_params *params, float *per_scale, float *sse, int32_t n_threads) try {
  using namespace irec;
  if (irec_status st = check_args("irec_quality_host", a, b, n, c, h, w, n_scales, params, per_scale, sse)) return st;
  std::vector<double> ws(workspace_bytes_of(n, c, h, w, n_scales) / 8 + 1);
  Q::Call call;
  Q::bind(call, a, b, n, c, h, w, n_scales, params, per_scale, sse, ws.data());
  Q::call_host(call, Chunks{n_threads, 4});   // (a thread is not worth fewer than 4 tiles)
  return IREC_OK;
} catch (const std::exception &e) { return irec::set_last_error(IREC_E_INVALID, "irec_quality_host", e.what()); }

} // extern "C"
