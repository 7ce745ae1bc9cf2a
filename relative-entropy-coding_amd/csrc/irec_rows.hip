// irec_rows.hip -- irec_decode_rows_status (include/irec.h): the per-image verdict on the rows a decode call is about to read, on the
// device.  The check itself is csrc/irec_rows_core.h, which the host hook at the end of this file runs over host memory in a plain loop.
//
// One workgroup per group (an image's blocks in one residual block), grid-strided; lane t looks at blocks t, t + 256, ...; the smallest
// (block << 2 | cause) of the lanes is found in LDS and lane 0 alone reads and writes status[g].  No atomics: launches of successive
// residual blocks on one stream accumulate the first cause per image.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "irec_call.h"
#include "irec_internal.h"
#include "irec_rows_core.h"

namespace irec {
namespace {
constexpr int ROWS_NT = 256;

__global__ __launch_bounds__(ROWS_NT) void rows_status_kernel(irec_rows::Call c) {
  __shared__ int32_t first[ROWS_NT];
  const int t = threadIdx.x;
  for (int64_t g = blockIdx.x; g < c.n_groups; g += gridDim.x) {
    first[t] = irec_rows::lane_first(c, g, t, ROWS_NT);
    __syncthreads();
    for (int d = ROWS_NT / 2; d > 0; d /= 2) {
      if (t < d && first[t + d] < first[t]) first[t] = first[t + d];
      __syncthreads();
    }
    if (t == 0) irec_rows::group_store(c, g, first[0]);
    __syncthreads();                                                              // (first[] is written again in the next turn)
  }
}
} // namespace
} // namespace irec

extern "C" {

irec_status irec_decode_rows_status(int64_t n_groups, int32_t blocks_per_group, const int32_t *block_row, const int32_t *K, int64_t k_stride,
                                    const int32_t *idx, int64_t idx_stride, int32_t max_K, int32_t min_K, int32_t k_limit, int32_t n_samples,
                                    int32_t *status, void *hip_stream) {
  using namespace irec;
  const irec_rows::Call c{n_groups, blocks_per_group, block_row, K, k_stride, idx, idx_stride, max_K, min_K, k_limit, n_samples, status};
  if (!irec_rows::args_ok(c)) return set_last_error(IREC_E_INVALID, "irec_decode_rows_status", "bad arguments");
  if (n_groups == 0) return IREC_OK;
  hipLaunchKernelGGL(rows_status_kernel, dim3((unsigned)(n_groups < 65536 ? n_groups : 65536)), dim3(ROWS_NT), 0, (hipStream_t)hip_stream, c);
  IREC_HIP_AS("irec_decode_rows_status", hipGetLastError());
  return IREC_OK;
}

// ---- the same lane function over host memory, in a plain loop (csrc/irec_internal.h) ------------------------------------------------
irec_status irec_test_rows_status_host(int64_t n_groups, int32_t blocks_per_group, const int32_t *block_row, const int32_t *K, int64_t k_stride,
                                       const int32_t *idx, int64_t idx_stride, int32_t max_K, int32_t min_K, int32_t k_limit, int32_t n_samples,
                                       int32_t *status) {
  using namespace irec;
  const irec_rows::Call c{n_groups, blocks_per_group, block_row, K, k_stride, idx, idx_stride, max_K, min_K, k_limit, n_samples, status};
  if (!irec_rows::args_ok(c)) return set_last_error(IREC_E_INVALID, "irec_test_rows_status_host", "bad arguments");
  irec_rows::call_host(c);
  return IREC_OK;
}

} // extern "C"
