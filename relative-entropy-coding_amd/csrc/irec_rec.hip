// irec_rec.hip -- the .rec container on the device: a batch's files built from, and read into, device memory (include/irec.h:
// irec_rec_encode_files_device / irec_rec_decode_files_device).  The coder itself is csrc/irec_rec_core.h, which the host hooks at the
// end of this file run over host memory in a plain loop; the kernels here only deal its lane functions out.
//
// One lane per stream, 2 N R streams per call, index streams first and count streams after them, so that a wave holds streams of one
// kind.  256-lane workgroups, plain launches, no atomics: every store goes into a byte range that only its lane owns.
//   encode:  rec_size_kernel (bits of every stream, input checks) -> rec_layout_kernel (bytes per file, exclusive scan: offsets, status)
//            -> rec_write_kernel (headers, streams; nothing at all if the files do not fit cap)
//   decode:  rec_decode_counts_kernel (header checks, K) -> rec_decode_indices_kernel (index rows by that K)
//            -> rec_decode_status_kernel (one status per image; the outputs of an image with an error zeroed)
// (the layout scan, the verdict and the argument checks live in irec_rec_kernels.h, which irec_rec_tables.hip shares)
#include <hip/hip_runtime.h>

#include <cstdint>
#include <exception>
#include <vector>

#include "irec_rec_kernels.h"

namespace irec {
namespace {
__global__ __launch_bounds__(REC_NT) void rec_size_kernel(irec_rec::EncodeCall c) {
  const int64_t lane = (int64_t)blockIdx.x * REC_NT + threadIdx.x;
  if (lane < 2 * (int64_t)c.N * c.R) irec_rec::encode_size_lane(c, lane);
}

__global__ __launch_bounds__(REC_NT) void rec_layout_kernel(irec_rec::EncodeCall c) { rec_layout_body(c); }

__global__ __launch_bounds__(REC_NT) void rec_write_kernel(irec_rec::EncodeCall c) {
  const int64_t lane = (int64_t)blockIdx.x * REC_NT + threadIdx.x;
  if (lane < 2 * (int64_t)c.N * c.R + c.N) irec_rec::encode_write_lane(c, lane);
}

__global__ __launch_bounds__(REC_NT) void rec_decode_counts_kernel(irec_rec::DecodeCall c) {
  const int64_t lane = (int64_t)blockIdx.x * REC_NT + threadIdx.x;
  if (lane < (int64_t)c.N * c.R) irec_rec::decode_counts_lane(c, lane);
}

__global__ __launch_bounds__(REC_NT) void rec_decode_indices_kernel(irec_rec::DecodeCall c) {
  const int64_t lane = (int64_t)blockIdx.x * REC_NT + threadIdx.x;
  if (lane < (int64_t)c.N * c.R) irec_rec::decode_indices_lane(c, lane);
}

__global__ __launch_bounds__(REC_NT) void rec_decode_status_kernel(irec_rec::DecodeCall c) { rec_decode_status_body(c); }
} // namespace
} // namespace irec

namespace irec {
namespace {
// the three launches of a call whose arguments and workspace have been checked, uniform or ragged
irec_status launch_encode(irec_rec::EncodeCall &c, void *workspace, void *hip_stream) {
  irec_rec::encode_bind_workspace(c, workspace);
  hipStream_t st = (hipStream_t)hip_stream;
  const int64_t streams = 2 * (int64_t)c.N * c.R;
  if (streams > 0) {
    hipLaunchKernelGGL(rec_size_kernel, dim3(rec_grid(streams)), dim3(REC_NT), 0, st, c);
    REC_HIP(hipGetLastError());
  }
  hipLaunchKernelGGL(rec_layout_kernel, dim3(1), dim3(REC_NT), 0, st, c);
  REC_HIP(hipGetLastError());
  if (streams > 0) {
    hipLaunchKernelGGL(rec_write_kernel, dim3(rec_grid(streams + c.N)), dim3(REC_NT), 0, st, c);
    REC_HIP(hipGetLastError());
  }
  return IREC_OK;
}
irec_status launch_decode(const irec_rec::DecodeCall &c, void *hip_stream) {
  hipStream_t st = (hipStream_t)hip_stream;
  const int64_t lanes = (int64_t)c.N * c.R;
  hipLaunchKernelGGL(rec_decode_counts_kernel, dim3(rec_grid(lanes)), dim3(REC_NT), 0, st, c);
  REC_HIP(hipGetLastError());
  hipLaunchKernelGGL(rec_decode_indices_kernel, dim3(rec_grid(lanes)), dim3(REC_NT), 0, st, c);
  REC_HIP(hipGetLastError());
  hipLaunchKernelGGL(rec_decode_status_kernel, dim3(c.N < 65536 ? c.N : 65536), dim3(REC_NT), 0, st, c);
  REC_HIP(hipGetLastError());
  return IREC_OK;
}
} // namespace
} // namespace irec

extern "C" {

size_t irec_rec_device_workspace_bytes(int32_t n_images, int32_t n_res_blocks) {
  if (n_images < 0 || n_res_blocks < 1) return 0;
  const int64_t e = irec_rec::encode_workspace_bytes(n_images, n_res_blocks), d = irec_rec::decode_workspace_bytes(n_images, n_res_blocks);
  return (size_t)((e > d ? e : d) + 256);
}

irec_status irec_rec_encode_files_device(uint32_t seed, uint32_t block_size, uint32_t max_index, uint32_t height, uint32_t width,
                                         uint32_t channels, int32_t n_images, int32_t n_res_blocks, int32_t blocks_per_res, int32_t max_K,
                                         const int32_t *K, int64_t k_stride, const int32_t *idx, int64_t idx_stride, uint8_t *out, int64_t cap,
                                         int64_t *offsets, int32_t *status, void *workspace, size_t workspace_bytes, void *hip_stream) {
  using namespace irec;
  if (!encode_args_ok(height, width, channels, n_images, n_res_blocks, blocks_per_res, max_K, K, k_stride, idx, idx_stride, out, cap, offsets, status))
    return set_last_error(IREC_E_INVALID, "irec_rec_encode_files_device", "bad arguments");
  if (!workspace || ((uintptr_t)workspace & 7) || workspace_bytes < irec_rec_device_workspace_bytes(n_images, n_res_blocks))
    return set_last_error(IREC_E_WORKSPACE, "irec_rec_encode_files_device", "workspace too small (irec_rec_device_workspace_bytes) or not 8-byte aligned");
  irec_rec::EncodeCall c{seed, block_size, max_index, height, width, channels, n_images, n_res_blocks, blocks_per_res, max_K,
                         K, k_stride, idx, idx_stride, out, cap, offsets, status, nullptr, nullptr, nullptr, {}};
  return launch_encode(c, workspace, hip_stream);
}

irec_status irec_rec_encode_files_device_ragged(uint32_t seed, uint32_t block_size, uint32_t max_index, uint32_t height, uint32_t width,
                                                uint32_t channels, int32_t n_images, int32_t n_res_blocks, const int32_t *blocks_per_res,
                                                int32_t max_K, const int32_t *K, int64_t k_stride, const int32_t *idx, int64_t idx_stride,
                                                uint8_t *out, int64_t cap, int64_t *offsets, int32_t *status, void *workspace,
                                                size_t workspace_bytes, void *hip_stream) {
  using namespace irec;
  irec_rec::EncodeCall c{seed, block_size, max_index, height, width, channels, n_images, n_res_blocks, 0, max_K,
                         K, k_stride, idx, idx_stride, out, cap, offsets, status, nullptr, nullptr, nullptr, {}};
  if (const char *why = ragged_layout(n_res_blocks, blocks_per_res, c.first))
    return set_last_error(IREC_E_INVALID, "irec_rec_encode_files_device_ragged", why);
  if (!encode_args_ok(height, width, channels, n_images, n_res_blocks, 1, max_K, K, k_stride, idx, idx_stride, out, cap, offsets, status))
    return set_last_error(IREC_E_INVALID, "irec_rec_encode_files_device_ragged", "bad arguments");
  if (!workspace || ((uintptr_t)workspace & 7) || workspace_bytes < irec_rec_device_workspace_bytes(n_images, n_res_blocks))
    return set_last_error(IREC_E_WORKSPACE, "irec_rec_encode_files_device_ragged", "workspace too small (irec_rec_device_workspace_bytes) or not 8-byte aligned");
  return launch_encode(c, workspace, hip_stream);
}

irec_status irec_rec_decode_files_device(const uint8_t *bytes, const int64_t *offsets, int32_t n_images, int32_t n_res_blocks,
                                         int32_t blocks_per_res, int32_t max_K, uint32_t *headers, int32_t *K, int32_t *idx, int32_t *status,
                                         void *workspace, size_t workspace_bytes, void *hip_stream) {
  using namespace irec;
  if (!decode_args_ok(bytes, offsets, n_images, n_res_blocks, blocks_per_res, max_K, headers, K, idx, status))
    return set_last_error(IREC_E_INVALID, "irec_rec_decode_files_device", "bad arguments");
  if (!workspace || ((uintptr_t)workspace & 7) || workspace_bytes < irec_rec_device_workspace_bytes(n_images, n_res_blocks))
    return set_last_error(IREC_E_WORKSPACE, "irec_rec_decode_files_device", "workspace too small (irec_rec_device_workspace_bytes) or not 8-byte aligned");
  if (n_images == 0) return IREC_OK;
  irec_rec::DecodeCall c{bytes, offsets, n_images, n_res_blocks, blocks_per_res, max_K, headers, K, idx, status, (int32_t *)workspace, {}};
  return launch_decode(c, hip_stream);
}

irec_status irec_rec_decode_files_device_ragged(const uint8_t *bytes, const int64_t *offsets, int32_t n_images, int32_t n_res_blocks,
                                                const int32_t *blocks_per_res, int32_t max_K, uint32_t *headers, int32_t *K, int32_t *idx,
                                                int32_t *status, void *workspace, size_t workspace_bytes, void *hip_stream) {
  using namespace irec;
  irec_rec::DecodeCall c{bytes, offsets, n_images, n_res_blocks, 0, max_K, headers, K, idx, status, (int32_t *)workspace, {}};
  if (const char *why = ragged_layout(n_res_blocks, blocks_per_res, c.first))
    return set_last_error(IREC_E_INVALID, "irec_rec_decode_files_device_ragged", why);
  if (!decode_args_ok(bytes, offsets, n_images, n_res_blocks, 1, max_K, headers, K, idx, status))
    return set_last_error(IREC_E_INVALID, "irec_rec_decode_files_device_ragged", "bad arguments");
  if (!workspace || ((uintptr_t)workspace & 7) || workspace_bytes < irec_rec_device_workspace_bytes(n_images, n_res_blocks))
    return set_last_error(IREC_E_WORKSPACE, "irec_rec_decode_files_device_ragged", "workspace too small (irec_rec_device_workspace_bytes) or not 8-byte aligned");
  if (n_images == 0) return IREC_OK;
  return launch_decode(c, hip_stream);
}

// ---- the same lane functions over host memory, in a plain loop (csrc/irec_internal.h) ------------------------------------------------
} // extern "C"
namespace irec {
namespace {
irec_status core_encode_host(irec_rec::EncodeCall &c, const char *who) try {
  std::vector<int64_t> ws((size_t)(irec_rec_device_workspace_bytes(c.N, c.R) / 8 + 1));
  irec_rec::encode_bind_workspace(c, ws.data());
  irec_rec::encode_call_host(c);
  return IREC_OK;
} catch (const std::exception &e) { return set_last_error(IREC_E_INVALID, who, e.what()); }
irec_status core_decode_host(irec_rec::DecodeCall &c, const char *who) try {
  std::vector<int32_t> ws((size_t)(2 * (int64_t)c.N * c.R + 1));
  c.stream_status = ws.data();
  irec_rec::decode_call_host(c);
  return IREC_OK;
} catch (const std::exception &e) { return set_last_error(IREC_E_INVALID, who, e.what()); }
} // namespace
} // namespace irec
extern "C" {

irec_status irec_rec_test_core_encode_files(uint32_t seed, uint32_t block_size, uint32_t max_index, uint32_t height, uint32_t width,
                                            uint32_t channels, int32_t n_images, int32_t n_res_blocks, int32_t blocks_per_res, int32_t max_K,
                                            const int32_t *K, int64_t k_stride, const int32_t *idx, int64_t idx_stride, uint8_t *out, int64_t cap,
                                            int64_t *offsets, int32_t *status) {
  using namespace irec;
  if (!encode_args_ok(height, width, channels, n_images, n_res_blocks, blocks_per_res, max_K, K, k_stride, idx, idx_stride, out, cap, offsets, status))
    return set_last_error(IREC_E_INVALID, "irec_rec_test_core_encode_files", "bad arguments");
  irec_rec::EncodeCall c{seed, block_size, max_index, height, width, channels, n_images, n_res_blocks, blocks_per_res, max_K,
                         K, k_stride, idx, idx_stride, out, cap, offsets, status, nullptr, nullptr, nullptr, {}};
  return core_encode_host(c, "irec_rec_test_core_encode_files");
}

irec_status irec_rec_test_core_encode_files_ragged(uint32_t seed, uint32_t block_size, uint32_t max_index, uint32_t height, uint32_t width,
                                                   uint32_t channels, int32_t n_images, int32_t n_res_blocks, const int32_t *blocks_per_res,
                                                   int32_t max_K, const int32_t *K, int64_t k_stride, const int32_t *idx, int64_t idx_stride,
                                                   uint8_t *out, int64_t cap, int64_t *offsets, int32_t *status) {
  using namespace irec;
  irec_rec::EncodeCall c{seed, block_size, max_index, height, width, channels, n_images, n_res_blocks, 0, max_K,
                         K, k_stride, idx, idx_stride, out, cap, offsets, status, nullptr, nullptr, nullptr, {}};
  if (const char *why = ragged_layout(n_res_blocks, blocks_per_res, c.first))
    return set_last_error(IREC_E_INVALID, "irec_rec_test_core_encode_files_ragged", why);
  if (!encode_args_ok(height, width, channels, n_images, n_res_blocks, 1, max_K, K, k_stride, idx, idx_stride, out, cap, offsets, status))
    return set_last_error(IREC_E_INVALID, "irec_rec_test_core_encode_files_ragged", "bad arguments");
  return core_encode_host(c, "irec_rec_test_core_encode_files_ragged");
}

irec_status irec_rec_test_core_decode_files(const uint8_t *bytes, const int64_t *offsets, int32_t n_images, int32_t n_res_blocks,
                                            int32_t blocks_per_res, int32_t max_K, uint32_t *headers, int32_t *K, int32_t *idx,
                                            int32_t *status) {
  using namespace irec;
  if (!decode_args_ok(bytes, offsets, n_images, n_res_blocks, blocks_per_res, max_K, headers, K, idx, status))
    return set_last_error(IREC_E_INVALID, "irec_rec_test_core_decode_files", "bad arguments");
  irec_rec::DecodeCall c{bytes, offsets, n_images, n_res_blocks, blocks_per_res, max_K, headers, K, idx, status, nullptr, {}};
  return core_decode_host(c, "irec_rec_test_core_decode_files");
}

irec_status irec_rec_test_core_decode_files_ragged(const uint8_t *bytes, const int64_t *offsets, int32_t n_images, int32_t n_res_blocks,
                                                   const int32_t *blocks_per_res, int32_t max_K, uint32_t *headers, int32_t *K, int32_t *idx,
                                                   int32_t *status) {
  using namespace irec;
  irec_rec::DecodeCall c{bytes, offsets, n_images, n_res_blocks, 0, max_K, headers, K, idx, status, nullptr, {}};
  if (const char *why = ragged_layout(n_res_blocks, blocks_per_res, c.first))
    return set_last_error(IREC_E_INVALID, "irec_rec_test_core_decode_files_ragged", why);
  if (!decode_args_ok(bytes, offsets, n_images, n_res_blocks, 1, max_K, headers, K, idx, status))
    return set_last_error(IREC_E_INVALID, "irec_rec_test_core_decode_files_ragged", "bad arguments");
  return core_decode_host(c, "irec_rec_test_core_decode_files_ragged");
}

} // extern "C"
