// irec_rec.hip -- the .rec container on the device: a batch's files built from, and read into, device memory (include/irec.h:
// irec_rec_*_files_device, _device_ragged, _device_tables), the host forms under tables (irec_rec_*_files_tables) and the test hooks
// (csrc/irec_internal.h).  The coder itself is csrc/irec_rec_core.h; the kernels here only deal its lane functions out, compiled over
// irec_rec::NoTables (the default models) and over irec_rec::Tables (empirical tables).  Every entry point, at the end of this file,
// is: the call, irec_rec_call.h's preparation, then the launches here or that header's host runner.
//
// One lane per stream, 2 N R streams per call, index streams first and count streams after them, so that a wave holds streams of one
// kind.  256-lane workgroups, plain launches, plain vector loads and stores, no atomics: every store goes into a byte range that only
// its lane owns.
//   encode:  rec[_tables]_size_kernel (bits of every stream, input checks) -> rec_layout_kernel (bytes per file, exclusive scan: offsets,
//            status) -> rec[_tables]_write_kernel (headers, streams; nothing at all if the files do not fit cap)
//   decode:  rec[_tables]_decode_counts_kernel (header checks, K) -> rec[_tables]_decode_indices_kernel (index rows by that K)
//            -> rec_decode_status_kernel (one status per image; the outputs of an image with an error zeroed)
// No model enters the layout and the status kernel: they serve both.  Under tables, a workgroup that codes index streams first copies
// an index table of at most IREC_REC_TABLE_LDS_SYMBOLS symbols into LDS (every one of its lanes walks that table once per symbol: a
// look-up per value when writing, a binary search per value when reading); a larger one, and the count tables (one short table per
// residual block, read a few times per stream), are read from global memory.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "irec_rec_call.h"

namespace irec {
namespace {
using irec_rec::NoTables;
using irec_rec::Tables;

// ---- the default models ----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(REC_NT) void rec_size_kernel(irec_rec::EncodeCall c) {
  const int64_t lane = (int64_t)blockIdx.x * REC_NT + threadIdx.x;
  if (lane < 2 * (int64_t)c.N * c.R) irec_rec::encode_size_lane(c, lane);
}

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

// ---- empirical tables ------------------------------------------------------------------------------------------------------------------
// the call's tables with the index table in LDS, if this workgroup is to have it there (`wanted` is uniform over the workgroup)
__device__ inline Tables stage_index_table(const Tables &tb, uint32_t *lds, bool wanted) {
  Tables t = tb;
  if (wanted && tb.index_cum && tb.n_index_symbols <= IREC_REC_TABLE_LDS_SYMBOLS) {
    for (int32_t e = threadIdx.x; e <= tb.n_index_symbols; e += REC_NT) lds[e] = tb.index_cum[e];
    __syncthreads();
    t.index_cum = lds;
  }
  return t;
}

__global__ __launch_bounds__(REC_NT) void rec_tables_size_kernel(irec_rec::EncodeCall c, Tables tb) {
  __shared__ uint32_t lds[IREC_REC_TABLE_LDS_SYMBOLS + 1];
  const int64_t lane = (int64_t)blockIdx.x * REC_NT + threadIdx.x, NR = (int64_t)c.N * c.R;
  const Tables t = stage_index_table(tb, lds, (int64_t)blockIdx.x * REC_NT < NR);
  if (lane < 2 * NR) irec_rec::encode_size_lane(c, t, lane);
}

__global__ __launch_bounds__(REC_NT) void rec_tables_write_kernel(irec_rec::EncodeCall c, Tables tb) {
  __shared__ uint32_t lds[IREC_REC_TABLE_LDS_SYMBOLS + 1];
  const int64_t lane = (int64_t)blockIdx.x * REC_NT + threadIdx.x, NR = (int64_t)c.N * c.R;
  const Tables t = stage_index_table(tb, lds, (int64_t)blockIdx.x * REC_NT < NR);
  if (lane < 2 * NR + c.N) irec_rec::encode_write_lane(c, t, lane);
}

__global__ __launch_bounds__(REC_NT) void rec_tables_decode_counts_kernel(irec_rec::DecodeCall c, Tables tb) {
  const int64_t lane = (int64_t)blockIdx.x * REC_NT + threadIdx.x;
  if (lane < (int64_t)c.N * c.R) irec_rec::decode_counts_lane(c, tb, lane);
}

__global__ __launch_bounds__(REC_NT) void rec_tables_decode_indices_kernel(irec_rec::DecodeCall c, Tables tb) {
  __shared__ uint32_t lds[IREC_REC_TABLE_LDS_SYMBOLS + 1];
  const int64_t lane = (int64_t)blockIdx.x * REC_NT + threadIdx.x;
  const Tables t = stage_index_table(tb, lds, true);
  if (lane < (int64_t)c.N * c.R) irec_rec::decode_indices_lane(c, t, lane);
}

// ---- the two launches that no model enters ---------------------------------------------------------------------------------------------
// One workgroup: lane t takes the images [t * per, (t + 1) * per), so any N is covered; the 256 partial sums are scanned in LDS.
__global__ __launch_bounds__(REC_NT) void rec_layout_kernel(irec_rec::EncodeCall c) {
  __shared__ int64_t part[REC_NT];
  const int t = threadIdx.x;
  const int64_t per = ((int64_t)c.N + REC_NT - 1) / REC_NT, lo = t * per, hi = lo + per < c.N ? lo + per : c.N;
  int64_t sum = 0;
  for (int64_t i = lo; i < hi; ++i) sum += irec_rec::encode_image_bytes(c, i);   // (also leaves status[i])
  part[t] = sum;
  __syncthreads();
  for (int d = 1; d < REC_NT; d *= 2) {
    const int64_t add = t >= d ? part[t - d] : 0;
    __syncthreads();
    part[t] += add;
    __syncthreads();
  }
  int64_t at = part[t] - sum;                                                    // exclusive
  // the sizes once more, from the statuses just written by this very lane
  for (int64_t i = lo; i < hi; ++i) { c.offsets[i] = at; at += irec_rec::encode_image_bytes(c, i); }
  if (t == REC_NT - 1) c.offsets[c.N] = part[t];
}

// One workgroup per image: the first cause among its residual blocks, and zeroed outputs if there is one.
// (A function that takes its own copy of the call, as it was when two kernels shared it: written straight into the kernel, the same
// statements are scheduled otherwise, and scripts/isa_identity.py holds this library's device code to its predecessor's.)
__device__ inline void rec_decode_status_body(irec_rec::DecodeCall c) {
  __shared__ int32_t first[REC_NT];
  const int t = threadIdx.x;
  for (int64_t i = blockIdx.x; i < c.N; i += gridDim.x) {
    int32_t mine = 0x7fffffff;                                                   // (r << 8 | status) of the first failing block this lane saw
    for (int32_t r = t; r < c.R; r += REC_NT) {
      const int32_t st = irec_rec::decode_block_status(c, i * c.R + r);
      if (st && mine == 0x7fffffff) mine = (r << 8) | st;
    }
    first[t] = mine;
    __syncthreads();
    for (int d = REC_NT / 2; d > 0; d /= 2) {
      if (t < d && first[t + d] < first[t]) first[t] = first[t + d];
      __syncthreads();
    }
    const int32_t st = first[0] == 0x7fffffff ? 0 : (first[0] & 0xff);
    __syncthreads();
    if (t == 0) c.status[i] = st;
    if (st) {
      const int64_t nK = irec_rec::image_blocks(c), nI = nK * c.max_K;
      if (t < 9) c.headers[9 * i + t] = 0;
      for (int64_t e = t; e < nK; e += REC_NT) c.K[i * nK + e] = 0;
      for (int64_t e = t; e < nI; e += REC_NT) c.idx[i * nI + e] = 0;
    }
  }
}
__global__ __launch_bounds__(REC_NT) void rec_decode_status_kernel(irec_rec::DecodeCall c) { rec_decode_status_body(c); }

// ---- the three launches of a prepared call, uniform or ragged; T = NoTables or Tables picks the kernels that a model enters ------------
template <class T>
irec_status launch_encode(irec_rec::EncodeCall &c, const T &tb, void *workspace, void *hip_stream) {
  irec_rec::encode_bind_workspace(c, workspace);
  hipStream_t st = (hipStream_t)hip_stream;
  const int64_t streams = 2 * (int64_t)c.N * c.R;
  if (streams > 0) {
    if constexpr (T::any) hipLaunchKernelGGL(rec_tables_size_kernel, dim3(rec_grid(streams)), dim3(REC_NT), 0, st, c, tb);
    else hipLaunchKernelGGL(rec_size_kernel, dim3(rec_grid(streams)), dim3(REC_NT), 0, st, c);
    IREC_HIP(hipGetLastError());
  }
  hipLaunchKernelGGL(rec_layout_kernel, dim3(1), dim3(REC_NT), 0, st, c);
  IREC_HIP(hipGetLastError());
  if (streams > 0) {
    if constexpr (T::any) hipLaunchKernelGGL(rec_tables_write_kernel, dim3(rec_grid(streams + c.N)), dim3(REC_NT), 0, st, c, tb);
    else hipLaunchKernelGGL(rec_write_kernel, dim3(rec_grid(streams + c.N)), dim3(REC_NT), 0, st, c);
    IREC_HIP(hipGetLastError());
  }
  return IREC_OK;
}
template <class T>
irec_status launch_decode(const irec_rec::DecodeCall &c, const T &tb, void *hip_stream) {
  if (c.N == 0) return IREC_OK;
  hipStream_t st = (hipStream_t)hip_stream;
  const int64_t lanes = (int64_t)c.N * c.R;
  if constexpr (T::any) hipLaunchKernelGGL(rec_tables_decode_counts_kernel, dim3(rec_grid(lanes)), dim3(REC_NT), 0, st, c, tb);
  else hipLaunchKernelGGL(rec_decode_counts_kernel, dim3(rec_grid(lanes)), dim3(REC_NT), 0, st, c);
  IREC_HIP(hipGetLastError());
  if constexpr (T::any) hipLaunchKernelGGL(rec_tables_decode_indices_kernel, dim3(rec_grid(lanes)), dim3(REC_NT), 0, st, c, tb);
  else hipLaunchKernelGGL(rec_decode_indices_kernel, dim3(rec_grid(lanes)), dim3(REC_NT), 0, st, c);
  IREC_HIP(hipGetLastError());
  hipLaunchKernelGGL(rec_decode_status_kernel, dim3(c.N < 65536 ? c.N : 65536), dim3(REC_NT), 0, st, c);
  IREC_HIP(hipGetLastError());
  return IREC_OK;
}
} // namespace
} // namespace irec

using namespace irec;
using irec_rec::DecodeCall;
using irec_rec::EncodeCall;

extern "C" {

size_t irec_rec_device_workspace_bytes(int32_t n_images, int32_t n_res_blocks) {
  if (n_images < 0 || n_res_blocks < 1) return 0;
  const int64_t e = irec_rec::encode_workspace_bytes(n_images, n_res_blocks), d = irec_rec::decode_workspace_bytes(n_images, n_res_blocks);
  return (size_t)((e > d ? e : d) + 256);
}

// ---- the device entries: one count of blocks for every residual block; one per residual block ("ragged"); ragged under tables ---------
irec_status irec_rec_encode_files_device(uint32_t seed, uint32_t block_size, uint32_t max_index, uint32_t height, uint32_t width,
                                         uint32_t channels, int32_t n_images, int32_t n_res_blocks, int32_t blocks_per_res, int32_t max_K,
                                         const int32_t *K, int64_t k_stride, const int32_t *idx, int64_t idx_stride, uint8_t *out, int64_t cap,
                                         int64_t *offsets, int32_t *status, void *workspace, size_t workspace_bytes, void *hip_stream) {
  EncodeCall c{seed, block_size, max_index, height, width, channels, n_images, n_res_blocks, 0, max_K, K, k_stride, idx, idx_stride, out, cap, offsets, status};
  if (irec_status e = prepare_device(c, Layout::uniform(blocks_per_res), nullptr, workspace, workspace_bytes, "irec_rec_encode_files_device")) return e;
  return launch_encode(c, NoTables{}, workspace, hip_stream);
}

irec_status irec_rec_encode_files_device_ragged(uint32_t seed, uint32_t block_size, uint32_t max_index, uint32_t height, uint32_t width,
                                                uint32_t channels, int32_t n_images, int32_t n_res_blocks, const int32_t *blocks_per_res,
                                                int32_t max_K, const int32_t *K, int64_t k_stride, const int32_t *idx, int64_t idx_stride,
                                                uint8_t *out, int64_t cap, int64_t *offsets, int32_t *status, void *workspace,
                                                size_t workspace_bytes, void *hip_stream) {
  EncodeCall c{seed, block_size, max_index, height, width, channels, n_images, n_res_blocks, 0, max_K, K, k_stride, idx, idx_stride, out, cap, offsets, status};
  if (irec_status e = prepare_device(c, Layout::ragged(blocks_per_res), nullptr, workspace, workspace_bytes, "irec_rec_encode_files_device_ragged")) return e;
  return launch_encode(c, NoTables{}, workspace, hip_stream);
}

irec_status irec_rec_encode_files_device_tables(uint32_t seed, uint32_t block_size, uint32_t max_index, uint32_t height, uint32_t width,
                                                uint32_t channels, int32_t n_images, int32_t n_res_blocks, const int32_t *blocks_per_res,
                                                int32_t max_K, const int32_t *K, int64_t k_stride, const int32_t *idx, int64_t idx_stride,
                                                const uint32_t *index_cum, int32_t n_index_symbols, const uint32_t *count_cum,
                                                const int32_t *count_first, int64_t n_count_cum, uint8_t *out, int64_t cap, int64_t *offsets,
                                                int32_t *status, void *workspace, size_t workspace_bytes, void *hip_stream) {
  EncodeCall c{seed, block_size, max_index, height, width, channels, n_images, n_res_blocks, 0, max_K, K, k_stride, idx, idx_stride, out, cap, offsets, status};
  const Tables tb{index_cum, n_index_symbols, count_cum, count_first, n_count_cum};
  if (irec_status e = prepare_device(c, Layout::ragged(blocks_per_res), &tb, workspace, workspace_bytes, "irec_rec_encode_files_device_tables")) return e;
  return launch_encode(c, tb, workspace, hip_stream);
}

irec_status irec_rec_decode_files_device(const uint8_t *bytes, const int64_t *offsets, int32_t n_images, int32_t n_res_blocks,
                                         int32_t blocks_per_res, int32_t max_K, uint32_t *headers, int32_t *K, int32_t *idx, int32_t *status,
                                         void *workspace, size_t workspace_bytes, void *hip_stream) {
  DecodeCall c{bytes, offsets, n_images, n_res_blocks, 0, max_K, headers, K, idx, status, (int32_t *)workspace};
  if (irec_status e = prepare_device(c, Layout::uniform(blocks_per_res), nullptr, workspace, workspace_bytes, "irec_rec_decode_files_device")) return e;
  return launch_decode(c, NoTables{}, hip_stream);
}

irec_status irec_rec_decode_files_device_ragged(const uint8_t *bytes, const int64_t *offsets, int32_t n_images, int32_t n_res_blocks,
                                                const int32_t *blocks_per_res, int32_t max_K, uint32_t *headers, int32_t *K, int32_t *idx,
                                                int32_t *status, void *workspace, size_t workspace_bytes, void *hip_stream) {
  DecodeCall c{bytes, offsets, n_images, n_res_blocks, 0, max_K, headers, K, idx, status, (int32_t *)workspace};
  if (irec_status e = prepare_device(c, Layout::ragged(blocks_per_res), nullptr, workspace, workspace_bytes, "irec_rec_decode_files_device_ragged")) return e;
  return launch_decode(c, NoTables{}, hip_stream);
}

irec_status irec_rec_decode_files_device_tables(const uint8_t *bytes, const int64_t *offsets, int32_t n_images, int32_t n_res_blocks,
                                                const int32_t *blocks_per_res, int32_t max_K, const uint32_t *index_cum, int32_t n_index_symbols,
                                                const uint32_t *count_cum, const int32_t *count_first, int64_t n_count_cum, uint32_t *headers,
                                                int32_t *K, int32_t *idx, int32_t *status, void *workspace, size_t workspace_bytes,
                                                void *hip_stream) {
  DecodeCall c{bytes, offsets, n_images, n_res_blocks, 0, max_K, headers, K, idx, status, (int32_t *)workspace};
  const Tables tb{index_cum, n_index_symbols, count_cum, count_first, n_count_cum};
  if (irec_status e = prepare_device(c, Layout::ragged(blocks_per_res), &tb, workspace, workspace_bytes, "irec_rec_decode_files_device_tables")) return e;
  return launch_decode(c, tb, hip_stream);
}

// ---- the host forms under tables: the same lane functions over host memory, dealt to n_threads -----------------------------------------
int64_t irec_rec_encode_files_tables(uint32_t seed, uint32_t block_size, uint32_t max_index, uint32_t height, uint32_t width, uint32_t channels,
                                     int32_t n_images, int32_t n_res_blocks, const int32_t *blocks_per_res, int32_t max_K, const int32_t *K,
                                     const int32_t *idx, const uint32_t *index_cum, int32_t n_index_symbols, const uint32_t *count_cum,
                                     const int32_t *count_first, int64_t n_count_cum, uint8_t *out, int64_t cap, int64_t *offsets, int32_t *status,
                                     int32_t n_threads) {
  EncodeCall c{seed, block_size, max_index, height, width, channels, n_images, n_res_blocks, 0, max_K, K, 1, idx, max_K, out, cap, offsets, status};
  const Tables tb{index_cum, n_index_symbols, count_cum, count_first, n_count_cum};
  if (prepare(c, Layout::ragged(blocks_per_res), &tb, "irec_rec_encode_files_tables")) return -1;
  return run_encode_host(c, tb, n_threads, "irec_rec_encode_files_tables") ? -1 : offsets[n_images];
}

irec_status irec_rec_decode_files_tables(const uint8_t *bytes, const int64_t *offsets, int32_t n_images, int32_t n_res_blocks,
                                         const int32_t *blocks_per_res, int32_t max_K, const uint32_t *index_cum, int32_t n_index_symbols,
                                         const uint32_t *count_cum, const int32_t *count_first, int64_t n_count_cum, uint32_t *headers, int32_t *K,
                                         int32_t *idx, int32_t *status, int32_t n_threads) {
  DecodeCall c{bytes, offsets, n_images, n_res_blocks, 0, max_K, headers, K, idx, status};
  const Tables tb{index_cum, n_index_symbols, count_cum, count_first, n_count_cum};
  if (irec_status e = prepare(c, Layout::ragged(blocks_per_res), &tb, "irec_rec_decode_files_tables")) return e;
  return run_decode_host(c, tb, n_threads, "irec_rec_decode_files_tables");
}

// ---- the test hooks (csrc/irec_internal.h): the device entries without workspace and stream, the core over host memory on one thread ----
irec_status irec_rec_test_core_encode_files(uint32_t seed, uint32_t block_size, uint32_t max_index, uint32_t height, uint32_t width,
                                            uint32_t channels, int32_t n_images, int32_t n_res_blocks, int32_t blocks_per_res, int32_t max_K,
                                            const int32_t *K, int64_t k_stride, const int32_t *idx, int64_t idx_stride, uint8_t *out, int64_t cap,
                                            int64_t *offsets, int32_t *status) {
  EncodeCall c{seed, block_size, max_index, height, width, channels, n_images, n_res_blocks, 0, max_K, K, k_stride, idx, idx_stride, out, cap, offsets, status};
  if (irec_status e = prepare(c, Layout::uniform(blocks_per_res), nullptr, "irec_rec_test_core_encode_files")) return e;
  return run_encode_host(c, NoTables{}, 1, "irec_rec_test_core_encode_files");
}

irec_status irec_rec_test_core_encode_files_ragged(uint32_t seed, uint32_t block_size, uint32_t max_index, uint32_t height, uint32_t width,
                                                   uint32_t channels, int32_t n_images, int32_t n_res_blocks, const int32_t *blocks_per_res,
                                                   int32_t max_K, const int32_t *K, int64_t k_stride, const int32_t *idx, int64_t idx_stride,
                                                   uint8_t *out, int64_t cap, int64_t *offsets, int32_t *status) {
  EncodeCall c{seed, block_size, max_index, height, width, channels, n_images, n_res_blocks, 0, max_K, K, k_stride, idx, idx_stride, out, cap, offsets, status};
  if (irec_status e = prepare(c, Layout::ragged(blocks_per_res), nullptr, "irec_rec_test_core_encode_files_ragged")) return e;
  return run_encode_host(c, NoTables{}, 1, "irec_rec_test_core_encode_files_ragged");
}

irec_status irec_rec_test_core_encode_files_tables(uint32_t seed, uint32_t block_size, uint32_t max_index, uint32_t height, uint32_t width,
                                                   uint32_t channels, int32_t n_images, int32_t n_res_blocks, const int32_t *blocks_per_res,
                                                   int32_t max_K, const int32_t *K, int64_t k_stride, const int32_t *idx, int64_t idx_stride,
                                                   const uint32_t *index_cum, int32_t n_index_symbols, const uint32_t *count_cum,
                                                   const int32_t *count_first, int64_t n_count_cum, uint8_t *out, int64_t cap, int64_t *offsets,
                                                   int32_t *status) {
  EncodeCall c{seed, block_size, max_index, height, width, channels, n_images, n_res_blocks, 0, max_K, K, k_stride, idx, idx_stride, out, cap, offsets, status};
  const Tables tb{index_cum, n_index_symbols, count_cum, count_first, n_count_cum};
  if (irec_status e = prepare(c, Layout::ragged(blocks_per_res), &tb, "irec_rec_test_core_encode_files_tables")) return e;
  return run_encode_host(c, tb, 1, "irec_rec_test_core_encode_files_tables");
}

irec_status irec_rec_test_core_decode_files(const uint8_t *bytes, const int64_t *offsets, int32_t n_images, int32_t n_res_blocks,
                                            int32_t blocks_per_res, int32_t max_K, uint32_t *headers, int32_t *K, int32_t *idx,
                                            int32_t *status) {
  DecodeCall c{bytes, offsets, n_images, n_res_blocks, 0, max_K, headers, K, idx, status};
  if (irec_status e = prepare(c, Layout::uniform(blocks_per_res), nullptr, "irec_rec_test_core_decode_files")) return e;
  return run_decode_host(c, NoTables{}, 1, "irec_rec_test_core_decode_files");
}

irec_status irec_rec_test_core_decode_files_ragged(const uint8_t *bytes, const int64_t *offsets, int32_t n_images, int32_t n_res_blocks,
                                                   const int32_t *blocks_per_res, int32_t max_K, uint32_t *headers, int32_t *K, int32_t *idx,
                                                   int32_t *status) {
  DecodeCall c{bytes, offsets, n_images, n_res_blocks, 0, max_K, headers, K, idx, status};
  if (irec_status e = prepare(c, Layout::ragged(blocks_per_res), nullptr, "irec_rec_test_core_decode_files_ragged")) return e;
  return run_decode_host(c, NoTables{}, 1, "irec_rec_test_core_decode_files_ragged");
}

irec_status irec_rec_test_core_decode_files_tables(const uint8_t *bytes, const int64_t *offsets, int32_t n_images, int32_t n_res_blocks,
                                                   const int32_t *blocks_per_res, int32_t max_K, const uint32_t *index_cum, int32_t n_index_symbols,
                                                   const uint32_t *count_cum, const int32_t *count_first, int64_t n_count_cum, uint32_t *headers,
                                                   int32_t *K, int32_t *idx, int32_t *status) {
  DecodeCall c{bytes, offsets, n_images, n_res_blocks, 0, max_K, headers, K, idx, status};
  const Tables tb{index_cum, n_index_symbols, count_cum, count_first, n_count_cum};
  if (irec_status e = prepare(c, Layout::ragged(blocks_per_res), &tb, "irec_rec_test_core_decode_files_tables")) return e;
  return run_decode_host(c, tb, 1, "irec_rec_test_core_decode_files_tables");
}

} // extern "C"
