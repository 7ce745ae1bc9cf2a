// irec_rec_tables.hip -- the .rec container under empirical symbol tables (include/irec.h: irec_rec_tables_build, irec_rec_*_tables,
// irec_rec_hist_rows*).  The coder is csrc/irec_rec_core.h once more, its lane functions compiled over irec_rec::Tables; irec_rec.hip
// keeps the default models and is not touched by anything here.
//
// Codec: the three launches per direction of irec_rec.hip, one lane per stream (index streams first, count streams after them).
//   rec_tables_size_kernel -> rec_tables_layout_kernel -> rec_tables_write_kernel
//   rec_tables_decode_counts_kernel -> rec_tables_decode_indices_kernel -> rec_tables_decode_status_kernel
// A workgroup that codes index streams first copies an index table of at most IREC_REC_TABLE_LDS_SYMBOLS symbols into LDS (every one of
// its lanes walks that table once per symbol: a look-up per value when writing, a binary search per value when reading); a larger one,
// and the count tables (one short table per residual block, read a few times per stream), are read from global memory.  Plain vector
// loads and stores, no atomics: every store goes into a byte range that only its lane owns.
// Histograms: rec_hist_rows_kernel, one lane per row, the bins of a workgroup in LDS, one integer atomicAdd per non-empty bin per workgroup.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <exception>
#include <thread>
#include <vector>

#include "irec_rec_kernels.h"

namespace irec {
namespace {
using irec_rec::Tables;

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

__global__ __launch_bounds__(REC_NT) void rec_tables_layout_kernel(irec_rec::EncodeCall c) { rec_layout_body(c); }

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

__global__ __launch_bounds__(REC_NT) void rec_tables_decode_status_kernel(irec_rec::DecodeCall c) { rec_decode_status_body(c); }

// ---- histograms ----------------------------------------------------------------------------------------------------------------------
// What one row adds: its K to the bins of its residual block, its first K indices to the index bins (include/irec.h has the ranges).
struct HistCall {
  int32_t N, R, max_K, n_index_values, n_count_values;
  const int32_t *K; int64_t k_stride; const int32_t *idx; int64_t idx_stride;
  uint64_t *index_hist, *count_hist, *streams, *rejected;
  int32_t first[IREC_REC_RAGGED_MAX_RES + 1];
};
inline __host__ __device__ int32_t hist_res_of(const HistCall &c, int32_t row_in_image) {   // the residual block of a row: first[r] <= row < first[r + 1]
  int32_t lo = 0, hi = c.R - 1;
  while (lo < hi) { const int32_t mid = (lo + hi + 1) / 2; if (c.first[mid] <= row_in_image) lo = mid; else hi = mid - 1; }
  return lo;
}
// add_index(v), add_count(r, k), reject(): where the three kinds of result go
template <class AddIndex, class AddCount, class Reject>
inline __host__ __device__ void hist_row(const HistCall &c, int64_t b, AddIndex &&add_index, AddCount &&add_count, Reject &&reject) {
  const int32_t T = c.first[c.R], k = c.K[b * c.k_stride];
  if (k < 0 || k > c.max_K || k >= c.n_count_values) { reject(); return; }
  add_count(hist_res_of(c, (int32_t)(b % T)), k);
  for (int32_t t = 0; t < k; ++t) {
    const int32_t v = c.idx[b * c.idx_stride + t];
    if (v < 0 || v >= c.n_index_values) reject(); else add_index(v);
  }
}

// LDS bins of a workgroup: the first HIST_INDEX_BINS index values and, if they all fit, the R * n_count_values count bins; a value past
// them goes to global memory at once (still an integer add).  256 rows of at most 65536 indices: a 32-bit bin cannot wrap.
constexpr int32_t HIST_INDEX_BINS = 8192, HIST_COUNT_BINS = 4096;
__global__ __launch_bounds__(REC_NT) void rec_hist_rows_kernel(HistCall c) {
  __shared__ uint32_t index_bins[HIST_INDEX_BINS], count_bins[HIST_COUNT_BINS], rejected;
  const int64_t rows = (int64_t)c.N * c.first[c.R], b = (int64_t)blockIdx.x * REC_NT + threadIdx.x;
  const int32_t n_ib = c.n_index_values < HIST_INDEX_BINS ? c.n_index_values : HIST_INDEX_BINS;
  const int64_t n_cb_all = (int64_t)c.R * c.n_count_values;
  const int32_t n_cb = n_cb_all <= HIST_COUNT_BINS ? (int32_t)n_cb_all : 0;
  for (int32_t e = threadIdx.x; e < n_ib; e += REC_NT) index_bins[e] = 0;
  for (int32_t e = threadIdx.x; e < n_cb; e += REC_NT) count_bins[e] = 0;
  if (threadIdx.x == 0) rejected = 0;
  __syncthreads();
  if (b < rows)
    hist_row(c, b,
             [&](int32_t v) { if (v < n_ib) atomicAdd(&index_bins[v], 1u); else atomicAdd((unsigned long long *)&c.index_hist[v], 1ull); },
             [&](int32_t r, int32_t k) {
               const int64_t e = (int64_t)r * c.n_count_values + k;
               if (e < n_cb) atomicAdd(&count_bins[e], 1u); else atomicAdd((unsigned long long *)&c.count_hist[e], 1ull);
             },
             [&]() { atomicAdd(&rejected, 1u); });
  __syncthreads();
  for (int32_t e = threadIdx.x; e < n_ib; e += REC_NT) if (index_bins[e]) atomicAdd((unsigned long long *)&c.index_hist[e], (unsigned long long)index_bins[e]);
  for (int32_t e = threadIdx.x; e < n_cb; e += REC_NT) if (count_bins[e]) atomicAdd((unsigned long long *)&c.count_hist[e], (unsigned long long)count_bins[e]);
  if (threadIdx.x == 0 && rejected) atomicAdd((unsigned long long *)c.rejected, (unsigned long long)rejected);
  if (blockIdx.x == 0 && (int32_t)threadIdx.x <= c.R)                           // streams seen, once per call
    atomicAdd((unsigned long long *)&c.streams[threadIdx.x], (unsigned long long)(threadIdx.x == 0 ? (int64_t)c.N * c.R : (int64_t)c.N));
}

// ---- argument checks and launches -----------------------------------------------------------------------------------------------------
const char *tables_args(const uint32_t *index_cum, int32_t n_index_symbols, const uint32_t *count_cum, const int32_t *count_first, int64_t n_count_cum) {
  if (index_cum && n_index_symbols < 2) return "an index table of fewer than 2 symbols";
  if (count_cum && (!count_first || n_count_cum < 0)) return "count tables without count_first, or a negative n_count_cum";
  return nullptr;
}

irec_status launch_encode(irec_rec::EncodeCall &c, const Tables &tb, void *workspace, void *hip_stream) {
  irec_rec::encode_bind_workspace(c, workspace);
  hipStream_t st = (hipStream_t)hip_stream;
  const int64_t streams = 2 * (int64_t)c.N * c.R;
  if (streams > 0) {
    hipLaunchKernelGGL(rec_tables_size_kernel, dim3(rec_grid(streams)), dim3(REC_NT), 0, st, c, tb);
    REC_HIP(hipGetLastError());
  }
  hipLaunchKernelGGL(rec_tables_layout_kernel, dim3(1), dim3(REC_NT), 0, st, c);
  REC_HIP(hipGetLastError());
  if (streams > 0) {
    hipLaunchKernelGGL(rec_tables_write_kernel, dim3(rec_grid(streams + c.N)), dim3(REC_NT), 0, st, c, tb);
    REC_HIP(hipGetLastError());
  }
  return IREC_OK;
}
irec_status launch_decode(const irec_rec::DecodeCall &c, const Tables &tb, void *hip_stream) {
  hipStream_t st = (hipStream_t)hip_stream;
  const int64_t lanes = (int64_t)c.N * c.R;
  hipLaunchKernelGGL(rec_tables_decode_counts_kernel, dim3(rec_grid(lanes)), dim3(REC_NT), 0, st, c, tb);
  REC_HIP(hipGetLastError());
  hipLaunchKernelGGL(rec_tables_decode_indices_kernel, dim3(rec_grid(lanes)), dim3(REC_NT), 0, st, c, tb);
  REC_HIP(hipGetLastError());
  hipLaunchKernelGGL(rec_tables_decode_status_kernel, dim3(c.N < 65536 ? c.N : 65536), dim3(REC_NT), 0, st, c);
  REC_HIP(hipGetLastError());
  return IREC_OK;
}

// [lo, hi) dealt to n_threads host threads (0 = one per core, at most 32) in contiguous ranges; body(e) must not throw
template <class F>
void parallel_range(int64_t n, int32_t n_threads, F &&body) {
  int64_t T = n_threads > 0 ? n_threads : (int64_t)std::thread::hardware_concurrency();
  T = T < 1 ? 1 : (T > 32 ? 32 : T);
  if (T > n) T = n;
  if (T <= 1) { for (int64_t e = 0; e < n; ++e) body(e); return; }
  std::vector<std::thread> pool;
  for (int64_t t = 0; t < T; ++t) pool.emplace_back([&, t]() { for (int64_t e = n * t / T; e < n * (t + 1) / T; ++e) body(e); });
  for (auto &th : pool) th.join();
}

const char *hist_args(HistCall &c, const int32_t *blocks_per_res) {
  if (const char *why = ragged_layout(c.R, blocks_per_res, c.first)) return why;
  if (c.N < 0 || c.max_K < 0 || c.n_index_values < 1 || c.n_count_values < 1 || !c.K || (c.max_K > 0 && !c.idx) || c.k_stride < 1 || c.idx_stride < c.max_K ||
      !c.index_hist || !c.count_hist || !c.streams || !c.rejected)
    return "bad arguments";
  if (((int64_t)c.N * c.first[c.R]) / REC_NT >= 0x7fffffff) return "too many rows for one call";
  return nullptr;
}
} // namespace
} // namespace irec

extern "C" {

irec_status irec_rec_tables_build(const int64_t *counts, int32_t n_symbols, uint32_t *cum) {
  using namespace irec;
  if (!counts || !cum) return set_last_error(IREC_E_INVALID, "irec_rec_tables_build", "null pointer");
  if (n_symbols < 2) return set_last_error(IREC_E_INVALID, "irec_rec_tables_build", "a table needs the terminator and at least one value (n_symbols >= 2)");
  int64_t total = 0;
  for (int32_t m = 0; m < n_symbols; ++m) {
    if (counts[m] < 1) return set_last_error(IREC_E_INVALID, "irec_rec_tables_build", "every count must be at least 1");
    if (counts[m] > (int64_t)irec_rec::QUARTER || (total += counts[m]) > (int64_t)irec_rec::QUARTER)
      return set_last_error(IREC_E_INVALID, "irec_rec_tables_build", "the counts sum to more than 2^30");
  }
  total = 0;
  cum[0] = 0;
  for (int32_t m = 0; m < n_symbols; ++m) { total += counts[m]; cum[m + 1] = (uint32_t)total; }
  return IREC_OK;
}

irec_status irec_rec_encode_files_device_tables(uint32_t seed, uint32_t block_size, uint32_t max_index, uint32_t height, uint32_t width,
                                                uint32_t channels, int32_t n_images, int32_t n_res_blocks, const int32_t *blocks_per_res,
                                                int32_t max_K, const int32_t *K, int64_t k_stride, const int32_t *idx, int64_t idx_stride,
                                                const uint32_t *index_cum, int32_t n_index_symbols, const uint32_t *count_cum,
                                                const int32_t *count_first, int64_t n_count_cum, uint8_t *out, int64_t cap, int64_t *offsets,
                                                int32_t *status, void *workspace, size_t workspace_bytes, void *hip_stream) {
  using namespace irec;
  const char *who = "irec_rec_encode_files_device_tables";
  irec_rec::EncodeCall c{seed, block_size, max_index, height, width, channels, n_images, n_res_blocks, 0, max_K,
                         K, k_stride, idx, idx_stride, out, cap, offsets, status, nullptr, nullptr, nullptr, {}};
  if (const char *why = ragged_layout(n_res_blocks, blocks_per_res, c.first)) return set_last_error(IREC_E_INVALID, who, why);
  if (const char *why = tables_args(index_cum, n_index_symbols, count_cum, count_first, n_count_cum)) return set_last_error(IREC_E_INVALID, who, why);
  if (!encode_args_ok(height, width, channels, n_images, n_res_blocks, 1, max_K, K, k_stride, idx, idx_stride, out, cap, offsets, status))
    return set_last_error(IREC_E_INVALID, who, "bad arguments");
  if (!workspace || ((uintptr_t)workspace & 7) || workspace_bytes < irec_rec_device_workspace_bytes(n_images, n_res_blocks))
    return set_last_error(IREC_E_WORKSPACE, who, "workspace too small (irec_rec_device_workspace_bytes) or not 8-byte aligned");
  return launch_encode(c, Tables{index_cum, n_index_symbols, count_cum, count_first, n_count_cum}, workspace, hip_stream);
}

irec_status irec_rec_decode_files_device_tables(const uint8_t *bytes, const int64_t *offsets, int32_t n_images, int32_t n_res_blocks,
                                                const int32_t *blocks_per_res, int32_t max_K, const uint32_t *index_cum, int32_t n_index_symbols,
                                                const uint32_t *count_cum, const int32_t *count_first, int64_t n_count_cum, uint32_t *headers,
                                                int32_t *K, int32_t *idx, int32_t *status, void *workspace, size_t workspace_bytes,
                                                void *hip_stream) {
  using namespace irec;
  const char *who = "irec_rec_decode_files_device_tables";
  irec_rec::DecodeCall c{bytes, offsets, n_images, n_res_blocks, 0, max_K, headers, K, idx, status, (int32_t *)workspace, {}};
  if (const char *why = ragged_layout(n_res_blocks, blocks_per_res, c.first)) return set_last_error(IREC_E_INVALID, who, why);
  if (const char *why = tables_args(index_cum, n_index_symbols, count_cum, count_first, n_count_cum)) return set_last_error(IREC_E_INVALID, who, why);
  if (!decode_args_ok(bytes, offsets, n_images, n_res_blocks, 1, max_K, headers, K, idx, status))
    return set_last_error(IREC_E_INVALID, who, "bad arguments");
  if (!workspace || ((uintptr_t)workspace & 7) || workspace_bytes < irec_rec_device_workspace_bytes(n_images, n_res_blocks))
    return set_last_error(IREC_E_WORKSPACE, who, "workspace too small (irec_rec_device_workspace_bytes) or not 8-byte aligned");
  if (n_images == 0) return IREC_OK;
  return launch_decode(c, Tables{index_cum, n_index_symbols, count_cum, count_first, n_count_cum}, hip_stream);
}

// ---- the host forms: the same lane functions over host memory, dealt to threads ---------------------------------------------------------
int64_t irec_rec_encode_files_tables(uint32_t seed, uint32_t block_size, uint32_t max_index, uint32_t height, uint32_t width, uint32_t channels,
                                     int32_t n_images, int32_t n_res_blocks, const int32_t *blocks_per_res, int32_t max_K, const int32_t *K,
                                     const int32_t *idx, const uint32_t *index_cum, int32_t n_index_symbols, const uint32_t *count_cum,
                                     const int32_t *count_first, int64_t n_count_cum, uint8_t *out, int64_t cap, int64_t *offsets, int32_t *status,
                                     int32_t n_threads) try {
  using namespace irec;
  const char *who = "irec_rec_encode_files_tables";
  irec_rec::EncodeCall c{seed, block_size, max_index, height, width, channels, n_images, n_res_blocks, 0, max_K,
                         K, 1, idx, max_K, out, cap, offsets, status, nullptr, nullptr, nullptr, {}};
  const char *why = ragged_layout(n_res_blocks, blocks_per_res, c.first);
  if (!why) why = tables_args(index_cum, n_index_symbols, count_cum, count_first, n_count_cum);
  if (!why && !encode_args_ok(height, width, channels, n_images, n_res_blocks, 1, max_K, K, 1, idx, max_K, out, cap, offsets, status)) why = "bad arguments";
  if (why) { set_last_error(IREC_E_INVALID, who, why); return -1; }
  const Tables tb{index_cum, n_index_symbols, count_cum, count_first, n_count_cum};
  std::vector<int64_t> ws((size_t)(irec_rec::encode_workspace_bytes(n_images, n_res_blocks) / 8 + 1));
  irec_rec::encode_bind_workspace(c, ws.data());
  const int64_t streams = 2 * (int64_t)n_images * n_res_blocks;
  parallel_range(streams, n_threads, [&](int64_t lane) { irec_rec::encode_size_lane(c, tb, lane); });
  int64_t at = 0;
  for (int64_t i = 0; i < n_images; ++i) { offsets[i] = at; at += irec_rec::encode_image_bytes(c, i); }
  offsets[n_images] = at;
  parallel_range(streams + n_images, n_threads, [&](int64_t lane) { irec_rec::encode_write_lane(c, tb, lane); });
  return at;
} catch (const std::exception &e) { irec::set_last_error(IREC_E_INVALID, "irec_rec_encode_files_tables", e.what()); return -1; }

irec_status irec_rec_decode_files_tables(const uint8_t *bytes, const int64_t *offsets, int32_t n_images, int32_t n_res_blocks,
                                         const int32_t *blocks_per_res, int32_t max_K, const uint32_t *index_cum, int32_t n_index_symbols,
                                         const uint32_t *count_cum, const int32_t *count_first, int64_t n_count_cum, uint32_t *headers, int32_t *K,
                                         int32_t *idx, int32_t *status, int32_t n_threads) try {
  using namespace irec;
  const char *who = "irec_rec_decode_files_tables";
  irec_rec::DecodeCall c{bytes, offsets, n_images, n_res_blocks, 0, max_K, headers, K, idx, status, nullptr, {}};
  const char *why = ragged_layout(n_res_blocks, blocks_per_res, c.first);
  if (!why) why = tables_args(index_cum, n_index_symbols, count_cum, count_first, n_count_cum);
  if (!why && !decode_args_ok(bytes, offsets, n_images, n_res_blocks, 1, max_K, headers, K, idx, status)) why = "bad arguments";
  if (why) return set_last_error(IREC_E_INVALID, who, why);
  const Tables tb{index_cum, n_index_symbols, count_cum, count_first, n_count_cum};
  std::vector<int32_t> ws((size_t)(2 * (int64_t)n_images * n_res_blocks + 1));
  c.stream_status = ws.data();
  const int64_t lanes = (int64_t)n_images * n_res_blocks;
  parallel_range(lanes, n_threads, [&](int64_t s) { irec_rec::decode_counts_lane(c, tb, s); });
  parallel_range(lanes, n_threads, [&](int64_t s) { irec_rec::decode_indices_lane(c, tb, s); });
  irec_rec::decode_finish_host(c);
  return IREC_OK;
} catch (const std::exception &e) { return irec::set_last_error(IREC_E_INVALID, "irec_rec_decode_files_tables", e.what()); }

// the core in a plain loop on one thread (irec_rec::encode_call_host / decode_call_host over Tables): the test hooks (csrc/irec_internal.h)
irec_status irec_rec_test_core_encode_files_tables(uint32_t seed, uint32_t block_size, uint32_t max_index, uint32_t height, uint32_t width,
                                                   uint32_t channels, int32_t n_images, int32_t n_res_blocks, const int32_t *blocks_per_res,
                                                   int32_t max_K, const int32_t *K, int64_t k_stride, const int32_t *idx, int64_t idx_stride,
                                                   const uint32_t *index_cum, int32_t n_index_symbols, const uint32_t *count_cum,
                                                   const int32_t *count_first, int64_t n_count_cum, uint8_t *out, int64_t cap, int64_t *offsets,
                                                   int32_t *status) try {
  using namespace irec;
  const char *who = "irec_rec_test_core_encode_files_tables";
  irec_rec::EncodeCall c{seed, block_size, max_index, height, width, channels, n_images, n_res_blocks, 0, max_K,
                         K, k_stride, idx, idx_stride, out, cap, offsets, status, nullptr, nullptr, nullptr, {}};
  const char *why = ragged_layout(n_res_blocks, blocks_per_res, c.first);
  if (!why) why = tables_args(index_cum, n_index_symbols, count_cum, count_first, n_count_cum);
  if (!why && !encode_args_ok(height, width, channels, n_images, n_res_blocks, 1, max_K, K, k_stride, idx, idx_stride, out, cap, offsets, status)) why = "bad arguments";
  if (why) return set_last_error(IREC_E_INVALID, who, why);
  std::vector<int64_t> ws((size_t)(irec_rec::encode_workspace_bytes(n_images, n_res_blocks) / 8 + 1));
  irec_rec::encode_bind_workspace(c, ws.data());
  irec_rec::encode_call_host(c, Tables{index_cum, n_index_symbols, count_cum, count_first, n_count_cum});
  return IREC_OK;
} catch (const std::exception &e) { return irec::set_last_error(IREC_E_INVALID, "irec_rec_test_core_encode_files_tables", e.what()); }

irec_status irec_rec_test_core_decode_files_tables(const uint8_t *bytes, const int64_t *offsets, int32_t n_images, int32_t n_res_blocks,
                                                   const int32_t *blocks_per_res, int32_t max_K, const uint32_t *index_cum, int32_t n_index_symbols,
                                                   const uint32_t *count_cum, const int32_t *count_first, int64_t n_count_cum, uint32_t *headers,
                                                   int32_t *K, int32_t *idx, int32_t *status) try {
  using namespace irec;
  const char *who = "irec_rec_test_core_decode_files_tables";
  irec_rec::DecodeCall c{bytes, offsets, n_images, n_res_blocks, 0, max_K, headers, K, idx, status, nullptr, {}};
  const char *why = ragged_layout(n_res_blocks, blocks_per_res, c.first);
  if (!why) why = tables_args(index_cum, n_index_symbols, count_cum, count_first, n_count_cum);
  if (!why && !decode_args_ok(bytes, offsets, n_images, n_res_blocks, 1, max_K, headers, K, idx, status)) why = "bad arguments";
  if (why) return set_last_error(IREC_E_INVALID, who, why);
  std::vector<int32_t> ws((size_t)(2 * (int64_t)n_images * n_res_blocks + 1));
  c.stream_status = ws.data();
  irec_rec::decode_call_host(c, Tables{index_cum, n_index_symbols, count_cum, count_first, n_count_cum});
  return IREC_OK;
} catch (const std::exception &e) { return irec::set_last_error(IREC_E_INVALID, "irec_rec_test_core_decode_files_tables", e.what()); }

// ---- histograms -------------------------------------------------------------------------------------------------------------------------
irec_status irec_rec_hist_rows(int32_t n_images, int32_t n_res_blocks, const int32_t *blocks_per_res, int32_t max_K, const int32_t *K,
                               int64_t k_stride, const int32_t *idx, int64_t idx_stride, int32_t n_index_values, int32_t n_count_values,
                               uint64_t *index_hist, uint64_t *count_hist, uint64_t *streams, uint64_t *rejected) {
  using namespace irec;
  HistCall c{n_images, n_res_blocks, max_K, n_index_values, n_count_values, K, k_stride, idx, idx_stride, index_hist, count_hist, streams, rejected, {}};
  if (const char *why = hist_args(c, blocks_per_res)) return set_last_error(IREC_E_INVALID, "irec_rec_hist_rows", why);
  const int64_t rows = (int64_t)n_images * c.first[c.R];
  for (int64_t b = 0; b < rows; ++b)
    hist_row(c, b, [&](int32_t v) { ++index_hist[v]; }, [&](int32_t r, int32_t k) { ++count_hist[(int64_t)r * n_count_values + k]; }, [&]() { ++*rejected; });
  streams[0] += (uint64_t)((int64_t)n_images * n_res_blocks);
  for (int32_t r = 0; r < n_res_blocks; ++r) streams[1 + r] += (uint64_t)n_images;
  return IREC_OK;
}

irec_status irec_rec_hist_rows_device(int32_t n_images, int32_t n_res_blocks, const int32_t *blocks_per_res, int32_t max_K, const int32_t *K,
                                      int64_t k_stride, const int32_t *idx, int64_t idx_stride, int32_t n_index_values, int32_t n_count_values,
                                      uint64_t *index_hist, uint64_t *count_hist, uint64_t *streams, uint64_t *rejected, void *hip_stream) {
  using namespace irec;
  HistCall c{n_images, n_res_blocks, max_K, n_index_values, n_count_values, K, k_stride, idx, idx_stride, index_hist, count_hist, streams, rejected, {}};
  if (const char *why = hist_args(c, blocks_per_res)) return set_last_error(IREC_E_INVALID, "irec_rec_hist_rows_device", why);
  hipLaunchKernelGGL(rec_hist_rows_kernel, dim3(rec_grid((int64_t)n_images * c.first[c.R])), dim3(REC_NT), 0, (hipStream_t)hip_stream, c);
  REC_HIP(hipGetLastError());
  return IREC_OK;
}

} // extern "C"
