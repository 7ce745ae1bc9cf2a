// irec_rec_tables.hip -- what the empirical symbol tables of the .rec container are made from (include/irec.h: irec_rec_tables_build,
// irec_rec_hist_rows*).  The codec under such tables (irec_rec_*_tables) is in irec_rec.hip with the rest of the codec.
// Histograms: rec_hist_rows_kernel, one lane per row, the bins of a workgroup in LDS, one integer atomicAdd per non-empty bin per workgroup.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "irec_rec_call.h"

namespace irec {
namespace {
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
  IREC_HIP(hipGetLastError());
  return IREC_OK;
}

} // extern "C"
