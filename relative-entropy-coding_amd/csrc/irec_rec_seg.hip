// irec_rec_seg.hip -- the segmented .rec container (NAME.recs) on the device and on host threads: include/irec.h's
// irec_rec_*_files_segmented, irec_rec_*_files_device_segmented, and the test hooks (csrc/irec_internal.h).  The coder is
// csrc/irec_rec_core.h, the lane functions csrc/irec_rec_seg_core.h; the kernels here only deal those lanes out.
//
// One lane per stream of a segment, 2 N S streams per call (S segments per image), index streams first and count streams after them,
// so that a wave holds streams of one kind.  The rules of irec_rec.hip: 256-lane workgroups, plain launches, plain vector loads and
// stores, no atomics, every store into a byte range that only its lane owns, every loop with a budget.
//   encode:  rec_seg_size_kernel (bits of every stream, input checks, the largest K of every segment)
//            -> rec_seg_layout_kernel (one workgroup per image: its segments scanned in chunks into stream positions, its status, its bytes)
//            -> rec_seg_offsets_kernel (exclusive scan over the images' bytes: offsets; a file with an error has none)
//            -> rec_seg_write_kernel (headers, directory, streams; nothing at all if the files do not fit cap)
//   decode:  rec_seg_locate_kernel (one workgroup per image: header and directory held against the call and the file's length, the
//            directory scanned in chunks into stream positions) -> rec_seg_decode_counts_kernel (K) -> rec_seg_decode_indices_kernel
//            (index rows by that K) -> rec_seg_decode_status_kernel (one status per image; the outputs of a refused image zeroed)
// An image has up to several thousand segments (a Kodak image at g = 1: 315), so the two per-image scans give lane t the segments
// [t per, (t + 1) per) and scan the 256 partial sums in LDS, as rec_layout_kernel does over images: 3 KB of LDS, no limit on occupancy.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "irec_rec_call.h"
#include "irec_rec_seg_core.h"

namespace irec {
namespace {
using irec_rec::SegDecodeCall;
using irec_rec::SegEncodeCall;
using irec_rec::SegLayout;

__global__ __launch_bounds__(REC_NT) void rec_seg_size_kernel(SegEncodeCall c) {
  const int64_t lane = (int64_t)blockIdx.x * REC_NT + threadIdx.x;
  if (lane < 2 * (int64_t)c.e.N * c.L.S) irec_rec::seg_encode_size_lane(c, lane);
}

__global__ __launch_bounds__(REC_NT) void rec_seg_write_kernel(SegEncodeCall c) {
  const int64_t lane = (int64_t)blockIdx.x * REC_NT + threadIdx.x;
  if (lane < 2 * (int64_t)c.e.N * c.L.S + c.e.N) irec_rec::seg_encode_write_lane(c, lane);
}

// part[] inclusive-scanned and keys[] reduced to keys[0], over the workgroup; every lane has stored its own entry of both
__device__ inline void scan_and_least(int64_t *part, int32_t *keys) {
  const int t = threadIdx.x;
  __syncthreads();
  for (int d = 1; d < REC_NT; d *= 2) {
    const int64_t add = t >= d ? part[t - d] : 0;
    __syncthreads();
    part[t] += add;
    __syncthreads();
  }
  for (int d = REC_NT / 2; d > 0; d /= 2) {
    if (t < d && keys[t + d] < keys[t]) keys[t] = keys[t + d];
    __syncthreads();
  }
}

// One workgroup per image: what irec_rec::seg_encode_layout_image does in a plain loop.
__global__ __launch_bounds__(REC_NT) void rec_seg_layout_kernel(SegEncodeCall c) {
  __shared__ int64_t part[REC_NT];
  __shared__ int32_t keys[REC_NT];
  const int t = threadIdx.x;
  const int32_t S = c.L.S, per = (S + REC_NT - 1) / REC_NT;
  const int32_t lo = t * per < S ? t * per : S, hi = lo + per < S ? lo + per : S;
  for (int64_t i = blockIdx.x; i < c.e.N; i += gridDim.x) {
    int64_t sum = 0;
    int32_t key = irec_rec::SEG_NO_KEY;
    for (int32_t sl = lo; sl < hi; ++sl) {
      const int32_t k = irec_rec::seg_encode_key(c, i * S + sl, sl);
      key = k < key ? k : key;
      sum += irec_rec::seg_pair_bytes(c, i * S + sl);
    }
    part[t] = sum; keys[t] = key;
    scan_and_least(part, keys);
    int64_t at = irec_rec::seg_header_bytes(c.e.R, S) + part[t] - sum;             // exclusive
    for (int32_t sl = lo; sl < hi; ++sl) { c.seg_pos[i * S + sl] = at; at += irec_rec::seg_pair_bytes(c, i * S + sl); }
    if (t == REC_NT - 1) {
      c.e.status[i] = irec_rec::seg_key_status(keys[0]);
      c.image_bytes[i] = keys[0] == irec_rec::SEG_NO_KEY ? irec_rec::seg_header_bytes(c.e.R, S) + part[t] : 0;
    }
    __syncthreads();
  }
}

// One workgroup: lane t takes the images [t per, (t + 1) per), so any N is covered (rec_layout_kernel's scan, over bytes already summed).
__global__ __launch_bounds__(REC_NT) void rec_seg_offsets_kernel(SegEncodeCall c) {
  __shared__ int64_t part[REC_NT];
  const int t = threadIdx.x;
  const int64_t per = ((int64_t)c.e.N + REC_NT - 1) / REC_NT, lo = t * per < c.e.N ? t * per : c.e.N, hi = lo + per < c.e.N ? lo + per : c.e.N;
  int64_t sum = 0;
  for (int64_t i = lo; i < hi; ++i) sum += c.image_bytes[i];
  part[t] = sum;
  __syncthreads();
  for (int d = 1; d < REC_NT; d *= 2) {
    const int64_t add = t >= d ? part[t - d] : 0;
    __syncthreads();
    part[t] += add;
    __syncthreads();
  }
  int64_t at = part[t] - sum;
  for (int64_t i = lo; i < hi; ++i) { c.e.offsets[i] = at; at += c.image_bytes[i]; }
  if (t == REC_NT - 1) c.e.offsets[c.e.N] = part[t];
}

// One workgroup per image: what irec_rec::seg_decode_locate_image does in a plain loop.  Every lane holds the fixed header against the
// call for itself (the verdict is uniform over the workgroup); a directory that lies inside the file is then scanned in chunks.
__global__ __launch_bounds__(REC_NT) void rec_seg_locate_kernel(SegDecodeCall c) {
  __shared__ int64_t part[REC_NT];
  __shared__ int32_t keys[REC_NT];
  const int t = threadIdx.x;
  const int32_t S = c.L.S, per = (S + REC_NT - 1) / REC_NT;
  const int32_t lo = t * per < S ? t * per : S, hi = lo + per < S ? lo + per : S;
  for (int64_t i = blockIdx.x; i < c.d.N; i += gridDim.x) {
    const int64_t first = c.d.offsets[i], n_bytes = c.d.offsets[i + 1] - first;
    const uint8_t *file = c.d.bytes + first;
    const int32_t hs = first < 0 || n_bytes < 0 ? IREC_REC_E_TRUNCATED_HEADER
                                                : irec_rec::seg_locate_header(c, file, n_bytes, t == 0 ? c.d.headers + 9 * i : nullptr);
    int64_t sum = 0;
    int32_t key = irec_rec::SEG_NO_KEY;
    if (!hs)
      for (int32_t sl = lo; sl < hi; ++sl) {
        const irec_rec::SegEntry e = irec_rec::seg_entry(file, c.d.R, sl);
        const int32_t k = irec_rec::seg_locate_key(c, e, sl);
        key = k < key ? k : key;
        sum += e.cb + e.xb;
      }
    part[t] = sum; keys[t] = key;
    scan_and_least(part, keys);
    int64_t at = irec_rec::seg_header_bytes(c.d.R, S) + part[t] - sum;             // exclusive
    for (int32_t sl = lo; sl < hi; ++sl) {
      c.seg_pos[i * S + sl] = at;
      if (!hs) { const irec_rec::SegEntry e = irec_rec::seg_entry(file, c.d.R, sl); at += e.cb + e.xb; }
    }
    if (t == REC_NT - 1) c.loc_status[i] = irec_rec::seg_locate_status(hs, irec_rec::seg_header_bytes(c.d.R, S) + part[t], n_bytes, keys[0]);
    __syncthreads();
  }
}

__global__ __launch_bounds__(REC_NT) void rec_seg_decode_counts_kernel(SegDecodeCall c) {
  const int64_t lane = (int64_t)blockIdx.x * REC_NT + threadIdx.x;
  if (lane < (int64_t)c.d.N * c.L.S) irec_rec::seg_decode_counts_lane(c, lane);
}

__global__ __launch_bounds__(REC_NT) void rec_seg_decode_indices_kernel(SegDecodeCall c) {
  const int64_t lane = (int64_t)blockIdx.x * REC_NT + threadIdx.x;
  if (lane < (int64_t)c.d.N * c.L.S) irec_rec::seg_decode_indices_lane(c, lane);
}

// One workgroup per image: the first cause among its segments, and zeroed outputs if there is one (rec_decode_status_kernel's form).
__global__ __launch_bounds__(REC_NT) void rec_seg_decode_status_kernel(SegDecodeCall c) {
  __shared__ int32_t first[REC_NT];
  const int t = threadIdx.x;
  for (int64_t i = blockIdx.x; i < c.d.N; i += gridDim.x) {
    int32_t mine = irec_rec::SEG_NO_KEY;                                           // (sl << 8 | status) of the first failing segment this lane saw
    for (int32_t sl = t; sl < c.L.S; sl += REC_NT) {
      const int32_t st = irec_rec::seg_decode_status(c, i * c.L.S + sl);
      if (st && mine == irec_rec::SEG_NO_KEY) mine = (sl << 8) | st;
    }
    first[t] = mine;
    __syncthreads();
    for (int d = REC_NT / 2; d > 0; d /= 2) {
      if (t < d && first[t + d] < first[t]) first[t] = first[t + d];
      __syncthreads();
    }
    const int32_t st = irec_rec::seg_key_status(first[0]);
    __syncthreads();
    if (t == 0) c.d.status[i] = st;
    if (st) {
      const int64_t nK = c.d.first[c.d.R], nI = nK * c.d.max_K;
      if (t < 9) c.d.headers[9 * i + t] = 0;
      for (int64_t e = t; e < nK; e += REC_NT) c.d.K[i * nK + e] = 0;
      for (int64_t e = t; e < nI; e += REC_NT) c.d.idx[i * nI + e] = 0;
    }
  }
}

// ---- from an entry point's arguments to a checked call: irec_rec_call.h's preparation under the ragged layout, then the segments -----
template <class Call>
irec_status prepare_segmented(Call &inner, SegLayout &L, const int32_t *blocks_per_res, int32_t segment_blocks, const char *who) {
  if (irec_status e = prepare(inner, Layout::ragged(blocks_per_res), nullptr, who)) return e;
  if (segment_blocks < 1) return set_last_error(IREC_E_INVALID, who, "segment_blocks is below 1");
  if (!irec_rec::seg_layout(inner.R, inner.first, segment_blocks, &L)) return set_last_error(IREC_E_INVALID, who, "more than 2^22 segments per image");
  if ((2 * (int64_t)inner.N * L.S + inner.N) / REC_NT >= 0x7fffffff) return set_last_error(IREC_E_INVALID, who, "more segments than a launch holds");
  return IREC_OK;
}

// The threads worth starting for a call of `rows` blocks: starting and joining a thread costs what coding some two thousand symbols
// does, so a thread is started per SEG_SLOTS_PER_THREAD symbol slots (rows (1 + max_K): an upper bound that needs no pass over K), at
// most irec_call.h's host_threads(n_threads).  The two per-image steps (a few adds per segment) run on the calling thread.
constexpr int64_t SEG_SLOTS_PER_THREAD = 8192;
inline int32_t seg_threads(int32_t n_threads, int64_t rows, int32_t max_K) {
  const int64_t T = host_threads(n_threads);
  const int64_t worth = 1 + rows * (1 + (int64_t)max_K) / SEG_SLOTS_PER_THREAD;
  return (int32_t)(T < worth ? T : worth);
}

// the coder over host memory, the lanes dealt to threads
irec_status run_seg_encode_host(SegEncodeCall &c, int32_t n_threads, bool plain_loop, const char *who) try {
  std::vector<int64_t> ws((size_t)(irec_rec::seg_encode_workspace_bytes(c.e.N, c.L.S) / 8 + 1));
  irec_rec::seg_encode_bind_workspace(c, ws.data());
  if (plain_loop) { irec_rec::seg_encode_call_host(c); return IREC_OK; }
  const int64_t streams = 2 * (int64_t)c.e.N * c.L.S;
  const int32_t T = seg_threads(n_threads, (int64_t)c.e.N * c.e.first[c.e.R], c.e.max_K);
  parallel_chunks(streams, T, 1, [&](int64_t lo, int64_t hi) { for (int64_t l = lo; l < hi; ++l) irec_rec::seg_encode_size_lane(c, l); });
  int64_t at = 0;
  for (int64_t i = 0; i < c.e.N; ++i) { irec_rec::seg_encode_layout_image(c, i); c.e.offsets[i] = at; at += c.image_bytes[i]; }
  c.e.offsets[c.e.N] = at;
  parallel_chunks(streams + c.e.N, T, 1, [&](int64_t lo, int64_t hi) { for (int64_t l = lo; l < hi; ++l) irec_rec::seg_encode_write_lane(c, l); });
  return IREC_OK;
} catch (const std::exception &e) { return set_last_error(IREC_E_INVALID, who, e.what()); }

irec_status run_seg_decode_host(SegDecodeCall &c, int32_t n_threads, bool plain_loop, const char *who) try {
  std::vector<int64_t> ws((size_t)(irec_rec::seg_decode_workspace_bytes(c.d.N, c.L.S) / 8 + 1));
  irec_rec::seg_decode_bind_workspace(c, ws.data());
  if (plain_loop) { irec_rec::seg_decode_call_host(c); return IREC_OK; }
  const int64_t lanes = (int64_t)c.d.N * c.L.S;
  const int32_t T = seg_threads(n_threads, (int64_t)c.d.N * c.d.first[c.d.R], c.d.max_K);
  for (int64_t i = 0; i < c.d.N; ++i) irec_rec::seg_decode_locate_image(c, i);
  parallel_chunks(lanes, T, 1, [&](int64_t lo, int64_t hi) { for (int64_t l = lo; l < hi; ++l) irec_rec::seg_decode_counts_lane(c, l); });
  parallel_chunks(lanes, T, 1, [&](int64_t lo, int64_t hi) { for (int64_t l = lo; l < hi; ++l) irec_rec::seg_decode_indices_lane(c, l); });
  irec_rec::seg_decode_finish_host(c);
  return IREC_OK;
} catch (const std::exception &e) { return set_last_error(IREC_E_INVALID, who, e.what()); }

inline int per_image_grid(int32_t n) { return n < 65536 ? (n < 1 ? 1 : n) : 65536; }
} // namespace
} // namespace irec

using namespace irec;
using irec_rec::DecodeCall;
using irec_rec::EncodeCall;

extern "C" {

size_t irec_rec_seg_workspace_bytes(int32_t n_images, int32_t n_res_blocks, const int32_t *blocks_per_res, int32_t segment_blocks) {
  int32_t first[IREC_REC_RAGGED_MAX_RES + 1];
  SegLayout L;
  if (n_images < 0 || !irec_rec::ragged_first(n_res_blocks, blocks_per_res, first) || !irec_rec::seg_layout(n_res_blocks, first, segment_blocks, &L)) return 0;
  const int64_t e = irec_rec::seg_encode_workspace_bytes(n_images, L.S), d = irec_rec::seg_decode_workspace_bytes(n_images, L.S);
  return (size_t)((e > d ? e : d) + 256);
}

irec_status irec_rec_encode_files_device_segmented(uint32_t seed, uint32_t block_size, uint32_t max_index, uint32_t height, uint32_t width,
                                                   uint32_t channels, int32_t n_images, int32_t n_res_blocks, const int32_t *blocks_per_res,
                                                   int32_t segment_blocks, int32_t max_K, const int32_t *K, int64_t k_stride, const int32_t *idx,
                                                   int64_t idx_stride, uint8_t *out, int64_t cap, int64_t *offsets, int32_t *status, void *workspace,
                                                   size_t workspace_bytes, void *hip_stream) {
  const char *who = "irec_rec_encode_files_device_segmented";
  SegEncodeCall c{EncodeCall{seed, block_size, max_index, height, width, channels, n_images, n_res_blocks, 0, max_K, K, k_stride, idx, idx_stride, out, cap, offsets, status}};
  if (irec_status e = prepare_segmented(c.e, c.L, blocks_per_res, segment_blocks, who)) return e;
  if (irec_status e = check_workspace(irec_rec::seg_encode_workspace_bytes(c.e.N, c.L.S), workspace, workspace_bytes, who, "irec_rec_seg_workspace_bytes")) return e;
  irec_rec::seg_encode_bind_workspace(c, workspace);
  hipStream_t st = (hipStream_t)hip_stream;
  const int64_t streams = 2 * (int64_t)c.e.N * c.L.S;
  if (streams > 0) {
    hipLaunchKernelGGL(rec_seg_size_kernel, dim3(rec_grid(streams)), dim3(REC_NT), 0, st, c);
    IREC_HIP(hipGetLastError());
    hipLaunchKernelGGL(rec_seg_layout_kernel, dim3(per_image_grid(c.e.N)), dim3(REC_NT), 0, st, c);
    IREC_HIP(hipGetLastError());
  }
  hipLaunchKernelGGL(rec_seg_offsets_kernel, dim3(1), dim3(REC_NT), 0, st, c);
  IREC_HIP(hipGetLastError());
  if (streams > 0) {
    hipLaunchKernelGGL(rec_seg_write_kernel, dim3(rec_grid(streams + c.e.N)), dim3(REC_NT), 0, st, c);
    IREC_HIP(hipGetLastError());
  }
  return IREC_OK;
}

irec_status irec_rec_decode_files_device_segmented(const uint8_t *bytes, const int64_t *offsets, int32_t n_images, int32_t n_res_blocks,
                                                   const int32_t *blocks_per_res, int32_t segment_blocks, int32_t max_K, uint32_t *headers,
                                                   int32_t *K, int32_t *idx, int32_t *status, void *workspace, size_t workspace_bytes,
                                                   void *hip_stream) {
  const char *who = "irec_rec_decode_files_device_segmented";
  SegDecodeCall c{DecodeCall{bytes, offsets, n_images, n_res_blocks, 0, max_K, headers, K, idx, status}};
  if (irec_status e = prepare_segmented(c.d, c.L, blocks_per_res, segment_blocks, who)) return e;
  if (irec_status e = check_workspace(irec_rec::seg_decode_workspace_bytes(c.d.N, c.L.S), workspace, workspace_bytes, who, "irec_rec_seg_workspace_bytes")) return e;
  irec_rec::seg_decode_bind_workspace(c, workspace);
  if (c.d.N == 0) return IREC_OK;
  hipStream_t st = (hipStream_t)hip_stream;
  const int64_t lanes = (int64_t)c.d.N * c.L.S;
  hipLaunchKernelGGL(rec_seg_locate_kernel, dim3(per_image_grid(c.d.N)), dim3(REC_NT), 0, st, c);
  IREC_HIP(hipGetLastError());
  hipLaunchKernelGGL(rec_seg_decode_counts_kernel, dim3(rec_grid(lanes)), dim3(REC_NT), 0, st, c);
  IREC_HIP(hipGetLastError());
  hipLaunchKernelGGL(rec_seg_decode_indices_kernel, dim3(rec_grid(lanes)), dim3(REC_NT), 0, st, c);
  IREC_HIP(hipGetLastError());
  hipLaunchKernelGGL(rec_seg_decode_status_kernel, dim3(per_image_grid(c.d.N)), dim3(REC_NT), 0, st, c);
  IREC_HIP(hipGetLastError());
  return IREC_OK;
}

// ---- the host forms: the same lane functions over host memory, dealt to n_threads over (image, segment) ----------------------------------
int64_t irec_rec_encode_files_segmented(uint32_t seed, uint32_t block_size, uint32_t max_index, uint32_t height, uint32_t width, uint32_t channels,
                                        int32_t n_images, int32_t n_res_blocks, const int32_t *blocks_per_res, int32_t segment_blocks, int32_t max_K,
                                        const int32_t *K, const int32_t *idx, uint8_t *out, int64_t cap, int64_t *offsets, int32_t *status,
                                        int32_t n_threads) {
  const char *who = "irec_rec_encode_files_segmented";
  SegEncodeCall c{EncodeCall{seed, block_size, max_index, height, width, channels, n_images, n_res_blocks, 0, max_K, K, 1, idx, max_K, out, cap, offsets, status}};
  if (prepare_segmented(c.e, c.L, blocks_per_res, segment_blocks, who)) return -1;
  return run_seg_encode_host(c, n_threads, false, who) ? -1 : offsets[n_images];
}

irec_status irec_rec_decode_files_segmented(const uint8_t *bytes, const int64_t *offsets, int32_t n_images, int32_t n_res_blocks,
                                            const int32_t *blocks_per_res, int32_t segment_blocks, int32_t max_K, uint32_t *headers, int32_t *K,
                                            int32_t *idx, int32_t *status, int32_t n_threads) {
  const char *who = "irec_rec_decode_files_segmented";
  SegDecodeCall c{DecodeCall{bytes, offsets, n_images, n_res_blocks, 0, max_K, headers, K, idx, status}};
  if (irec_status e = prepare_segmented(c.d, c.L, blocks_per_res, segment_blocks, who)) return e;
  return run_seg_decode_host(c, n_threads, false, who);
}

// ---- the test hooks (csrc/irec_internal.h): the device entries without workspace and stream, the core over host memory in a plain loop ---
irec_status irec_rec_test_core_encode_files_segmented(uint32_t seed, uint32_t block_size, uint32_t max_index, uint32_t height, uint32_t width,
                                                      uint32_t channels, int32_t n_images, int32_t n_res_blocks, const int32_t *blocks_per_res,
                                                      int32_t segment_blocks, int32_t max_K, const int32_t *K, int64_t k_stride, const int32_t *idx,
                                                      int64_t idx_stride, uint8_t *out, int64_t cap, int64_t *offsets, int32_t *status) {
  const char *who = "irec_rec_test_core_encode_files_segmented";
  SegEncodeCall c{EncodeCall{seed, block_size, max_index, height, width, channels, n_images, n_res_blocks, 0, max_K, K, k_stride, idx, idx_stride, out, cap, offsets, status}};
  if (irec_status e = prepare_segmented(c.e, c.L, blocks_per_res, segment_blocks, who)) return e;
  return run_seg_encode_host(c, 1, true, who);
}

irec_status irec_rec_test_core_decode_files_segmented(const uint8_t *bytes, const int64_t *offsets, int32_t n_images, int32_t n_res_blocks,
                                                      const int32_t *blocks_per_res, int32_t segment_blocks, int32_t max_K, uint32_t *headers,
                                                      int32_t *K, int32_t *idx, int32_t *status) {
  const char *who = "irec_rec_test_core_decode_files_segmented";
  SegDecodeCall c{DecodeCall{bytes, offsets, n_images, n_res_blocks, 0, max_K, headers, K, idx, status}};
  if (irec_status e = prepare_segmented(c.d, c.L, blocks_per_res, segment_blocks, who)) return e;
  return run_seg_decode_host(c, 1, true, who);
}

} // extern "C"
