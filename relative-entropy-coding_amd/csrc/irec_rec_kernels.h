// irec_rec_kernels.h -- what the two device units of the .rec container share (irec_rec.hip: the default models; irec_rec_tables.hip:
// empirical tables): the workgroup size, the bodies of the two launches that no model enters (the layout scan of the writer, the
// per-image verdict of the reader), the argument checks of the entry points and the error macro.
#ifndef IREC_REC_KERNELS_H_
#define IREC_REC_KERNELS_H_
#include <hip/hip_runtime.h>

#include <cstdint>

#include "irec_internal.h"
#include "irec_rec_core.h"

namespace irec {
irec_status set_last_error(irec_status code, const char *who, const char *what);   // irec_host.cpp

namespace {
constexpr int REC_NT = 256;

// One workgroup: lane t takes the images [t * per, (t + 1) * per), so any N is covered; the 256 partial sums are scanned in LDS.
__device__ inline void rec_layout_body(irec_rec::EncodeCall c) {
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

inline int rec_grid(int64_t lanes) { const int64_t g = (lanes + REC_NT - 1) / REC_NT; return (int)(g < 1 ? 1 : g); }

inline bool encode_args_ok(uint32_t height, uint32_t width, uint32_t channels, int32_t N, int32_t R, int32_t bpt, int32_t max_K, const int32_t *K,
                           int64_t k_stride, const int32_t *idx, int64_t idx_stride, const uint8_t *out, int64_t cap, const int64_t *offsets,
                           const int32_t *status) {
  return N >= 0 && R >= 1 && R <= 65535 && bpt >= 1 && max_K >= 0 && K && (max_K == 0 || idx) && offsets && (N == 0 || status) && cap >= 0 &&
         (cap == 0 || out) && k_stride >= 1 && idx_stride >= max_K && height <= 65535 && width <= 65535 && channels <= 65535 &&
         (2 * (int64_t)N * R + N) / REC_NT < 0x7fffffff;
}
inline bool decode_args_ok(const uint8_t *bytes, const int64_t *offsets, int32_t N, int32_t R, int32_t bpt, int32_t max_K, const uint32_t *headers,
                           const int32_t *K, const int32_t *idx, const int32_t *status) {
  return bytes && offsets && N >= 0 && R >= 1 && R <= 65535 && bpt >= 1 && max_K >= 0 && (N == 0 || (headers && K && status)) &&
         (N == 0 || max_K == 0 || idx) && ((int64_t)N * R) / REC_NT < 0x7fffffff;
}
// blocks_per_res[R] of a ragged call (a host array) as the prefix sums the call carries; nullptr, or why not
inline const char *ragged_layout(int32_t R, const int32_t *blocks_per_res, int32_t *first) {
  if (R < 1 || R > IREC_REC_RAGGED_MAX_RES) return "n_res_blocks outside [1, IREC_REC_RAGGED_MAX_RES]";
  if (!blocks_per_res) return "blocks_per_res is null";
  for (int32_t r = 0; r < R; ++r) if (blocks_per_res[r] < 1) return "an entry of blocks_per_res is below 1";
  if (!irec_rec::ragged_first(R, blocks_per_res, first)) return "the blocks of an image do not fit int32";
  return nullptr;
}
} // namespace
} // namespace irec

#define REC_HIP(expr)                                                                                   \
  do {                                                                                                  \
    hipError_t e_ = (expr);                                                                             \
    if (e_ != hipSuccess) return irec::set_last_error(IREC_E_HIP, #expr, hipGetErrorString(e_));         \
  } while (0)

#endif // IREC_REC_KERNELS_H_
