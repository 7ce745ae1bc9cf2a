// irec_rows_core.h -- the verdict on a decoder's rows (include/irec.h: irec_decode_rows_status) in a form that a GPU lane and a host loop
// run alike.  The decode entry points answer a row they cannot decode (K out of range, an index outside [0, S)) with p_loc, silently;
// this is the check the Python layer makes on the host before a launch, for rows that never leave the device.
// Plain C++: no allocation, no HIP header; IREC_ROWS_HD is `__host__ __device__` under hipcc and nothing under g++
// (scripts/rows_core_check.cpp runs this header under the host sanitizers).
//
// A group is one image's blocks in one residual block: blocks j = 0 .. bpg - 1, block j at row b = block_row[g * bpg + j] (or
// g * bpg + j), its count at K[b * k_stride], its indices at idx[b * idx_stride + t].  A block's cause, first that applies:
//   K < min_K or K > max_K -> K_RANGE;  K > k_limit -> RATIO_TABLE;  an index outside [0, n_samples) among the first K -> INDEX_RANGE.
// The index loop runs only for min_K <= K <= max_K, so no read goes past idx[b * idx_stride + max_K - 1], whatever K holds.
// A group's status is the cause of its LOWEST failing block; a nonzero status already present is kept.
#ifndef IREC_ROWS_CORE_H_
#define IREC_ROWS_CORE_H_

#include <stdint.h>

#include "irec.h"

#if defined(__HIPCC__)
#define IREC_ROWS_HD __host__ __device__
#else
#define IREC_ROWS_HD
#endif

namespace irec_rows {

struct Call {
  int64_t n_groups; int32_t bpg; const int32_t *block_row;
  const int32_t *K; int64_t k_stride; const int32_t *idx; int64_t idx_stride;
  int32_t max_K, min_K, k_limit, n_samples; int32_t *status;
};

constexpr int32_t NONE = 0x7fffffff;            // "no failing block seen": larger than every (j << 2 | cause), j < 2^28
constexpr int32_t MAX_BPG = 1 << 28;

IREC_ROWS_HD inline int32_t block_cause(const Call &c, int64_t b) {
  const int32_t k = c.K[b * c.k_stride];
  if (k < c.min_K || k > c.max_K) return IREC_ROWS_E_K_RANGE;
  if (k > c.k_limit) return IREC_ROWS_E_RATIO_TABLE;
  const int32_t *row = c.idx + b * c.idx_stride;
  for (int32_t t = 0; t < k; ++t) {             // (k <= max_K here)
    const int32_t v = row[t];
    if (v < 0 || v >= c.n_samples) return IREC_ROWS_E_INDEX_RANGE;
  }
  return IREC_ROWS_OK;
}

// The lane function: (j << 2 | cause) of the first failing block among j = first, first + step, ... of group g, or NONE.
IREC_ROWS_HD inline int32_t lane_first(const Call &c, int64_t g, int32_t first, int32_t step) {
  for (int64_t j = first; j < c.bpg; j += step) {
    const int64_t at = g * c.bpg + j, b = c.block_row ? (int64_t)c.block_row[at] : at;
    const int32_t cause = block_cause(c, b);
    if (cause) return (int32_t)(j << 2) | cause;
  }
  return NONE;
}

// What ONE lane of a group does with the smallest code of its lanes: the only read and the only write of status[g].
IREC_ROWS_HD inline void group_store(const Call &c, int64_t g, int32_t code) {
  if (code != NONE && c.status[g] == 0) c.status[g] = code & 3;
}

IREC_ROWS_HD inline bool args_ok(const Call &c) {
  return c.n_groups >= 0 && c.bpg >= 1 && c.bpg <= MAX_BPG && c.max_K >= 0 && c.K && (c.max_K == 0 || c.idx) && c.k_stride >= 1 &&
         c.idx_stride >= c.max_K && c.n_samples >= 1 && (c.n_groups == 0 || c.status);
}

// a whole call over host memory, group after group: what rows_status_kernel does
inline void call_host(const Call &c) {
  for (int64_t g = 0; g < c.n_groups; ++g) group_store(c, g, lane_first(c, g, 0, 1));
}

} // namespace irec_rows
#endif /* IREC_ROWS_CORE_H_ */
