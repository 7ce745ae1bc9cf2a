// irec_rec_call.h -- the one way from the arguments of a .rec entry point (include/irec.h, csrc/irec_internal.h) to a checked call of the
// coder (csrc/irec_rec_core.h): the layout, the tables, the argument and workspace checks with the texts and the order every entry
// keeps, and the coder over host memory dealt to threads.  Host code only, no HIP header; irec_rec.hip (the codec) and irec_rec_tables.hip
// (the histograms) add the kernels.
#ifndef IREC_REC_CALL_H_
#define IREC_REC_CALL_H_
#include <cstdint>
#include <exception>
#include <vector>

#include "irec_call.h"
#include "irec_internal.h"
#include "irec_rec_core.h"

namespace irec {
namespace {
constexpr int REC_NT = 256;   // lanes of a workgroup
inline int rec_grid(int64_t lanes) { const int64_t g = (lanes + REC_NT - 1) / REC_NT; return (int)(g < 1 ? 1 : g); }

// blocks_per_res[R] of a ragged call (a host array) as the prefix sums the call carries; nullptr, or why not
inline const char *ragged_layout(int32_t R, const int32_t *blocks_per_res, int32_t *first) {
  if (R < 1 || R > IREC_REC_RAGGED_MAX_RES) return "n_res_blocks outside [1, IREC_REC_RAGGED_MAX_RES]";
  if (!blocks_per_res) return "blocks_per_res is null";
  for (int32_t r = 0; r < R; ++r) if (blocks_per_res[r] < 1) return "an entry of blocks_per_res is below 1";
  if (!irec_rec::ragged_first(R, blocks_per_res, first)) return "the blocks of an image do not fit int32";
  return nullptr;
}
// The blocks per residual block as an entry point is given them: one count for the whole call (any R up to 65535), or a host array of
// R <= IREC_REC_RAGGED_MAX_RES counts.
struct Layout {
  bool is_ragged; int32_t bpt; const int32_t *per_res;
  static Layout uniform(int32_t bpt) { return {false, bpt, nullptr}; }
  static Layout ragged(const int32_t *per_res) { return {true, 0, per_res}; }
};

inline const char *tables_args(const irec_rec::Tables &tb) {
  if (tb.index_cum && tb.n_index_symbols < 2) return "an index table of fewer than 2 symbols";
  if (tb.count_cum && (!tb.count_first || tb.n_count_cum < 0)) return "count tables without count_first, or a negative n_count_cum";
  return nullptr;
}
inline bool args_ok(const irec_rec::EncodeCall &c) {
  return c.N >= 0 && c.R >= 1 && c.R <= 65535 && c.max_K >= 0 && c.K && (c.max_K == 0 || c.idx) && c.offsets && (c.N == 0 || c.status) && c.cap >= 0 &&
         (c.cap == 0 || c.out) && c.k_stride >= 1 && c.idx_stride >= c.max_K && c.height <= 65535 && c.width <= 65535 && c.channels <= 65535 &&
         (2 * (int64_t)c.N * c.R + c.N) / REC_NT < 0x7fffffff;
}
inline bool args_ok(const irec_rec::DecodeCall &c) {
  return c.bytes && c.offsets && c.N >= 0 && c.R >= 1 && c.R <= 65535 && c.max_K >= 0 && (c.N == 0 || (c.headers && c.K && c.status)) &&
         (c.N == 0 || c.max_K == 0 || c.idx) && ((int64_t)c.N * c.R) / REC_NT < 0x7fffffff;
}

// A call (EncodeCall or DecodeCall) whose other fields hold the entry point's arguments gets its layout, and it and the tables (nullptr:
// none) are held to include/irec.h.  IREC_OK, or IREC_E_INVALID under the entry's name with the first cause, in the one order: the
// layout, the tables, everything else as "bad arguments".
template <class Call>
irec_status prepare(Call &c, const Layout &lay, const irec_rec::Tables *tb, const char *who) {
  c.bpt = lay.bpt;
  const char *why = lay.is_ragged ? ragged_layout(c.R, lay.per_res, c.first) : nullptr;
  if (!why && tb) why = tables_args(*tb);
  if (!why && !((lay.is_ragged || lay.bpt >= 1) && args_ok(c))) why = "bad arguments";
  return why ? set_last_error(IREC_E_INVALID, who, why) : IREC_OK;
}
// the same for a device entry: then the workspace
template <class Call>
irec_status prepare_device(Call &c, const Layout &lay, const irec_rec::Tables *tb, const void *workspace, size_t workspace_bytes, const char *who) {
  if (irec_status e = prepare(c, lay, tb, who)) return e;
  return check_workspace(irec_rec_device_workspace_bytes(c.N, c.R), workspace, workspace_bytes, who, "irec_rec_device_workspace_bytes");
}

// A prepared call over host memory, what the three launches of a direction do: the lanes sized, the files laid out, the lanes written
// (offsets[N] = the bytes of all files); the counts, the indices, the verdicts.  tb: irec_rec::NoTables or Tables.
template <class T>
irec_status run_encode_host(irec_rec::EncodeCall &c, const T &tb, int32_t n_threads, const char *who) try {
  std::vector<int64_t> ws((size_t)(irec_rec::encode_workspace_bytes(c.N, c.R) / 8 + 1));
  irec_rec::encode_bind_workspace(c, ws.data());
  const int64_t streams = 2 * (int64_t)c.N * c.R;
  parallel_chunks(streams, n_threads, 1, [&](int64_t lo, int64_t hi) { for (int64_t l = lo; l < hi; ++l) irec_rec::encode_size_lane(c, tb, l); });
  int64_t at = 0;
  for (int64_t i = 0; i < c.N; ++i) { c.offsets[i] = at; at += irec_rec::encode_image_bytes(c, i); }
  c.offsets[c.N] = at;
  parallel_chunks(streams + c.N, n_threads, 1, [&](int64_t lo, int64_t hi) { for (int64_t l = lo; l < hi; ++l) irec_rec::encode_write_lane(c, tb, l); });
  return IREC_OK;
} catch (const std::exception &e) { return set_last_error(IREC_E_INVALID, who, e.what()); }

template <class T>
irec_status run_decode_host(irec_rec::DecodeCall &c, const T &tb, int32_t n_threads, const char *who) try {
  std::vector<int32_t> ws((size_t)(2 * (int64_t)c.N * c.R + 1));
  c.stream_status = ws.data();
  const int64_t lanes = (int64_t)c.N * c.R;
  parallel_chunks(lanes, n_threads, 1, [&](int64_t lo, int64_t hi) { for (int64_t l = lo; l < hi; ++l) irec_rec::decode_counts_lane(c, tb, l); });
  parallel_chunks(lanes, n_threads, 1, [&](int64_t lo, int64_t hi) { for (int64_t l = lo; l < hi; ++l) irec_rec::decode_indices_lane(c, tb, l); });
  irec_rec::decode_finish_host(c);
  return IREC_OK;
} catch (const std::exception &e) { return set_last_error(IREC_E_INVALID, who, e.what()); }
} // namespace
} // namespace irec

#endif // IREC_REC_CALL_H_
