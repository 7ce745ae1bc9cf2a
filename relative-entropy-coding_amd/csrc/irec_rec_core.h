// irec_rec_core.h -- the .rec container and its arithmetic coder once more, in a form that a GPU lane and a host loop run alike:
// irec_ac_encode, ac_decode_impl, irec_rec_pack_bits / unpack_bits and the header layout of irec_rec_encode_file /
// irec_rec_decode_file (irec_io.cpp, which stays the referee: tests/test_rec_device_host.py holds every byte of this file against it).
// Precision 32; the default symbol models in closed form, and empirical ones as cumulative tables the caller owns (TableModel, Tables).
// Plain C++: no allocation, no HIP header; IREC_REC_HD is
// `__host__ __device__` under hipcc and nothing under g++ (scripts/rec_core_check.cpp runs this header under the host sanitizers).
//
// The default models need no table.  A stream over n_values values with weight w (100: partition counts, 1000: indices) has the
// terminator as symbol 0 and value m - 1 as symbol m >= 1:  C[0] = 0, D[0] = 1, C[m] = 1 + (m - 1)(1 + w), D[m] = C[m] + 1 + w,
// R = 1 + n_values (1 + w).  Decoding: v = ((target + 1) R - 1) / width; symbol 0 if v < 1, else min(n_values, 1 + (v - 1) / (1 + w)).
// width <= 2^32 and R <= 2^30 (checked), so width * D and (target + 1) * R stay below 2^62.
//
// One call is 2 N R streams, one lane each: lanes [0, N R) the index streams, [N R, 2 N R) the count streams (a wave holds streams
// of one kind), stream (i, r) of a kind at i R + r.  Every lane function below touches only memory that its lane owns.
//
// Blocks per residual block: one count for the whole call (bpt >= 1, any R), or one per residual block (bpt = 0: "ragged", R <=
// IREC_REC_RAGGED_MAX_RES) as the prefix sums first[r] = sum_{q < r} blocks[q], which travel by value inside the call so that a kernel
// argument carries them.  Either way an image is T = first[R] rows, block j of residual block r of image i is row i T + first[r] + j.
#ifndef IREC_REC_CORE_H_
#define IREC_REC_CORE_H_

#include <stdint.h>

#include "irec.h"

#if defined(__HIPCC__)
#define IREC_REC_HD __host__ __device__
#else
#define IREC_REC_HD
#endif

namespace irec_rec {

constexpr uint64_t WHOLE = (uint64_t)1 << 32, HALF = WHOLE >> 1, QUARTER = WHOLE >> 2;
constexpr int64_t COUNT_WEIGHT = 100, INDEX_WEIGHT = 1000;

enum { ENC_OK = 0, ENC_VALUE = 1, ENC_TABLE = 2 };   // encode_stream: a value without a symbol; a table whose entries cannot be coded under
// What encode_stream / decode_stream ask of a model: R; valid() once per stream; interval(v, C, D) of value v and terminator(C, D) (on
// entry C = 0, D = 1), ENC_*; find(v, sym, C, D): the symbol of decoder quotient v and its interval, false for a table whose entries there
// cannot be coded under.  (Model's forms are, inlined, the statements encode_stream / decode_stream held before they took a model type.)
struct Model {                                        // the closed form above; step = 1 + weight
  uint64_t step, n_values, R;
  IREC_REC_HD bool valid() const { return true; }
  IREC_REC_HD int interval(int64_t v, uint64_t &C, uint64_t &D) const {
    if (v < 0 || (uint64_t)v >= n_values) return ENC_VALUE;
    C = 1 + (uint64_t)v * step; D = C + step;
    return ENC_OK;
  }
  IREC_REC_HD int terminator(uint64_t &, uint64_t &) const { return ENC_OK; }
  IREC_REC_HD bool find(uint64_t v, uint64_t &sym, uint64_t &C, uint64_t &D) const {
    sym = 0;
    if (v >= 1) { sym = 1 + (v - 1) / step; if (sym > n_values) sym = n_values; }
    C = sym ? 1 + (sym - 1) * step : 0; D = sym ? C + step : 1;
    return true;
  }
};
IREC_REC_HD inline Model make_model(uint64_t n_values, int64_t weight) { return Model{(uint64_t)(1 + weight), n_values, 1 + n_values * (uint64_t)(1 + weight)}; }
IREC_REC_HD inline bool model_fits(const Model &m) { return m.R <= QUARTER; }   // (n_values < 2^32: R cannot wrap 64 bits)

// An empirical model: n symbols under the cumulative counts cum[0 .. n], cum[0] = 0, cum[n] = R <= 2^30, symbol m over [cum[m], cum[m + 1])
// (irec_rec_tables_build makes one from counts >= 1).  The array is the caller's: nothing about its CONTENT is taken on trust.  The
// encoder's renormalisation loop ends only because C < D <= R <= 2^30, so valid() holds the ends once per stream and every interval is
// held as it is read; an entry that fails gives ENC_TABLE / false (IREC_REC_E_TABLE), never a loop without end, and no read leaves cum[0 .. n].
struct TableModel {
  const uint32_t *cum; int64_t n; uint64_t R;
  IREC_REC_HD TableModel(const uint32_t *c, int64_t n_) : cum(c), n(c && n_ >= 1 ? n_ : 0), R(n ? c[n] : 0) {}
  IREC_REC_HD bool valid() const { return n >= 1 && cum[0] == 0 && R >= 1 && R <= QUARTER; }
  IREC_REC_HD int interval(int64_t v, uint64_t &C, uint64_t &D) const {
    if (v < 0 || v + 1 >= n) return ENC_VALUE;
    C = cum[v + 1]; D = cum[v + 2];
    return C < D && D <= R ? ENC_OK : ENC_TABLE;
  }
  IREC_REC_HD int terminator(uint64_t &C, uint64_t &D) const { C = cum[0]; D = cum[1]; return C < D && D <= R ? ENC_OK : ENC_TABLE; }
  IREC_REC_HD bool find(uint64_t v, uint64_t &sym, uint64_t &C, uint64_t &D) const {   // the largest j with cum[j] <= v (ac_decode_impl's search)
    int64_t lo = 0, hi = n - 1, j = 0;
    while (lo <= hi) { const int64_t mid = (lo + hi) / 2; if (cum[mid] <= v) { j = mid; lo = mid + 1; } else hi = mid - 1; }
    sym = (uint64_t)j; C = cum[j]; D = cum[j + 1];
    return C < D && D <= R;
  }
};

// ---- bit sinks of the encoder ----------------------------------------------------------------------------------------------------
struct CountingSink {
  int64_t n = 0;
  IREC_REC_HD void put(int, int64_t follow) { n += 1 + follow; }
};
// The marker bit and the code bits, MSB first, right-aligned in nbytes = (n_bits + 8) / 8 bytes (int('1' + code, 2).to_bytes(.., 'big')):
// nbytes * 8 - n_bits - 1 leading zero bits.  Each byte is built in a register and stored whole, inside [out, out + nbytes) only.
struct WritingSink {
  uint8_t *out; int64_t nbytes, pos = 0; uint32_t acc = 1; int nacc; bool bad = false;
  IREC_REC_HD WritingSink(uint8_t *o, int64_t n_bits) : out(o), nbytes((n_bits + 8) / 8), nacc((int)(((n_bits + 8) / 8) * 8 - n_bits)) {
    if (nacc == 8) flush();
  }
  IREC_REC_HD void flush() { if (pos < nbytes) out[pos] = (uint8_t)acc; else bad = true; ++pos; acc = 0; nacc = 0; }
  IREC_REC_HD void push(int bit) { acc = (acc << 1) | (uint32_t)bit; if (++nacc == 8) flush(); }
  IREC_REC_HD void run(int bit, int64_t count) {
    while (count > 0 && nacc != 0) { push(bit); --count; }
    for (; count >= 8; count -= 8) { acc = bit ? 0xFFu : 0u; flush(); }
    for (; count > 0; --count) push(bit);
  }
  IREC_REC_HD void put(int bit, int64_t follow) { push(bit); run(bit ^ 1, follow); }
  IREC_REC_HD bool complete() const { return !bad && pos == nbytes && nacc == 0; }
};

// ArithmeticCoder.encode over n values (fetch(k) = value k, coded as symbol value + 1) and the terminator -- irec_ac_encode.
// The follow-bit counter is 64-bit: max_index = 1 packs thousands of symbols into a bit.  ENC_OK, ENC_VALUE for a value outside the
// model, ENC_TABLE (TableModel only).
template <class M, class Fetch, class Sink>
IREC_REC_HD inline int encode_stream(const M &m, int64_t n, Fetch &fetch, Sink &sink) {
  uint64_t low = 0, high = WHOLE;
  int64_t s = 0;
  if (!m.valid()) return ENC_TABLE;
  for (int64_t k = 0; k <= n; ++k) {
    uint64_t C = 0, D = 1;
    if (k < n) {
      const int64_t v = fetch(k);
      if (const int e = m.interval(v, C, D)) return e;
    } else if (const int e = m.terminator(C, D)) return e;
    const uint64_t width = high - low;
    high = low + (width * D) / m.R;
    low = low + (width * C) / m.R;
    // (width > 2^30 >= R on entry, so high > low here and each loop doubles the width: at most 32 turns)
    while (high < HALF || low > HALF) {
      if (high < HALF) { sink.put(0, s); s = 0; low *= 2; high *= 2; }
      else { sink.put(1, s); s = 0; low = (low - HALF) * 2; high = (high - HALF) * 2; }
    }
    while (low > QUARTER && high < 3 * QUARTER) { s += 1; low = (low - QUARTER) * 2; high = (high - QUARTER) * 2; }
  }
  s += 1;
  sink.put(low <= QUARTER ? 0 : 1, s);
  return 0;
}

// ---- the decoder -----------------------------------------------------------------------------------------------------------------
// The code bits of one stream: bin(int.from_bytes(b, 'big'))[3:] without materialising them.  A bit past the end reads as 0.
struct BitReader {
  const uint8_t *p = nullptr; int64_t n_bytes = 0, first = -1, n_bits = 0;
  IREC_REC_HD bool open(const uint8_t *bytes, int64_t n) {   // false: no marker bit
    p = bytes; n_bytes = n;
    for (int64_t b = 0; b < n; ++b)
      if (bytes[b]) { int k = 0; while (!(bytes[b] & (0x80u >> k))) ++k; first = b * 8 + k; n_bits = n * 8 - first - 1; return true; }
    return false;
  }
  IREC_REC_HD uint64_t bit(int64_t i) const {
    if (i >= n_bits) return 0;
    const int64_t q = first + 1 + i;
    return (q >> 3) < n_bytes ? (uint64_t)((p[q >> 3] >> (7 - (q & 7))) & 1) : 0;
  }
};

enum { DEC_OK = 0, DEC_CORRUPT = 1, DEC_TOO_MANY = 2, DEC_BUDGET = 3, DEC_TABLE = 4 };   // target < 0 or width <= 0; more values than the header allows; shifts ran out; a table entry that cannot be coded under
// ArithmeticCoder.decode_fast -- ac_decode_impl: emit(value) for every symbol before the terminator.  Budgets: at most max_values
// values (the header says how many there are), and n_bits + 64 renormalisation shifts in all (a stream its encoder wrote takes
// n_bits - 2).  *n_out = values emitted.
template <class M, class Emit>
IREC_REC_HD inline int decode_stream(const M &m, const BitReader &in, int64_t max_values, Emit &emit, int64_t *n_out) {
  uint64_t low = 0, high = WHOLE, z = 0;
  int64_t i = 0, n = 0, shifts_left = in.n_bits + 64;
  *n_out = 0;
  if (!m.valid()) return DEC_TABLE;
  while (i < 32 && i < in.n_bits) { z += in.bit(i) << (31 - i); ++i; }
  for (;;) {
    if (z < low || high <= low) return DEC_CORRUPT;   // target < 0 or width <= 0
    const uint64_t width = high - low, target = z - low;
    const uint64_t v = ((target + 1) * m.R - 1) / width;
    uint64_t sym, C, D;
    if (!m.find(v, sym, C, D)) return DEC_TABLE;
    high = low + (width * D) / m.R;
    low = low + (width * C) / m.R;
    if (sym == 0) { *n_out = n; return DEC_OK; }
    if (n >= max_values) return DEC_TOO_MANY;
    emit((int32_t)(sym - 1));
    ++n;
    while (high < HALF || low > HALF) {
      if (--shifts_left < 0) return DEC_BUDGET;
      if (high < HALF) { low *= 2; high *= 2; z *= 2; }
      else { low = (low - HALF) * 2; high = (high - HALF) * 2; z = (z - HALF) * 2; }
      z += in.bit(i); ++i;
    }
    while (low > QUARTER && high < 3 * QUARTER) {
      if (--shifts_left < 0) return DEC_BUDGET;
      low = (low - QUARTER) * 2; high = (high - QUARTER) * 2; z = (z - QUARTER) * 2;
      z += in.bit(i); ++i;
    }
  }
}

// ---- little-endian fields at any alignment -----------------------------------------------------------------------------------------
IREC_REC_HD inline void put_u32(uint8_t *p, uint32_t v) { for (int k = 0; k < 4; ++k) p[k] = (uint8_t)(v >> (8 * k)); }
IREC_REC_HD inline void put_u16(uint8_t *p, uint32_t v) { p[0] = (uint8_t)v; p[1] = (uint8_t)(v >> 8); }
IREC_REC_HD inline uint32_t get_u32(const uint8_t *p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); }
IREC_REC_HD inline uint32_t get_u16(const uint8_t *p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8); }

// ================================================================================================================================
//  Encoding a call: size every stream, lay the files out, write
// ================================================================================================================================
struct EncodeCall {
  uint32_t seed, block_size, max_index, height, width, channels;
  int32_t N, R, bpt, max_K;
  const int32_t *K; int64_t k_stride; const int32_t *idx; int64_t idx_stride;   // block b = i T + first[r] + j: K[b k_stride], idx[b idx_stride + t]
  uint8_t *out; int64_t cap; int64_t *offsets; int32_t *status;
  // workspace: bits of every stream, its status, the largest K of every residual block
  int64_t *n_bits; int32_t *stream_status; int32_t *max_part;
  int32_t first[IREC_REC_RAGGED_MAX_RES + 1];   // bpt = 0 only
};
// the layout of a call (EncodeCall or DecodeCall): blocks of residual block r, its first row within an image, rows per image
template <class Call> IREC_REC_HD inline int32_t res_blocks(const Call &c, int32_t r) { return c.bpt ? c.bpt : c.first[r + 1] - c.first[r]; }
template <class Call> IREC_REC_HD inline int64_t res_first(const Call &c, int32_t r) { return c.bpt ? (int64_t)r * c.bpt : (int64_t)c.first[r]; }
template <class Call> IREC_REC_HD inline int64_t image_blocks(const Call &c) { return c.bpt ? (int64_t)c.R * c.bpt : (int64_t)c.first[c.R]; }
// first[0 .. R] from blocks_per_res[R]; false for R outside [1, IREC_REC_RAGGED_MAX_RES], an entry < 1 or a sum that leaves int32
inline bool ragged_first(int32_t R, const int32_t *blocks_per_res, int32_t *first) {
  if (R < 1 || R > IREC_REC_RAGGED_MAX_RES || !blocks_per_res) return false;
  int64_t at = 0;
  for (int32_t r = 0; r < R; ++r) {
    first[r] = (int32_t)at;
    if (blocks_per_res[r] < 1) return false;
    at += blocks_per_res[r];
    if (at > 0x7fffffff) return false;
  }
  for (int32_t r = R; r <= IREC_REC_RAGGED_MAX_RES; ++r) first[r] = (int32_t)at;
  return true;
}
IREC_REC_HD inline int64_t encode_workspace_bytes(int64_t N, int64_t R) { return 2 * N * R * 8 + 2 * N * R * 4 + N * R * 4; }
IREC_REC_HD inline void encode_bind_workspace(EncodeCall &c, void *ws) {
  const int64_t NR = (int64_t)c.N * c.R;
  c.n_bits = (int64_t *)ws; c.stream_status = (int32_t *)(c.n_bits + 2 * NR); c.max_part = c.stream_status + 2 * NR;
}

// The symbol tables of a call.  NoTables: the default models and nothing else -- what every entry point without "_tables" in its name
// is compiled with, so that its code is what it was.  Tables: either pointer may be null (the default model for that kind of stream).
//   index_cum [n_index_symbols + 1]: the one table of every index stream;
//   count_cum [n_count_cum], count_first [R + 1]: the table of residual block r is count_cum[count_first[r] .. count_first[r + 1]), that
//   is n_r + 1 entries for n_r symbols (K <= n_r - 2).  count_first is caller data like the rest: a lane holds its two entries against
//   n_count_cum before it reads a table through them.
struct NoTables { static constexpr bool any = false; };
struct Tables {
  static constexpr bool any = true;
  const uint32_t *index_cum; int32_t n_index_symbols;
  const uint32_t *count_cum; const int32_t *count_first; int64_t n_count_cum;
};
// the count table of residual block r: false if count_first does not describe one inside count_cum
IREC_REC_HD inline bool count_table(const Tables &tb, int32_t r, const uint32_t **cum, int64_t *n) {
  const int64_t f0 = tb.count_first[r], f1 = tb.count_first[r + 1];
  if (f0 < 0 || f1 - f0 < 2 || f1 > tb.n_count_cum) return false;
  *cum = tb.count_cum + f0; *n = f1 - f0 - 1;
  return true;
}
IREC_REC_HD inline int32_t encode_status(int e, int32_t value_status) { return e == ENC_OK ? IREC_REC_OK : e == ENC_TABLE ? IREC_REC_E_TABLE : value_status; }

struct CountFetch {
  const int32_t *K; int64_t k_stride, b0;
  IREC_REC_HD int64_t operator()(int64_t k) const { return K[(b0 + k) * k_stride]; }
};
struct IndexFetch {   // value number k of a residual block, asked for in order: row j up to its K, then row j + 1
  const int32_t *K; int64_t k_stride; const int32_t *idx; int64_t idx_stride, b0; int32_t j = 0, t = 0, kj;
  IREC_REC_HD IndexFetch(const int32_t *K_, int64_t ks, const int32_t *idx_, int64_t is, int64_t b0_)
      : K(K_), k_stride(ks), idx(idx_), idx_stride(is), b0(b0_), kj(K_[b0_ * ks]) {}
  IREC_REC_HD int64_t operator()(int64_t) {
    while (t >= kj) { ++j; t = 0; kj = K[(b0 + j) * k_stride]; }
    return idx[(b0 + j) * idx_stride + t++];
  }
};

// the bits of one stream, through `sink`; what the sizing pass and the writing pass share
template <class T, class Sink>
IREC_REC_HD inline int32_t encode_lane_stream(const EncodeCall &c, const T &tb, int64_t lane, Sink &sink, int32_t *max_part_out) {
  const int64_t NR = (int64_t)c.N * c.R;
  const bool counts = lane >= NR;
  const int64_t s = counts ? lane - NR : lane;
  const int32_t r = (int32_t)(s % c.R), nb = res_blocks(c, r);
  const int64_t b0 = (s / c.R) * image_blocks(c) + res_first(c, r);
  int32_t mx = 0; int64_t tot = 0;
  for (int32_t j = 0; j < nb; ++j) {
    const int32_t k = c.K[(b0 + j) * c.k_stride];
    if (k < 0 || k > c.max_K) return IREC_REC_E_K_RANGE;
    mx = k > mx ? k : mx; tot += k;
  }
  if (max_part_out) *max_part_out = mx;
  if (counts) {
    if constexpr (T::any) if (tb.count_cum) {
      const uint32_t *cum; int64_t n;
      if (!count_table(tb, r, &cum, &n)) return IREC_REC_E_TABLE;
      CountFetch f{c.K, c.k_stride, b0};
      return encode_status(encode_stream(TableModel(cum, n), nb, f, sink), IREC_REC_E_K_RANGE);
    }
    const Model m = make_model((uint64_t)mx + 1, COUNT_WEIGHT);
    if (!model_fits(m)) return IREC_REC_E_MODEL_RANGE;
    CountFetch f{c.K, c.k_stride, b0};
    return encode_stream(m, nb, f, sink) ? IREC_REC_E_K_RANGE : IREC_REC_OK;
  }
  if constexpr (T::any) if (tb.index_cum) {
    IndexFetch f(c.K, c.k_stride, c.idx, c.idx_stride, b0);
    return encode_status(encode_stream(TableModel(tb.index_cum, tb.n_index_symbols), tot, f, sink), IREC_REC_E_INDEX_RANGE);
  }
  const Model m = make_model(c.max_index, INDEX_WEIGHT);
  if (!model_fits(m)) return IREC_REC_E_MODEL_RANGE;
  IndexFetch f(c.K, c.k_stride, c.idx, c.idx_stride, b0);
  return encode_stream(m, tot, f, sink) ? IREC_REC_E_INDEX_RANGE : IREC_REC_OK;
}

// launch 1, lane < 2 N R
template <class T>
IREC_REC_HD inline void encode_size_lane(const EncodeCall &c, const T &tb, int64_t lane) {
  const int64_t NR = (int64_t)c.N * c.R;
  CountingSink sink;
  int32_t mx = 0;
  const int32_t st = encode_lane_stream(c, tb, lane, sink, &mx);
  c.stream_status[lane] = st;
  c.n_bits[lane] = st ? 0 : sink.n;
  if (lane >= NR) c.max_part[lane - NR] = mx;
}
IREC_REC_HD inline void encode_size_lane(const EncodeCall &c, int64_t lane) { encode_size_lane(c, NoTables{}, lane); }
IREC_REC_HD inline int64_t stream_bytes(int64_t n_bits) { return (n_bits + 8) / 8; }

// launch 2, per image: its status (a K out of range first, as the host reports it) and its file's bytes (0 with an error status)
IREC_REC_HD inline int64_t encode_image_bytes(const EncodeCall &c, int64_t i) {
  const int64_t NR = (int64_t)c.N * c.R;
  int32_t st = IREC_REC_OK;
  int64_t bytes = 28 + 16 * (int64_t)c.R;
  for (int32_t r = 0; r < c.R; ++r) {
    const int32_t sc = c.stream_status[NR + i * c.R + r], sx = c.stream_status[i * c.R + r];
    if (sc == IREC_REC_E_K_RANGE || sx == IREC_REC_E_K_RANGE) st = IREC_REC_E_K_RANGE;
    else if (st == IREC_REC_OK) st = sc ? sc : sx;
    bytes += stream_bytes(c.n_bits[NR + i * c.R + r]) + stream_bytes(c.n_bits[i * c.R + r]);
  }
  c.status[i] = st;
  return st ? 0 : bytes;
}

// launch 3, lane < 2 N R + N: the streams, then one header per image.  Nothing at all is written when the files do not fit cap.
// A kind of stream coded under a table sets its header flag (words 6: counts, 7: indices); with count tables the largest-K words are
// 0xFFFFFFFF, the reference's pack of -1.
template <class T>
IREC_REC_HD inline void encode_write_lane(const EncodeCall &c, const T &tb, int64_t lane) {
  const int64_t NR = (int64_t)c.N * c.R;
  if (c.offsets[c.N] > c.cap) return;
  if (lane >= 2 * NR) {                           // header of image i, fields as irec_rec_encode_file puts them
    const int64_t i = lane - 2 * NR;
    if (c.status[i]) return;
    uint8_t *f = c.out + c.offsets[i];
    put_u32(f, c.seed); put_u32(f + 4, c.block_size); put_u32(f + 8, c.max_index); put_u32(f + 12, c.height); put_u32(f + 16, c.width);
    bool count_flag = false, index_flag = false;
    if constexpr (T::any) { count_flag = tb.count_cum != nullptr; index_flag = tb.index_cum != nullptr; }
    put_u16(f + 20, c.channels); put_u16(f + 22, count_flag ? 1 : 0); put_u16(f + 24, index_flag ? 1 : 0); put_u16(f + 26, (uint32_t)c.R);
    for (int32_t r = 0; r < c.R; ++r) {
      uint8_t *d = f + 28 + 4 * r;
      put_u32(d, (uint32_t)res_blocks(c, r));
      put_u32(d + 4 * c.R, (uint32_t)stream_bytes(c.n_bits[NR + i * c.R + r]));
      put_u32(d + 8 * c.R, (uint32_t)stream_bytes(c.n_bits[i * c.R + r]));
      put_u32(d + 12 * c.R, count_flag ? 0xFFFFFFFFu : (uint32_t)c.max_part[i * c.R + r]);
    }
    return;
  }
  const bool counts = lane >= NR;
  const int64_t s = counts ? lane - NR : lane, i = s / c.R, r = s % c.R;
  if (c.status[i]) return;
  int64_t at = c.offsets[i] + 28 + 16 * (int64_t)c.R;    // count streams first, then index streams
  for (int32_t q = 0; q < (counts ? r : c.R); ++q) at += stream_bytes(c.n_bits[NR + i * c.R + q]);
  if (!counts) for (int32_t q = 0; q < r; ++q) at += stream_bytes(c.n_bits[i * c.R + q]);
  const int64_t nb = c.n_bits[lane];
  if (at < c.offsets[i] || at + stream_bytes(nb) > c.offsets[i + 1]) return;   // (cannot happen: the layout pass summed these very sizes)
  WritingSink sink(c.out + at, nb);
  encode_lane_stream(c, tb, lane, sink, nullptr);
}
IREC_REC_HD inline void encode_write_lane(const EncodeCall &c, int64_t lane) { encode_write_lane(c, NoTables{}, lane); }

// ================================================================================================================================
//  Decoding a call: headers and count streams, index streams, one status per image
// ================================================================================================================================
struct DecodeCall {
  const uint8_t *bytes; const int64_t *offsets; int32_t N, R, bpt, max_K;
  uint32_t *headers; int32_t *K; int32_t *idx; int32_t *status;   // K [N][T], idx [N][T][max_K]: residual block r of image i from row i T + first[r]
  int32_t *stream_status;   // workspace [2 N R], laid out like the encoder's lanes
  int32_t first[IREC_REC_RAGGED_MAX_RES + 1];   // bpt = 0 only
};
IREC_REC_HD inline int64_t decode_workspace_bytes(int64_t N, int64_t R) { return 2 * N * R * 4; }

struct StreamLoc { int64_t c_pos, c_len, x_pos, x_len; uint32_t max_part, max_index; bool count_flag, index_flag; };

// Every check of irec_rec_decode_file that does not need a stream decoded, for residual block r of a file, plus the batched reader's
// (R and the blocks of residual block r as the caller says).  The file is only read inside [file, file + n_bytes).
// have_count / have_index: the call brought a table for that kind.  A kind whose flag the file sets is read under the call's table
// (loc->count_flag / index_flag), or is IREC_REC_E_COUNT_FILES without one; a kind whose flag is clear is read under the default model
// whatever the call brought.  With the count flag the largest-K word is not a number (0xFFFFFFFF) and the two checks that rest on the
// default model's least bits per symbol do not hold: what bounds the blocks then is the call's own count (IREC_REC_E_STRUCTURE below).
// TB = false (the entry points without tables) is the reader as it was: either flag set is IREC_REC_E_COUNT_FILES.
template <bool TB>
IREC_REC_HD inline int32_t decode_locate(const uint8_t *file, int64_t n_bytes, int32_t R, int32_t bpt, int32_t r, StreamLoc *loc, uint32_t *hdr9,
                                         bool have_count, bool have_index) {
  if (n_bytes < 28) return IREC_REC_E_TRUNCATED_HEADER;
  uint32_t h[9];
  for (int k = 0; k < 5; ++k) h[k] = get_u32(file + 4 * k);
  for (int k = 0; k < 4; ++k) h[5 + k] = get_u16(file + 20 + 2 * k);
  if (hdr9) for (int k = 0; k < 9; ++k) hdr9[k] = h[k];
  if constexpr (!TB) { if (h[6] || h[7]) return IREC_REC_E_COUNT_FILES; }
  else if ((h[6] && !have_count) || (h[7] && !have_index)) return IREC_REC_E_COUNT_FILES;
  const int64_t Rf = h[8];
  if (n_bytes < 28 + 16 * Rf) return IREC_REC_E_TRUNCATED_HEADER;
  if (h[2] < 1u || h[2] > (1u << 24)) return IREC_REC_E_MAX_INDEX;
  if (Rf != R) return IREC_REC_E_STRUCTURE;
  const uint8_t *dyn = file + 28;
  int64_t pos = 28 + 16 * Rf, off_x = pos;
  for (int64_t q = 0; q < Rf; ++q) off_x += get_u32(dyn + 4 * (Rf + q));
  for (int64_t q = 0; q < r; ++q) { pos += get_u32(dyn + 4 * (Rf + q)); off_x += get_u32(dyn + 4 * (2 * Rf + q)); }
  const int64_t nc = get_u32(dyn + 4 * (Rf + r)), nx = get_u32(dyn + 4 * (2 * Rf + r)), mx = get_u32(dyn + 4 * (3 * Rf + r));
  const int64_t blocks = get_u32(dyn + 4 * r), blocks_cap = (mx >= 1 ? 1 : 72) * (8 * nc + 8);
  if ((!TB || !h[6]) && (mx > IREC_MAX_PARTITIONS || blocks > blocks_cap)) return IREC_REC_E_BLOCK_COUNTS;
  if (pos + nc > n_bytes || off_x + nx > n_bytes) return IREC_REC_E_TRUNCATED_STREAMS;
  if (blocks != bpt) return IREC_REC_E_STRUCTURE;
  loc->c_pos = pos; loc->c_len = nc; loc->x_pos = off_x; loc->x_len = nx; loc->max_part = (uint32_t)mx; loc->max_index = h[2];
  if constexpr (TB) { loc->count_flag = h[6] != 0; loc->index_flag = h[7] != 0; }
  return IREC_REC_OK;
}

struct CountEmit {
  int32_t *row; int32_t bpt, max_K, n = 0; bool over = false;
  IREC_REC_HD void operator()(int32_t v) { if (v > max_K) over = true; if (n < bpt) row[n] = v; ++n; }
};
struct IndexEmit {   // value after value into row j up to its K, the rest of every row zero
  const int32_t *Krow; int32_t *rows; int32_t bpt, max_K, j = 0, t = 0;
  IREC_REC_HD void skip() { while (j < bpt && t >= Krow[j]) { for (int32_t q = t; q < max_K; ++q) rows[(int64_t)j * max_K + q] = 0; ++j; t = 0; } }
  IREC_REC_HD void operator()(int32_t v) { skip(); if (j < bpt) rows[(int64_t)j * max_K + t++] = v; }
  IREC_REC_HD void finish() { skip(); while (j < bpt) { for (int32_t q = t; q < max_K; ++q) rows[(int64_t)j * max_K + q] = 0; ++j; t = 0; } }
};

// launch 1, lane < N R: the checks of residual block r of image i, its K row; lane r = 0 also leaves the image's header
template <class T>
IREC_REC_HD inline void decode_counts_lane(const DecodeCall &c, const T &tb, int64_t s) {
  const int64_t NR = (int64_t)c.N * c.R, i = s / c.R;
  const int32_t r = (int32_t)(s % c.R), nb = res_blocks(c, r);
  int32_t *row = c.K + i * image_blocks(c) + res_first(c, r);
  c.stream_status[s] = IREC_REC_OK;
  const int64_t lo = c.offsets[i], n_bytes = c.offsets[i + 1] - lo;
  StreamLoc loc;
  bool have_count = false, have_index = false;
  if constexpr (T::any) { have_count = tb.count_cum != nullptr; have_index = tb.index_cum != nullptr; }
  int32_t st = lo < 0 || n_bytes < 0 ? IREC_REC_E_TRUNCATED_HEADER
                                     : decode_locate<T::any>(c.bytes + lo, n_bytes, c.R, nb, r, &loc, r == 0 ? c.headers + 9 * i : nullptr, have_count, have_index);
  if (st == IREC_REC_OK) {
    BitReader in;
    CountEmit emit{row, nb, c.max_K};
    int64_t n = 0;
    if (!in.open(c.bytes + lo + loc.c_pos, loc.c_len)) st = IREC_REC_E_COUNT_MARKER;
    else {
      int d = DEC_TABLE;
      bool by_table = false;
      if constexpr (T::any) if (loc.count_flag) {
        const uint32_t *cum; int64_t nt;
        by_table = true;
        if (count_table(tb, r, &cum, &nt)) d = decode_stream(TableModel(cum, nt), in, nb, emit, &n);
      }
      if (!by_table) d = decode_stream(make_model((uint64_t)loc.max_part + 1, COUNT_WEIGHT), in, nb, emit, &n);
      if (d == DEC_TABLE) st = IREC_REC_E_TABLE;
      else if (d == DEC_CORRUPT) st = IREC_REC_E_COUNT_CORRUPT;
      else if (d == DEC_BUDGET) st = IREC_REC_E_COUNT_BUDGET;
      else if (d == DEC_TOO_MANY || n != nb) st = IREC_REC_E_MISMATCH;
      else if (emit.over) st = IREC_REC_E_MAX_K;
    }
  }
  c.stream_status[NR + s] = st;
}

IREC_REC_HD inline void decode_counts_lane(const DecodeCall &c, int64_t s) { decode_counts_lane(c, NoTables{}, s); }

// launch 2, lane < N R: the index stream of (i, r) into its rows, by the K of launch 1
template <class T>
IREC_REC_HD inline void decode_indices_lane(const DecodeCall &c, const T &tb, int64_t s) {
  const int64_t NR = (int64_t)c.N * c.R, i = s / c.R;
  const int32_t r = (int32_t)(s % c.R), nb = res_blocks(c, r);
  const int64_t row0 = i * image_blocks(c) + res_first(c, r);
  if (c.stream_status[NR + s]) return;            // no K to go by (the image's outputs are zeroed by the last launch)
  const int64_t lo = c.offsets[i], n_bytes = c.offsets[i + 1] - lo;
  StreamLoc loc;
  bool have_count = false, have_index = false;
  if constexpr (T::any) { have_count = tb.count_cum != nullptr; have_index = tb.index_cum != nullptr; }
  int32_t st = decode_locate<T::any>(c.bytes + lo, n_bytes, c.R, nb, r, &loc, nullptr, have_count, have_index);
  if (st == IREC_REC_OK) {
    const int32_t *Krow = c.K + row0;
    int64_t tot = 0, n = 0;
    for (int32_t j = 0; j < nb; ++j) tot += Krow[j];
    const Model m = make_model(loc.max_index, INDEX_WEIGHT);
    BitReader in;
    IndexEmit emit{Krow, c.idx + row0 * (int64_t)c.max_K, nb, c.max_K};
    bool by_table = false;
    if constexpr (T::any) by_table = loc.index_flag;
    if (!by_table && !model_fits(m)) st = IREC_REC_E_INDEX_MODEL;
    else if (!in.open(c.bytes + lo + loc.x_pos, loc.x_len)) st = IREC_REC_E_INDEX_MARKER;
    else {
      int d = DEC_TABLE;
      if constexpr (T::any) if (by_table) d = decode_stream(TableModel(tb.index_cum, tb.n_index_symbols), in, tot, emit, &n);
      if (!by_table) d = decode_stream(m, in, tot, emit, &n);
      if (d == DEC_TABLE) st = IREC_REC_E_TABLE;
      else if (d == DEC_CORRUPT) st = IREC_REC_E_INDEX_CORRUPT;
      else if (d == DEC_BUDGET) st = IREC_REC_E_INDEX_BUDGET;
      else if (d == DEC_TOO_MANY || n != tot) st = IREC_REC_E_MISMATCH;
    }
    emit.finish();
  }
  c.stream_status[s] = st;
}

IREC_REC_HD inline void decode_indices_lane(const DecodeCall &c, int64_t s) { decode_indices_lane(c, NoTables{}, s); }

// launch 3: the status of image i = the first cause among its residual blocks, counts before indices as the host reads them
IREC_REC_HD inline int32_t decode_block_status(const DecodeCall &c, int64_t s) {
  const int64_t NR = (int64_t)c.N * c.R;
  return c.stream_status[NR + s] ? c.stream_status[NR + s] : c.stream_status[s];
}

// ---- a whole call over host memory, lane after lane in a plain loop: what the kernels of irec_rec.hip do, for the stand-alone check
//      programs (scripts/rec_*_check.cpp; the workspace bound by the caller).  The library's own host forms deal the same lanes to
//      threads: irec_rec_call.h -------------------------------------------------------------------------------------------------------
template <class T>
inline void encode_call_host(const EncodeCall &c, const T &tb) {
  const int64_t streams = 2 * (int64_t)c.N * c.R;
  for (int64_t lane = 0; lane < streams; ++lane) encode_size_lane(c, tb, lane);
  int64_t at = 0;
  for (int64_t i = 0; i < c.N; ++i) { c.offsets[i] = at; at += encode_image_bytes(c, i); }
  c.offsets[c.N] = at;
  for (int64_t lane = 0; lane < streams + c.N; ++lane) encode_write_lane(c, tb, lane);
}
inline void encode_call_host(const EncodeCall &c) { encode_call_host(c, NoTables{}); }
inline void decode_finish_host(const DecodeCall &c);
template <class T>
inline void decode_call_host(const DecodeCall &c, const T &tb) {
  const int64_t lanes = (int64_t)c.N * c.R;
  for (int64_t s = 0; s < lanes; ++s) decode_counts_lane(c, tb, s);
  for (int64_t s = 0; s < lanes; ++s) decode_indices_lane(c, tb, s);
  decode_finish_host(c);
}
inline void decode_call_host(const DecodeCall &c) { decode_call_host(c, NoTables{}); }
inline void decode_finish_host(const DecodeCall &c) {   // launch 3
  const int64_t nK = image_blocks(c), nI = nK * c.max_K;
  for (int64_t i = 0; i < c.N; ++i) {
    int32_t st = 0;
    for (int32_t r = 0; r < c.R && !st; ++r) st = decode_block_status(c, i * c.R + r);
    c.status[i] = st;
    if (st) {
      for (int k = 0; k < 9; ++k) c.headers[9 * i + k] = 0;
      for (int64_t e = 0; e < nK; ++e) c.K[i * nK + e] = 0;
      for (int64_t e = 0; e < nI; ++e) c.idx[i * nI + e] = 0;
    }
  }
}

} // namespace irec_rec
#endif // IREC_REC_CORE_H_
