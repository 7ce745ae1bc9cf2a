// irec_res_core.h -- the .res container: an image's pixels, arithmetic-coded under the model's discretized-logistic likelihood given the
// reconstruction, in a form that a GPU lane and a host loop run alike (the manner of irec_rec_core.h, whose 32-bit coder this is:
// WHOLE / HALF / QUARTER, follow bits).  Plain C++: no allocation, no libm, no HIP header; compiled with -ffp-contract=off.
//
// The model of a pixel (DESIGN.md §3 "residual"): symbol x in [0, 255] stands for x/256 - 0.5.  With m = rint(loc * 4096) clamped to
// [-2048, 2047] and inv = 1 / (4096 s) in float64, the cumulative counts over 2^16 are
//     C(0) = 0,  C(256) = 65536,  C(k) = k + floor(G(k) * 65280),  G(k) = 1 / (1 + exp(-(16 k - 2048 - m) * inv))      (0 < k < 256)
// so that every symbol has a count of at least 1 and the edge bins take the tails.  exp is res_exp below: float64 + - * / in a fixed
// order, the argument clamped to [-700, 700].  The scale is confined to [2^-24, 2^24]: there a step of k moves the argument of exp by at
// least 2^-32, ten thousand times what res_exp's last bits can do, so C is strictly increasing whatever those bits are.
//
// The coder differs from irec_rec_core.h's in two things: every symbol brings its own (C, D) over R = 2^16 (the two divisions of the
// encoder are shifts), and the number of symbols is known, so there is no terminator symbol.  A stream is its code bits MSB first,
// padded with zero bits to whole bytes; a bit past the end reads as 0.
//
// Container, little-endian, fields at any alignment:
//     0 magic 'IRES' u32 | 4 version u16 | 6 channels u16 | 8 stream_len u32 | 12 height u32 | 16 width u32 | 20 float32 bits of s u32 |
//     24 checksum u32 | 28 n_streams x u16 byte length | the streams back to back
// Version 2 (one scale per channel; the policy ChannelScales below) differs in the version word and in the scale words alone:
//     0 .. 19 as above with version 2 | 20 + 4 c float32 bits of s_c u32, c < channels | 20 + 4 channels checksum u32 |
//     24 + 4 channels n_streams x u16 byte length | the streams back to back
// Symbol p of an image belongs to channel p / (height width); a stream that crosses a channel boundary goes on under the next
// channel's inv = 1 / (4096 s_c) from the boundary's symbol on.  The model of a pixel given (m, s_c) is the one above.
// Image i's symbols are its C H W bytes in tensor order; stream j covers [j L, min((j + 1) L, C H W)); lane i n_streams + j.
// checksum = sum mod 2^32 over symbols of mix(((p << 8) | x) + 0x9E3779B9) with p the symbol's position and mix the 32-bit finalizer
// below, a bijection: one wrong pixel always changes it, and being linear in neither p nor x it does not cancel over the +1 / -1
// patterns that a decoder on another loc produces (a term linear in x and p did, in scripts/res_core_check.cpp's damaged set).  Every lane function below stores only into memory that its lane owns.
#ifndef IREC_RES_CORE_H_
#define IREC_RES_CORE_H_

#include <stdint.h>

#include "irec.h"
#include "irec_rec_core.h"

namespace irec_res {

using irec_rec::WHOLE;
using irec_rec::HALF;
using irec_rec::QUARTER;
using irec_rec::put_u32;
using irec_rec::put_u16;
using irec_rec::get_u32;
using irec_rec::get_u16;

constexpr uint32_t MAGIC = 0x53455249u, VERSION = 1, VERSION_SCALES = 2;   // "IRES"
constexpr int TOTAL_BITS = 16;
constexpr uint32_t TOTAL = 1u << TOTAL_BITS, N_SYMBOLS = 256;
constexpr int64_t HEADER_BYTES = 28, MAX_STREAM_LEN = 4096;
// Bits of a stream of n symbols: a symbol leaves a width above 2^14 (count >= 1 of 2^16, width above 2^30 on entry), so at most 18
// shifts bring it back above 2^30; every shift is one bit, the end adds two.  4096 symbols: 9217 bytes, inside the u16 length word.
constexpr int64_t MAX_BITS_PER_SYMBOL = 18;

// ---- the model --------------------------------------------------------------------------------------------------------------------
// exp over [-700, 700] in float64: the operation sequence of det_exp (irec_device.h), restated here so that this header stays plain C++.
IREC_REC_HD inline double res_exp(double x) {
  const double kf = __builtin_floor(x * 1.4426950408889634 + 0.5);
  const double r = (x - kf * 0.693147180369123816490) - kf * 1.90821492927058770002e-10;
  double p = 1.0 / 6227020800.0;
  p = p * r + 1.0 / 479001600.0;
  p = p * r + 1.0 / 39916800.0;
  p = p * r + 1.0 / 3628800.0;
  p = p * r + 1.0 / 362880.0;
  p = p * r + 1.0 / 40320.0;
  p = p * r + 1.0 / 5040.0;
  p = p * r + 1.0 / 720.0;
  p = p * r + 1.0 / 120.0;
  p = p * r + 1.0 / 24.0;
  p = p * r + 1.0 / 6.0;
  p = p * r + 0.5;
  p = p * r + 1.0;
  p = p * r + 1.0;
  const int64_t k = (int64_t)kf;                                                // in [-1010, 1010]
  return p * __builtin_bit_cast(double, (uint64_t)(k + 1023) << 52);
}

IREC_REC_HD inline bool scale_ok(float s) { return s >= 5.9604644775390625e-08f && s <= 16777216.0f; }   // [2^-24, 2^24]; a NaN fails both
IREC_REC_HD inline double model_inv(float s) { return 1.0 / (4096.0 * (double)s); }
IREC_REC_HD inline bool is_finite(float v) { return (__builtin_bit_cast(uint32_t, v) & 0x7F800000u) != 0x7F800000u; }

// m = rint(loc * 4096) clamped to [-2048, 2047].  The product is exact; adding and taking away 1.5 * 2^23 rounds it to an integer,
// ties to even, in the rounding mode both sides run in.  A NaN gives -2048.
IREC_REC_HD inline int32_t loc_to_m(float loc) {
  const float v = loc * 4096.0f;
  if (!(v >= -2048.0f)) return -2048;
  if (v >= 2047.0f) return 2047;
  const float r = (v + 12582912.0f) - 12582912.0f;
  return (int32_t)r;
}

IREC_REC_HD inline uint32_t cum(int32_t m, double inv, int32_t k) {
  if (k <= 0) return 0;
  if (k >= (int32_t)N_SYMBOLS) return TOTAL;
  double t = (double)(16 * k - 2048 - m) * inv;
  t = t < -700.0 ? -700.0 : (t > 700.0 ? 700.0 : t);
  const double G = 1.0 / (1.0 + res_exp(-t));
  return (uint32_t)k + (uint32_t)(G * (double)(TOTAL - N_SYMBOLS));           // (G >= 0: the conversion is the floor)
}

IREC_REC_HD inline uint32_t checksum_term(int64_t p, uint32_t x) {
  uint32_t h = (((uint32_t)p << 8) | x) + 0x9E3779B9u;
  h ^= h >> 16; h *= 0x85EBCA6Bu; h ^= h >> 13; h *= 0xC2B2AE35u; h ^= h >> 16;
  return h;
}

// ---- bit sinks and the bit source -------------------------------------------------------------------------------------------------
struct CountingSink {
  int64_t n = 0;
  IREC_REC_HD void put(int, int64_t follow) { n += 1 + follow; }
};
// The code bits MSB first into nbytes = (n_bits + 7) / 8 bytes, the last one padded with zero bits.  Each byte is built in a register
// and stored whole, inside [out, out + nbytes) only.
struct WritingSink {
  uint8_t *out; int64_t nbytes, pos = 0; uint32_t acc = 0; int nacc = 0; bool bad = false;
  IREC_REC_HD WritingSink(uint8_t *o, int64_t n_bits) : out(o), nbytes((n_bits + 7) / 8) {}
  IREC_REC_HD void flush() { if (pos < nbytes) out[pos] = (uint8_t)acc; else bad = true; ++pos; acc = 0; nacc = 0; }
  IREC_REC_HD void push(int bit) { acc = (acc << 1) | (uint32_t)bit; if (++nacc == 8) flush(); }
  IREC_REC_HD void put(int bit, int64_t follow) { push(bit); for (; follow > 0; --follow) push(bit ^ 1); }
  IREC_REC_HD void finish() { while (nacc != 0) push(0); }
};
struct BitReader {
  const uint8_t *p; int64_t n_bits;
  IREC_REC_HD uint64_t bit(int64_t i) const { return i < n_bits ? (uint64_t)((p[i >> 3] >> (7 - (i & 7))) & 1) : 0; }
};

// ---- the scales of a call ---------------------------------------------------------------------------------------------------------
// CallScale: the call's one scale (EncodeCall::scale, DecodeCall::scale) and version 1 -- what every entry point without "_scales" in
// its name is compiled with, and nothing else: its stream walks under one constant inv.  ChannelScales: scales[channels], version 2.
// A policy gives the header's size, writes and compares the scale words, and makes the cursor that a stream asks for the inv of each
// of its symbols' positions, which are consecutive: the cursor of ChannelScales divides once per channel that the stream enters.
struct FixedInv {
  static constexpr bool fixed = true;
  double inv;
  IREC_REC_HD double at(int64_t) const { return inv; }
};
struct ChannelInv {
  static constexpr bool fixed = false;
  const float *scales; int64_t plane, next; double inv;
  IREC_REC_HD double at(int64_t p) {
    if (p >= next) { const int64_t ch = p / plane; inv = model_inv(scales[ch]); next = (ch + 1) * plane; }
    return inv;
  }
};
struct CallScale {
  static constexpr bool per_channel = false;
  static constexpr uint32_t version = VERSION;
  IREC_REC_HD int64_t header_bytes(uint32_t) const { return HEADER_BYTES; }
  IREC_REC_HD bool ok(float scale, uint32_t) const { return scale_ok(scale); }
  IREC_REC_HD FixedInv cursor(float scale) const { return FixedInv{model_inv(scale)}; }
};
struct ChannelScales {
  static constexpr bool per_channel = true;
  static constexpr uint32_t version = VERSION_SCALES;
  const float *scales; int64_t plane;                                             // [channels]; height * width
  IREC_REC_HD int64_t header_bytes(uint32_t channels) const { return HEADER_BYTES + 4 * ((int64_t)channels - 1); }
  IREC_REC_HD bool ok(float, uint32_t channels) const {
    bool all = true;
    for (uint32_t ch = 0; ch < channels; ++ch) all = all && scale_ok(scales[ch]);
    return all;
  }
  IREC_REC_HD ChannelInv cursor(float) const { return ChannelInv{scales, plane, 0, 0.0}; }
};

// ---- one stream ---------------------------------------------------------------------------------------------------------------------
// n symbols x[k] under m[k] = loc_to_m(loc[k]) and the cursor's inv at p0 + k.  0, or IREC_RES_E_LOC for a loc that is not finite.
// *share: the checksum terms.
template <class Sink, class Inv>
IREC_REC_HD inline int32_t encode_stream(const uint8_t *x, const float *loc, Inv inv_at, int64_t p0, int64_t n, Sink &sink, uint32_t *share) {
  uint64_t low = 0, high = WHOLE;
  int64_t s = 0;
  uint32_t sum = 0;
  for (int64_t k = 0; k < n; ++k) {
    if (!is_finite(loc[k])) return IREC_RES_E_LOC;
    const double inv = inv_at.at(p0 + k);
    const int32_t m = loc_to_m(loc[k]);
    const uint32_t sym = x[k];
    sum += checksum_term(p0 + k, sym);
    const uint64_t C = cum(m, inv, (int32_t)sym), D = cum(m, inv, (int32_t)sym + 1);
    const uint64_t width = high - low;
    high = low + ((width * D) >> TOTAL_BITS);
    low = low + ((width * C) >> TOTAL_BITS);
    // (width > 2^30 on entry and D > C, so high > low here and each loop doubles the width: at most MAX_BITS_PER_SYMBOL turns in all)
    while (high < HALF || low > HALF) {
      if (high < HALF) { sink.put(0, s); s = 0; low *= 2; high *= 2; }
      else { sink.put(1, s); s = 0; low = (low - HALF) * 2; high = (high - HALF) * 2; }
    }
    while (low > QUARTER && high < 3 * QUARTER) { s += 1; low = (low - QUARTER) * 2; high = (high - QUARTER) * 2; }
  }
  s += 1;
  sink.put(low <= QUARTER ? 0 : 1, s);
  *share = sum;
  return IREC_RES_OK;
}

// The inverse: n symbols into out[0, n), nothing else written.  0 or IREC_RES_E_CORRUPT (target < 0, width <= 0, target >= width, or
// more than n_bits + 64 renormalisation shifts).  Every loop is bounded on entry: n symbols, 8 bisection steps, the shift budget.
template <class Inv>
IREC_REC_HD inline int32_t decode_stream(const BitReader &in, const float *loc, Inv inv_at, int64_t p0, int64_t n, uint8_t *out, uint32_t *share) {
  uint64_t low = 0, high = WHOLE, z = 0;
  int64_t i = 0, shifts_left = in.n_bits + 64;
  uint32_t sum = 0;
  *share = 0;
  while (i < 32) { z += in.bit(i) << (31 - i); ++i; }
  double inv = inv_at.at(p0);
  for (int64_t k = 0; k < n; ++k) {
    if constexpr (!Inv::fixed) inv = inv_at.at(p0 + k);
    if (z < low || high <= low || z >= high) return IREC_RES_E_CORRUPT;
    const uint64_t width = high - low, target = z - low;
    const uint64_t v = (((target + 1) << TOTAL_BITS) - 1) / width;                // < 2^16, as target < width
    const int32_t m = loc_to_m(loc[k]);
    int32_t lo = 0, hi = (int32_t)N_SYMBOLS;
    uint64_t C = 0, D = TOTAL;
    while (hi - lo > 1) {                                                         // C(lo) <= v < C(hi)
      const int32_t mid = (lo + hi) >> 1;
      const uint64_t cm = cum(m, inv, mid);
      if (cm <= v) { lo = mid; C = cm; } else { hi = mid; D = cm; }
    }
    out[k] = (uint8_t)lo;
    sum += checksum_term(p0 + k, (uint32_t)lo);
    high = low + ((width * D) >> TOTAL_BITS);
    low = low + ((width * C) >> TOTAL_BITS);
    if (k + 1 == n) break;
    while (high < HALF || low > HALF) {
      if (--shifts_left < 0) return IREC_RES_E_CORRUPT;
      if (high < HALF) { low *= 2; high *= 2; z *= 2; }
      else { low = (low - HALF) * 2; high = (high - HALF) * 2; z = (z - HALF) * 2; }
      z += in.bit(i); ++i;
    }
    while (low > QUARTER && high < 3 * QUARTER) {
      if (--shifts_left < 0) return IREC_RES_E_CORRUPT;
      low = (low - QUARTER) * 2; high = (high - QUARTER) * 2; z = (z - QUARTER) * 2;
      z += in.bit(i); ++i;
    }
  }
  *share = sum;
  return IREC_RES_OK;
}

// ================================================================================================================================
//  Encoding a call: size every stream, lay the files out (offsets, stream positions, headers), write the streams
// ================================================================================================================================
struct EncodeCall {
  const uint8_t *pixels; const float *loc; float scale;
  int32_t N, ns; uint32_t height, width, channels, stream_len; int64_t n_sym;
  uint8_t *out; int64_t cap; int64_t *offsets; int32_t *status;
  // workspace, per stream: its position in its file, its bits, its status, its checksum share
  int64_t *pos; int32_t *n_bits; int32_t *stream_status; uint32_t *share;
};
IREC_REC_HD inline int64_t n_streams_of(int64_t n_sym, int64_t stream_len) { return (n_sym + stream_len - 1) / stream_len; }
IREC_REC_HD inline int64_t workspace_bytes(int64_t N, int64_t ns) { return N * ns * 20 + N * 8; }
IREC_REC_HD inline void encode_bind_workspace(EncodeCall &c, void *ws) {
  const int64_t S = (int64_t)c.N * c.ns;
  c.pos = (int64_t *)ws; c.n_bits = (int32_t *)(c.pos + S); c.stream_status = c.n_bits + S; c.share = (uint32_t *)(c.stream_status + S);
}
IREC_REC_HD inline int64_t stream_bytes(int64_t n_bits) { return (n_bits + 7) / 8; }

template <class Sink, class Scales>
IREC_REC_HD inline int32_t encode_lane_stream(const EncodeCall &c, const Scales &sc, int64_t lane, Sink &sink, uint32_t *share) {
  const int64_t i = lane / c.ns, j = lane % c.ns, k0 = j * (int64_t)c.stream_len;
  const int64_t k1 = k0 + c.stream_len < c.n_sym ? k0 + c.stream_len : c.n_sym;
  if (!sc.ok(c.scale, c.channels)) return IREC_RES_E_SCALE;
  return encode_stream(c.pixels + i * c.n_sym + k0, c.loc + i * c.n_sym + k0, sc.cursor(c.scale), k0, k1 - k0, sink, share);
}

// launch 1, lane < N ns
template <class Scales>
IREC_REC_HD inline void encode_size_lane(const EncodeCall &c, const Scales &sc, int64_t lane) {
  CountingSink sink;
  uint32_t share = 0;
  const int32_t st = encode_lane_stream(c, sc, lane, sink, &share);
  c.stream_status[lane] = st;
  c.n_bits[lane] = st ? 0 : (int32_t)sink.n;
  c.share[lane] = st ? 0u : share;
}
IREC_REC_HD inline void encode_size_lane(const EncodeCall &c, int64_t lane) { encode_size_lane(c, CallScale{}, lane); }

// launch 2, per image: its status (the first cause in stream order) and its file's bytes (0 with an error status) ...
template <class Scales>
IREC_REC_HD inline int64_t encode_image_bytes(const EncodeCall &c, const Scales &sc, int64_t i) {
  int32_t st = IREC_RES_OK;
  int64_t bytes = sc.header_bytes(c.channels) + 2 * (int64_t)c.ns;
  for (int64_t j = 0; j < c.ns; ++j) {
    if (st == IREC_RES_OK) st = c.stream_status[i * c.ns + j];
    bytes += stream_bytes(c.n_bits[i * c.ns + j]);
  }
  c.status[i] = st;
  return st ? 0 : bytes;
}
IREC_REC_HD inline int64_t encode_image_bytes(const EncodeCall &c, int64_t i) { return encode_image_bytes(c, CallScale{}, i); }
// ... and, once the call's total is known, the positions of its streams and (if the files fit cap) its header
template <class Scales>
IREC_REC_HD inline void encode_image_layout(const EncodeCall &c, const Scales &sc, int64_t i, int64_t at, bool fits) {
  c.offsets[i] = at;
  if (c.status[i]) return;
  const int64_t head = sc.header_bytes(c.channels);
  int64_t pos = head + 2 * (int64_t)c.ns;
  uint32_t sum = 0;
  uint8_t *f = c.out + at;
  for (int64_t j = 0; j < c.ns; ++j) {
    const int64_t nb = stream_bytes(c.n_bits[i * c.ns + j]);
    c.pos[i * c.ns + j] = pos;
    sum += c.share[i * c.ns + j];
    if (fits) put_u16(f + head + 2 * j, (uint32_t)nb);
    pos += nb;
  }
  if (!fits) return;
  put_u32(f, MAGIC); put_u16(f + 4, Scales::version); put_u16(f + 6, c.channels); put_u32(f + 8, c.stream_len); put_u32(f + 12, c.height);
  put_u32(f + 16, c.width);
  if constexpr (Scales::per_channel) {
    for (uint32_t ch = 0; ch < c.channels; ++ch) put_u32(f + 20 + 4 * (int64_t)ch, __builtin_bit_cast(uint32_t, sc.scales[ch]));
  } else {
    put_u32(f + 20, __builtin_bit_cast(uint32_t, c.scale));
  }
  put_u32(f + head - 4, sum);
}
IREC_REC_HD inline void encode_image_layout(const EncodeCall &c, int64_t i, int64_t at, bool fits) { encode_image_layout(c, CallScale{}, i, at, fits); }

// launch 3, lane < N ns: the stream of the lane.  Nothing at all is written when the files do not fit cap.
template <class Scales>
IREC_REC_HD inline void encode_write_lane(const EncodeCall &c, const Scales &sc, int64_t lane) {
  const int64_t i = lane / c.ns;
  if (c.offsets[c.N] > c.cap || c.status[i]) return;
  const int64_t at = c.offsets[i] + c.pos[lane], nb = c.n_bits[lane];
  if (at < c.offsets[i] || at + stream_bytes(nb) > c.offsets[i + 1]) return;      // (cannot happen: the layout pass summed these very sizes)
  WritingSink sink(c.out + at, nb);
  uint32_t share;
  encode_lane_stream(c, sc, lane, sink, &share);
  sink.finish();
}
IREC_REC_HD inline void encode_write_lane(const EncodeCall &c, int64_t lane) { encode_write_lane(c, CallScale{}, lane); }

// ================================================================================================================================
//  Decoding a call: headers and stream positions, the streams, one status per image
// ================================================================================================================================
struct DecodeCall {
  const uint8_t *bytes; const int64_t *offsets; const float *loc; float scale;
  int32_t N, ns; uint32_t height, width, channels, stream_len; int64_t n_sym;
  uint8_t *pixels; int32_t *status;
  int64_t *pos; int32_t *len; int32_t *stream_status; uint32_t *share;            // workspace per stream, as the encoder's
  int32_t *head_status; uint32_t *head_sum;                                        // workspace per image
};
IREC_REC_HD inline void decode_bind_workspace(DecodeCall &c, void *ws) {
  const int64_t S = (int64_t)c.N * c.ns;
  c.pos = (int64_t *)ws; c.len = (int32_t *)(c.pos + S); c.stream_status = c.len + S; c.share = (uint32_t *)(c.stream_status + S);
  c.head_status = (int32_t *)(c.share + S); c.head_sum = (uint32_t *)(c.head_status + c.N);
}

// launch 1, lane i < N: every check that needs no stream decoded, and the position of every stream.  Reads [file, file + n_bytes) only.
// (version 2 looks at the magic and version words as soon as the file holds them: a version-1 file shorter than a version-2 header is
//  still "not this version")
IREC_REC_HD inline bool scale_words_differ(const DecodeCall &c, const ChannelScales &sc, const uint8_t *f) {
  bool differ = false;
  for (uint32_t ch = 0; ch < c.channels; ++ch)
    differ = differ || get_u32(f + 20 + 4 * (int64_t)ch) != __builtin_bit_cast(uint32_t, sc.scales[ch]) || !scale_ok(sc.scales[ch]);
  return differ;
}
IREC_REC_HD inline bool scale_words_differ(const DecodeCall &, const CallScale &, const uint8_t *) { return false; }
template <class Scales>
IREC_REC_HD inline void decode_head_lane(const DecodeCall &c, const Scales &sc, int64_t i) {
  const int64_t lo = c.offsets[i], n_bytes = c.offsets[i + 1] - lo, head = sc.header_bytes(c.channels);
  const uint8_t *f = c.bytes + lo;
  int32_t st = IREC_RES_OK;
  c.head_sum[i] = 0;
  if (lo < 0 || n_bytes < (Scales::per_channel ? 6 : head)) st = IREC_RES_E_TRUNCATED_HEADER;
  else if (get_u32(f) != MAGIC || get_u16(f + 4) != Scales::version) st = IREC_RES_E_MAGIC;
  else if (Scales::per_channel && n_bytes < head) st = IREC_RES_E_TRUNCATED_HEADER;
  else if (get_u16(f + 6) != c.channels || get_u32(f + 8) != c.stream_len || get_u32(f + 12) != c.height || get_u32(f + 16) != c.width)
    st = IREC_RES_E_SHAPE;
  else if (Scales::per_channel ? scale_words_differ(c, sc, f) : get_u32(f + 20) != __builtin_bit_cast(uint32_t, c.scale) || !scale_ok(c.scale))
    st = IREC_RES_E_SCALE_WORD;
  else if (n_bytes < head + 2 * (int64_t)c.ns) st = IREC_RES_E_TRUNCATED_HEADER;
  if (st == IREC_RES_OK) {
    c.head_sum[i] = get_u32(f + head - 4);
    int64_t pos = head + 2 * (int64_t)c.ns;
    for (int64_t j = 0; j < c.ns; ++j) {
      const int64_t nb = get_u16(f + head + 2 * j);
      c.pos[i * c.ns + j] = pos; c.len[i * c.ns + j] = (int32_t)nb;
      pos += nb;
    }
    if (pos > n_bytes) st = IREC_RES_E_TRUNCATED_STREAMS;
  }
  c.head_status[i] = st;
}
IREC_REC_HD inline void decode_head_lane(const DecodeCall &c, int64_t i) { decode_head_lane(c, CallScale{}, i); }

// launch 2, lane < N ns: its stream into its own pixels
template <class Scales>
IREC_REC_HD inline void decode_stream_lane(const DecodeCall &c, const Scales &sc, int64_t lane) {
  const int64_t i = lane / c.ns, j = lane % c.ns, k0 = j * (int64_t)c.stream_len;
  const int64_t k1 = k0 + c.stream_len < c.n_sym ? k0 + c.stream_len : c.n_sym;
  c.stream_status[lane] = IREC_RES_OK; c.share[lane] = 0;
  if (c.head_status[i]) return;                     // (the image's pixels are zeroed by the last launch)
  const int64_t lo = c.offsets[i], n_bytes = c.offsets[i + 1] - lo, pos = c.pos[lane], nb = c.len[lane];
  if (pos < 0 || nb < 0 || pos + nb > n_bytes) { c.stream_status[lane] = IREC_RES_E_TRUNCATED_STREAMS; return; }   // (the head lane checked)
  const BitReader in{c.bytes + lo + pos, nb * 8};
  uint32_t share = 0;
  c.stream_status[lane] = decode_stream(in, c.loc + i * c.n_sym + k0, sc.cursor(c.scale), k0, k1 - k0, c.pixels + i * c.n_sym + k0, &share);
  c.share[lane] = share;
}
IREC_REC_HD inline void decode_stream_lane(const DecodeCall &c, int64_t lane) { decode_stream_lane(c, CallScale{}, lane); }

// ---- a whole call over host memory: what the kernels of irec_res.hip do, the lanes of a launch dealt out by par(n, body) with
//      body(lo, hi) running lanes [lo, hi) in a plain loop (the workspace bound by the caller).  The host entry points pass a pool of
//      threads, scripts/res_core_check.cpp a serial loop and a pool of its own. -------------------------------------------------------
struct SerialLanes {
  template <class F> void operator()(int64_t n, F &&body) const { body((int64_t)0, n); }
};
template <class Scales, class Par>
inline void encode_call_host(const EncodeCall &c, const Scales &sc, Par &&par) {
  const int64_t lanes = (int64_t)c.N * c.ns;
  par(lanes, [&c, &sc](int64_t lo, int64_t hi) { for (int64_t l = lo; l < hi; ++l) encode_size_lane(c, sc, l); });
  int64_t total = 0, at = 0;
  for (int64_t i = 0; i < c.N; ++i) total += encode_image_bytes(c, sc, i);
  for (int64_t i = 0; i < c.N; ++i) { encode_image_layout(c, sc, i, at, total <= c.cap); at += encode_image_bytes(c, sc, i); }
  c.offsets[c.N] = total;
  par(lanes, [&c, &sc](int64_t lo, int64_t hi) { for (int64_t l = lo; l < hi; ++l) encode_write_lane(c, sc, l); });
}
template <class Par>
inline void encode_call_host(const EncodeCall &c, Par &&par) { encode_call_host(c, CallScale{}, par); }
inline void decode_image_status(const DecodeCall &c, int64_t i) {
  int32_t st = c.head_status[i];
  uint32_t sum = 0;
  for (int64_t j = 0; j < c.ns && !st; ++j) { st = c.stream_status[i * c.ns + j]; sum += c.share[i * c.ns + j]; }
  if (!st && sum != c.head_sum[i]) st = IREC_RES_E_CHECKSUM;
  c.status[i] = st;
  if (st) for (int64_t e = 0; e < c.n_sym; ++e) c.pixels[i * c.n_sym + e] = 0;
}
template <class Scales, class Par>
inline void decode_call_host(const DecodeCall &c, const Scales &sc, Par &&par) {
  for (int64_t i = 0; i < c.N; ++i) decode_head_lane(c, sc, i);
  par((int64_t)c.N * c.ns, [&c, &sc](int64_t lo, int64_t hi) { for (int64_t l = lo; l < hi; ++l) decode_stream_lane(c, sc, l); });
  for (int64_t i = 0; i < c.N; ++i) decode_image_status(c, i);
}
template <class Par>
inline void decode_call_host(const DecodeCall &c, Par &&par) { decode_call_host(c, CallScale{}, par); }

} // namespace irec_res
#endif // IREC_RES_CORE_H_
