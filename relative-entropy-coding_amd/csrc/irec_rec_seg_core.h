// irec_rec_seg_core.h -- the segmented .rec container (NAME.recs) over the coder of irec_rec_core.h: no second coder.
// A residual block's rows are cut into segments of g coder blocks, every segment is a pair of ordinary streams -- what the plain
// container would hold for those blocks alone -- and one lane codes one stream of one segment.  encode_stream / decode_stream, the
// sinks, Model, BitReader, the fetch and the emit objects are irec_rec_core.h's, untouched: a segment reaches them as a call of one
// image and one residual block whose rows start at the segment's first block.  New here: the number of a segment and its block range,
// the directory arithmetic, the lane functions and the host runners.  Plain C++ like the header it rests on (IREC_REC_HD).
//
//   0  "IRSG" | 4  version u16 = 1, reserved u16 = 0 | 8  the 28-byte static header of .rec (both flags 0) | 36  g u32 | 40  R x u32 blocks
//   40 + 4 R  directory, for r in order, for s < n_seg[r] = ceil(blocks[r] / g):  max_part u32, count_bytes u32, index_bytes u32
//   then the streams in directory order: each segment's count stream, then its index stream
//
// Segments of an image are numbered sl = seg_first[r] + s < S, those of a call n = i S + sl.  One call is 2 N S lanes: [0, N S) the
// index streams, [N S, 2 N S) the count streams (a wave holds streams of one kind).  Default symbol models only.
#ifndef IREC_REC_SEG_CORE_H_
#define IREC_REC_SEG_CORE_H_

#include "irec_rec_core.h"

namespace irec_rec {

constexpr uint32_t SEG_MAGIC = 0x47535249u;           // the bytes "IRSG"
constexpr uint32_t SEG_VERSION = 1;
constexpr int64_t SEG_MAX_PER_IMAGE = (int64_t)1 << 22;   // segments of one image: a segment's number and a status share an int32 key

// the segments of an image: seg_first[r] = sum_{q < r} ceil(blocks[q] / g), S = seg_first[R]; travels by value like first[]
struct SegLayout {
  int32_t g, S;
  int32_t seg_first[IREC_REC_RAGGED_MAX_RES + 1];
};
// from first[0 .. R] (ragged_first); false for g < 1 or more than SEG_MAX_PER_IMAGE segments
inline bool seg_layout(int32_t R, const int32_t *first, int32_t g, SegLayout *L) {
  if (g < 1) return false;
  int64_t at = 0;
  for (int32_t r = 0; r < R; ++r) {
    L->seg_first[r] = (int32_t)at;
    at += ((int64_t)(first[r + 1] - first[r]) + g - 1) / g;
    if (at > SEG_MAX_PER_IMAGE) return false;
  }
  for (int32_t r = R; r <= IREC_REC_RAGGED_MAX_RES; ++r) L->seg_first[r] = (int32_t)at;
  L->g = g; L->S = (int32_t)at;
  return true;
}
IREC_REC_HD inline int64_t seg_header_bytes(int64_t R, int64_t S) { return 40 + 4 * R + 12 * S; }

// segment n of a call: image i, residual block r, segment s of it (sl within the image), its nb blocks from row b0
struct SegId { int64_t i, b0; int32_t r, s, sl, nb; };
template <class Call>
IREC_REC_HD inline SegId seg_id(const Call &c, const SegLayout &L, int64_t n) {
  SegId id;
  id.i = n / L.S; id.sl = (int32_t)(n % L.S);
  int32_t r = 0;
  while (r + 1 < c.R && L.seg_first[r + 1] <= id.sl) ++r;
  id.r = r; id.s = id.sl - L.seg_first[r];
  const int64_t blocks = c.first[r + 1] - c.first[r], j0 = (int64_t)id.s * L.g;
  id.nb = (int32_t)(blocks - j0 < L.g ? blocks - j0 : L.g);
  id.b0 = id.i * (int64_t)c.first[c.R] + c.first[r] + j0;
  return id;
}

// ================================================================================================================================
//  Encoding: size every stream, lay every image out, the offsets, write
// ================================================================================================================================
struct SegEncodeCall {
  EncodeCall e;                    // bpt = 0: first[]; n_bits, stream_status [2 N S] and max_part [N S] per segment
  SegLayout L;
  int64_t *seg_pos;                // workspace [N S]: where a segment's count stream starts within its file
  int64_t *image_bytes;            // workspace [N]
};
IREC_REC_HD inline int64_t seg_encode_workspace_bytes(int64_t N, int64_t S) { return 2 * N * S * 8 + N * S * 8 + N * 8 + 2 * N * S * 4 + N * S * 4; }
IREC_REC_HD inline void seg_encode_bind_workspace(SegEncodeCall &c, void *ws) {
  const int64_t NS = (int64_t)c.e.N * c.L.S;
  c.e.n_bits = (int64_t *)ws; c.seg_pos = c.e.n_bits + 2 * NS; c.image_bytes = c.seg_pos + NS;
  c.e.stream_status = (int32_t *)(c.image_bytes + c.e.N); c.e.max_part = c.e.stream_status + 2 * NS;
}

// the bits of one stream of one segment through `sink`: encode_lane_stream on the call of one image and one residual block that
// starts at the segment's first row (its lane 0 the index stream, lane 1 the count stream), so the input checks are that function's
template <class Sink>
IREC_REC_HD inline int32_t seg_encode_stream(const SegEncodeCall &c, int64_t lane, Sink &sink, int32_t *max_part_out) {
  const int64_t NS = (int64_t)c.e.N * c.L.S;
  const bool counts = lane >= NS;
  const SegId id = seg_id(c.e, c.L, counts ? lane - NS : lane);
  EncodeCall sub{};
  sub.max_index = c.e.max_index; sub.N = 1; sub.R = 1; sub.bpt = id.nb; sub.max_K = c.e.max_K;
  sub.K = c.e.K + id.b0 * c.e.k_stride; sub.k_stride = c.e.k_stride;
  sub.idx = c.e.idx ? c.e.idx + id.b0 * c.e.idx_stride : nullptr; sub.idx_stride = c.e.idx_stride;
  return encode_lane_stream(sub, NoTables{}, counts ? 1 : 0, sink, max_part_out);
}

// launch 1, lane < 2 N S
IREC_REC_HD inline void seg_encode_size_lane(const SegEncodeCall &c, int64_t lane) {
  const int64_t NS = (int64_t)c.e.N * c.L.S;
  CountingSink sink;
  int32_t mx = 0;
  const int32_t st = seg_encode_stream(c, lane, sink, &mx);
  c.e.stream_status[lane] = st;
  c.e.n_bits[lane] = st ? 0 : sink.n;
  if (lane >= NS) c.e.max_part[lane - NS] = mx;
}

// launch 2, per image: the two things a scan over its segments carries.  The bytes of a segment's pair of streams, and its claim on
// the image's status as a key whose minimum is the status: a K out of range anywhere first, else the first segment's cause, counts
// before indices (encode_image_bytes' rule).
constexpr int32_t SEG_NO_KEY = 0x7fffffff;
IREC_REC_HD inline int64_t seg_pair_bytes(const SegEncodeCall &c, int64_t n) {
  return stream_bytes(c.e.n_bits[(int64_t)c.e.N * c.L.S + n]) + stream_bytes(c.e.n_bits[n]);
}
IREC_REC_HD inline int32_t seg_encode_key(const SegEncodeCall &c, int64_t n, int32_t sl) {
  const int32_t sc = c.e.stream_status[(int64_t)c.e.N * c.L.S + n], sx = c.e.stream_status[n];
  if (sc == IREC_REC_E_K_RANGE || sx == IREC_REC_E_K_RANGE) return IREC_REC_E_K_RANGE;
  const int32_t st = sc ? sc : sx;
  return st ? ((1 + sl) << 8) | st : SEG_NO_KEY;
}
IREC_REC_HD inline int32_t seg_key_status(int32_t key) { return key == SEG_NO_KEY ? IREC_REC_OK : (key & 0xff); }
// the whole of launch 2 for image i in a plain loop
inline void seg_encode_layout_image(const SegEncodeCall &c, int64_t i) {
  int32_t key = SEG_NO_KEY;
  int64_t at = seg_header_bytes(c.e.R, c.L.S);
  for (int32_t sl = 0; sl < c.L.S; ++sl) {
    const int64_t n = i * c.L.S + sl;
    const int32_t k = seg_encode_key(c, n, sl);
    key = k < key ? k : key;
    c.seg_pos[n] = at; at += seg_pair_bytes(c, n);
  }
  c.e.status[i] = seg_key_status(key);
  c.image_bytes[i] = key == SEG_NO_KEY ? at : 0;
}

// launch 4, lane < 2 N S + N: the streams (a count lane also its segment's directory entry), then the fixed part of every header.
// Nothing at all is written when the files do not fit cap.
IREC_REC_HD inline void seg_encode_write_lane(const SegEncodeCall &c, int64_t lane) {
  const int64_t NS = (int64_t)c.e.N * c.L.S;
  const int32_t R = c.e.R;
  if (c.e.offsets[c.e.N] > c.e.cap) return;
  if (lane >= 2 * NS) {
    const int64_t i = lane - 2 * NS;
    if (c.e.status[i]) return;
    uint8_t *f = c.e.out + c.e.offsets[i];
    put_u32(f, SEG_MAGIC); put_u16(f + 4, SEG_VERSION); put_u16(f + 6, 0);
    put_u32(f + 8, c.e.seed); put_u32(f + 12, c.e.block_size); put_u32(f + 16, c.e.max_index); put_u32(f + 20, c.e.height); put_u32(f + 24, c.e.width);
    put_u16(f + 28, c.e.channels); put_u16(f + 30, 0); put_u16(f + 32, 0); put_u16(f + 34, (uint32_t)R);
    put_u32(f + 36, (uint32_t)c.L.g);
    for (int32_t r = 0; r < R; ++r) put_u32(f + 40 + 4 * r, (uint32_t)(c.e.first[r + 1] - c.e.first[r]));
    return;
  }
  const bool counts = lane >= NS;
  const int64_t n = counts ? lane - NS : lane, i = n / c.L.S;
  if (c.e.status[i]) return;
  const int64_t cb = stream_bytes(c.e.n_bits[NS + n]), xb = stream_bytes(c.e.n_bits[n]);
  const int64_t at = c.e.offsets[i] + c.seg_pos[n] + (counts ? 0 : cb);
  if (c.seg_pos[n] < seg_header_bytes(R, c.L.S) || at + (counts ? cb : xb) > c.e.offsets[i + 1]) return;   // (cannot happen: the layout pass summed these very sizes)
  if (counts) {
    uint8_t *d = c.e.out + c.e.offsets[i] + 40 + 4 * (int64_t)R + 12 * (n % c.L.S);
    put_u32(d, (uint32_t)c.e.max_part[n]); put_u32(d + 4, (uint32_t)cb); put_u32(d + 8, (uint32_t)xb);
  }
  WritingSink sink(c.e.out + at, c.e.n_bits[lane]);
  seg_encode_stream(c, lane, sink, nullptr);
}

// ================================================================================================================================
//  Decoding: locate every image's segments, the count streams, the index streams, one status per image
// ================================================================================================================================
struct SegDecodeCall {
  DecodeCall d;                    // bpt = 0: first[]; stream_status [2 N S], laid out like the encoder's lanes
  SegLayout L;
  int64_t *seg_pos;                // workspace [N S]: where a segment's count stream starts within its file
  int32_t *loc_status;             // workspace [N]: what launch 1 found
};
IREC_REC_HD inline int64_t seg_decode_workspace_bytes(int64_t N, int64_t S) { return N * S * 8 + 2 * N * S * 4 + N * 4; }
IREC_REC_HD inline void seg_decode_bind_workspace(SegDecodeCall &c, void *ws) {
  const int64_t NS = (int64_t)c.d.N * c.L.S;
  c.seg_pos = (int64_t *)ws; c.d.stream_status = (int32_t *)(c.seg_pos + NS); c.loc_status = c.d.stream_status + 2 * NS;
}

// launch 1, the part every lane of an image's workgroup computes alike: all that the fixed header says, held against the call, and
// that the directory lies inside the file.  Reads [file, file + n_bytes) only.  hdr9: the static header's words as the plain reader
// gives them (may be null).
IREC_REC_HD inline int32_t seg_locate_header(const SegDecodeCall &c, const uint8_t *file, int64_t n_bytes, uint32_t *hdr9) {
  if (n_bytes < 40) return IREC_REC_E_TRUNCATED_HEADER;
  if (get_u32(file) != SEG_MAGIC || get_u16(file + 4) != SEG_VERSION || get_u16(file + 6) != 0) return IREC_REC_E_SEG_MAGIC;
  uint32_t h[9];
  for (int k = 0; k < 5; ++k) h[k] = get_u32(file + 8 + 4 * k);
  for (int k = 0; k < 4; ++k) h[5 + k] = get_u16(file + 28 + 2 * k);
  if (hdr9) for (int k = 0; k < 9; ++k) hdr9[k] = h[k];
  if (h[6] || h[7]) return IREC_REC_E_COUNT_FILES;
  const int64_t Rf = h[8];
  if (n_bytes < 40 + 4 * Rf) return IREC_REC_E_TRUNCATED_HEADER;
  if (h[2] < 1u || h[2] > (1u << 24)) return IREC_REC_E_MAX_INDEX;
  if (Rf != c.d.R) return IREC_REC_E_STRUCTURE;
  for (int32_t r = 0; r < c.d.R; ++r)
    if ((int64_t)get_u32(file + 40 + 4 * r) != (int64_t)(c.d.first[r + 1] - c.d.first[r])) return IREC_REC_E_STRUCTURE;
  const uint32_t g = get_u32(file + 36);
  if (g == 0 || g != (uint32_t)c.L.g) return IREC_REC_E_SEG_BLOCKS;
  if (n_bytes < seg_header_bytes(c.d.R, c.L.S)) return IREC_REC_E_TRUNCATED_HEADER;
  return IREC_REC_OK;
}
// a directory entry of a file whose header passed: its streams' bytes, and its claim on the image's status (the first segment's wins)
struct SegEntry { uint32_t max_part; int64_t cb, xb; };
IREC_REC_HD inline SegEntry seg_entry(const uint8_t *file, int32_t R, int32_t sl) {
  const uint8_t *d = file + 40 + 4 * (int64_t)R + 12 * (int64_t)sl;
  return SegEntry{get_u32(d), (int64_t)get_u32(d + 4), (int64_t)get_u32(d + 8)};
}
IREC_REC_HD inline int32_t seg_locate_key(const SegDecodeCall &c, const SegEntry &e, int32_t sl) {
  const int32_t st = e.max_part > (uint32_t)IREC_MAX_PARTITIONS ? IREC_REC_E_BLOCK_COUNTS : (int64_t)e.max_part > (int64_t)c.d.max_K ? IREC_REC_E_MAX_K : IREC_REC_OK;
  return st ? (sl << 8) | st : SEG_NO_KEY;
}
// the verdict of launch 1 from the header's, the end of the scan and the least key: header, directory and streams must be the file
IREC_REC_HD inline int32_t seg_locate_status(int32_t header_status, int64_t end, int64_t n_bytes, int32_t key) {
  return header_status ? header_status : end != n_bytes ? IREC_REC_E_SEG_DIRECTORY : seg_key_status(key);
}
// the whole of launch 1 for image i in a plain loop
inline void seg_decode_locate_image(const SegDecodeCall &c, int64_t i) {
  const int64_t lo = c.d.offsets[i], n_bytes = c.d.offsets[i + 1] - lo;
  const uint8_t *file = c.d.bytes + lo;
  const int32_t hs = lo < 0 || n_bytes < 0 ? IREC_REC_E_TRUNCATED_HEADER : seg_locate_header(c, file, n_bytes, c.d.headers + 9 * i);
  int32_t key = SEG_NO_KEY;
  int64_t at = seg_header_bytes(c.d.R, c.L.S);
  for (int32_t sl = 0; sl < c.L.S; ++sl) {
    c.seg_pos[i * c.L.S + sl] = at;
    if (hs) continue;
    const SegEntry e = seg_entry(file, c.d.R, sl);
    const int32_t k = seg_locate_key(c, e, sl);
    key = k < key ? k : key;
    at += e.cb + e.xb;
  }
  c.loc_status[i] = seg_locate_status(hs, at, n_bytes, key);
}

// launch 2, lane n < N S: the K of segment n.  An image that launch 1 refused gives every one of its segments that cause.
IREC_REC_HD inline void seg_decode_counts_lane(const SegDecodeCall &c, int64_t n) {
  const int64_t NS = (int64_t)c.d.N * c.L.S;
  const SegId id = seg_id(c.d, c.L, n);
  c.d.stream_status[n] = IREC_REC_OK;
  int32_t st = c.loc_status[id.i];
  if (st == IREC_REC_OK) {
    const uint8_t *file = c.d.bytes + c.d.offsets[id.i];
    const SegEntry e = seg_entry(file, c.d.R, id.sl);
    BitReader in;
    CountEmit emit{c.d.K + id.b0, id.nb, c.d.max_K};
    int64_t got = 0;
    if (!in.open(file + c.seg_pos[n], e.cb)) st = IREC_REC_E_COUNT_MARKER;
    else {
      const int d = decode_stream(make_model((uint64_t)e.max_part + 1, COUNT_WEIGHT), in, id.nb, emit, &got);
      if (d == DEC_CORRUPT) st = IREC_REC_E_COUNT_CORRUPT;
      else if (d == DEC_BUDGET) st = IREC_REC_E_COUNT_BUDGET;
      else if (d != DEC_OK || got != id.nb) st = IREC_REC_E_MISMATCH;
      else if (emit.over) st = IREC_REC_E_MAX_K;
    }
  }
  c.d.stream_status[NS + n] = st;
}

// launch 3, lane n < N S: the index rows of segment n, by the K of launch 2
IREC_REC_HD inline void seg_decode_indices_lane(const SegDecodeCall &c, int64_t n) {
  const int64_t NS = (int64_t)c.d.N * c.L.S;
  if (c.d.stream_status[NS + n]) return;          // no K to go by (the image's outputs are zeroed by the last launch)
  const SegId id = seg_id(c.d, c.L, n);
  const uint8_t *file = c.d.bytes + c.d.offsets[id.i];
  const SegEntry e = seg_entry(file, c.d.R, id.sl);
  const int32_t *Krow = c.d.K + id.b0;
  int64_t tot = 0, got = 0;
  for (int32_t j = 0; j < id.nb; ++j) tot += Krow[j];
  const Model m = make_model(get_u32(file + 16), INDEX_WEIGHT);
  BitReader in;
  IndexEmit emit{Krow, c.d.idx + id.b0 * (int64_t)c.d.max_K, id.nb, c.d.max_K};
  int32_t st = IREC_REC_OK;
  if (!model_fits(m)) st = IREC_REC_E_INDEX_MODEL;
  else if (!in.open(file + c.seg_pos[n] + e.cb, e.xb)) st = IREC_REC_E_INDEX_MARKER;
  else {
    const int d = decode_stream(m, in, tot, emit, &got);
    if (d == DEC_CORRUPT) st = IREC_REC_E_INDEX_CORRUPT;
    else if (d == DEC_BUDGET) st = IREC_REC_E_INDEX_BUDGET;
    else if (d != DEC_OK || got != tot) st = IREC_REC_E_MISMATCH;
  }
  emit.finish();
  c.d.stream_status[n] = st;
}

// launch 4: what segment n says of its image, counts before indices
IREC_REC_HD inline int32_t seg_decode_status(const SegDecodeCall &c, int64_t n) {
  const int64_t NS = (int64_t)c.d.N * c.L.S;
  return c.d.stream_status[NS + n] ? c.d.stream_status[NS + n] : c.d.stream_status[n];
}
inline void seg_decode_finish_host(const SegDecodeCall &c) {
  const int64_t nK = c.d.first[c.d.R], nI = nK * c.d.max_K;
  for (int64_t i = 0; i < c.d.N; ++i) {
    int32_t st = 0;
    for (int32_t sl = 0; sl < c.L.S && !st; ++sl) st = seg_decode_status(c, i * c.L.S + sl);
    c.d.status[i] = st;
    if (st) {
      for (int k = 0; k < 9; ++k) c.d.headers[9 * i + k] = 0;
      for (int64_t e = 0; e < nK; ++e) c.d.K[i * nK + e] = 0;
      for (int64_t e = 0; e < nI; ++e) c.d.idx[i * nI + e] = 0;
    }
  }
}

// ---- a whole call over host memory in plain loops (the workspace bound by the caller), beside encode_call_host / decode_call_host:
//      what the kernels of irec_rec_seg.hip do, for scripts/rec_seg_check.cpp -----------------------------------------------------------
inline void seg_encode_call_host(const SegEncodeCall &c) {
  const int64_t streams = 2 * (int64_t)c.e.N * c.L.S;
  for (int64_t lane = 0; lane < streams; ++lane) seg_encode_size_lane(c, lane);
  int64_t at = 0;
  for (int64_t i = 0; i < c.e.N; ++i) { seg_encode_layout_image(c, i); c.e.offsets[i] = at; at += c.image_bytes[i]; }
  c.e.offsets[c.e.N] = at;
  for (int64_t lane = 0; lane < streams + c.e.N; ++lane) seg_encode_write_lane(c, lane);
}
inline void seg_decode_call_host(const SegDecodeCall &c) {
  const int64_t lanes = (int64_t)c.d.N * c.L.S;
  for (int64_t i = 0; i < c.d.N; ++i) seg_decode_locate_image(c, i);
  for (int64_t n = 0; n < lanes; ++n) seg_decode_counts_lane(c, n);
  for (int64_t n = 0; n < lanes; ++n) seg_decode_indices_lane(c, n);
  seg_decode_finish_host(c);
}

} // namespace irec_rec
#endif // IREC_REC_SEG_CORE_H_
