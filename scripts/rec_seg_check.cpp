// rec_seg_check.cpp -- the segmented .rec container's core (csrc/irec_rec_seg_core.h over csrc/irec_rec_core.h) under the host sanitizers,
// against irec_io.cpp.  A stand-alone program in the manner of scripts/rec_ragged_check.cpp: it includes both, so that every line of the
// core the kernels of csrc/irec_rec_seg.hip run is compiled here by g++ and runs with AddressSanitizer and UndefinedBehaviorSanitizer.
// Build and run from the repository root, on a CPU:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude -Irelative-entropy-coding_amd/csrc \
//       scripts/rec_seg_check.cpp -o /tmp/rec_seg_check -lpthread && /tmp/rec_seg_check
// It walks the structures of tests/test_rec_segmented_host.py -- (1), (1, 4), (3, 1, 5), (2, 2, 2), (13, 302) -- at N = 1 and 3,
// max_index = 1, 20, 36 and segment_blocks = 1, 2, 4, 16, 512 (contiguous and strided input, an exact and a short cap, decoding), and a
// damaged set of a (3, 1, 9), g = 4 file (every prefix, one byte more, every header and directory byte replaced, 800 copies with one
// to three bytes replaced), with every buffer sized EXACTLY, so that one byte or one index past a range is a report; every damaged file
// is read twice, inside the blob of all of them and alone in a buffer of its own size, and the two verdicts must be one.  The referee
// of every segment is irec_rec_encode_file on that segment's blocks alone, as a container of one residual block: its two streams and its
// largest-K word are the segment's.  Exit status 0 and the last line "rec_seg_check: all equal" mean: same bytes, same rows, and no
// sanitizer report (profiles/rec_segmented/sanitizer_core.log is this program's output).
#include <cstdio>
#include <cstdlib>
#include <numeric>
#include <vector>

#include "irec_io.cpp"
#include "irec_rec_seg_core.h"

namespace {
uint64_t g_state = 0x9E3779B97F4A7C15ull;
uint64_t rnd() { g_state += 0x9E3779B97F4A7C15ull; uint64_t z = g_state; z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; return z ^ (z >> 31); }
int64_t below(int64_t n) { return (int64_t)(rnd() % (uint64_t)n); }
int g_failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++g_failures; } } while (0)

struct Packed { int32_t N, mk; uint32_t S; std::vector<int32_t> bpr; int32_t T; std::vector<int32_t> K, idx; };
Packed make(int32_t N, const std::vector<int32_t> &bpr, int32_t mk, uint32_t S, int32_t g) {
  const int32_t T = std::accumulate(bpr.begin(), bpr.end(), 0);
  Packed p{N, mk, S, bpr, T, std::vector<int32_t>((size_t)N * T), std::vector<int32_t>((size_t)N * T * mk)};
  for (auto &k : p.K) k = (int32_t)below(mk + 1);
  if (T > g + 1) for (int32_t j = 0; j < g; ++j) p.K[(size_t)j] = 0;        // a first segment of blocks without indices (where it is not the whole call)
  else if (p.K.size() > 1) p.K[0] = 0;
  p.K.back() = mk;                                                          // and a full row
  for (auto &v : p.idx) v = (int32_t)below(S);
  return p;
}
void put32(std::vector<uint8_t> &f, uint32_t v) { for (int k = 0; k < 4; ++k) f.push_back((uint8_t)(v >> (8 * k))); }
void put16(std::vector<uint8_t> &f, uint32_t v) { f.push_back((uint8_t)v); f.push_back((uint8_t)(v >> 8)); }

// the segmented file of image i, every segment's streams from irec_rec_encode_file on its blocks alone
std::vector<uint8_t> file_of(const Packed &p, int32_t i, int32_t g) {
  std::vector<uint8_t> f{'I', 'R', 'S', 'G'}, directory, streams;
  put16(f, 1); put16(f, 0);
  put32(f, 42); put32(f, 1000); put32(f, p.S); put32(f, 32); put32(f, 48); put16(f, 3); put16(f, 0); put16(f, 0); put16(f, (uint32_t)p.bpr.size());
  put32(f, (uint32_t)g);
  for (int32_t b : p.bpr) put32(f, (uint32_t)b);
  int32_t row = 0;
  for (int32_t blocks : p.bpr) {
    for (int32_t j0 = 0; j0 < blocks; j0 += g) {
      const int32_t nb = blocks - j0 < g ? blocks - j0 : g;
      const int32_t *K = p.K.data() + (size_t)i * p.T + row + j0;
      std::vector<int32_t> flat;
      for (int32_t j = 0; j < nb; ++j)
        for (int32_t t = 0; t < K[j]; ++t) flat.push_back(p.idx[((size_t)i * p.T + row + j0 + j) * p.mk + t]);
      flat.push_back(0);                                                 // (never read: keeps data() non-null for a segment without indices)
      const int64_t n = irec_rec_encode_file(42, 1000, p.S, 32, 48, 3, 1, &nb, K, flat.data(), nullptr, 0);
      CHECK(n > 44);
      std::vector<uint8_t> one((size_t)(n > 0 ? n : 0));
      CHECK(irec_rec_encode_file(42, 1000, p.S, 32, 48, 3, 1, &nb, K, flat.data(), one.data(), n) == n);
      const uint32_t cb = irec_rec::get_u32(one.data() + 32), xb = irec_rec::get_u32(one.data() + 36), mp = irec_rec::get_u32(one.data() + 40);
      CHECK(44 + (int64_t)cb + xb == n);
      put32(directory, mp); put32(directory, cb); put32(directory, xb);
      streams.insert(streams.end(), one.begin() + 44, one.end());
    }
    row += blocks;
  }
  f.insert(f.end(), directory.begin(), directory.end());
  f.insert(f.end(), streams.begin(), streams.end());
  return f;
}

bool layouts(const std::vector<int32_t> &bpr, int32_t g, int32_t *first, irec_rec::SegLayout *L) {
  return irec_rec::ragged_first((int32_t)bpr.size(), bpr.data(), first) && irec_rec::seg_layout((int32_t)bpr.size(), first, g, L);
}

// the core over exactly-sized host buffers: out [cap], offsets [N + 1], status [N], the workspace of its sizing function
void core_encode(const Packed &p, int32_t g, bool strided, int64_t cap, std::vector<uint8_t> &out, std::vector<int64_t> &off, std::vector<int32_t> &status) {
  std::vector<int32_t> joined;
  const int32_t *K = p.K.data(), *idx = p.idx.data();
  int64_t ks = 1, is = p.mk;
  if (strided) {
    const size_t rows = p.K.size();
    joined.resize(rows * (1 + (size_t)p.mk));
    for (size_t b = 0; b < rows; ++b) { joined[b * (1 + p.mk)] = p.K[b]; for (int32_t t = 0; t < p.mk; ++t) joined[b * (1 + p.mk) + 1 + t] = p.idx[b * p.mk + t]; }
    K = joined.data(); idx = joined.data() + 1; ks = is = 1 + p.mk;
  }
  const int32_t R = (int32_t)p.bpr.size();
  out.assign((size_t)cap, 0xAB); off.assign((size_t)p.N + 1, -1); status.assign((size_t)p.N, -1);
  irec_rec::SegEncodeCall c{irec_rec::EncodeCall{42, 1000, p.S, 32, 48, 3, p.N, R, 0, p.mk, K, ks, idx, is, out.data(), cap, off.data(), status.data(), nullptr, nullptr, nullptr, {}},
                            {}, nullptr, nullptr};
  CHECK(layouts(p.bpr, g, c.e.first, &c.L));
  std::vector<int64_t> ws((size_t)(irec_rec::seg_encode_workspace_bytes(p.N, c.L.S) + 7) / 8);
  irec_rec::seg_encode_bind_workspace(c, ws.data());
  irec_rec::seg_encode_call_host(c);
}

void core_decode(const std::vector<uint8_t> &blob, const std::vector<int64_t> &off, const std::vector<int32_t> &bpr, int32_t g, int32_t mk,
                 std::vector<uint32_t> &hdr, std::vector<int32_t> &K, std::vector<int32_t> &idx, std::vector<int32_t> &status) {
  const int32_t N = (int32_t)off.size() - 1, R = (int32_t)bpr.size(), T = std::accumulate(bpr.begin(), bpr.end(), 0);
  hdr.assign((size_t)N * 9, 0xFFFFFFFFu); K.assign((size_t)N * T, -1); idx.assign((size_t)N * T * mk, -1); status.assign((size_t)N, -1);
  // (a copy of exactly the blob's size: a read past the last file is a heap-buffer-overflow report)
  std::vector<uint8_t> exact(blob.begin(), blob.end());
  if (exact.empty()) exact.push_back(0);
  irec_rec::SegDecodeCall c{irec_rec::DecodeCall{exact.data(), off.data(), N, R, 0, mk, hdr.data(), K.data(), idx.data(), status.data(), nullptr, {}}, {}, nullptr, nullptr};
  CHECK(layouts(bpr, g, c.d.first, &c.L));
  std::vector<int64_t> ws((size_t)(irec_rec::seg_decode_workspace_bytes(N, c.L.S) + 7) / 8);
  irec_rec::seg_decode_bind_workspace(c, ws.data());
  irec_rec::seg_decode_call_host(c);
}

void check_structure(int32_t N, const std::vector<int32_t> &bpr, int32_t mk, uint32_t S, int32_t g) {
  const Packed p = make(N, bpr, mk, S, g);
  std::vector<uint8_t> ref; std::vector<int64_t> ref_off{0};
  for (int32_t i = 0; i < N; ++i) { const auto f = file_of(p, i, g); ref.insert(ref.end(), f.begin(), f.end()); ref_off.push_back((int64_t)ref.size()); }
  const int64_t total = (int64_t)ref.size();
  std::vector<uint8_t> out; std::vector<int64_t> off; std::vector<int32_t> status;
  for (int strided = 0; strided < 2; ++strided) {
    core_encode(p, g, strided != 0, total, out, off, status);             // exactly enough room
    CHECK(out == ref); CHECK(off == ref_off);
    for (int32_t s : status) CHECK(s == 0);
  }
  core_encode(p, g, false, total - 1, out, off, status);                  // one byte short: nothing written, the size reported
  CHECK(off[(size_t)N] == total);
  for (uint8_t b : out) if (b != 0xAB) { CHECK(b == 0xAB); break; }
  std::vector<uint32_t> hdr; std::vector<int32_t> K, idx;
  core_decode(ref, ref_off, bpr, g, mk, hdr, K, idx, status);
  for (int32_t s : status) CHECK(s == 0);
  CHECK(K == p.K);
  for (size_t b = 0; b < p.K.size(); ++b)
    for (int32_t t = 0; t < mk; ++t) if (idx[b * mk + t] != (t < p.K[b] ? p.idx[b * mk + t] : 0)) { CHECK(idx[b * mk + t] == (t < p.K[b] ? p.idx[b * mk + t] : 0)); break; }
  for (int32_t i = 0; i < N; ++i) CHECK(hdr[9 * (size_t)i] == 42 && hdr[9 * (size_t)i + 2] == S && hdr[9 * (size_t)i + 8] == bpr.size());
  // one image refused (an index equal to max_index in its last block): its status alone, no bytes, the others unchanged
  if (N == 3) {
    Packed q = p;
    const size_t row = (size_t)2 * p.T - 1;
    if (q.K[row] < 1) q.K[row] = 1;
    std::vector<uint8_t> want; std::vector<int64_t> want_off{0};
    for (int32_t i = 0; i < N; ++i) { if (i != 1) { const auto f = file_of(q, i, g); want.insert(want.end(), f.begin(), f.end()); } want_off.push_back((int64_t)want.size()); }
    q.idx[row * (size_t)mk] = (int32_t)S;
    core_encode(q, g, true, (int64_t)want.size(), out, off, status);
    CHECK(out == want); CHECK(off == want_off); CHECK(status[0] == 0 && status[1] == IREC_REC_E_INDEX_RANGE && status[2] == 0);
  }
}

void check_damaged() {
  const std::vector<int32_t> bpr{3, 1, 9};
  const int32_t g = 4, T = 13, mk = 29, R = 3, n_seg = 5;
  const Packed p = make(1, bpr, mk, 36, 1);
  const std::vector<uint8_t> data = file_of(p, 0, g);
  const int64_t n = (int64_t)data.size(), head = 40 + 4 * R + 12 * n_seg;
  std::vector<std::vector<uint8_t>> files;
  for (int64_t k = 0; k < n; ++k) files.emplace_back(data.begin(), data.begin() + k);
  { std::vector<uint8_t> b = data; b.push_back(0); files.push_back(b); }
  for (int64_t k = 0; k < head; ++k)
    for (int v : {0x00, 0x01, 0xFF}) { std::vector<uint8_t> b = data; b[(size_t)k] = (uint8_t)(b[(size_t)k] == v ? v ^ 0x80 : v); files.push_back(b); }
  for (int c = 0; c < 800; ++c) {
    std::vector<uint8_t> b = data;
    for (int64_t q = 1 + below(3); q > 0; --q) b[(size_t)below(n)] = (uint8_t)below(256);
    files.push_back(b);
  }
  files.push_back(data);
  std::vector<uint8_t> blob; std::vector<int64_t> off{0};
  for (auto &f : files) { blob.insert(blob.end(), f.begin(), f.end()); off.push_back((int64_t)blob.size()); }
  std::vector<uint32_t> hdr, h1; std::vector<int32_t> K, idx, status, k1, i1, s1;
  core_decode(blob, off, bpr, g, mk, hdr, K, idx, status);
  int64_t accepted = 0, rejected = 0;
  const size_t nK = (size_t)T, nI = nK * mk;
  int seen[32] = {0};
  for (size_t f = 0; f < files.size(); ++f) {
    core_decode(files[f], {0, (int64_t)files[f].size()}, bpr, g, mk, h1, k1, i1, s1);   // alone, in a buffer of its own size
    CHECK(s1[0] == status[f]);
    CHECK(std::equal(h1.begin(), h1.end(), hdr.begin() + 9 * f)); CHECK(std::equal(k1.begin(), k1.end(), K.begin() + nK * f));
    CHECK(std::equal(i1.begin(), i1.end(), idx.begin() + nI * f));
    if (status[f] >= 0 && status[f] < 32) seen[status[f]] = 1;
    if (status[f] == 0) ++accepted;
    else {
      ++rejected;
      for (size_t e = 0; e < 9; ++e) CHECK(hdr[9 * f + e] == 0);
      for (size_t e = 0; e < nK; ++e) if (K[nK * f + e]) { CHECK(K[nK * f + e] == 0); break; }
      for (size_t e = 0; e < nI; ++e) if (idx[nI * f + e]) { CHECK(idx[nI * f + e] == 0); break; }
    }
  }
  for (int64_t k = 0; k <= n; ++k) CHECK(status[(size_t)k] != 0);            // every prefix and the file with a byte more
  CHECK(status.back() == 0 && std::equal(p.K.begin(), p.K.end(), K.end() - (int64_t)nK));
  CHECK(seen[IREC_REC_E_SEG_MAGIC] && seen[IREC_REC_E_SEG_DIRECTORY] && seen[IREC_REC_E_SEG_BLOCKS] && seen[IREC_REC_E_TRUNCATED_HEADER] && seen[IREC_REC_E_STRUCTURE]);
  // the call's own words: another segment size, a max_K below the file's largest max_part
  core_decode(data, {0, n}, bpr, 2, mk, h1, k1, i1, s1); CHECK(s1[0] == IREC_REC_E_SEG_BLOCKS);
  core_decode(data, {0, n}, bpr, g, mk - 1, h1, k1, i1, s1); CHECK(s1[0] == IREC_REC_E_MAX_K);
  core_decode(data, {0, n}, {3, 1, 8}, g, mk, h1, k1, i1, s1); CHECK(s1[0] == IREC_REC_E_STRUCTURE);
  std::printf("damaged set: %zu files of a %lld-byte (3, 1, 9), g = 4 container, %lld accepted and %lld rejected, in the blob and alone alike; statuses reached:",
              files.size(), (long long)n, (long long)accepted, (long long)rejected);
  for (int s = 0; s < 32; ++s) if (seen[s]) std::printf(" %d", s);
  std::printf("\n");
}

void check_layout_bounds() {
  int32_t first[IREC_REC_RAGGED_MAX_RES + 1];
  irec_rec::SegLayout L;
  CHECK(!layouts({4, 1}, 0, first, &L)); CHECK(!layouts({4, 1}, -1, first, &L));
  CHECK(layouts({4, 1}, 3, first, &L) && L.S == 3 && L.seg_first[1] == 2 && L.seg_first[2] == 3 && L.seg_first[IREC_REC_RAGGED_MAX_RES] == 3);
  CHECK(!layouts({1 << 30}, 1, first, &L)); CHECK(layouts({1 << 22}, 1, first, &L) && L.S == 1 << 22); CHECK(!layouts({(1 << 22) + 1}, 1, first, &L));
  CHECK(layouts({0x7fffffff}, 0x7fffffff, first, &L) && L.S == 1);
  std::printf("layout bounds: segment_blocks below 1 and more than 2^22 segments per image refused\n");
}
} // namespace

int main() {
  const std::vector<std::pair<std::vector<int32_t>, int32_t>> structures{{{1}, 4}, {{1, 4}, 7}, {{3, 1, 5}, 12}, {{2, 2, 2}, 3}, {{13, 302}, 9}};
  for (const auto &s : structures) {
    for (int32_t N : {1, 3})
      for (uint32_t S : {1u, 20u, 36u})
        for (int32_t g : {1, 2, 4, 16, 512}) check_structure(N, s.first, s.second, S, g);
    std::printf("structure (");
    for (size_t r = 0; r < s.first.size(); ++r) std::printf(r ? ", %d" : "%d", s.first[r]);
    std::printf("), max_K = %d: N = 1, 3 x max_index = 1, 20, 36 x segment_blocks = 1, 2, 4, 16, 512: encode (contiguous, strided, exact and short cap, one image "
                "refused) equal to irec_io.cpp's streams, decode equal to the rows\n", s.second);
  }
  check_damaged();
  check_layout_bounds();
  if (g_failures) { std::printf("rec_seg_check: %d FAILED\n", g_failures); return 1; }
  std::printf("rec_seg_check: all equal\n");
  return 0;
}
