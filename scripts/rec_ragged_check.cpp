// rec_ragged_check.cpp -- the ragged layout of the device .rec coder's core (csrc/irec_rec_core.h: residual blocks of differing sizes)
// under the host sanitizers, against irec_io.cpp.  A stand-alone program in the manner of scripts/rec_core_check.cpp: it includes both, so
// that every line of the core the kernels run is compiled here by g++ and runs with AddressSanitizer and UndefinedBehaviorSanitizer.
// Build and run from the repository root, on a CPU:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude -Irelative-entropy-coding_amd/csrc \
//       scripts/rec_ragged_check.cpp -o /tmp/rec_ragged_check -lpthread && /tmp/rec_ragged_check
// It walks the structures of tests/test_rec_ragged_host.py -- (1), (1, 4), (3, 1, 5), (2, 2, 2), (13, 302) and 64 blocks of one -- at
// N = 1 and 3 and max_index = 1, 20, 36 (contiguous and strided input, a short cap, decoding, the same files read as another structure)
// and a damaged set of a (3, 1, 9) container (every prefix, 800 copies with one to three bytes replaced, 300 with a byte of the dynamic
// header or the count streams replaced), with every buffer sized EXACTLY, so that one byte or one index past a range is a report.  The
// referee of every file is irec_rec_encode_file / irec_rec_decode_file on that image alone.  Exit status 0 and the last line
// "rec_ragged_check: all equal" mean: same bytes, same verdicts, same indices as irec_io.cpp, and no sanitizer report
// (profiles/lossy/sanitizer_core.log is this program's output).
#include <cstdio>
#include <cstdlib>
#include <numeric>
#include <vector>

#include "irec_io.cpp"
#include "irec_rec_core.h"

namespace {
uint64_t g_state = 0x9E3779B97F4A7C15ull;
uint64_t rnd() { g_state += 0x9E3779B97F4A7C15ull; uint64_t z = g_state; z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; return z ^ (z >> 31); }
int64_t below(int64_t n) { return (int64_t)(rnd() % (uint64_t)n); }
int g_failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++g_failures; } } while (0)

struct Packed { int32_t N, mk; uint32_t S; std::vector<int32_t> bpr; int32_t T; std::vector<int32_t> K, idx; };
Packed make(int32_t N, const std::vector<int32_t> &bpr, int32_t mk, uint32_t S) {
  const int32_t T = std::accumulate(bpr.begin(), bpr.end(), 0);
  Packed p{N, mk, S, bpr, T, std::vector<int32_t>((size_t)N * T), std::vector<int32_t>((size_t)N * T * mk)};
  for (auto &k : p.K) k = (int32_t)below(mk + 1);
  if (p.K.size() > 1) p.K[0] = 0;                                        // a row without indices and a full one in every call
  p.K.back() = mk;
  for (auto &v : p.idx) v = (int32_t)below(S);
  return p;
}

// irec_rec_encode_file on image i alone
std::vector<uint8_t> file_of(const Packed &p, int32_t i, const std::vector<int32_t> &bpr) {
  std::vector<int32_t> flat;
  for (int32_t b = 0; b < p.T; ++b)
    for (int32_t t = 0; t < p.K[(size_t)i * p.T + b]; ++t) flat.push_back(p.idx[((size_t)i * p.T + b) * p.mk + t]);
  flat.push_back(0);                                                     // (never read: keeps data() non-null for an image without indices)
  const int64_t n = irec_rec_encode_file(42, 1000, p.S, 32, 48, 3, (int32_t)bpr.size(), bpr.data(), p.K.data() + (size_t)i * p.T, flat.data(), nullptr, 0);
  CHECK(n > 0);
  std::vector<uint8_t> f((size_t)(n > 0 ? n : 0));
  CHECK(irec_rec_encode_file(42, 1000, p.S, 32, 48, 3, (int32_t)bpr.size(), bpr.data(), p.K.data() + (size_t)i * p.T, flat.data(), f.data(), n) == n);
  return f;
}

bool layout_of(const std::vector<int32_t> &bpr, int32_t *first) { return irec_rec::ragged_first((int32_t)bpr.size(), bpr.data(), first); }

// the core over exactly-sized host buffers: out [cap], offsets [N + 1], status [N]
void core_encode(const Packed &p, bool strided, int64_t cap, std::vector<uint8_t> &out, std::vector<int64_t> &off, std::vector<int32_t> &status) {
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
  std::vector<uint8_t> ws((size_t)irec_rec::encode_workspace_bytes(p.N, R));
  irec_rec::EncodeCall c{42, 1000, p.S, 32, 48, 3, p.N, R, 0, p.mk, K, ks, idx, is, out.data(), cap, off.data(), status.data(), nullptr, nullptr, nullptr, {}};
  CHECK(layout_of(p.bpr, c.first));
  irec_rec::encode_bind_workspace(c, ws.data());
  irec_rec::encode_call_host(c);
}

void core_decode(const std::vector<uint8_t> &blob, const std::vector<int64_t> &off, const std::vector<int32_t> &bpr, int32_t mk, std::vector<uint32_t> &hdr,
                 std::vector<int32_t> &K, std::vector<int32_t> &idx, std::vector<int32_t> &status) {
  const int32_t N = (int32_t)off.size() - 1, R = (int32_t)bpr.size(), T = std::accumulate(bpr.begin(), bpr.end(), 0);
  hdr.assign((size_t)N * 9, 0xFFFFFFFFu); K.assign((size_t)N * T, -1); idx.assign((size_t)N * T * mk, -1); status.assign((size_t)N, -1);
  std::vector<int32_t> ws((size_t)(irec_rec::decode_workspace_bytes(N, R) / 4));
  // (a copy of exactly the blob's size: a read past the last file is a heap-buffer-overflow report)
  std::vector<uint8_t> exact(blob.begin(), blob.end());
  irec_rec::DecodeCall c{exact.data(), off.data(), N, R, 0, mk, hdr.data(), K.data(), idx.data(), status.data(), ws.data(), {}};
  CHECK(layout_of(bpr, c.first));
  irec_rec::decode_call_host(c);
}

void check_structure(int32_t N, const std::vector<int32_t> &bpr, int32_t mk, uint32_t S) {
  const Packed p = make(N, bpr, mk, S);
  const int32_t R = (int32_t)bpr.size();
  std::vector<uint8_t> ref; std::vector<int64_t> ref_off{0};
  for (int32_t i = 0; i < N; ++i) { const auto f = file_of(p, i, bpr); ref.insert(ref.end(), f.begin(), f.end()); ref_off.push_back((int64_t)ref.size()); }
  const int64_t total = (int64_t)ref.size();
  // the host-thread coder: the same bytes
  std::vector<int64_t> h_off((size_t)N + 1); std::vector<uint8_t> h_out((size_t)total);
  CHECK(irec_rec_encode_files_ragged(42, 1000, S, 32, 48, 3, N, R, bpr.data(), mk, p.K.data(), p.idx.data(), h_out.data(), total, h_off.data(), 2) == total);
  CHECK(h_out == ref); CHECK(h_off == ref_off);
  std::vector<uint8_t> out; std::vector<int64_t> off; std::vector<int32_t> status;
  for (int strided = 0; strided < 2; ++strided) {
    core_encode(p, strided != 0, total, out, off, status);               // exactly enough room
    CHECK(out == ref); CHECK(off == ref_off);
    for (int32_t s : status) CHECK(s == 0);
  }
  core_encode(p, false, total - 1, out, off, status);                    // one byte short: nothing written, the size reported
  CHECK(off[(size_t)N] == total);
  for (uint8_t b : out) if (b != 0xAB) { CHECK(b == 0xAB); break; }
  std::vector<uint32_t> hdr, ref_hdr((size_t)N * 9); std::vector<int32_t> K, idx, ref_K(p.K.size()), ref_idx(p.idx.size());
  core_decode(ref, ref_off, bpr, mk, hdr, K, idx, status);
  CHECK(irec_rec_decode_files_ragged(ref.data(), ref_off.data(), N, R, bpr.data(), mk, ref_hdr.data(), ref_K.data(), ref_idx.data(), 2) == IREC_OK);
  CHECK(hdr == ref_hdr); CHECK(K == ref_K); CHECK(idx == ref_idx); CHECK(K == p.K);
  for (int32_t s : status) CHECK(s == 0);
  // the same files read as another split of the same T: every image IREC_REC_E_STRUCTURE, every output zero
  if (R >= 2 && bpr[0] != bpr[(size_t)R - 1]) {
    std::vector<int32_t> other(bpr.rbegin(), bpr.rend());
    core_decode(ref, ref_off, other, mk, hdr, K, idx, status);
    for (int32_t s : status) CHECK(s == IREC_REC_E_STRUCTURE);
    for (uint32_t v : hdr) if (v) { CHECK(v == 0); break; }
    for (int32_t v : K) if (v) { CHECK(v == 0); break; }
    for (int32_t v : idx) if (v) { CHECK(v == 0); break; }
    CHECK(irec_rec_decode_files_ragged(ref.data(), ref_off.data(), N, R, other.data(), mk, ref_hdr.data(), ref_K.data(), ref_idx.data(), 1) == IREC_E_INVALID);
  }
  // one image refused (an index equal to max_index in its last residual block): its status alone, no bytes, the others unchanged
  if (N == 3) {
    Packed q = p;
    const size_t row = (size_t)1 * p.T + (size_t)(p.T - bpr[(size_t)R - 1]);
    if (q.K[row] < 1) q.K[row] = 1;
    std::vector<uint8_t> want; std::vector<int64_t> want_off{0};
    for (int32_t i = 0; i < N; ++i) { if (i != 1) { const auto f = file_of(q, i, bpr); want.insert(want.end(), f.begin(), f.end()); } want_off.push_back((int64_t)want.size()); }
    q.idx[row * (size_t)mk] = (int32_t)S;
    core_encode(q, true, (int64_t)want.size(), out, off, status);
    CHECK(out == want); CHECK(off == want_off); CHECK(status[0] == 0 && status[1] == IREC_REC_E_INDEX_RANGE && status[2] == 0);
  }
  std::printf("structure (");
  for (int32_t r = 0; r < R && r < 4; ++r) std::printf(r ? ", %d" : "%d", bpr[(size_t)r]);
  std::printf("%s) N = %d, max_K = %d, max_index = %u: %lld bytes, encode (contiguous, strided, short cap, host threads) and decode equal to irec_io.cpp\n",
              R > 4 ? ", ..." : "", N, mk, S, (long long)total);
}

void check_damaged() {
  const std::vector<int32_t> bpr{3, 1, 9};
  const int32_t R = 3, T = 13, mk = 29;
  const Packed p = make(1, bpr, mk, 36);
  const std::vector<uint8_t> data = file_of(p, 0, bpr);
  const int64_t n = (int64_t)data.size();
  std::vector<std::vector<uint8_t>> files;
  for (int64_t k = 0; k < n; ++k) files.emplace_back(data.begin(), data.begin() + k);
  for (int c = 0; c < 800; ++c) {
    std::vector<uint8_t> b = data;
    for (int64_t q = 1 + below(3); q > 0; --q) b[(size_t)below(n)] = (uint8_t)below(256);
    files.push_back(b);
  }
  int64_t counts_hi = 28 + 16 * R;
  for (int32_t r = 0; r < R; ++r) counts_hi += irec_rec::get_u32(data.data() + 28 + 4 * (R + r));
  for (int c = 0; c < 300; ++c) { std::vector<uint8_t> b = data; b[(size_t)(28 + below(counts_hi - 28))] = (uint8_t)below(256); files.push_back(b); }
  std::vector<uint8_t> blob; std::vector<int64_t> off{0};
  for (auto &f : files) { blob.insert(blob.end(), f.begin(), f.end()); off.push_back((int64_t)blob.size()); }
  std::vector<uint32_t> hdr; std::vector<int32_t> K, idx, status;
  core_decode(blob, off, bpr, mk, hdr, K, idx, status);
  int64_t accepted = 0, rejected = 0;
  const size_t nK = (size_t)T, nI = nK * mk;
  int seen[32] = {0};
  for (size_t f = 0; f < files.size(); ++f) {
    std::vector<uint8_t> one = files[f];
    if (one.empty()) one.push_back(0);                                   // (the host reader refuses a null pointer before it looks at the size)
    const int64_t o[2] = {0, (int64_t)files[f].size()};
    std::vector<uint32_t> h(9); std::vector<int32_t> k(nK), ix(nI);
    const bool ok = irec_rec_decode_files_ragged(one.data(), o, 1, R, bpr.data(), mk, h.data(), k.data(), ix.data(), 1) == IREC_OK;
    CHECK(ok == (status[f] == 0));
    if (status[f] >= 0 && status[f] < 32) seen[status[f]] = 1;
    if (ok && status[f] == 0) {
      ++accepted;
      CHECK(std::equal(h.begin(), h.end(), hdr.begin() + 9 * f)); CHECK(std::equal(k.begin(), k.end(), K.begin() + nK * f));
      CHECK(std::equal(ix.begin(), ix.end(), idx.begin() + nI * f));
    } else {
      ++rejected;
      for (size_t e = 0; e < 9; ++e) CHECK(hdr[9 * f + e] == 0);
      for (size_t e = 0; e < nK; ++e) if (K[nK * f + e]) { CHECK(K[nK * f + e] == 0); break; }
      for (size_t e = 0; e < nI; ++e) if (idx[nI * f + e]) { CHECK(idx[nI * f + e] == 0); break; }
    }
  }
  CHECK(accepted >= 1 && rejected >= (int64_t)n + 600);
  std::printf("damaged set: %zu files of a %lld-byte (3, 1, 9) container, %lld accepted and %lld rejected by both readers alike; statuses reached:", files.size(),
              (long long)n, (long long)accepted, (long long)rejected);
  for (int s = 0; s < 32; ++s) if (seen[s]) std::printf(" %d", s);
  std::printf("\n");
}

void check_layout_bounds() {
  int32_t first[IREC_REC_RAGGED_MAX_RES + 1];
  std::vector<int32_t> many((size_t)IREC_REC_RAGGED_MAX_RES + 1, 1);
  CHECK(!layout_of(many, first));                                             // 65 residual blocks
  many.pop_back();
  CHECK(layout_of(many, first) && first[IREC_REC_RAGGED_MAX_RES] == IREC_REC_RAGGED_MAX_RES);
  CHECK(!layout_of({2, 0, 1}, first)); CHECK(!layout_of({3, -1}, first)); CHECK(!layout_of({1 << 30, 1 << 30}, first));
  CHECK(layout_of({(1 << 30) - 1, 1 << 30}, first) && first[2] == 0x7fffffff);
  std::vector<int64_t> o(3);
  const int32_t big[2] = {1 << 30, 1 << 30}, K1[2] = {0, 0};
  CHECK(irec_rec_encode_files_ragged(1, 10, 36, 8, 8, 3, 1, 2, big, 0, K1, nullptr, nullptr, 0, o.data(), 1) == -1);
  std::printf("layout bounds: 64 residual blocks accepted; 65, an entry below 1 and a sum past int32 refused\n");
}
} // namespace

int main() {
  const std::vector<std::pair<std::vector<int32_t>, int32_t>> structures{{{1}, 4}, {{1, 4}, 7}, {{3, 1, 5}, 12}, {{2, 2, 2}, 3}, {{13, 302}, 9},
                                                                        {std::vector<int32_t>(64, 1), 2}};
  for (const auto &s : structures)
    for (int32_t N : {1, 3})
      for (uint32_t S : {1u, 20u, 36u}) check_structure(N, s.first, s.second, S);
  check_damaged();
  check_layout_bounds();
  if (g_failures) { std::printf("rec_ragged_check: %d FAILED\n", g_failures); return 1; }
  std::printf("rec_ragged_check: all equal\n");
  return 0;
}
