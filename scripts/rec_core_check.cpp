// rec_core_check.cpp -- the device .rec coder's core (csrc/irec_rec_core.h) under the host sanitizers, against irec_io.cpp.
// A stand-alone program: it includes both, so that every line of the core the kernels run is compiled here by g++ and runs with
// AddressSanitizer and UndefinedBehaviorSanitizer.  Build and run from the repository root:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude -Irelative-entropy-coding_amd/csrc \
//       scripts/rec_core_check.cpp -o /tmp/rec_core_check -lpthread && /tmp/rec_core_check
// It walks the six shapes of tests/test_rec_device_host.py (contiguous and strided input, a short cap, decoding) and a damaged set built
// like that test's (every prefix of a 6 x 9 x 29 container, 800 copies with one to three bytes replaced, 200 with a byte of the header's
// free fields replaced), with output buffers sized EXACTLY, so that one byte or one index past a range is a report.  Exit status 0 and
// the last line "rec_core_check: all equal" mean: same bytes, same verdicts, same indices as irec_io.cpp, and no sanitizer report
// (profiles/rec_device/sanitizer_core.log is this program's output).
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "irec_io.cpp"
#include "irec_rec_core.h"

namespace {
uint64_t g_state = 0x9E3779B97F4A7C15ull;
uint64_t rnd() { g_state += 0x9E3779B97F4A7C15ull; uint64_t z = g_state; z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; return z ^ (z >> 31); }
int64_t below(int64_t n) { return (int64_t)(rnd() % (uint64_t)n); }
int g_failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++g_failures; } } while (0)

struct Packed { int32_t N, R, bpt, mk; uint32_t S; std::vector<int32_t> K, idx; };
Packed make(int32_t N, int32_t R, int32_t bpt, int32_t mk, uint32_t S, bool zero_second) {
  Packed p{N, R, bpt, mk, S, std::vector<int32_t>((size_t)N * R * bpt), std::vector<int32_t>((size_t)N * R * bpt * mk)};
  for (auto &k : p.K) k = (int32_t)below(mk + 1);
  if (zero_second) for (int32_t i = 0; i < N; ++i) for (int32_t j = 0; j < bpt; ++j) p.K[((size_t)i * R + 1) * bpt + j] = 0;
  for (auto &v : p.idx) v = (int32_t)below(S);
  return p;
}

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
  out.assign((size_t)cap, 0xAB); off.assign((size_t)p.N + 1, -1); status.assign((size_t)p.N, -1);
  std::vector<uint8_t> ws((size_t)irec_rec::encode_workspace_bytes(p.N, p.R));
  irec_rec::EncodeCall c{42, 1000, p.S, 32, 32, 3, p.N, p.R, p.bpt, p.mk, K, ks, idx, is, out.data(), cap, off.data(), status.data(), nullptr, nullptr, nullptr};
  irec_rec::encode_bind_workspace(c, ws.data());
  irec_rec::encode_call_host(c);
}

void core_decode(const std::vector<uint8_t> &blob, const std::vector<int64_t> &off, int32_t R, int32_t bpt, int32_t mk, std::vector<uint32_t> &hdr,
                 std::vector<int32_t> &K, std::vector<int32_t> &idx, std::vector<int32_t> &status) {
  const int32_t N = (int32_t)off.size() - 1;
  hdr.assign((size_t)N * 9, 0xFFFFFFFFu); K.assign((size_t)N * R * bpt, -1); idx.assign((size_t)N * R * bpt * mk, -1); status.assign((size_t)N, -1);
  std::vector<int32_t> ws((size_t)(irec_rec::decode_workspace_bytes(N, R) / 4));
  // (a copy of exactly the blob's size: a read past the last file is a heap-buffer-overflow report)
  std::vector<uint8_t> exact(blob.begin(), blob.end());
  irec_rec::DecodeCall c{exact.data(), off.data(), N, R, bpt, mk, hdr.data(), K.data(), idx.data(), status.data(), ws.data()};
  irec_rec::decode_call_host(c);
}

void check_shape(int32_t N, int32_t R, int32_t bpt, int32_t mk, uint32_t S, bool zero_second) {
  const Packed p = make(N, R, bpt, mk, S, zero_second);
  std::vector<int64_t> ref_off((size_t)N + 1);
  int64_t total = irec_rec_encode_files(42, 1000, S, 32, 32, 3, N, R, bpt, mk, p.K.data(), p.idx.data(), nullptr, 0, ref_off.data(), 1);
  CHECK(total > 0);
  std::vector<uint8_t> ref((size_t)total);
  CHECK(irec_rec_encode_files(42, 1000, S, 32, 32, 3, N, R, bpt, mk, p.K.data(), p.idx.data(), ref.data(), total, ref_off.data(), 1) == total);
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
  core_decode(ref, ref_off, R, bpt, mk, hdr, K, idx, status);
  CHECK(irec_rec_decode_files(ref.data(), ref_off.data(), N, R, bpt, mk, ref_hdr.data(), ref_K.data(), ref_idx.data(), 1) == IREC_OK);
  CHECK(hdr == ref_hdr); CHECK(K == ref_K); CHECK(idx == ref_idx); CHECK(K == p.K);
  for (int32_t s : status) CHECK(s == 0);
  std::printf("shape (%d, %d, %d, %d, %u): %lld bytes, encode (contiguous, strided, short cap) and decode equal to irec_io.cpp\n", N, R, bpt, mk, S, (long long)total);
}

void check_damaged() {
  const int32_t R = 6, bpt = 9, mk = 29;
  const Packed p = make(1, R, bpt, mk, 36, false);
  std::vector<int64_t> o2(2);
  const int64_t n = irec_rec_encode_files(42, 1000, 36, 32, 32, 3, 1, R, bpt, mk, p.K.data(), p.idx.data(), nullptr, 0, o2.data(), 1);
  std::vector<uint8_t> data((size_t)n);
  CHECK(irec_rec_encode_files(42, 1000, 36, 32, 32, 3, 1, R, bpt, mk, p.K.data(), p.idx.data(), data.data(), n, o2.data(), 1) == n);
  std::vector<std::vector<uint8_t>> files;
  for (int64_t k = 0; k < n; ++k) files.emplace_back(data.begin(), data.begin() + k);
  for (int c = 0; c < 800; ++c) {
    std::vector<uint8_t> b = data;
    for (int64_t q = 1 + below(3); q > 0; --q) b[(size_t)below(n)] = (uint8_t)below(256);
    files.push_back(b);
  }
  const int fields[18] = {0, 1, 2, 3, 4, 5, 6, 7, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21};
  for (int c = 0; c < 200; ++c) { std::vector<uint8_t> b = data; b[(size_t)fields[below(18)]] = (uint8_t)below(256); files.push_back(b); }
  std::vector<uint8_t> blob; std::vector<int64_t> off{0};
  for (auto &f : files) { blob.insert(blob.end(), f.begin(), f.end()); off.push_back((int64_t)blob.size()); }
  std::vector<uint32_t> hdr; std::vector<int32_t> K, idx, status;
  core_decode(blob, off, R, bpt, mk, hdr, K, idx, status);
  int64_t accepted = 0, rejected = 0;
  const size_t nK = (size_t)R * bpt, nI = nK * mk;
  for (size_t f = 0; f < files.size(); ++f) {
    std::vector<uint8_t> one = files[f];
    if (one.empty()) one.push_back(0);                                   // (the host reader refuses a null pointer before it looks at the size)
    const int64_t o[2] = {0, (int64_t)files[f].size()};
    std::vector<uint32_t> h(9); std::vector<int32_t> k(nK), ix(nI);
    const bool ok = irec_rec_decode_files(one.data(), o, 1, R, bpt, mk, h.data(), k.data(), ix.data(), 1) == IREC_OK;
    CHECK(ok == (status[f] == 0));
    if (ok && status[f] == 0) {
      ++accepted;
      CHECK(std::equal(h.begin(), h.end(), hdr.begin() + 9 * f)); CHECK(std::equal(k.begin(), k.end(), K.begin() + nK * f));
      CHECK(std::equal(ix.begin(), ix.end(), idx.begin() + nI * f));
    } else ++rejected;
  }
  CHECK(accepted >= 200 && rejected >= (int64_t)n + 700);
  std::printf("damaged set: %zu files of a %lld-byte container, %lld accepted and %lld rejected by both readers alike\n", files.size(), (long long)n,
              (long long)accepted, (long long)rejected);
}
} // namespace

int main() {
  check_shape(3, 1, 1, 4, 20, false);
  check_shape(9, 5, 9, 12, 36, false);
  check_shape(2, 2, 64, 2, 36, true);
  check_shape(2, 1, 3, 300, 1, false);
  check_shape(2, 2, 5, 6, 1u << 20, false);
  check_shape(1500, 1, 1, 2, 36, false);
  check_damaged();
  if (g_failures) { std::printf("rec_core_check: %d FAILED\n", g_failures); return 1; }
  std::printf("rec_core_check: all equal\n");
  return 0;
}
