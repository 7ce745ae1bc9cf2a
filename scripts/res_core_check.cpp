// res_core_check.cpp -- the .res coder's core (csrc/irec_res_core.h: the model, the stream coder, the lane functions and the whole-call
// forms that the host entry points irec_res_encode_files / irec_res_decode_files run) under the host sanitizers.
// A stand-alone program: every line of the core that the kernels run is compiled here by g++ and runs with AddressSanitizer and
// UndefinedBehaviorSanitizer.  Build and run from the repository root:
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude \
//       -Irelative-entropy-coding_amd/csrc scripts/res_core_check.cpp -o /tmp/res_core_check -lpthread && /tmp/res_core_check
// It walks a set of shapes (ragged last streams, stream_len 1, one stream, tiny and huge scales), serially and on a pool of threads,
// with every buffer sized EXACTLY -- pixels, loc, the output at the size the sizing run reports, the workspace, and for the reader
// every file in an allocation of its own -- so that one byte past a range is a report.  Then a damaged set: every prefix of a file,
// 800 copies with one to three bytes replaced, and a loc moved under the decoder.  Exit status 0 and the last line
// "res_core_check: all equal" mean: every round trip exact, serial and threaded runs the same bytes, every damaged file answered with
// a status and zeroed pixels, and no sanitizer report (profiles/residual/sanitizer_core.log is this program's output).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>

#include "irec_res_core.h"

namespace {
uint64_t g_state = 0x9E3779B97F4A7C15ull;
uint64_t rnd() { g_state += 0x9E3779B97F4A7C15ull; uint64_t z = g_state; z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; return z ^ (z >> 31); }
int64_t below(int64_t n) { return (int64_t)(rnd() % (uint64_t)n); }
int g_failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++g_failures; } } while (0)

struct PoolLanes {   // chunks of 3 lanes over 4 threads: neighbouring lanes on different threads
  template <class F> void operator()(int64_t n, F &&body) const {
    std::vector<std::thread> pool;
    for (int t = 0; t < 4; ++t)
      pool.emplace_back([&body, t, n]() { for (int64_t lo = 3 * t; lo < n; lo += 12) body(lo, lo + 3 < n ? lo + 3 : n); });
    for (auto &th : pool) th.join();
  }
};

struct Images { int32_t N; uint32_t h, w, c, L; float scale; std::vector<uint8_t> pixels; std::vector<float> loc; int64_t n_sym, ns; };
Images make(int32_t N, uint32_t h, uint32_t w, uint32_t c, uint32_t L, float scale, int spread) {
  Images im{N, h, w, c, L, scale, {}, {}, (int64_t)h * w * c, 0};
  im.ns = irec_res::n_streams_of(im.n_sym, L);
  im.pixels.resize((size_t)(N * im.n_sym)); im.loc.resize((size_t)(N * im.n_sym));
  for (size_t e = 0; e < im.pixels.size(); ++e) {
    const int centre = (int)below(256);
    int x = centre + (int)below(2 * spread + 1) - spread;
    im.pixels[e] = (uint8_t)(x < 0 ? 0 : (x > 255 ? 255 : x));
    float l = ((float)centre + 0.5f) / 256.0f - 0.5f;
    im.loc[e] = l < -0.498046875f ? -0.498046875f : (l > 0.498046875f ? 0.498046875f : l);
  }
  return im;
}

template <class Par>
void core_encode(const Images &im, int64_t cap, std::vector<uint8_t> &out, std::vector<int64_t> &off, std::vector<int32_t> &status, Par par) {
  out.assign((size_t)cap, 0xAB); off.assign((size_t)im.N + 1, -1); status.assign((size_t)im.N, -1);
  std::vector<int64_t> ws((size_t)(irec_res::workspace_bytes(im.N, im.ns) + 7) / 8);
  irec_res::EncodeCall c{im.pixels.data(), im.loc.data(), im.scale, im.N, (int32_t)im.ns, im.h, im.w, im.c, im.L, im.n_sym,
                         cap ? out.data() : nullptr, cap, off.data(), status.data(), nullptr, nullptr, nullptr, nullptr};
  irec_res::encode_bind_workspace(c, ws.data());
  irec_res::encode_call_host(c, par);
}

// one file in an allocation of exactly its size, decoded with loc of exactly one image
template <class Par>
int32_t core_decode_one(const Images &im, const uint8_t *file, int64_t n_bytes, const float *loc, std::vector<uint8_t> &pixels, Par par) {
  std::vector<uint8_t> exact(file, file + n_bytes);
  std::vector<float> l(loc, loc + im.n_sym);
  pixels.assign((size_t)im.n_sym, 0xCD);
  const int64_t off[2] = {0, n_bytes};
  int32_t status = -1;
  std::vector<int64_t> ws((size_t)(irec_res::workspace_bytes(1, im.ns) + 7) / 8);
  irec_res::DecodeCall c{exact.data(), off, l.data(), im.scale, 1, (int32_t)im.ns, im.h, im.w, im.c, im.L, im.n_sym, pixels.data(), &status,
                         nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  irec_res::decode_bind_workspace(c, ws.data());
  irec_res::decode_call_host(c, par);
  return status;
}

bool all_zero(const std::vector<uint8_t> &v) { for (uint8_t b : v) if (b) return false; return true; }

void round_trip(const Images &im, std::vector<uint8_t> &blob, std::vector<int64_t> &off) {
  std::vector<uint8_t> none, out2; std::vector<int64_t> off0, off2; std::vector<int32_t> st0, st, st2;
  core_encode(im, 0, none, off0, st0, irec_res::SerialLanes{});                // the sizing run: nothing to write into
  for (int32_t s : st0) CHECK(s == IREC_RES_OK);
  const int64_t total = off0[im.N];
  core_encode(im, total - 1, blob, off, st, irec_res::SerialLanes{});         // one byte short: nothing written
  CHECK(off == off0);
  for (uint8_t b : blob) CHECK(b == 0xAB);
  core_encode(im, total, blob, off, st, irec_res::SerialLanes{});
  core_encode(im, total, out2, off2, st2, PoolLanes{});
  CHECK(off == off0 && off2 == off0 && blob == out2);
  std::vector<uint8_t> pixels;
  for (int32_t i = 0; i < im.N; ++i) {
    const std::vector<uint8_t> want(im.pixels.begin() + i * im.n_sym, im.pixels.begin() + (i + 1) * im.n_sym);
    CHECK(core_decode_one(im, blob.data() + off[i], off[i + 1] - off[i], im.loc.data() + i * im.n_sym, pixels, irec_res::SerialLanes{}) == IREC_RES_OK);
    CHECK(pixels == want);
    CHECK(core_decode_one(im, blob.data() + off[i], off[i + 1] - off[i], im.loc.data() + i * im.n_sym, pixels, PoolLanes{}) == IREC_RES_OK);
    CHECK(pixels == want);
  }
}
} // namespace

int main() {
  std::vector<uint8_t> blob, pixels; std::vector<int64_t> off;
  // the model: counts strictly increasing at the ends of m and of the scale's range
  for (float s : {5.9604644775390625e-08f, 1e-4f, 0.00390625f, 0.05f, 1.0f, 100.0f, 16777216.0f})
    for (int32_t m = -2048; m <= 2047; m += 13) {
      const double inv = irec_res::model_inv(s);
      uint32_t prev = 0;
      for (int32_t k = 1; k <= 256; ++k) { const uint32_t C = irec_res::cum(m, inv, k); CHECK(C > prev); prev = C; }
      CHECK(prev == 65536u);
    }
  const Images shapes[] = {make(2, 2, 2, 3, 5, 0.05f, 6), make(2, 2, 2, 3, 1, 0.05f, 6), make(1, 2, 2, 3, 4096, 0.05f, 6),
                           make(1, 4, 4, 3, 16, 1e-4f, 120), make(2, 4, 4, 3, 7, 100.0f, 100), make(6, 8, 8, 3, 4, 0.00390625f, 3),
                           make(3, 5, 7, 1, 9, 5.9604644775390625e-08f, 255), make(1, 32, 32, 3, 64, 0.02f, 10)};
  for (const Images &im : shapes) round_trip(im, blob, off);
  std::printf("round trips done, failures so far %d\n", g_failures);

  // damage, on the files of 6 x 8 x 8 x 3 at stream_len 4
  const Images &im = shapes[5];
  round_trip(im, blob, off);
  const uint8_t *file = blob.data() + off[1];
  const int64_t n_bytes = off[2] - off[1];
  const float *loc = im.loc.data() + im.n_sym;
  for (int64_t cut = 0; cut < n_bytes; ++cut) {
    const int32_t st = core_decode_one(im, file, cut, loc, pixels, irec_res::SerialLanes{});
    CHECK(st == (cut < 28 + 2 * im.ns ? IREC_RES_E_TRUNCATED_HEADER : IREC_RES_E_TRUNCATED_STREAMS));
    CHECK(all_zero(pixels));
  }
  int refused = 0;
  for (int rep = 0; rep < 800; ++rep) {
    std::vector<uint8_t> bad(file, file + n_bytes);
    for (int64_t k = 1 + below(3); k > 0; --k) bad[(size_t)below(n_bytes)] = (uint8_t)below(256);
    const int32_t st = core_decode_one(im, bad.data(), n_bytes, loc, pixels, irec_res::SerialLanes{});
    const bool same = std::memcmp(bad.data(), file, (size_t)n_bytes) == 0;
    CHECK(st >= 0 && st <= IREC_RES_E_CHECKSUM);
    if (st) { ++refused; CHECK(all_zero(pixels)); }
    else CHECK(same || std::memcmp(pixels.data(), im.pixels.data() + im.n_sym, (size_t)im.n_sym) == 0);   // (padding bits carry nothing)
  }
  std::printf("800 damaged copies: %d refused\n", refused);
  {   // another loc under the decoder
    std::vector<float> moved(loc, loc + im.n_sym);
    moved[17] -= 1.0f / 256.0f;
    const int32_t st = core_decode_one(im, file, n_bytes, moved.data(), pixels, PoolLanes{});
    CHECK(st == IREC_RES_E_CHECKSUM || st == IREC_RES_E_CORRUPT);
    CHECK(all_zero(pixels));
  }
  {   // encode statuses
    Images bad = shapes[0];
    std::vector<int32_t> st;
    bad.scale = 0.0f;
    core_encode(bad, 0, blob, off, st, irec_res::SerialLanes{});
    CHECK(st[0] == IREC_RES_E_SCALE && st[1] == IREC_RES_E_SCALE && off[2] == 0);
    bad.scale = 0.05f; bad.loc[(size_t)bad.n_sym + 3] = __builtin_nanf("");
    core_encode(bad, 4096, blob, off, st, irec_res::SerialLanes{});
    CHECK(st[0] == IREC_RES_OK && st[1] == IREC_RES_E_LOC && off[2] == off[1]);
  }
  if (g_failures) { std::printf("res_core_check: %d FAILURES\n", g_failures); return 1; }
  std::printf("res_core_check: all equal\n");
  return 0;
}
