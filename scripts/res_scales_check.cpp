// res_scales_check.cpp -- one likelihood scale per channel under the host sanitizers: the version-2 .res container of
// csrc/irec_res_core.h (the ChannelScales policy: the lane functions and whole-call forms that irec_res_encode_files_scales /
// irec_res_decode_files_scales run) and the cost of a batch under candidate scales of csrc/irec_res_fit_core.h (what
// irec_res_scale_bits runs).  A stand-alone program: every line of the two core headers that the kernels run is compiled here by
// g++ and runs with AddressSanitizer and UndefinedBehaviorSanitizer.  Build and run from the repository root:
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude \
//       -Irelative-entropy-coding_amd/csrc scripts/res_scales_check.cpp -o /tmp/res_scales_check -lpthread && /tmp/res_scales_check
// Every buffer is sized EXACTLY (pixels, loc, scales, the output at the size the sizing run reports, the workspaces, every file in an
// allocation of its own), so that one byte past a range is a report.  It walks the shapes whose streams cross channel boundaries,
// serially and on a pool of threads; checks that equal channel scales give version 1's stream bytes; answers a damaged set (every
// prefix of a file, 600 copies with one to three bytes replaced, the other version's file, a moved loc, a bad scale in one channel);
// and holds scale_bits to a plain loop over cum() and the table.  Exit status 0 and the last line "res_scales_check: all equal" mean
// all of that held with no sanitizer report (profiles/residual_scales/sanitizer_core.log is this program's output).
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>

#include "irec_res_fit_core.h"

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

struct Images { int32_t N; uint32_t h, w, c, L; std::vector<float> scales; std::vector<uint8_t> pixels; std::vector<float> loc; int64_t n_sym, ns; };
Images make(int32_t N, uint32_t c, uint32_t h, uint32_t w, uint32_t L, int spread) {
  static const float S[4] = {0.02f, 0.05f, 0.11f, 1.0f};
  Images im{N, h, w, c, L, {}, {}, {}, (int64_t)h * w * c, 0};
  for (uint32_t ch = 0; ch < c; ++ch) im.scales.push_back(S[ch % 4]);
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
irec_res::ChannelScales policy(const Images &im, const std::vector<float> &scales) { return irec_res::ChannelScales{scales.data(), (int64_t)im.h * im.w}; }

// version 2 with im.scales, or version 1 with scale1 (v1 = true)
template <class Par>
void core_encode(const Images &im, bool v1, float scale1, int64_t cap, std::vector<uint8_t> &out, std::vector<int64_t> &off, std::vector<int32_t> &status, Par par) {
  out.assign((size_t)cap, 0xAB); off.assign((size_t)im.N + 1, -1); status.assign((size_t)im.N, -1);
  std::vector<int64_t> ws((size_t)(irec_res::workspace_bytes(im.N, im.ns) + 7) / 8);
  const std::vector<float> scales(im.scales);                                  // exactly channels floats
  irec_res::EncodeCall c{im.pixels.data(), im.loc.data(), scale1, im.N, (int32_t)im.ns, im.h, im.w, im.c, im.L, im.n_sym,
                         cap ? out.data() : nullptr, cap, off.data(), status.data(), nullptr, nullptr, nullptr, nullptr};
  irec_res::encode_bind_workspace(c, ws.data());
  if (v1) irec_res::encode_call_host(c, par); else irec_res::encode_call_host(c, policy(im, scales), par);
}

// one file in an allocation of exactly its size, decoded with loc of exactly one image
template <class Par>
int32_t core_decode_one(const Images &im, bool v1, float scale1, const uint8_t *file, int64_t n_bytes, const float *loc, std::vector<uint8_t> &pixels, Par par) {
  std::vector<uint8_t> exact(file, file + n_bytes);
  std::vector<float> l(loc, loc + im.n_sym);
  const std::vector<float> scales(im.scales);
  pixels.assign((size_t)im.n_sym, 0xCD);
  const int64_t off[2] = {0, n_bytes};
  int32_t status = -1;
  std::vector<int64_t> ws((size_t)(irec_res::workspace_bytes(1, im.ns) + 7) / 8);
  irec_res::DecodeCall c{exact.data(), off, l.data(), scale1, 1, (int32_t)im.ns, im.h, im.w, im.c, im.L, im.n_sym, pixels.data(), &status,
                         nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  irec_res::decode_bind_workspace(c, ws.data());
  if (v1) irec_res::decode_call_host(c, par); else irec_res::decode_call_host(c, policy(im, scales), par);
  return status;
}

bool all_zero(const std::vector<uint8_t> &v) { for (uint8_t b : v) if (b) return false; return true; }

void round_trip(const Images &im, std::vector<uint8_t> &blob, std::vector<int64_t> &off) {
  std::vector<uint8_t> none, out2; std::vector<int64_t> off0, off2; std::vector<int32_t> st0, st, st2;
  core_encode(im, false, 0.0f, 0, none, off0, st0, irec_res::SerialLanes{});   // the sizing run: nothing to write into
  for (int32_t s : st0) CHECK(s == IREC_RES_OK);
  const int64_t total = off0[im.N];
  core_encode(im, false, 0.0f, total - 1, blob, off, st, irec_res::SerialLanes{});   // one byte short: nothing written
  CHECK(off == off0);
  for (uint8_t b : blob) CHECK(b == 0xAB);
  core_encode(im, false, 0.0f, total, blob, off, st, irec_res::SerialLanes{});
  core_encode(im, false, 0.0f, total, out2, off2, st2, PoolLanes{});
  CHECK(off == off0 && off2 == off0 && blob == out2);
  const int64_t head = 24 + 4 * (int64_t)im.c;
  std::vector<uint8_t> pixels;
  for (int32_t i = 0; i < im.N; ++i) {
    const uint8_t *f = blob.data() + off[i];
    CHECK(irec_res::get_u16(f + 4) == 2 && irec_res::get_u16(f + 6) == im.c);
    for (uint32_t ch = 0; ch < im.c; ++ch) CHECK(irec_res::get_u32(f + 20 + 4 * ch) == __builtin_bit_cast(uint32_t, im.scales[ch]));
    CHECK(off[i + 1] - off[i] >= head + 2 * im.ns);
    const std::vector<uint8_t> want(im.pixels.begin() + i * im.n_sym, im.pixels.begin() + (i + 1) * im.n_sym);
    CHECK(core_decode_one(im, false, 0.0f, f, off[i + 1] - off[i], im.loc.data() + i * im.n_sym, pixels, irec_res::SerialLanes{}) == IREC_RES_OK);
    CHECK(pixels == want);
    CHECK(core_decode_one(im, false, 0.0f, f, off[i + 1] - off[i], im.loc.data() + i * im.n_sym, pixels, PoolLanes{}) == IREC_RES_OK);
    CHECK(pixels == want);
  }
}

// all channels at one scale: the streams (and their length words) are version 1's
void equal_scales(Images im) {
  std::vector<uint8_t> a, b; std::vector<int64_t> oa, ob; std::vector<int32_t> st;
  for (float &s : im.scales) s = 0.05f;
  core_encode(im, true, 0.05f, 0, a, oa, st, irec_res::SerialLanes{});
  core_encode(im, true, 0.05f, oa[im.N], a, oa, st, irec_res::SerialLanes{});
  core_encode(im, false, 0.0f, 0, b, ob, st, irec_res::SerialLanes{});
  core_encode(im, false, 0.0f, ob[im.N], b, ob, st, irec_res::SerialLanes{});
  const int64_t extra = 4 * ((int64_t)im.c - 1);
  for (int32_t i = 0; i < im.N; ++i) {
    const int64_t na = oa[i + 1] - oa[i], nb = ob[i + 1] - ob[i];
    CHECK(nb == na + extra);
    CHECK(std::memcmp(a.data() + oa[i] + 28, b.data() + ob[i] + 28 + extra, (size_t)(na - 28)) == 0);
    CHECK(std::memcmp(a.data() + oa[i] + 24, b.data() + ob[i] + 24 + extra, 4) == 0);   // the checksum
  }
}

// bits[i][ch][k] by a plain loop
void scale_bits_check(const Images &im, int32_t n_cand, const std::vector<uint32_t> &cost) {
  const int64_t plane = (int64_t)im.h * im.w;
  std::vector<float> scales((size_t)im.c * n_cand);
  for (float &s : scales) s = std::exp(-7.0f + 8.0f * (float)below(1000) / 1000.0f);
  if (n_cand > 1) { scales[1] = 0.0f; scales[(size_t)n_cand * (im.c - 1)] = __builtin_nanf(""); }   // two refused candidates
  std::vector<float> loc(im.loc);
  if (im.n_sym > 3) { loc[2] = __builtin_inff(); loc[(size_t)im.n_sym - 1] = __builtin_nanf(""); }
  std::vector<int64_t> bits((size_t)im.N * im.c * n_cand, -7), skipped((size_t)im.N * im.c, -7), bits2(bits), skipped2(skipped);
  std::vector<int64_t> ws((size_t)(irec_res_fit::workspace_bytes(im.N, im.c, plane, n_cand) / 8));   // exactly the sized bytes
  irec_res_fit::FitCall c{im.pixels.data(), loc.data(), scales.data(), cost.data(), im.N, (int32_t)im.c, n_cand, plane,
                          irec_res_fit::tiles_of(plane), bits.data(), skipped.data(), ws.data()};
  irec_res_fit::scale_bits_host(c, irec_res::SerialLanes{});
  std::vector<int64_t> ws2(ws.size(), -1);
  c.bits = bits2.data(); c.skipped = skipped2.data(); c.part = ws2.data();
  irec_res_fit::scale_bits_host(c, PoolLanes{});
  CHECK(bits == bits2 && skipped == skipped2);
  for (int64_t pair = 0; pair < (int64_t)im.N * im.c; ++pair) {
    const int64_t ch = pair % im.c;
    int64_t skip = 0;
    for (int64_t e = 0; e < plane; ++e) skip += irec_res::is_finite(loc[(size_t)(pair * plane + e)]) ? 0 : 1;
    CHECK(skipped[(size_t)pair] == skip);
    for (int32_t k = 0; k < n_cand; ++k) {
      const float s = scales[(size_t)(ch * n_cand + k)];
      int64_t want = irec_res_fit::NO_BITS;
      if (irec_res::scale_ok(s)) {
        want = 0;
        for (int64_t e = 0; e < plane; ++e) {
          const float l = loc[(size_t)(pair * plane + e)];
          if (!irec_res::is_finite(l)) continue;
          const int32_t m = irec_res::loc_to_m(l), x = im.pixels[(size_t)(pair * plane + e)];
          const uint32_t n = irec_res::cum(m, irec_res::model_inv(s), x + 1) - irec_res::cum(m, irec_res::model_inv(s), x);
          CHECK(n >= 1 && n <= 65536);
          want += cost[n];
        }
      }
      CHECK(bits[(size_t)(pair * n_cand + k)] == want);
    }
  }
}
} // namespace

int main() {
  std::vector<uint8_t> blob, pixels; std::vector<int64_t> off;
  const Images shapes[] = {make(3, 3, 5, 7, 16, 6), make(3, 1, 1, 1, 1, 6), make(3, 4, 2, 2, 1, 6), make(2, 3, 4, 4, 4096, 6),
                           make(2, 3, 80, 81, 64, 10), make(6, 3, 8, 8, 4, 3), make(2, 5, 3, 3, 7, 100)};
  for (const Images &im : shapes) { round_trip(im, blob, off); equal_scales(im); }
  std::printf("version-2 round trips done, failures so far %d\n", g_failures);

  // damage, on the files of 6 x 3 x 8 x 8 at stream_len 4
  const Images &im = shapes[5];
  round_trip(im, blob, off);
  const uint8_t *file = blob.data() + off[1];
  const int64_t n_bytes = off[2] - off[1], head = 24 + 4 * (int64_t)im.c;
  const float *loc = im.loc.data() + im.n_sym;
  for (int64_t cut = 0; cut < n_bytes; ++cut) {
    const int32_t st = core_decode_one(im, false, 0.0f, file, cut, loc, pixels, irec_res::SerialLanes{});
    CHECK(st == (cut < head + 2 * im.ns ? IREC_RES_E_TRUNCATED_HEADER : IREC_RES_E_TRUNCATED_STREAMS));
    CHECK(all_zero(pixels));
  }
  int refused = 0;
  for (int rep = 0; rep < 600; ++rep) {
    std::vector<uint8_t> bad(file, file + n_bytes);
    for (int64_t k = 1 + below(3); k > 0; --k) bad[(size_t)below(n_bytes)] = (uint8_t)below(256);
    const int32_t st = core_decode_one(im, false, 0.0f, bad.data(), n_bytes, loc, pixels, irec_res::SerialLanes{});
    const bool same = std::memcmp(bad.data(), file, (size_t)n_bytes) == 0;
    CHECK(st >= 0 && st <= IREC_RES_E_CHECKSUM);
    if (st) { ++refused; CHECK(all_zero(pixels)); }
    else CHECK(same || std::memcmp(pixels.data(), im.pixels.data() + im.n_sym, (size_t)im.n_sym) == 0);   // (padding bits carry nothing)
  }
  std::printf("600 damaged copies: %d refused\n", refused);
  for (uint32_t ch = 0; ch < im.c; ++ch) {   // one scale word differs
    std::vector<uint8_t> bad(file, file + n_bytes);
    bad[20 + 4 * ch] ^= 1;
    CHECK(core_decode_one(im, false, 0.0f, bad.data(), n_bytes, loc, pixels, irec_res::SerialLanes{}) == IREC_RES_E_SCALE_WORD);
    CHECK(all_zero(pixels));
  }
  {   // the versions do not read each other
    CHECK(core_decode_one(im, true, im.scales[0], file, n_bytes, loc, pixels, irec_res::SerialLanes{}) == IREC_RES_E_MAGIC);
    CHECK(all_zero(pixels));
    std::vector<uint8_t> v1; std::vector<int64_t> o1; std::vector<int32_t> st;
    core_encode(im, true, im.scales[0], 0, v1, o1, st, irec_res::SerialLanes{});
    core_encode(im, true, im.scales[0], o1[im.N], v1, o1, st, irec_res::SerialLanes{});
    CHECK(core_decode_one(im, false, 0.0f, v1.data() + o1[1], o1[2] - o1[1], loc, pixels, irec_res::SerialLanes{}) == IREC_RES_E_MAGIC);
    CHECK(core_decode_one(im, false, 0.0f, v1.data() + o1[1], 30, loc, pixels, irec_res::SerialLanes{}) == IREC_RES_E_MAGIC);   // shorter than a version-2 header
    CHECK(all_zero(pixels));
  }
  {   // another loc under the decoder: the last symbol, so that every stream stays whole
    std::vector<float> moved(loc, loc + im.n_sym);
    moved[(size_t)im.n_sym - 1] += moved[(size_t)im.n_sym - 1] > 0 ? -0.25f : 0.25f;
    const int32_t st = core_decode_one(im, false, 0.0f, file, n_bytes, moved.data(), pixels, PoolLanes{});
    CHECK(st == IREC_RES_E_CHECKSUM);
    CHECK(all_zero(pixels));
  }
  {   // encode statuses: a bad scale in the last channel only; a loc that is not finite
    Images bad = shapes[0];
    std::vector<int32_t> st;
    for (float s : {0.0f, -1.0f, __builtin_nanf(""), __builtin_inff(), 2.9802322387695312e-08f, 33554432.0f}) {
      bad.scales[2] = s;
      core_encode(bad, false, 0.0f, 0, blob, off, st, irec_res::SerialLanes{});
      CHECK(st[0] == IREC_RES_E_SCALE && st[1] == IREC_RES_E_SCALE && st[2] == IREC_RES_E_SCALE && off[3] == 0);
    }
    bad.scales[2] = 0.11f; bad.loc[(size_t)bad.n_sym + 3] = __builtin_nanf("");
    core_encode(bad, false, 0.0f, 4096, blob, off, st, irec_res::SerialLanes{});
    CHECK(st[0] == IREC_RES_OK && st[1] == IREC_RES_E_LOC && st[2] == IREC_RES_OK && off[2] == off[1]);
  }

  // scale_bits against a plain loop: the container's shapes, and two tiles with a ragged second one
  std::vector<uint32_t> cost((size_t)irec_res_fit::COST_ENTRIES, 0);
  for (int64_t n = 1; n < irec_res_fit::COST_ENTRIES; ++n) cost[(size_t)n] = (uint32_t)std::rint((16.0 - std::log2((double)n)) * 65536.0);
  CHECK(cost[1] == (1u << 20) && cost[65536] == 0 && cost[256] == (8u << 16));
  for (const Images &s : shapes) for (int32_t n_cand : {1, 2}) scale_bits_check(s, n_cand, cost);
  const Images tiles = make(2, 3, 67, 71, 64, 20);
  for (int32_t n_cand : {1, 3, 64}) scale_bits_check(tiles, n_cand, cost);
  std::printf("scale_bits against the plain loop done, failures so far %d\n", g_failures);

  if (g_failures) { std::printf("res_scales_check: %d FAILURES\n", g_failures); return 1; }
  std::printf("res_scales_check: all equal\n");
  return 0;
}
