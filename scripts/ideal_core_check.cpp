// ideal_core_check.cpp -- the core of the ideal half of a results row (csrc/irec_ideal_core.h: the seeded noise, the draw with its KL,
// the likelihood term, a lane's runs, the ordered sums and the whole-call forms that irec_posterior_draw_host / irec_loglik_host run)
// under the host sanitizers.
// A stand-alone program: every line of the core that the kernels run is compiled here by g++ and runs with AddressSanitizer and
// UndefinedBehaviorSanitizer.  Build and run from the repository root:
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude \
//       -Irelative-entropy-coding_amd/csrc scripts/ideal_core_check.cpp -o /tmp/ideal_core_check -lpthread && /tmp/ideal_core_check
// It walks every tile-edge shape (dims 1, 3, 4, 5, 255, 256, 257, 1023, 1025, 4095, 4096, 4097, 8193; one image and three), serially
// and on a pool of threads, with every buffer sized EXACTLY -- the arrays, the outputs and the workspace at the bytes the sizing
// reports -- so that one element past a range is a report; once with every float32 array on a 16-byte boundary (the 16-byte runs
// where dims allows) and once 4 bytes past one.  Exit status 0 and the last line "ideal_core_check: all equal" mean: serial and
// threaded runs the same bits, aligned and misaligned placements the same bits, an image alone the bits it has inside a batch, kl and
// ll within n 2^-53 sum |term| of a long double sum of the same terms and within 1e-12 relative of libm's formulas, a NaN image
// changing no other image, |eps| < 5.5 with the moments of a standard normal, and no sanitizer report
// (profiles/ideal/sanitizer_core.log is this program's output).
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>

#include "irec_ideal_core.h"

namespace {
namespace I = irec_ideal;
uint64_t g_state = 0x9E3779B97F4A7C15ull;
uint64_t rnd() { g_state += 0x9E3779B97F4A7C15ull; uint64_t z = g_state; z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; return z ^ (z >> 31); }
double uniform() { return (double)(rnd() >> 11) / 9007199254740992.0; }
double normal() { return std::sqrt(-2.0 * std::log(uniform() + 1e-300)) * std::cos(6.283185307179586 * uniform()); }
int g_failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++g_failures; } } while (0)

struct PoolBlocks {   // single tiles dealt round-robin to 4 threads: neighbouring tiles on different threads
  template <class F> void operator()(int64_t n, F &&body) const {
    std::vector<std::thread> pool;
    for (int t = 0; t < 4; ++t)
      pool.emplace_back([&body, t, n]() { for (int64_t lo = t; lo < n; lo += 4) body(lo, lo + 1); });
    for (auto &th : pool) th.join();
  }
};

// exactly n floats whose first lies `shift` floats past a 16-byte boundary: the byte after the last is outside the allocation
struct Placed {
  void *raw = nullptr; float *p;
  Placed(size_t n, int shift) {
    if (posix_memalign(&raw, 16, (n + shift) * 4)) std::abort();
    p = (float *)raw + shift;
  }
  Placed(const Placed &) = delete;
  ~Placed() { std::free(raw); }
};

struct Draw { std::vector<float> sample; std::vector<double> kl; };
template <class Par>
Draw draw(const std::vector<float> st[4], int32_t n, int64_t dims, int64_t seed, uint32_t tag, int64_t base, int shift, Par par) {
  const size_t total = (size_t)n * dims;
  Draw r{std::vector<float>(total), std::vector<double>((size_t)n, -7.0)};
  std::vector<double> ws(irec_ideal::tiles_of(dims) * n);                     // exactly the sized doubles
  CHECK(I::shape_error(n, dims) == nullptr);
  I::DrawCall c;
  {
    Placed a(total, shift), b(total, shift), cc(total, shift), d(total, shift), out(total, shift);
    float *arr[4] = {a.p, b.p, cc.p, d.p};
    for (int k = 0; k < 4; ++k) std::memcpy(arr[k], st[k].data(), total * 4);
    CHECK(I::draw_error(a.p, b.p, cc.p, d.p, n, dims, base, out.p, r.kl.data()) == nullptr);
    I::bind(c, a.p, b.p, cc.p, d.p, n, dims, seed, tag, base, out.p, r.kl.data(), ws.data());
    CHECK(c.vec == (shift == 0 && dims % 4 == 0));
    I::draw_host(c, par);
    std::memcpy(r.sample.data(), out.p, total * 4);
  }
  return r;
}
bool same(const Draw &u, const Draw &v) {
  return u.sample.size() == v.sample.size() && std::memcmp(u.sample.data(), v.sample.data(), u.sample.size() * 4) == 0 &&
         std::memcmp(u.kl.data(), v.kl.data(), u.kl.size() * 8) == 0;
}

template <class Par>
std::vector<double> loglik(const std::vector<float> &x, const std::vector<float> &loc, const std::vector<float> &ls, int32_t n, int32_t ch,
                           int64_t plane, int shift, Par par) {
  const size_t total = (size_t)n * ch * plane;
  std::vector<double> ll((size_t)n, -7.0), ws(I::tiles_of(ch * plane) * n);
  Placed scales(ls.size(), 0);
  std::memcpy(scales.p, ls.data(), ls.size() * 4);
  I::LoglikCall c;
  {
    Placed a(total, shift), b(total, shift);
    std::memcpy(a.p, x.data(), total * 4); std::memcpy(b.p, loc.data(), total * 4);
    CHECK(I::loglik_error(a.p, b.p, scales.p, (int64_t)ls.size(), n, ch, plane, 1.0 / 256.0, ll.data()) == nullptr);
    I::bind(c, a.p, b.p, scales.p, (int32_t)ls.size(), n, ch, plane, 1.0 / 256.0, ll.data(), ws.data());
    CHECK(c.vec == (shift == 0 && (ch * plane) % 4 == 0));
    I::loglik_host(c, par);
  }
  return ll;
}

void draw_shape(int32_t n, int64_t dims) {
  const size_t total = (size_t)n * dims;
  std::vector<float> st[4];
  for (auto &v : st) v.resize(total);
  for (size_t e = 0; e < total; ++e) {
    st[2][e] = (float)normal(); st[3][e] = (float)std::exp(0.5 * normal());
    st[0][e] = st[2][e] + st[3][e] * (float)(0.7 * normal()); st[1][e] = st[3][e] * (float)std::exp(-0.5 + 0.5 * normal());
  }
  const int64_t seed = -1234567890123ll, base = 4294967296ll - n;                // (the last image numbers)
  const uint32_t tag = 23;
  const Draw serial = draw(st, n, dims, seed, tag, base, 0, I::SerialBlocks{});
  CHECK(same(serial, draw(st, n, dims, seed, tag, base, 0, PoolBlocks{})));
  CHECK(same(serial, draw(st, n, dims, seed, tag, base, 1, PoolBlocks{})));      // 4 bytes past a 16-byte boundary
  double worst_bound = 0, worst_libm = 0;
  for (int32_t i = 0; i < n; ++i) {
    long double sum = 0, mag = 0, libm = 0;
    for (int64_t e = 0; e < dims; ++e) {
      const size_t at = (size_t)i * dims + e;
      const double term = I::kl_dim(st[0][at], st[1][at], st[2][at], st[3][at]);
      sum += term; mag += std::fabs(term);
      const double t = (double)st[1][at] / (double)st[3][at], dm = ((double)st[0][at] - (double)st[2][at]) / (double)st[3][at];
      libm += 0.5 * dm * dm + 0.5 * (t * t - 1.0) - std::log(t);
      uint32_t w[4];
      I::philox_block(I::stream_of(seed, tag, base + i), (uint64_t)e >> 2, w);
      const float eps = I::eps_of(w[e & 3]);
      CHECK(std::fabs(eps) < 5.5f && serial.sample[at] == st[0][at] + st[1][at] * eps);
    }
    const double bound = (double)dims * std::ldexp(1.0, -53) * (double)mag + std::ldexp(std::fabs((double)sum), -60);   // (+ the long double sum's own error)
    CHECK(std::fabs(serial.kl[i] - (double)sum) <= bound);
    worst_bound = std::fmax(worst_bound, std::fabs(serial.kl[i] - (double)sum) / bound);
    worst_libm = std::fmax(worst_libm, std::fabs(serial.kl[i] - (double)libm) / std::fabs((double)libm));
    // the image alone: the bits it has in the batch
    std::vector<float> one[4];
    for (int k = 0; k < 4; ++k) one[k].assign(st[k].begin() + i * dims, st[k].begin() + (i + 1) * dims);
    const Draw alone = draw(one, 1, dims, seed, tag, base + i, 0, I::SerialBlocks{});
    CHECK(std::memcmp(alone.sample.data(), serial.sample.data() + (size_t)i * dims, dims * 4) == 0 && alone.kl[0] == serial.kl[i]);
  }
  CHECK(worst_libm < 1e-12);
  if (n == 3) {                                                                  // a NaN in image 1: images 0 and 2 keep their bits
    std::vector<float> bad[4] = {st[0], st[1], st[2], st[3]};
    bad[3][(size_t)dims + dims - 1] = std::nanf("");
    const Draw dirty = draw(bad, n, dims, seed, tag, base, 0, PoolBlocks{});
    CHECK(std::isnan(dirty.kl[1]) && dirty.kl[0] == serial.kl[0] && dirty.kl[2] == serial.kl[2]);
    CHECK(std::memcmp(dirty.sample.data(), serial.sample.data(), total * 4) == 0);
  }
  std::printf("draw %d x %lld: kl within %.3f of the summation bound, %.3e relative of libm\n", n, (long long)dims, worst_bound, worst_libm);
}

void loglik_shape(int32_t n, int32_t ch, int64_t plane, int n_scales) {
  const size_t total = (size_t)n * ch * plane;
  std::vector<float> x(total), loc(total), ls((size_t)n_scales);
  for (size_t e = 0; e < total; ++e) {
    x[e] = (float)((double)(rnd() % 256) / 256.0 - 0.5 + (rnd() % 10 == 0 ? uniform() / 300.0 : 0.0));
    const double v = (double)x[e] + 0.03 * normal();
    loc[e] = (float)(v < -0.498046875 ? -0.498046875 : (v > 0.498046875 ? 0.498046875 : v));
  }
  for (float &v : ls) v = (float)(-4.0 + uniform());
  const std::vector<double> serial = loglik(x, loc, ls, n, ch, plane, 0, I::SerialBlocks{});
  for (int shift : {0, 1}) {
    const std::vector<double> other = loglik(x, loc, ls, n, ch, plane, shift, PoolBlocks{});
    CHECK(std::memcmp(other.data(), serial.data(), serial.size() * 8) == 0);
  }
  double worst_bound = 0, worst_libm = 0;
  for (int32_t i = 0; i < n; ++i) {
    long double sum = 0, mag = 0, libm = 0;
    for (int64_t e = 0; e < ch * plane; ++e) {
      const size_t at = (size_t)i * ch * plane + e;
      const double log_scale = (double)ls[n_scales == 1 ? 0 : (size_t)(e / plane)], scale = I::det_exp(log_scale);
      const double term = I::loglik_term(x[at], loc[at], scale, (1.0 / 256.0) / scale, 1.0 / 256.0);
      sum += term; mag += std::fabs(term);
      const double s = std::exp(log_scale), a = (std::floor((double)x[at] * 256.0) / 256.0 - (double)loc[at]) / s, b = a + 1.0 / 256.0 / s;
      libm += std::log(1.0 / (1.0 + std::exp(-b)) - 1.0 / (1.0 + std::exp(-a)) + 1e-7);
    }
    const double bound = (double)(ch * plane) * std::ldexp(1.0, -53) * (double)mag + std::ldexp(std::fabs((double)sum), -60);
    CHECK(std::fabs(serial[i] - (double)sum) <= bound);
    worst_bound = std::fmax(worst_bound, std::fabs(serial[i] - (double)sum) / bound);
    worst_libm = std::fmax(worst_libm, std::fabs(serial[i] - (double)libm) / std::fabs((double)libm));
    const std::vector<float> x1(x.begin() + i * ch * plane, x.begin() + (i + 1) * ch * plane), l1(loc.begin() + i * ch * plane, loc.begin() + (i + 1) * ch * plane);
    CHECK(loglik(x1, l1, ls, 1, ch, plane, 0, I::SerialBlocks{})[0] == serial[i]);
  }
  CHECK(worst_libm < 1e-12);
  if (n == 3) {
    std::vector<float> bad = loc;
    bad[(size_t)ch * plane] = std::nanf("");
    const std::vector<double> dirty = loglik(x, bad, ls, n, ch, plane, 0, PoolBlocks{});
    CHECK(std::isnan(dirty[1]) && dirty[0] == serial[0] && dirty[2] == serial[2]);
  }
  std::printf("loglik %d x %d x %lld, %d scale(s): ll within %.3f of the summation bound, %.3e relative of libm\n", n, ch, (long long)plane, n_scales,
              worst_bound, worst_libm);
}

void noise() {
  // antisymmetry about 1/2, the extremes, and the moments of 2^20 draws of one stream
  for (uint32_t k : {0u, 1u, 12345u, (1u << 23) - 1u}) {
    const uint32_t lo = k << 8, hi = ((1u << 24) - 1u - k) << 8;
    CHECK(I::ndtri64(I::unit_of(lo)) == -I::ndtri64(I::unit_of(hi)));
  }
  CHECK(I::eps_of(0u) < -5.4f && I::eps_of(0u) > -5.5f && I::eps_of(0xFFFFFFFFu) == -I::eps_of(0u));
  CHECK(std::fabs(I::ndtri64(0.975) - 1.959963984540054) < 1e-14 && std::fabs(I::ndtri64(1e-6) + 4.753424308822899) < 1e-13);
  const int64_t n = 1 << 20;
  double sum = 0, sq = 0;
  const I::Stream st = I::stream_of(1234, 0, 0);
  for (int64_t b = 0; b < n / 4; ++b) {
    uint32_t w[4];
    I::philox_block(st, (uint64_t)b, w);
    for (uint32_t v : w) { const double e = (double)I::eps_of(v); sum += e; sq += e * e; }
  }
  const double mean = sum / n, var = sq / n - mean * mean;
  CHECK(std::fabs(mean) <= 5.0 / std::sqrt((double)n) && std::fabs(var - 1.0) <= 5.0 * std::sqrt(2.0 / n));
  std::printf("noise: mean %.3e, variance - 1 %.3e over 2^20 draws\n", mean, var - 1.0);
}
} // namespace

int main() {
  noise();
  for (int64_t dims : {1, 3, 4, 5, 255, 256, 257, 1023, 1025, 4095, 4096, 4097, 8193})
    for (int32_t n : {1, 3}) {
      draw_shape(n, dims);
      loglik_shape(n, 1, dims, 1);
    }
  loglik_shape(2, 3, 35, 3); loglik_shape(1, 3, 1366, 3); loglik_shape(3, 3, 2731, 3); loglik_shape(2, 3, 1024, 1);
  // argument errors of the core
  float f[8]; double d[2];
  CHECK(I::shape_error(0, 5) != nullptr && I::shape_error(1, 0) != nullptr && I::shape_error(1, ((int64_t)1 << 40) + 1) != nullptr);
  CHECK(I::draw_error(f, f, f, f, 1, 4, -1, f, d) != nullptr && I::draw_error(f, f, f, f, 1, 4, (int64_t)1 << 32, f, d) != nullptr);
  CHECK(I::draw_error(nullptr, f, f, f, 1, 4, 0, f, d) != nullptr && I::draw_error((float *)((char *)f + 2), f, f, f, 1, 4, 0, f, d) != nullptr);
  CHECK(I::loglik_error(f, f, f, 2, 1, 3, 2, 1.0 / 256.0, d) != nullptr && I::loglik_error(f, f, f, 1, 1, 3, 2, 0.0, d) != nullptr);
  CHECK(I::loglik_error(f, f, f, 1, 1, 3, 2, 1.0 / 256.0, d) == nullptr);
  if (g_failures) { std::printf("ideal_core_check: %d FAILURES\n", g_failures); return 1; }
  std::printf("ideal_core_check: all equal\n");
  return 0;
}
