// quality_core_check.cpp -- the quality metrics' core (csrc/irec_quality_core.h: the pixel arithmetic, the phases of a tile, the ordered
// sums and the whole-call form that the host entry point irec_quality_host runs) under the host sanitizers.
// A stand-alone program: every line of the core that the kernels run is compiled here by g++ and runs with AddressSanitizer and
// UndefinedBehaviorSanitizer.  Build and run from the repository root:
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude \
//       -Irelative-entropy-coding_amd/csrc scripts/quality_core_check.cpp -o /tmp/quality_core_check -lpthread && /tmp/quality_core_check
// It walks a set of shapes (the minimal 11 x 11, odd sizes at every scale, sizes one below, at and one above a tile and its halo, one
// to five scales, one and several images and channels), serially and on a pool of threads, with every buffer sized EXACTLY -- both
// images, both outputs and the workspace at the bytes the sizing reports -- so that one element past a range is a report.  Exit status
// 0 and the last line "quality_core_check: all equal" mean: serial and threaded runs the same bits, identical images exactly 1, the
// values within 1e-4 of a float64 direct restatement, an image alone the bits it has inside a batch, and no sanitizer report
// (profiles/quality/sanitizer_core.log is this program's output).
#include <cmath>
#include <cstdio>
#include <cstring>
#include <thread>
#include <vector>

#include "irec_quality_core.h"

namespace {
namespace Q = irec_quality;
uint64_t g_state = 0x9E3779B97F4A7C15ull;
uint64_t rnd() { g_state += 0x9E3779B97F4A7C15ull; uint64_t z = g_state; z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; return z ^ (z >> 31); }
double uniform() { return (double)(rnd() >> 11) / 9007199254740992.0; }
int g_failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++g_failures; } } while (0)

struct PoolBlocks {   // chunks of 3 blocks over 4 threads: neighbouring tiles on different threads
  template <class F> void operator()(int64_t n, F &&body) const {
    std::vector<std::thread> pool;
    for (int t = 0; t < 4; ++t)
      pool.emplace_back([&body, t, n]() { for (int64_t lo = 3 * t; lo < n; lo += 12) body(lo, lo + 3 < n ? lo + 3 : n); });
    for (auto &th : pool) th.join();
  }
};

const irec_quality_params PARAMS = {255.0f, 0.0f, 255.0f, 0.0f, 1, 0, 255.0f, 0.01f, 0.03f};

struct Result { std::vector<float> per_scale, sse; };
template <class Par>
Result run(const std::vector<float> &a, const std::vector<float> &b, int32_t N, int32_t C, int32_t H, int32_t W, int32_t S, Par par) {
  CHECK(Q::shape_error(N, C, H, W, S, &PARAMS) == nullptr);
  int64_t doubles = 0, floats = 0;
  Q::workspace_sizes((int64_t)N * C, H, W, S, &doubles, &floats);
  std::vector<double> ws((size_t)(doubles + (floats + 1) / 2));          // exactly the sized bytes, rounded up to a double
  Result r{std::vector<float>((size_t)N * C * S * 2, -7.0f), std::vector<float>((size_t)N, -7.0f)};
  Q::Call c;
  Q::bind(c, a.data(), b.data(), N, C, H, W, S, &PARAMS, r.per_scale.data(), r.sse.data(), ws.data());
  Q::call_host(c, par);
  return r;
}

// float64, direct 121 taps, uncentred: per (plane, scale) the two means
std::vector<double> direct(const std::vector<float> &a, const std::vector<float> &b, int32_t planes, int32_t H, int32_t W, int32_t S) {
  double g[11], sum = 0;
  for (int i = 0; i < 11; ++i) { g[i] = std::exp(-(i - 5) * (i - 5) / 4.5); sum += g[i]; }
  for (double &v : g) v /= sum;
  const double c1 = 2.55 * 2.55, c2 = 7.65 * 7.65;
  std::vector<double> out((size_t)planes * S * 2);
  for (int32_t p = 0; p < planes; ++p) {
    int32_t h = H, w = W;
    std::vector<double> x((size_t)h * w), y((size_t)h * w);
    for (int64_t e = 0; e < (int64_t)h * w; ++e) {
      double va = (double)a[(size_t)p * H * W + e] * 255.0;
      x[e] = va < 0 ? 0 : (va > 255 ? 255 : va);
      y[e] = (double)b[(size_t)p * H * W + e] * 255.0;
    }
    for (int32_t k = 0; k < S; ++k) {
      if (k) {
        const int32_t h2 = (h + 1) / 2, w2 = (w + 1) / 2;
        std::vector<double> nx((size_t)h2 * w2), ny((size_t)h2 * w2);
        for (int32_t i = 0; i < h2; ++i)
          for (int32_t j = 0; j < w2; ++j) {
            const int32_t i1 = 2 * i + 1 < h ? 2 * i + 1 : 2 * i, j1 = 2 * j + 1 < w ? 2 * j + 1 : 2 * j;
            nx[(size_t)i * w2 + j] = 0.25 * (x[(size_t)2 * i * w + 2 * j] + x[(size_t)2 * i * w + j1] + x[(size_t)i1 * w + 2 * j] + x[(size_t)i1 * w + j1]);
            ny[(size_t)i * w2 + j] = 0.25 * (y[(size_t)2 * i * w + 2 * j] + y[(size_t)2 * i * w + j1] + y[(size_t)i1 * w + 2 * j] + y[(size_t)i1 * w + j1]);
          }
        x.swap(nx); y.swap(ny); h = h2; w = w2;
      }
      double s_ssim = 0, s_cs = 0;
      for (int32_t oy = 0; oy < h - 10; ++oy)
        for (int32_t ox = 0; ox < w - 10; ++ox) {
          double m0 = 0, m1 = 0, xy = 0, sq = 0;
          for (int i = 0; i < 11; ++i)
            for (int j = 0; j < 11; ++j) {
              const double wt = g[i] * g[j], xv = x[(size_t)(oy + i) * w + ox + j], yv = y[(size_t)(oy + i) * w + ox + j];
              m0 += wt * xv; m1 += wt * yv; xy += wt * xv * yv; sq += wt * (xv * xv + yv * yv);
            }
          const double lum = (2 * m0 * m1 + c1) / (m0 * m0 + m1 * m1 + c1), cs = (2 * xy - 2 * m0 * m1 + c2) / (sq - m0 * m0 - m1 * m1 + c2);
          s_ssim += lum * cs; s_cs += cs;
        }
      const double n_out = (double)(h - 10) * (w - 10);
      out[((size_t)p * S + k) * 2] = s_ssim / n_out; out[((size_t)p * S + k) * 2 + 1] = s_cs / n_out;
    }
  }
  return out;
}

bool same_bits(const std::vector<float> &u, const std::vector<float> &v) {
  return u.size() == v.size() && std::memcmp(u.data(), v.data(), u.size() * sizeof(float)) == 0;
}

void shape(int32_t N, int32_t C, int32_t H, int32_t W, int32_t S) {
  const size_t n = (size_t)N * C * H * W;
  std::vector<float> a(n), b(n);
  for (size_t e = 0; e < n; ++e) {
    b[e] = (float)(0.5 + 0.3 * std::sin(0.11 * (double)(e % (size_t)W) + 0.07 * (double)(e / (size_t)W)) + 0.2 * (uniform() - 0.5));
    a[e] = b[e] + (float)(0.1 * (uniform() - 0.5)) + (e % 97 == 0 ? 0.6f : 0.0f) - (e % 89 == 0 ? 0.6f : 0.0f);   // (some beyond both ends of the clamp)
  }
  const Result serial = run(a, b, N, C, H, W, S, Q::SerialBlocks{}), pooled = run(a, b, N, C, H, W, S, PoolBlocks{});
  CHECK(same_bits(serial.per_scale, pooled.per_scale) && same_bits(serial.sse, pooled.sse));
  const std::vector<double> want = direct(a, b, N * C, H, W, S);
  double worst = 0;
  for (size_t i = 0; i < want.size(); ++i) { const double d = std::fabs((double)serial.per_scale[i] - want[i]); worst = d > worst ? d : worst; }
  CHECK(worst < 1e-4);
  for (int32_t i = 0; i < N; ++i) {
    double sse = 0;
    for (size_t e = (size_t)i * C * H * W; e < (size_t)(i + 1) * C * H * W; ++e) {
      double va = (double)a[e] * 255.0; va = va < 0 ? 0 : (va > 255 ? 255 : va);
      sse += (va - (double)b[e] * 255.0) * (va - (double)b[e] * 255.0);
    }
    CHECK(std::fabs((double)serial.sse[i] - sse) <= 1e-5 * sse);
  }
  // identical images (clipped alike: b is inside the range): exactly 1, sse exactly 0
  const Result same = run(b, b, N, C, H, W, S, PoolBlocks{});
  for (float v : same.per_scale) CHECK(v == 1.0f);
  for (float v : same.sse) CHECK(v == 0.0f);
  // the last image alone: the bits it has in the batch
  if (N > 1) {
    const size_t per = (size_t)C * H * W;
    const std::vector<float> a1(a.end() - per, a.end()), b1(b.end() - per, b.end());
    const Result alone = run(a1, b1, 1, C, H, W, S, Q::SerialBlocks{});
    CHECK(std::memcmp(alone.per_scale.data(), serial.per_scale.data() + (size_t)(N - 1) * C * S * 2, (size_t)C * S * 2 * sizeof(float)) == 0);
    CHECK(std::memcmp(alone.sse.data(), serial.sse.data() + (N - 1), sizeof(float)) == 0);
  }
  std::printf("%d x %d x %d x %d, %d scales: worst per-scale error against float64 direct %.3e\n", N, C, H, W, S, worst);
}
} // namespace

int main() {
  shape(1, 3, 11, 11, 1);                                   // the minimal image
  shape(2, 1, 11, 12, 1);
  shape(1, 1, 21, 21, 2);                                   // minimal for two scales, odd
  shape(1, 1, 31, 33, 2); shape(1, 1, 32, 32, 2); shape(1, 2, 33, 31, 2);   // around a tile
  shape(1, 1, 41, 43, 2); shape(1, 1, 42, 42, 2); shape(2, 1, 43, 41, 2);   // around a tile and its halo
  shape(1, 1, 75, 139, 3);
  shape(2, 3, 161, 163, 5);                                 // minimal for five scales: 161 -> 81 -> 41 -> 21 -> 11
  shape(3, 2, 177, 191, 5);                                 // odd at every scale but the last
  // argument errors of the core
  CHECK(Q::shape_error(1, 1, 160, 176, 5, &PARAMS) != nullptr && Q::shape_error(1, 1, 10, 11, 1, &PARAMS) != nullptr);
  CHECK(Q::shape_error(1, 1, 11, 11, 0, &PARAMS) != nullptr && Q::shape_error(1, 1, 11, 11, 6, &PARAMS) != nullptr);
  irec_quality_params bad = PARAMS; bad.max_val = 0.0f;
  CHECK(Q::shape_error(1, 1, 11, 11, 1, &bad) != nullptr && Q::shape_error(1, 1, 11, 11, 1, nullptr) != nullptr);
  if (g_failures) { std::printf("quality_core_check: %d FAILURES\n", g_failures); return 1; }
  std::printf("quality_core_check: all equal\n");
  return 0;
}
