// image_core_check.cpp -- the core of the driver's resize (csrc/irec_image_core.h: the coordinates of an axis, a lane's walk of a tile's
// rows, and the whole-call form that irec_resize_bilinear_host runs) under the host sanitizers.
// A stand-alone program: every line of the core that the kernel runs is compiled here by g++ and runs with AddressSanitizer and
// UndefinedBehaviorSanitizer.  Build and run from the repository root:
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude \
//       -Irelative-entropy-coding_amd/csrc scripts/image_core_check.cpp -o /tmp/image_core_check -lpthread && /tmp/image_core_check
// It walks the shapes of tests/resize_cases.py (65 x 67 -> 64 x 64, 127 x 64 -> 64 x 64, 64 x 64 -> 64 x 64, 130 x 201 -> 128 x 192,
// 191 x 129 -> 128 x 128) and the edges of the range (1 x 1, a shrink to one pixel, by more than 2, to one row), one image and three,
// both layouts, float32 and uint8 sources, serially and on a pool of threads, with source and destination sized EXACTLY, so that one
// element past a row, a plane or an image is a report.  Exit status 0 and the last line "image_core_check: all equal" mean: serial
// and threaded runs the same bits, the staged form of the diagnostic build (a tile's source rectangle copied first) the same bits and
// every copy inside its stage, an image alone the bits it has inside a batch, the planar and the interleaved layout the same
// values, every output the bits of a scalar restatement of the definition written here (which shares no line with the core's walk),
// equal sizes a copy, every tap inside its row, and no sanitizer report (profiles/resize/sanitizer_core.log is this program's output).
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>

#include "irec_image_core.h"

namespace {
namespace I = irec_image;
uint64_t g_state = 0x9E3779B97F4A7C15ull;
uint64_t rnd() { g_state += 0x9E3779B97F4A7C15ull; uint64_t z = g_state; z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; return z ^ (z >> 31); }
int g_failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++g_failures; } } while (0)

struct Serial { template <class F> void operator()(int64_t n, F &&body) const { body((int64_t)0, n); } };
struct PoolBlocks {   // single tiles dealt round-robin to 4 threads: neighbouring tiles on different threads
  template <class F> void operator()(int64_t n, F &&body) const {
    std::vector<std::thread> pool;
    for (int t = 0; t < 4; ++t)
      pool.emplace_back([&body, t, n]() { for (int64_t lo = t; lo < n; lo += 4) body(lo, lo + 1); });
    for (auto &th : pool) th.join();
  }
};

// exactly `bytes` bytes from malloc: the byte after the last is outside the allocation
struct Exact {
  void *p;
  explicit Exact(size_t bytes) : p(std::malloc(bytes ? bytes : 1)) { if (!p) std::abort(); }
  Exact(const Exact &) = delete;
  ~Exact() { std::free(p); }
};

template <class Par>
std::vector<float> run(const void *src, int32_t dtype, int32_t n, int32_t c, int32_t ih, int32_t iw, int32_t oh, int32_t ow, int32_t layout, Par par) {
  CHECK(I::shape_error(n, c, ih, iw, oh, ow, layout, dtype) == nullptr);
  const size_t total = (size_t)n * c * oh * ow;
  Exact dst(total * 4);
  std::memset(dst.p, 0xA5, total * 4);
  I::Call call;
  I::bind(call, src, dtype, n, c, ih, iw, oh, ow, layout, (float *)dst.p);
  I::call_host(call, par);
  return std::vector<float>((float *)dst.p, (float *)dst.p + total);
}

// the staged form of the diagnostic build (phase_stage into a tile's Stage, then lane_walk over it), tile by tile
std::vector<float> run_staged(const void *src, int32_t dtype, int32_t n, int32_t c, int32_t ih, int32_t iw, int32_t oh, int32_t ow, int32_t layout,
                              int64_t *staged_tiles) {
  const size_t total = (size_t)n * c * oh * ow;
  Exact dst(total * 4);
  std::memset(dst.p, 0xA5, total * 4);
  I::Call call;
  I::bind(call, src, dtype, n, c, ih, iw, oh, ow, layout, (float *)dst.p);
  for (int64_t tile = 0; tile < call.tiles(); ++tile) {
    const I::Tile T = I::tile_of(call, tile);
    const I::Span s = I::span_of(call, T);
    if (!s.fits) { for (int32_t lane = 0; lane < I::NT; ++lane) I::lane_of_tile(call, tile, lane); continue; }
    Exact mem(sizeof(I::Stage));                                          // exactly a Stage: one float past it is a report
    I::Stage &m = *(I::Stage *)mem.p;
    for (int32_t tid = 0; tid < I::NT; ++tid) I::phase_stage(call, T, s, m, tid);
    for (int32_t lane = 0; lane < I::NT; ++lane) I::lane_walk(call, T, lane, I::Staged{m, s});
    ++*staged_tiles;
  }
  return std::vector<float>((float *)dst.p, (float *)dst.p + total);
}

// the definition once more, a pixel at a time, from include/irec.h's words
float tap(const void *src, int32_t dtype, size_t at) { return dtype == IREC_IMAGE_U8 ? (float)((const uint8_t *)src)[at] / 255.0f : ((const float *)src)[at]; }
void coords(int32_t o, int32_t in, int32_t out, int32_t *lo, int32_t *hi, float *t) {
  const float scale = (float)in / (float)out;
  const float s = ((float)o + 0.5f) * scale - 0.5f;
  *lo = (int32_t)std::fmax(std::floor(s), 0.0f);
  *hi = (int32_t)std::fmin(std::ceil(s), (float)(in - 1));
  *t = s - std::floor(s);
  CHECK(*lo >= 0 && *lo <= *hi && *hi <= in - 1);
}
float restated(const void *src, int32_t dtype, int32_t c, int32_t ih, int32_t iw, int32_t oh, int32_t ow, int32_t layout, int32_t i, int32_t ch, int32_t y,
               int32_t x) {
  auto at = [&](int32_t yy, int32_t xx) {
    return layout == IREC_IMAGE_NHWC ? (((size_t)i * ih + yy) * iw + xx) * c + ch : (((size_t)i * c + ch) * ih + yy) * iw + xx;
  };
  int32_t ylo = y, yhi = y, xlo = x, xhi = x;
  float ty = 0.0f, tx = 0.0f;
  if (ih != oh) coords(y, ih, oh, &ylo, &yhi, &ty);
  if (iw != ow) coords(x, iw, ow, &xlo, &xhi, &tx);
  const float tl = tap(src, dtype, at(ylo, xlo)), tr = tap(src, dtype, at(ylo, xhi)), bl = tap(src, dtype, at(yhi, xlo)), br = tap(src, dtype, at(yhi, xhi));
  const float top = iw == ow ? tl : tl + (tr - tl) * tx, bot = iw == ow ? bl : bl + (br - bl) * tx;
  return ih == oh ? top : top + (bot - top) * ty;
}

bool same_bits(const float *a, const float *b, size_t n) { return std::memcmp(a, b, n * 4) == 0; }

void check_shape(int32_t ih, int32_t iw, int32_t oh, int32_t ow) {
  const int32_t c = 3;
  for (int32_t dtype : {IREC_IMAGE_F32, IREC_IMAGE_U8}) {
    for (int32_t n : {1, 3}) {
      const size_t in_total = (size_t)n * c * ih * iw, item = dtype == IREC_IMAGE_U8 ? 1 : 4, out_image = (size_t)c * oh * ow;
      // the planar source, and the same images interleaved
      Exact planar(in_total * item), inter(in_total * item);
      for (size_t e = 0; e < in_total; ++e) {
        if (dtype == IREC_IMAGE_U8) ((uint8_t *)planar.p)[e] = (uint8_t)(rnd() >> 56);
        else ((float *)planar.p)[e] = (float)((double)(rnd() >> 11) / 9007199254740992.0 - 0.5);
      }
      for (int32_t i = 0; i < n; ++i)
        for (int32_t ch = 0; ch < c; ++ch)
          for (int32_t y = 0; y < ih; ++y)
            for (int32_t x = 0; x < iw; ++x)
              std::memcpy((char *)inter.p + ((((size_t)i * ih + y) * iw + x) * c + ch) * item,
                          (char *)planar.p + ((((size_t)i * c + ch) * ih + y) * iw + x) * item, item);
      const std::vector<float> p = run(planar.p, dtype, n, c, ih, iw, oh, ow, IREC_IMAGE_NCHW, Serial{});
      const std::vector<float> q = run(inter.p, dtype, n, c, ih, iw, oh, ow, IREC_IMAGE_NHWC, Serial{});
      CHECK(same_bits(p.data(), run(planar.p, dtype, n, c, ih, iw, oh, ow, IREC_IMAGE_NCHW, PoolBlocks{}).data(), p.size()));
      CHECK(same_bits(q.data(), run(inter.p, dtype, n, c, ih, iw, oh, ow, IREC_IMAGE_NHWC, PoolBlocks{}).data(), q.size()));
      int64_t staged = 0;
      CHECK(same_bits(p.data(), run_staged(planar.p, dtype, n, c, ih, iw, oh, ow, IREC_IMAGE_NCHW, &staged).data(), p.size()));
      CHECK(same_bits(q.data(), run_staged(inter.p, dtype, n, c, ih, iw, oh, ow, IREC_IMAGE_NHWC, &staged).data(), q.size()));
      CHECK(staged > 0 || ih >= 2 * oh || iw >= 2 * ow);                          // a shrink by less than 2 always fits its stage
      size_t differ = 0;
      for (int32_t i = 0; i < n; ++i)
        for (int32_t ch = 0; ch < c; ++ch)
          for (int32_t y = 0; y < oh; ++y)
            for (int32_t x = 0; x < ow; ++x) {
              const float a = p[(((size_t)i * c + ch) * oh + y) * ow + x], b = q[(((size_t)i * oh + y) * ow + x) * c + ch];
              const float want = restated(planar.p, dtype, c, ih, iw, oh, ow, IREC_IMAGE_NCHW, i, ch, y, x);
              differ += !same_bits(&a, &b, 1) || !same_bits(&a, &want, 1);
              if (ih == oh && iw == ow) {
                const float v = tap(planar.p, dtype, (((size_t)i * c + ch) * ih + y) * iw + x);
                differ += !same_bits(&a, &v, 1);
              }
            }
      CHECK(differ == 0);
      for (int32_t i = 0; i < n && n > 1; ++i) {                                                    // an image alone
        const std::vector<float> alone = run((char *)planar.p + (size_t)i * c * ih * iw * item, dtype, 1, c, ih, iw, oh, ow, IREC_IMAGE_NCHW, Serial{});
        CHECK(same_bits(alone.data(), p.data() + i * out_image, out_image));
        const std::vector<float> alone_q = run((char *)inter.p + (size_t)i * c * ih * iw * item, dtype, 1, c, ih, iw, oh, ow, IREC_IMAGE_NHWC, PoolBlocks{});
        CHECK(same_bits(alone_q.data(), q.data() + i * out_image, out_image));
      }
      std::printf("%d x %d -> %d x %d, %d image(s), %s: planar, interleaved, threaded, staged, alone and restated equal\n", ih, iw, oh, ow, n,
                  dtype == IREC_IMAGE_U8 ? "uint8" : "float32");
    }
  }
}

void check_non_finite() {
  const int32_t ih = 65, iw = 67, oh = 64, ow = 64;
  std::vector<float> src((size_t)ih * iw, 0.25f);
  src[20 * iw + 30] = NAN;
  src[40 * iw + 11] = INFINITY;
  const std::vector<float> out = run(src.data(), IREC_IMAGE_F32, 1, 1, ih, iw, oh, ow, IREC_IMAGE_NCHW, Serial{});
  int bad = 0;
  for (int32_t y = 0; y < oh; ++y)
    for (int32_t x = 0; x < ow; ++x) {
      int32_t ylo, yhi, xlo, xhi; float ty, tx;
      coords(y, ih, oh, &ylo, &yhi, &ty);
      coords(x, iw, ow, &xlo, &xhi, &tx);
      bool hit = false;
      for (int32_t yy : {ylo, yhi}) for (int32_t xx : {xlo, xhi}) hit = hit || !std::isfinite(src[(size_t)yy * iw + xx]);
      const float v = out[(size_t)y * ow + x];
      CHECK(hit ? !std::isfinite(v) : v == 0.25f);
      bad += hit;
    }
  CHECK(bad >= 2 && bad <= 18);
  // equal sizes: the bits pass through, -0 and non-finite values included
  src[50 * iw + 50] = -0.0f;
  const std::vector<float> copy = run(src.data(), IREC_IMAGE_F32, 1, 1, ih, iw, ih, iw, IREC_IMAGE_NCHW, PoolBlocks{});
  CHECK(same_bits(copy.data(), src.data(), src.size()));
  std::printf("non-finite taps: %d outputs reached, every other output clean; equal sizes pass -0, inf and NaN through\n", bad);
}

void check_refusals() {
  CHECK(I::shape_error(0, 3, 8, 8, 8, 8, 0, 0) && I::shape_error(1, 0, 8, 8, 8, 8, 0, 0) && I::shape_error(1, 3, 0, 8, 8, 8, 0, 0));
  CHECK(I::shape_error(1, 3, 8, 8, 9, 8, 0, 0) && I::shape_error(1, 3, 8, 8, 8, 9, 0, 0) && I::shape_error(1, 3, 8, 8, 0, 8, 0, 0));
  CHECK(I::shape_error(1, 3, 8, 8, 8, 8, 2, 0) && I::shape_error(1, 3, 8, 8, 8, 8, 0, 2) && I::shape_error(1, 3, 65537, 8, 8, 8, 0, 0));
  CHECK(I::shape_error(1, 40000, 8, 65536, 8, 8, IREC_IMAGE_NHWC, 0));                             // a row past 2^31 - 1 elements
  CHECK(I::shape_error(INT32_MAX, 3, 64, 64, 64, 64, 0, 0));                                       // tiles past 2^31 - 1
  CHECK(!I::shape_error(1, 3, 65536, 65536, 1, 1, 0, 1));
  // the largest sides: every tap of every position inside its row, whatever s rounds to
  for (int32_t out : {1, 2, 3, 32767, 32768, 65535}) {
    const float scale = (float)65536 / (float)out;
    for (int32_t o = 0; o < out; ++o) {
      const I::Axis a = I::axis_of(o, 65536, out, scale);
      if (!(a.lo >= 0 && a.lo <= a.hi && a.hi <= 65535 && a.t >= 0.0f && a.t < 1.0f)) { CHECK(!"a tap outside its row"); break; }
    }
  }
  std::printf("refusals and the largest sides: every tap inside its row\n");
}
} // namespace

int main() {
  const int32_t shapes[][4] = {{65, 67, 64, 64}, {127, 64, 64, 64}, {64, 64, 64, 64}, {130, 201, 128, 192}, {191, 129, 128, 128},
                               {1, 1, 1, 1}, {5, 7, 1, 1}, {200, 150, 64, 64}, {17, 300, 1, 130}, {33, 2, 32, 1}};
  for (const auto &s : shapes) check_shape(s[0], s[1], s[2], s[3]);
  check_non_finite();
  check_refusals();
  if (g_failures) { std::printf("image_core_check: %d FAILED\n", g_failures); return 1; }
  std::printf("image_core_check: all equal\n");
  return 0;
}
