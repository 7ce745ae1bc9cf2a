// irec_ideal_core.h -- the ideal half of a results row (include/irec.h: irec_posterior_draw_*, irec_loglik_*) in a form that a GPU
// workgroup and a host loop run alike: the seeded noise, the draw with its KL term, the likelihood term, what a lane of a tile does,
// the order of every sum, and the whole-call host forms.  Plain C++: no allocation, no libm, no HIP header; compiled with
// -ffp-contract=off, so no operation below is fused.  Only IEEE + - * / sqrt and floor, which host and device round alike: the host
// twins give the device's bits.
//
// ---- the noise ----------------------------------------------------------------------------------------------------------------------
// This project's OWN seeded stream, not TensorFlow's: the reference's sampling pass (`model(image)`) is unseeded, so there is no
// stream to be faithful to.  eps(seed, tag, image, e), a property of those four numbers only:
//   Philox4x32-10, key (seed lo32, seed hi32) of the int64 seed in two's complement, counter (block lo32, block hi32, image, tag);
//   element e of an image takes word e & 3 of block e >> 2;  u = ((word >> 8) + 0.5) * 2^-24, in (0, 1), never 1/2, symmetric;
//   eps = (float)ndtri64(u).
// ndtri64, the Cephes rational form (the coefficients of irec_host.cpp:ndtri_f32) in float64, made exactly antisymmetric about 1/2:
//   p = u < 1/2 ? u : 1 - u                                            (1 - u is exact)
//   p > exp(-2):  w = p - 1/2;  ww = w w;  x = (w + (w ww) (P0(ww) / Q0(ww))) * sqrt(2 pi)
//   otherwise:    z = sqrt(-2 det_log(p));  first = z - det_log(z) / z;  rz = 1 / z;  x = -(first - (P1(rz) / Q1(rz)) / z)
//   ndtri64 = u < 1/2 ? x : -x
// with every polynomial in Horner form, highest power first, "multiply, then add".  p >= 2^-25, so z <= 5.887: Cephes' third branch
// (z >= 8) cannot be reached and is not built, and |eps| <= 5.42 < 5.5.
//
// ---- the draw (a) -------------------------------------------------------------------------------------------------------------------
//   sample = mq + sq * eps in float32: one rounding for the product, one for the sum
//   kl_dim(mq, sq, mp, sp) in float64, irec_device.h's operation sequence:
//     t = sq / sp;  r = t t;  dm = (mq - mp) / sp;  kl = 0.5 (dm dm) + (0.5 (r - 1) - det_log(t))        (a NaN statistic stays a NaN)
//
// ---- the likelihood term (b): the reference's discretized_logistic (rec/models/resnet_vae.py:640-650), float64 throughout -----------
//   scale = det_exp((double)log_scale)              per channel, or the one scalar's
//   step  = binsize / scale
//   q     = floor((double)x / binsize) * binsize
//   a     = (q - (double)loc) / scale
//   b     = a + step
//   v     = (sigmoid(b) - sigmoid(a)) + 1e-7,       sigmoid(t) = 1 / (1 + det_exp(-t))
//   term  = det_log(v)                              (a NaN v stays a NaN)
// det_log and det_exp are the operation sequences of irec_device.h, restated here so that this header stays plain C++.
//
// ---- tiles and sums -----------------------------------------------------------------------------------------------------------------
// An image's `dims` elements are cut into tiles of TILE = 4096; a tile is one workgroup of NT = 256 lanes.  Lane l takes the runs of 4
// consecutive elements that start at tile * TILE + (r * NT + l) * 4, r = 0 .. 3 (one Philox block each), and adds its terms in element
// order into one float64.  The 256 lane sums are added wave by wave (64 lanes) in the tree that pairs lanes at distance 32, 16, 8, 4,
// 2, 1, and the four wave sums in order: ((w0 + w1) + w2) + w3 is the tile's partial, workspace[image][tile].  The last stage adds an
// image's partials in tile order, from 0.0.  No atomics; every store goes to an address that only its lane owns, so a NaN in one
// image reaches that image's outputs only, and an image has the same bits alone or inside any batch.
#ifndef IREC_IDEAL_CORE_H_
#define IREC_IDEAL_CORE_H_

#include <stdint.h>

#include "irec.h"

#if defined(__HIPCC__)
#define IREC_IDEAL_HD __host__ __device__
#else
#define IREC_IDEAL_HD
#endif

namespace irec_ideal {

constexpr int NT = 256, WAVE = 64, RUN = 4, RUNS = IREC_IDEAL_TILE / (NT * RUN), FINISH_NT = 64;
constexpr int64_t TILE = IREC_IDEAL_TILE;
constexpr int64_t MAX_DIMS = (int64_t)1 << 40, MAX_TILES = ((int64_t)1 << 31) - 1, MAX_IMAGE = (int64_t)1 << 32;
static_assert(RUNS * NT * RUN == IREC_IDEAL_TILE, "a tile is a whole number of runs per lane");

IREC_IDEAL_HD inline int64_t tiles_of(int64_t dims) { return (dims + TILE - 1) / TILE; }

// ---- float64 log and exp: irec_device.h's det_log / det_exp, operation by operation ------------------------------------------------
IREC_IDEAL_HD inline double det_log(double x) {
  uint64_t bits = __builtin_bit_cast(uint64_t, x);
  int64_t e = (int64_t)((bits >> 52) & 0x7FF);
  if (e == 0) {
    x = x * 18014398509481984.0;
    bits = __builtin_bit_cast(uint64_t, x);
    e = (int64_t)((bits >> 52) & 0x7FF) - 54;
  }
  e -= 1023;
  bits = (bits & 0x000FFFFFFFFFFFFFull) | 0x3FF0000000000000ull;
  double m = __builtin_bit_cast(double, bits);
  if (m > 1.4142135623730951) { m = m * 0.5; e += 1; }
  const double s = (m - 1.0) / (m + 1.0);
  const double s2 = s * s;
  double q = 1.0 / 25.0;
  q = q * s2 + 1.0 / 23.0;
  q = q * s2 + 1.0 / 21.0;
  q = q * s2 + 1.0 / 19.0;
  q = q * s2 + 1.0 / 17.0;
  q = q * s2 + 1.0 / 15.0;
  q = q * s2 + 1.0 / 13.0;
  q = q * s2 + 1.0 / 11.0;
  q = q * s2 + 1.0 / 9.0;
  q = q * s2 + 1.0 / 7.0;
  q = q * s2 + 1.0 / 5.0;
  q = q * s2 + 1.0 / 3.0;
  const double lnm = 2.0 * s + (2.0 * s) * (s2 * q);
  return (double)e * 0.6931471805599453 + lnm;
}
IREC_IDEAL_HD inline double det_exp(double x) {
  if (!(x == x)) return x;
  if (x < -708.0) return 0.0;
  if (x > 709.0) return __builtin_bit_cast(double, (uint64_t)0x7FF0000000000000ull);
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
  const int64_t k = (int64_t)kf;                                              // in [-1021, 1023]
  return p * __builtin_bit_cast(double, (uint64_t)(k + 1023) << 52);
}

// ---- the noise ------------------------------------------------------------------------------------------------------------------------
struct Stream { uint32_t k0, k1, image, tag; };
IREC_IDEAL_HD inline Stream stream_of(int64_t seed, uint32_t tag, int64_t image) {
  const uint64_t s = (uint64_t)seed;
  return Stream{(uint32_t)s, (uint32_t)(s >> 32), (uint32_t)image, tag};
}
IREC_IDEAL_HD inline void philox_block(const Stream &st, uint64_t block, uint32_t out[4]) {
  uint32_t c0 = (uint32_t)block, c1 = (uint32_t)(block >> 32), c2 = st.image, c3 = st.tag, k0 = st.k0, k1 = st.k1;
  for (int r = 0; r < 10; ++r) {
    const uint64_t a = (uint64_t)0xD2511F53u * c0, b = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(b >> 32) ^ c1 ^ k0, n2 = (uint32_t)(a >> 32) ^ c3 ^ k1;
    c1 = (uint32_t)b; c3 = (uint32_t)a; c0 = n0; c2 = n2;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}
IREC_IDEAL_HD inline double unit_of(uint32_t word) { return ((double)(word >> 8) + 0.5) * 5.9604644775390625e-08; }   // 2^-24: exact

IREC_IDEAL_HD inline double ndtri64(double u) {
  const bool low = u < 0.5;
  const double p = low ? u : 1.0 - u;
  double x;
  if (p > 0.1353352832366127) {                                                 // exp(-2)
    const double w = p - 0.5, ww = w * w;
    double n = -5.99633501014107895267E1;
    n = n * ww + 9.80010754185999661536E1;
    n = n * ww + -5.66762857469070293439E1;
    n = n * ww + 1.39312609387279679503E1;
    n = n * ww + -1.23916583867381258016E0;
    double d = 1.0;
    d = d * ww + 1.95448858338141759834E0;
    d = d * ww + 4.67627912898881538453E0;
    d = d * ww + 8.63602421390890590575E1;
    d = d * ww + -2.25462687854119370527E2;
    d = d * ww + 2.00260212380060660359E2;
    d = d * ww + -8.20372256168333339912E1;
    d = d * ww + 1.59056225126211695515E1;
    d = d * ww + -1.18331621121330003142E0;
    x = (w + (w * ww) * (n / d)) * 2.5066282746310002;                           // sqrt(2 pi)
  } else {
    const double z = __builtin_sqrt(-2.0 * det_log(p));
    const double first = z - det_log(z) / z;
    const double rz = 1.0 / z;
    double n = 4.05544892305962419923E0;
    n = n * rz + 3.15251094599893866154E1;
    n = n * rz + 5.71628192246421288162E1;
    n = n * rz + 4.40805073893200834700E1;
    n = n * rz + 1.46849561928858024014E1;
    n = n * rz + 2.18663306850790267539E0;
    n = n * rz + -1.40256079171354495875E-1;
    n = n * rz + -3.50424626827848203418E-2;
    n = n * rz + -8.57456785154685413611E-4;
    double d = 1.0;
    d = d * rz + 1.57799883256466749731E1;
    d = d * rz + 4.53907635128879210584E1;
    d = d * rz + 4.13172038254672030440E1;
    d = d * rz + 1.50425385692907503408E1;
    d = d * rz + 2.50464946208309415979E0;
    d = d * rz + -1.42182922854787788574E-1;
    d = d * rz + -3.80806407691578277194E-2;
    d = d * rz + -9.33259480895457427372E-4;
    x = -(first - (n / d) / z);
  }
  return low ? x : -x;
}
IREC_IDEAL_HD inline float eps_of(uint32_t word) { return (float)ndtri64(unit_of(word)); }

// ---- the per-element terms ----------------------------------------------------------------------------------------------------------
IREC_IDEAL_HD inline double kl_dim(float mq, float sq, float mp, float sp) {
  const double t = (double)sq / (double)sp;
  const double r = t * t;
  const double dm = ((double)mq - (double)mp) / (double)sp;
  return 0.5 * (dm * dm) + (0.5 * (r - 1.0) - det_log(t));
}
IREC_IDEAL_HD inline float draw_of(float mq, float sq, float eps) {
  const float prod = sq * eps;
  return mq + prod;
}
IREC_IDEAL_HD inline double sigmoid(double t) { return 1.0 / (1.0 + det_exp(-t)); }
IREC_IDEAL_HD inline double loglik_term(float x, float loc, double scale, double step, double binsize) {
  const double q = __builtin_floor((double)x / binsize) * binsize;
  const double a = (q - (double)loc) / scale;
  const double b = a + step;
  const double v = (sigmoid(b) - sigmoid(a)) + 1e-7;
  return v == v ? det_log(v) : v;
}

// ---- the calls ------------------------------------------------------------------------------------------------------------------------
struct DrawCall {
  const float *mq, *sq, *mp, *sp;                   // [n_images][dims]
  int32_t n_images; int64_t dims, seed; uint32_t tag; int64_t image_base;
  float *sample;                                    // out [n_images][dims]
  double *kl;                                       // out [n_images]
  double *partials;                                 // workspace [n_images][tiles_of(dims)]
  int32_t vec;                                      // the five arrays are 16-byte aligned and dims is a multiple of 4: float4 runs
};
struct LoglikCall {
  const float *x, *loc;                             // [n_images][channels][plane]
  const float *log_scales;                          // [n_scales], n_scales 1 or channels
  int32_t n_scales, n_images, channels; int64_t plane, dims; double binsize;
  double *ll;                                       // out [n_images]
  double *partials;                                 // workspace [n_images][tiles_of(dims)]
  int32_t vec;
};
struct alignas(16) F4 { float v[4]; };
// a run of four floats at a 16-byte aligned address, as one 16-byte access
IREC_IDEAL_HD inline F4 load4(const float *p) { F4 r; __builtin_memcpy(&r, __builtin_assume_aligned(p, 16), 16); return r; }
IREC_IDEAL_HD inline void store4(float *p, const F4 &r) { __builtin_memcpy(__builtin_assume_aligned(p, 16), &r, 16); }

inline bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }
inline bool aligned_to(const void *p, uintptr_t a) { return p && ((uintptr_t)p & (a - 1)) == 0; }

// NULL, or what is wrong with a call's shape
inline const char *shape_error(int64_t n_images, int64_t dims) {
  if (n_images < 1 || dims < 1 || dims > MAX_DIMS) return "shape out of range (n_images >= 1, 1 <= dims <= 2^40)";
  if (n_images > MAX_TILES / tiles_of(dims)) return "shape out of range (n_images * tiles must stay below 2^31)";
  return nullptr;
}
inline const char *draw_error(const float *mq, const float *sq, const float *mp, const float *sp, int64_t n_images, int64_t dims,
                              int64_t image_base, const float *sample, const double *kl) {
  if (!aligned_to(mq, 4) || !aligned_to(sq, 4) || !aligned_to(mp, 4) || !aligned_to(sp, 4) || !aligned_to(sample, 4) || !aligned_to(kl, 8))
    return "null or misaligned pointer";
  if (const char *what = shape_error(n_images, dims)) return what;
  if (image_base < 0 || image_base + n_images > MAX_IMAGE) return "image_base + n_images must lie in [0, 2^32]";
  return nullptr;
}
inline const char *loglik_error(const float *x, const float *loc, const float *log_scales, int64_t n_scales, int64_t n_images,
                                int64_t channels, int64_t plane, double binsize, const double *ll) {
  if (!aligned_to(x, 4) || !aligned_to(loc, 4) || !aligned_to(log_scales, 4) || !aligned_to(ll, 8)) return "null or misaligned pointer";
  if (channels < 1 || channels > 65535 || plane < 1 || plane > MAX_DIMS / channels) return "shape out of range (channels 1 .. 65535, plane >= 1, channels * plane <= 2^40)";
  if (const char *what = shape_error(n_images, channels * plane)) return what;
  if (n_scales != 1 && n_scales != channels) return "n_scales must be 1 or channels";
  if (!(binsize > 0.0) || !(binsize < 1.0e300)) return "binsize must be positive and finite";
  return nullptr;
}
inline void bind(DrawCall &c, const float *mq, const float *sq, const float *mp, const float *sp, int32_t n_images, int64_t dims,
                 int64_t seed, uint32_t tag, int64_t image_base, float *sample, double *kl, void *workspace) {
  const int32_t vec = dims % RUN == 0 && aligned16(mq) && aligned16(sq) && aligned16(mp) && aligned16(sp) && aligned16(sample);
  c = DrawCall{mq, sq, mp, sp, n_images, dims, seed, tag, image_base, sample, kl, (double *)workspace, vec};
}
inline void bind(LoglikCall &c, const float *x, const float *loc, const float *log_scales, int32_t n_scales, int32_t n_images,
                 int32_t channels, int64_t plane, double binsize, double *ll, void *workspace) {
  const int64_t dims = (int64_t)channels * plane;
  const int32_t vec = dims % RUN == 0 && aligned16(x) && aligned16(loc);
  c = LoglikCall{x, loc, log_scales, n_scales, n_images, channels, plane, dims, binsize, ll, (double *)workspace, vec};
}

// ---- a lane of a tile: its runs, its float64 sum -------------------------------------------------------------------------------------
IREC_IDEAL_HD inline double draw_lane(const DrawCall &c, int64_t image, int64_t tile, int lane) {
  const Stream st = stream_of(c.seed, c.tag, c.image_base + image);
  const int64_t base = image * c.dims;
  double acc = 0.0;
  for (int r = 0; r < RUNS; ++r) {
    const int64_t e0 = tile * TILE + ((int64_t)r * NT + lane) * RUN;
    if (e0 >= c.dims) break;
    uint32_t word[4];
    philox_block(st, (uint64_t)e0 >> 2, word);
    if (c.vec) {                                                                 // (dims is a multiple of 4: the run is whole)
      const F4 mq = load4(c.mq + base + e0), sq = load4(c.sq + base + e0), mp = load4(c.mp + base + e0), sp = load4(c.sp + base + e0);
      F4 out;
      for (int j = 0; j < RUN; ++j) {
        out.v[j] = draw_of(mq.v[j], sq.v[j], eps_of(word[j]));
        acc += kl_dim(mq.v[j], sq.v[j], mp.v[j], sp.v[j]);
      }
      store4(c.sample + base + e0, out);
    } else {
      const int n = c.dims - e0 < RUN ? (int)(c.dims - e0) : RUN;
      for (int j = 0; j < n; ++j) {
        const int64_t at = base + e0 + j;
        const float mq = c.mq[at], sq = c.sq[at];
        c.sample[at] = draw_of(mq, sq, eps_of(word[j]));
        acc += kl_dim(mq, sq, c.mp[at], c.sp[at]);
      }
    }
  }
  return acc;
}
IREC_IDEAL_HD inline double loglik_lane(const LoglikCall &c, int64_t image, int64_t tile, int lane) {
  const int64_t base = image * c.dims;
  double acc = 0.0, scale = 1.0, step = 0.0;
  int64_t have = -1;                                                             // the channel scale and step were formed for
  for (int r = 0; r < RUNS; ++r) {
    const int64_t e0 = tile * TILE + ((int64_t)r * NT + lane) * RUN;
    if (e0 >= c.dims) break;
    const int n = c.dims - e0 < RUN ? (int)(c.dims - e0) : RUN;
    F4 x, loc;
    if (c.vec) {
      x = load4(c.x + base + e0); loc = load4(c.loc + base + e0);
    } else {
      for (int j = 0; j < n; ++j) { x.v[j] = c.x[base + e0 + j]; loc.v[j] = c.loc[base + e0 + j]; }
    }
    int64_t ch = c.n_scales == 1 ? 0 : e0 / c.plane, left = c.n_scales == 1 ? c.dims : (ch + 1) * c.plane - e0;
    for (int j = 0; j < n; ++j) {
      if (left == 0) { ++ch; left = c.plane; }
      --left;
      if (ch != have) {
        scale = det_exp((double)c.log_scales[ch]);
        step = c.binsize / scale;
        have = ch;
      }
      acc += loglik_term(x.v[j], loc.v[j], scale, step, c.binsize);
    }
  }
  return acc;
}

// the tile's partial from its NT lane sums, in place (host form; the device runs the same tree over lanes)
inline double tile_sum(double *lane_sum) {
  for (int w = 0; w < NT / WAVE; ++w)
    for (int d = WAVE / 2; d >= 1; d /= 2)
      for (int l = 0; l < d; ++l) lane_sum[w * WAVE + l] = lane_sum[w * WAVE + l] + lane_sum[w * WAVE + l + d];
  double s = lane_sum[0];
  for (int w = 1; w < NT / WAVE; ++w) s = s + lane_sum[w * WAVE];
  return s;
}
IREC_IDEAL_HD inline double ordered_sum(const double *p, int64_t n) {
  double acc = 0.0;
  for (int64_t i = 0; i < n; ++i) acc += p[i];
  return acc;
}

// ---- the whole call over host memory --------------------------------------------------------------------------------------------------
struct SerialBlocks {
  template <class F> void operator()(int64_t n, F &&body) const { body((int64_t)0, n); }
};
// par(n, body): body(lo, hi) over [0, n) in any split, on any threads
template <class Par>
inline void draw_host(const DrawCall &c, Par &&par) {
  const int64_t tiles = tiles_of(c.dims);
  par(c.n_images * tiles, [&c, tiles](int64_t lo, int64_t hi) {
    double lane_sum[NT];
    for (int64_t block = lo; block < hi; ++block) {
      for (int lane = 0; lane < NT; ++lane) lane_sum[lane] = draw_lane(c, block / tiles, block % tiles, lane);
      c.partials[block] = tile_sum(lane_sum);
    }
  });
  for (int64_t i = 0; i < c.n_images; ++i) c.kl[i] = ordered_sum(c.partials + i * tiles, tiles);
}
template <class Par>
inline void loglik_host(const LoglikCall &c, Par &&par) {
  const int64_t tiles = tiles_of(c.dims);
  par(c.n_images * tiles, [&c, tiles](int64_t lo, int64_t hi) {
    double lane_sum[NT];
    for (int64_t block = lo; block < hi; ++block) {
      for (int lane = 0; lane < NT; ++lane) lane_sum[lane] = loglik_lane(c, block / tiles, block % tiles, lane);
      c.partials[block] = tile_sum(lane_sum);
    }
  });
  for (int64_t i = 0; i < c.n_images; ++i) c.ll[i] = ordered_sum(c.partials + i * tiles, tiles);
}

} // namespace irec_ideal
#endif // IREC_IDEAL_CORE_H_
