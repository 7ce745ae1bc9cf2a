// irec_quality_core.h -- PSNR and MS-SSIM of a batch (include/irec.h: irec_quality_*) in a form that a GPU workgroup and a host loop run
// alike: the per-pixel arithmetic, the phases of a tile, the ordered sums of the last stage, and the whole-call host form that
// irec_quality_host runs.  Plain C++: no allocation (the host form keeps a tile's 42 KB on its thread's stack), no libm, no HIP header; compiled with -ffp-contract=off,
// so the only fused multiply-adds are the __builtin_fmaf written below.
//
// The definition (DESIGN.md §3 "quality"; tf.image.ssim_multiscale of TF 2.1 with filter_size 11, filter_sigma 1.5):
//   pix = v * mul + add, clamped to [0, max_val] where the image's clip flag is set (a NaN stays a NaN)
//   scale k > 0: both images replaced by their 2 x 2 means, stride 2, an odd height or width extended by its own last row or column
//   F = VALID filtering by the separable 11-tap Gaussian g;  m0 = F(x), m1 = F(y)
//   lum = (2 m0 m1 + c1) / (m0^2 + m1^2 + c1),  cs = (2 F(x y) - 2 m0 m1 + c2) / (F(x^2 + y^2) - (m0^2 + m1^2) + c2)
//   per (image, channel, scale): ssim_k = mean(lum cs), cs_k = mean(cs) over the VALID outputs -- written UNCLAMPED; the clamp at 0, the
//   powers, the product and the channel mean are the caller's (irec/metrics.py), as are mse = sse / (C H W) and the logarithm.
// All of it on data centred at max_val / 2 (x' = pix - max_val / 2): variances and covariances do not move under the shift and the
// means get it back before lum, which takes the cancellation in F(x^2 + y^2) - (m0^2 + m1^2) from magnitude max_val^2 to what the
// images' distance from mid-grey makes it.  The planes of the scales below 0 are kept centred.  sse is taken from the uncentred pixels.
//
// A tile owns TILE x TILE pixels of a plane and the outputs at the same coordinates (output (oy, ox) reads rows oy .. oy + 10, columns
// ox .. ox + 10, so the halo is below and to the right); TILE is even, so the 2 x 2 cells of the next scale never straddle tiles.
// Phases, a barrier between each on the device, a loop over tid on the host:
//   load    the (TILE + 10)^2 region of both images into sx / sy, 0 outside the plane; sse of the pixels the tile owns (scale 0)
//   down    the tile's (TILE / 2)^2 cells of the next scale's planes, from sx / sy                       (not at the last scale)
//   h       hq[q][r][c] = sum_k g[k] q(r, c + k) for the four quantities x, y, x y, x^2 + y^2, rows 0 .. TILE + 9
//   v       the vertical sums, lum and cs of the outputs the tile owns; per-thread float sums of lum cs and cs
//   reduce  a float64 tree over the NT threads; thread 0 stores the tile's partial (sum lum cs, sum cs, sse)
// The last stage adds a plane's partials in tile order in float64: the same bits whatever ran beside it, on any number of threads.
#ifndef IREC_QUALITY_CORE_H_
#define IREC_QUALITY_CORE_H_

#include <stdint.h>

#include "irec.h"

#if defined(__HIPCC__)
#define IREC_Q_HD __host__ __device__
#else
#define IREC_Q_HD
#endif

namespace irec_quality {

constexpr int TAPS = 11, HALO = TAPS - 1, TILE = 32, REGION = TILE + HALO, PITCH = REGION + 1, NT = 256, MAX_SCALES = 5, PART = 3;
constexpr int FINISH_NT = 64;                     // the last stage: one wave per value, its lanes staging what lane 0 adds in order
constexpr int32_t MAX_SIDE = 32768;

struct Call {
  const float *a, *b;                             // [N][C][H][W]
  int32_t N, C, H, W, n_scales;
  float mul_a, add_a, mul_b, add_b;
  int32_t clip_a, clip_b;
  float max_val, half, c1, c2;
  float g[TAPS];
  double *partials;                               // workspace: per scale, plane, tile: PART doubles
  float *planes;                                  // workspace: per scale k >= 1 the centred planes of a, then of b
  float *per_scale;                               // out [N][C][n_scales][2]
  float *sse;                                     // out [N]
};

// the geometry of scale k: plane size, tiles, and where its partials and planes start in the workspace
struct Level {
  int32_t h, w, tiles_y, tiles_x;
  int64_t part_at, plane_at;                      // doubles into partials; floats into planes (scale 0: unused)
  IREC_Q_HD int64_t tiles() const { return (int64_t)tiles_y * tiles_x; }
};
IREC_Q_HD inline Level level_of(int64_t planes, int32_t H, int32_t W, int32_t k) {
  Level L{H, W, (H + TILE - 1) / TILE, (W + TILE - 1) / TILE, 0, 0};
  for (int32_t s = 0; s < k; ++s) {
    L.part_at += planes * L.tiles() * PART;
    if (s > 0) L.plane_at += 2 * planes * L.h * L.w;
    L.h = (L.h + 1) / 2; L.w = (L.w + 1) / 2;
    L.tiles_y = (L.h + TILE - 1) / TILE; L.tiles_x = (L.w + TILE - 1) / TILE;
  }
  return L;
}
// the doubles of partials and the floats of planes that a call of n_scales needs
IREC_Q_HD inline void workspace_sizes(int64_t planes, int32_t H, int32_t W, int32_t n_scales, int64_t *doubles, int64_t *floats) {
  const Level end = level_of(planes, H, W, n_scales);       // (one past the last scale: the running offsets are the totals)
  *doubles = end.part_at;
  *floats = end.plane_at;
}

// NULL, or what is wrong with the call's shape and parameters (the entry points' argument errors)
inline const char *shape_error(int32_t N, int32_t C, int32_t H, int32_t W, int32_t n_scales, const irec_quality_params *p) {
  if (!p) return "null pointer (params)";
  if (n_scales < 1 || n_scales > MAX_SCALES) return "n_scales must be 1 .. 5";
  if (!(p->max_val > 0.0f) || p->max_val > 3.0e38f) return "max_val must be positive and finite";
  if (N < 1 || C < 1 || H < 1 || W < 1 || H > MAX_SIDE || W > MAX_SIDE || (int64_t)N * C > 65535 ||
      (int64_t)N * C * H * W >= ((int64_t)1 << 31))
    return "shape out of range (n, c, h, w >= 1, h and w at most 32768, n c at most 65535, n c h w below 2^31)";
  int32_t h = H, w = W;
  for (int32_t k = 0; k < n_scales; ++k) {
    if (h < TAPS || w < TAPS) return "image too small: height or width below 11 at one of the scales";
    h = (h + 1) / 2; w = (w + 1) / 2;
  }
  return nullptr;
}

// the 11 taps: exp(-(i - 5)^2 / (2 sigma^2)) normalised to sum 1, in float64, rounded once
inline void gaussian_taps(float g[TAPS]) {
  // exp(-d^2 / 4.5) for d = 0 .. 5, to float64 precision
  const double e[6] = {1.0, 0.8007374029168081,0.41111229050718745, 0.1353352832366127, 0.028565500784550377, 0.0038659201394728076};
  double sum = e[0];
  for (int d = 1; d <= 5; ++d) sum += 2.0 * e[d];
  for (int i = 0; i < TAPS; ++i) g[i] = (float)(e[i < 5 ? 5 - i : i - 5] / sum);
}

inline void bind(Call &c, const float *a, const float *b, int32_t N, int32_t C, int32_t H, int32_t W, int32_t n_scales,
                 const irec_quality_params *p, float *per_scale, float *sse, void *workspace) {
  int64_t doubles = 0, floats = 0;
  workspace_sizes((int64_t)N * C, H, W, n_scales, &doubles, &floats);
  const double c1 = (double)p->k1 * (double)p->max_val, c2 = (double)p->k2 * (double)p->max_val;
  c = Call{a, b, N, C, H, W, n_scales, p->mul_a, p->add_a, p->mul_b, p->add_b, p->clip_a, p->clip_b, p->max_val, 0.5f * p->max_val,
           (float)(c1 * c1), (float)(c2 * c2), {}, (double *)workspace, (float *)((double *)workspace + doubles), per_scale, sse};
  gaussian_taps(c.g);
}

// ---- per-pixel arithmetic ---------------------------------------------------------------------------------------------------------
IREC_Q_HD inline float pixel(float v, float mul, float add, int32_t clip, float max_val) {
  float p = v * mul + add;
  if (clip) p = p < 0.0f ? 0.0f : (p > max_val ? max_val : p);           // (comparisons, not fmin / fmax: a NaN stays)
  return p;
}

// the four filtered quantities from 11 samples of x and y, `step` apart
IREC_Q_HD inline void taps_xy(const float *x, const float *y, int step, const float *g, float out[4]) {
  float m0 = 0.0f, m1 = 0.0f, xy = 0.0f, sq = 0.0f;
  for (int k = 0; k < TAPS; ++k) {
    const float xv = x[k * step], yv = y[k * step], w = g[k];
    m0 = __builtin_fmaf(w, xv, m0);
    m1 = __builtin_fmaf(w, yv, m1);
    xy = __builtin_fmaf(w, xv * yv, xy);
    sq = __builtin_fmaf(w, xv * xv + yv * yv, sq);
  }
  out[0] = m0; out[1] = m1; out[2] = xy; out[3] = sq;
}
IREC_Q_HD inline float taps_one(const float *q, int step, const float *g) {
  float s = 0.0f;
  for (int k = 0; k < TAPS; ++k) s = __builtin_fmaf(g[k], q[k * step], s);
  return s;
}
// lum cs and cs from the centred moments.  Identical images give exactly 1 and 1: 2 (m0 m1) is m0 m0 + m1 m1 and 2 F(x y) is
// F(x x + y y) bit for bit when x is y.
IREC_Q_HD inline void ssim_pixel(float m0, float m1, float xy, float sq, float half, float c1, float c2, float *lum_cs, float *cs) {
  const float M0 = m0 + half, M1 = m1 + half;
  const float lum = (2.0f * (M0 * M1) + c1) / ((M0 * M0 + M1 * M1) + c1);
  const float num = (2.0f * xy - 2.0f * (m0 * m1)) + c2;
  const float den = (sq - (m0 * m0 + m1 * m1)) + c2;
  *cs = num / den;
  *lum_cs = lum * *cs;
}

// ---- a tile -----------------------------------------------------------------------------------------------------------------------
struct TileMem {
  float sx[REGION * PITCH], sy[REGION * PITCH];
  float hq[4][REGION * TILE];
  double red[PART][NT];
};
struct Tile {
  const float *a, *b;                             // this plane at this scale
  float *next_a, *next_b;                         // the plane at the next scale (NULL at the last)
  int32_t h, w, h2, w2, y0, x0, first;
  double *part;
};
IREC_Q_HD inline Tile tile_of(const Call &c, int32_t k, int64_t block) {
  const int64_t planes = (int64_t)c.N * c.C;
  const Level L = level_of(planes, c.H, c.W, k);
  const int64_t plane = block / L.tiles(), t = block % L.tiles();
  Tile T;
  const int64_t px = (int64_t)L.h * L.w;
  T.a = k == 0 ? c.a + plane * px : c.planes + L.plane_at + plane * px;
  T.b = k == 0 ? c.b + plane * px : c.planes + L.plane_at + (planes + plane) * px;
  T.h = L.h; T.w = L.w; T.h2 = (L.h + 1) / 2; T.w2 = (L.w + 1) / 2;
  T.y0 = (int32_t)(t / L.tiles_x) * TILE; T.x0 = (int32_t)(t % L.tiles_x) * TILE;
  T.first = k == 0;
  T.part = c.partials + L.part_at + block * PART;
  T.next_a = T.next_b = nullptr;
  if (k + 1 < c.n_scales) {
    const Level D = level_of(planes, c.H, c.W, k + 1);
    T.next_a = c.planes + D.plane_at + plane * ((int64_t)D.h * D.w);
    T.next_b = c.planes + D.plane_at + (planes + plane) * ((int64_t)D.h * D.w);
  }
  return T;
}

// load: returns this thread's share of sum (pa - pb)^2 over the pixels the tile owns (0 below scale 0)
IREC_Q_HD inline float phase_load(const Call &c, const Tile &T, TileMem &m, int tid) {
  float sse = 0.0f;
  for (int i = tid; i < REGION * REGION; i += NT) {
    const int ry = i / REGION, rx = i - ry * REGION;
    const int32_t gy = T.y0 + ry, gx = T.x0 + rx;
    float xa = 0.0f, xb = 0.0f;
    if (gy < T.h && gx < T.w) {
      const int64_t at = (int64_t)gy * T.w + gx;
      if (T.first) {
        const float pa = pixel(T.a[at], c.mul_a, c.add_a, c.clip_a, c.max_val), pb = pixel(T.b[at], c.mul_b, c.add_b, c.clip_b, c.max_val);
        if (ry < TILE && rx < TILE) { const float d = pa - pb; sse += d * d; }
        xa = pa - c.half; xb = pb - c.half;
      } else {
        xa = T.a[at]; xb = T.b[at];
      }
    }
    m.sx[ry * PITCH + rx] = xa; m.sy[ry * PITCH + rx] = xb;
  }
  return sse;
}
// down: thread tid's cell of the next scale, (y0 / 2 + tid / 16, x0 / 2 + tid % 16)
IREC_Q_HD inline void phase_down(const Tile &T, const TileMem &m, int tid) {
  static_assert(NT == (TILE / 2) * (TILE / 2), "one cell of the next scale per thread");
  const int dy = tid / (TILE / 2), dx = tid - dy * (TILE / 2);
  const int32_t oy = T.y0 / 2 + dy, ox = T.x0 / 2 + dx;
  if (oy >= T.h2 || ox >= T.w2) return;
  const int r0 = 2 * dy, c0 = 2 * dx;
  const int r1 = T.y0 + r0 + 1 < T.h ? r0 + 1 : r0, c1 = T.x0 + c0 + 1 < T.w ? c0 + 1 : c0;      // the symmetric edge
  const int64_t at = (int64_t)oy * T.w2 + ox;
  T.next_a[at] = 0.25f * ((m.sx[r0 * PITCH + c0] + m.sx[r0 * PITCH + c1]) + (m.sx[r1 * PITCH + c0] + m.sx[r1 * PITCH + c1]));
  T.next_b[at] = 0.25f * ((m.sy[r0 * PITCH + c0] + m.sy[r0 * PITCH + c1]) + (m.sy[r1 * PITCH + c0] + m.sy[r1 * PITCH + c1]));
}
IREC_Q_HD inline void phase_h(const Call &c, TileMem &m, int tid) {
  for (int i = tid; i < REGION * TILE; i += NT) {
    const int r = i / TILE, col = i - r * TILE;
    float q[4];
    taps_xy(m.sx + r * PITCH + col, m.sy + r * PITCH + col, 1, c.g, q);
    for (int j = 0; j < 4; ++j) m.hq[j][i] = q[j];
  }
}
// v: leaves this thread's float sums in red[0 .. 1][tid] as float64
IREC_Q_HD inline void phase_v(const Call &c, const Tile &T, TileMem &m, int tid, float sse) {
  float s_ssim = 0.0f, s_cs = 0.0f;
  for (int i = tid; i < TILE * TILE; i += NT) {
    const int r = i / TILE, col = i - r * TILE;
    if (T.y0 + r >= T.h - HALO || T.x0 + col >= T.w - HALO) continue;
    float lum_cs, cs;
    ssim_pixel(taps_one(m.hq[0] + i, TILE, c.g), taps_one(m.hq[1] + i, TILE, c.g), taps_one(m.hq[2] + i, TILE, c.g),
               taps_one(m.hq[3] + i, TILE, c.g), c.half, c.c1, c.c2, &lum_cs, &cs);
    s_ssim += lum_cs; s_cs += cs;
  }
  m.red[0][tid] = (double)s_ssim; m.red[1][tid] = (double)s_cs; m.red[2][tid] = (double)sse;
}
IREC_Q_HD inline void phase_reduce_step(TileMem &m, int tid, int d) {
  if (tid < d) for (int j = 0; j < PART; ++j) m.red[j][tid] += m.red[j][tid + d];
}
IREC_Q_HD inline void phase_store(const Tile &T, const TileMem &m) {
  for (int j = 0; j < PART; ++j) T.part[j] = m.red[j][0];
}

// ---- the last stage ---------------------------------------------------------------------------------------------------------------
// value v of a call: v < planes * n_scales is (plane, scale) = (v / n_scales, v % n_scales), two sums over the plane's tiles; the N
// values after those are the images' sse, over the channels' tiles at scale 0.
IREC_Q_HD inline double ordered_sum(const double *p, int64_t stride, int64_t n, double acc) {
  for (int64_t i = 0; i < n; ++i) acc += p[i * stride];
  return acc;
}
IREC_Q_HD inline int64_t n_values(const Call &c) { return (int64_t)c.N * c.C * c.n_scales + c.N; }
IREC_Q_HD inline void finish_plane_store(const Call &c, int64_t plane, int32_t k, const Level &L, double s_ssim, double s_cs) {
  const double n_out = (double)(L.h - HALO) * (double)(L.w - HALO);
  float *out = c.per_scale + (plane * c.n_scales + k) * 2;
  out[0] = (float)(s_ssim / n_out); out[1] = (float)(s_cs / n_out);
}

// ---- the whole call over host memory ----------------------------------------------------------------------------------------------
struct SerialBlocks {
  template <class F> void operator()(int64_t n, F &&body) const { body((int64_t)0, n); }
};
inline void tile_host(const Call &c, int32_t k, int64_t block, TileMem &m) {
  const Tile T = tile_of(c, k, block);
  float sse[NT];
  for (int tid = 0; tid < NT; ++tid) sse[tid] = phase_load(c, T, m, tid);
  if (T.next_a) for (int tid = 0; tid < NT; ++tid) phase_down(T, m, tid);
  for (int tid = 0; tid < NT; ++tid) phase_h(c, m, tid);
  for (int tid = 0; tid < NT; ++tid) phase_v(c, T, m, tid, sse[tid]);
  for (int d = NT / 2; d > 0; d /= 2) for (int tid = 0; tid < d; ++tid) phase_reduce_step(m, tid, d);
  phase_store(T, m);
}
inline void finish_host(const Call &c) {
  const int64_t planes = (int64_t)c.N * c.C;
  const Level L0 = level_of(planes, c.H, c.W, 0);
  for (int64_t plane = 0; plane < planes; ++plane)
    for (int32_t k = 0; k < c.n_scales; ++k) {
      const Level L = level_of(planes, c.H, c.W, k);
      const double *p = c.partials + L.part_at + plane * L.tiles() * PART;
      finish_plane_store(c, plane, k, L, ordered_sum(p, PART, L.tiles(), 0.0), ordered_sum(p + 1, PART, L.tiles(), 0.0));
    }
  for (int64_t n = 0; n < c.N; ++n)
    c.sse[n] = (float)ordered_sum(c.partials + L0.part_at + n * c.C * L0.tiles() * PART + 2, PART, c.C * L0.tiles(), 0.0);
}
// par(n, body): body(lo, hi) over [0, n) in any split, on any threads; a scale is complete before the next begins
template <class Par>
inline void call_host(const Call &c, Par &&par) {
  const int64_t planes = (int64_t)c.N * c.C;
  for (int32_t k = 0; k < c.n_scales; ++k) {
    const Level L = level_of(planes, c.H, c.W, k);
    par(planes * L.tiles(), [&c, k](int64_t lo, int64_t hi) {
      TileMem m;                                             // (42 KB of the thread's stack)
      for (int64_t block = lo; block < hi; ++block) tile_host(c, k, block, m);
    });
  }
  finish_host(c);
}

} // namespace irec_quality
#endif // IREC_QUALITY_CORE_H_
