// irec_image_core.h -- the bilinear shrink of a batch of images (include/irec.h: irec_resize_bilinear_*) in a form that a GPU lane and
// a host loop run alike: the coordinates of an axis, the taps of a pixel, the rows of a tile.  Plain C++: no allocation, no libm (floor
// and ceil are compiler builtins, exact), no HIP header; compiled with -ffp-contract=off, so no multiply-add below is fused.
//
// The definition (DESIGN.md §3 "resize"; tf.image.resize(image, [out_h, out_w]) of TF 2.1: ResizeBilinear, half_pixel_centers=True,
// antialias=False), float32 throughout, per axis of `in` source and `out <= in` output positions:
//   scale = float32(in) / float32(out)
//   s  = (float32(o) + 0.5f) * scale - 0.5f              (one rounding for the product, one for the difference)
//   lo = min(max(floor(s), 0), in - 1),  hi = min(ceil(s), in - 1),  t = s - floor(s)
// and per pixel, with (ylo, yhi, ty) of its row and (xlo, xhi, tx) of its column:
//   top = tl + (tr - tl) * tx,  bot = bl + (br - bl) * tx,  out = top + (bot - top) * ty
// An axis with in == out is not interpolated: lo = hi = o and the value passes through (top = tl, out = top), so equal sizes are a
// bit-for-bit copy, -0 and non-finite values included.  On an interpolated axis both taps always enter the arithmetic, also under a
// weight of 0: a NaN or an infinity reaches exactly the outputs that have it among their taps.  (The upper clamp of lo never binds
// while 3 * 2^-24 * in < 0.5 / out; it is there so that no rounding of s can put a tap outside the row.)
// A uint8 source is converted on load, v = float32(u) / 255.0f (one IEEE division), as the driver's dataset does.
//
// Rows are runs of ROW = width * inner elements, inner = C for [N][H][W][C] (element j of a row is channel j % C of column j / C) and 1
// for the N * C planes of [N][C][H][W]; a tile is TILE_Y rows of TILE_X consecutive elements of one plane's output, one lane per element
// column.  A lane computes its column's (xlo, xhi, tx) ONCE per tile and walks the tile's rows downwards; where a row's upper source row
// is the lower source row of the row before (the usual case of a shrink by less than 2), its `top` is that row's `bot` -- the same taps
// under the same weight, hence the same bits -- and only two taps are loaded.  Every output element is written by exactly one lane.
#ifndef IREC_IMAGE_CORE_H_
#define IREC_IMAGE_CORE_H_

#include <stdint.h>

#include "irec.h"

#if defined(__HIPCC__)
#define IREC_I_HD __host__ __device__
#else
#define IREC_I_HD
#endif

namespace irec_image {

constexpr int NT = 64, TILE_X = NT, TILE_Y = 16;
constexpr int32_t MAX_SIDE = 65536;

struct Call {
  const void *src;                                // [N][C][H][W] or [N][H][W][C], float32 or uint8
  float *dst;                                     // the same layout, float32
  int32_t in_h, in_w, out_h, out_w, src_u8;
  int32_t inner;                                  // channels interleaved in a row
  int64_t planes;                                 // N * C planar, N interleaved
  int32_t row_in, row_out;                        // elements of a source / output row
  int32_t tiles_y, tiles_x;
  float scale_y, scale_x;
  IREC_I_HD int64_t tiles() const { return planes * tiles_y * tiles_x; }
};

// nullptr, or why the entries refuse the call
inline const char *shape_error(int32_t n, int32_t c, int32_t in_h, int32_t in_w, int32_t out_h, int32_t out_w, int32_t layout, int32_t src_dtype) {
  if (n < 1 || c < 1 || in_h < 1 || in_w < 1 || out_h < 1 || out_w < 1) return "n, c and every size must be positive";
  if (out_h > in_h || out_w > in_w) return "out_h <= in_h and out_w <= in_w: the resize only shrinks";
  if (in_h > MAX_SIDE || in_w > MAX_SIDE) return "a side of more than 65536 pixels";
  if (layout != IREC_IMAGE_NCHW && layout != IREC_IMAGE_NHWC) return "layout must be IREC_IMAGE_NCHW or IREC_IMAGE_NHWC";
  if (src_dtype != IREC_IMAGE_F32 && src_dtype != IREC_IMAGE_U8) return "src_dtype must be IREC_IMAGE_F32 or IREC_IMAGE_U8";
  const int64_t inner = layout == IREC_IMAGE_NHWC ? c : 1, planes = layout == IREC_IMAGE_NHWC ? n : (int64_t)n * c;
  if (inner * in_w > INT32_MAX) return "a row of more than 2^31 - 1 elements";
  const int64_t tiles_x = (inner * out_w + TILE_X - 1) / TILE_X, tiles_y = (out_h + TILE_Y - 1) / TILE_Y;
  if (planes > INT32_MAX / (tiles_x * tiles_y)) return "more than 2^31 - 1 tiles";
  return nullptr;
}

// a call that shape_error passed
inline void bind(Call &k, const void *src, int32_t src_dtype, int32_t n, int32_t c, int32_t in_h, int32_t in_w, int32_t out_h, int32_t out_w,
                 int32_t layout, float *dst) {
  k.src = src; k.dst = dst;
  k.in_h = in_h; k.in_w = in_w; k.out_h = out_h; k.out_w = out_w; k.src_u8 = src_dtype == IREC_IMAGE_U8;
  k.inner = layout == IREC_IMAGE_NHWC ? c : 1;
  k.planes = layout == IREC_IMAGE_NHWC ? n : (int64_t)n * c;
  k.row_in = in_w * k.inner; k.row_out = out_w * k.inner;
  k.tiles_y = (out_h + TILE_Y - 1) / TILE_Y; k.tiles_x = (k.row_out + TILE_X - 1) / TILE_X;
  k.scale_y = (float)in_h / (float)out_h; k.scale_x = (float)in_w / (float)out_w;
}

struct Axis { int32_t lo, hi; float t; };
IREC_I_HD inline Axis axis_of(int32_t o, int32_t in, int32_t out, float scale) {
  if (in == out) return Axis{o, o, 0.0f};
  const float s = ((float)o + 0.5f) * scale - 0.5f;
  const float fl = __builtin_floorf(s);
  int32_t lo = (int32_t)fl, hi = (int32_t)__builtin_ceilf(s);
  lo = lo < 0 ? 0 : lo;
  lo = lo > in - 1 ? in - 1 : lo;
  hi = hi > in - 1 ? in - 1 : hi;
  return Axis{lo, hi, s - fl};
}

IREC_I_HD inline float load(const Call &k, int64_t at) {
  return k.src_u8 ? (float)((const uint8_t *)k.src)[at] / 255.0f : ((const float *)k.src)[at];
}
IREC_I_HD inline float lerp(float a, float b, float t) { return a + (b - a) * t; }

// where a tile lies: its plane, its first element column, its rows [y0, y1)
struct Tile { int64_t plane; int32_t j0, y0, y1; };
IREC_I_HD inline Tile tile_of(const Call &k, int64_t tile) {
  const int32_t tx = (int32_t)(tile % k.tiles_x), ty = (int32_t)(tile / k.tiles_x % k.tiles_y);
  const int32_t y0 = ty * TILE_Y;
  return Tile{tile / ((int64_t)k.tiles_x * k.tiles_y), tx * TILE_X, y0, y0 + TILE_Y < k.out_h ? y0 + TILE_Y : k.out_h};
}

// the taps of a plane read where they lie: element j of source row `row`
struct Direct {
  const Call &k; int64_t src_at;
  IREC_I_HD float operator()(int32_t row, int32_t j) const { return load(k, src_at + (int64_t)row * k.row_in + j); }
};

// what lane `lane` of a tile does, its taps coming from `tap(row, j)`: its element column of the tile's rows
template <class Tap>
IREC_I_HD inline void lane_walk(const Call &k, const Tile &T, int32_t lane, const Tap &tap) {
  const int32_t j = T.j0 + lane;
  if (j >= k.row_out) return;
  const int32_t ch = j % k.inner;
  const Axis ax = axis_of(j / k.inner, k.in_w, k.out_w, k.scale_x);            // once per tile
  const int32_t jlo = ax.lo * k.inner + ch, jhi = ax.hi * k.inner + ch;
  const bool lerp_x = k.in_w != k.out_w;
  float *dst = k.dst + T.plane * k.out_h * k.row_out + j;
  int32_t have = -1;                                                          // the source row `below` was taken from
  float below = 0.0f;
  for (int32_t y = T.y0; y < T.y1; ++y) {
    const Axis ay = axis_of(y, k.in_h, k.out_h, k.scale_y);
    const float top = ay.lo == have ? below : (lerp_x ? lerp(tap(ay.lo, jlo), tap(ay.lo, jhi), ax.t) : tap(ay.lo, jlo));
    if (k.in_h == k.out_h) {
      dst[(int64_t)y * k.row_out] = top;
      continue;
    }
    below = ay.hi == ay.lo ? top : (lerp_x ? lerp(tap(ay.hi, jlo), tap(ay.hi, jhi), ax.t) : tap(ay.hi, jlo));
    have = ay.hi;
    dst[(int64_t)y * k.row_out] = lerp(top, below, ay.t);
  }
}
IREC_I_HD inline void lane_of_tile(const Call &k, int64_t tile, int32_t lane) {
  const Tile T = tile_of(k, tile);
  lane_walk(k, T, lane, Direct{k, T.plane * k.in_h * k.row_in});
}

// ---- the staged form (a diagnostic build, IREC_IMAGE_STAGE: the product reads the taps where they lie) ---------------------------------
// The source rectangle a tile's taps come from -- rows r0 .. r0 + rows - 1, elements e0 .. e0 + cols - 1 -- copied into LDS by the
// whole workgroup (consecutive lanes, consecutive elements), a barrier, then lane_walk over the copy: the same taps, the same bits.  A
// tile whose rectangle is larger than the stage (a shrink by 2 or more) is walked directly.
constexpr int STAGE_ROWS = 2 * TILE_Y + 2, STAGE_COLS = 2 * TILE_X + 16;
struct Stage { float v[STAGE_ROWS * STAGE_COLS]; };
struct Span { int32_t r0, rows, e0, cols; bool fits; };
IREC_I_HD inline Span span_of(const Call &k, const Tile &T) {
  const int32_t j1 = T.j0 + TILE_X < k.row_out ? T.j0 + TILE_X : k.row_out;
  const int32_t r0 = axis_of(T.y0, k.in_h, k.out_h, k.scale_y).lo, r1 = axis_of(T.y1 - 1, k.in_h, k.out_h, k.scale_y).hi;
  const int32_t e0 = axis_of(T.j0 / k.inner, k.in_w, k.out_w, k.scale_x).lo * k.inner;
  const int32_t e1 = axis_of((j1 - 1) / k.inner, k.in_w, k.out_w, k.scale_x).hi * k.inner + k.inner - 1;
  const Span s{r0, r1 - r0 + 1, e0, e1 - e0 + 1, false};
  return Span{s.r0, s.rows, s.e0, s.cols, s.rows >= 1 && s.rows <= STAGE_ROWS && s.cols >= 1 && s.cols <= STAGE_COLS};
}
IREC_I_HD inline void phase_stage(const Call &k, const Tile &T, const Span &s, Stage &m, int32_t tid) {
  const int64_t src_at = T.plane * k.in_h * k.row_in;
  for (int32_t at = tid; at < s.rows * s.cols; at += NT) {
    const int32_t r = at / s.cols, c = at % s.cols;
    m.v[r * STAGE_COLS + c] = load(k, src_at + (int64_t)(s.r0 + r) * k.row_in + s.e0 + c);
  }
}
struct Staged {
  const Stage &m; Span s;
  IREC_I_HD float operator()(int32_t row, int32_t j) const { return m.v[(row - s.r0) * STAGE_COLS + (j - s.e0)]; }
};

// the whole call on the host: par(n, body) deals [0, n) to threads
template <class Par>
inline void call_host(const Call &k, Par &&par) {
  par(k.tiles(), [&k](int64_t lo, int64_t hi) {
    for (int64_t tile = lo; tile < hi; ++tile)
      for (int32_t lane = 0; lane < NT; ++lane) lane_of_tile(k, tile, lane);
  });
}

} // namespace irec_image
#endif // IREC_IMAGE_CORE_H_
