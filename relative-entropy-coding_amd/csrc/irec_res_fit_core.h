// irec_res_fit_core.h -- what a batch's pixels cost under candidate likelihood scales: the exact code length of the integer model of
// irec_res_core.h, summed per (image, channel, candidate), in a form that a workgroup and a host loop run alike.  Plain C++: no
// allocation, no libm, no HIP header; compiled with -ffp-contract=off.
//
// A pixel x under (m, s) has the count n = C(x + 1) - C(x) of irec_res_core.h's model, 1 <= n <= 65536, and costs cost[n] units of
// 2^-16 bit, cost[n] = rint((16 - log2 n) 2^16) (irec_res_cost_table: data, built once by the host and passed to both forms).
//     bits[i][ch][k] = sum over the pixels of image i, channel ch, of cost[n(x, m, scales[ch][k])]
// A pixel whose loc is not finite is left out of every sum and counted in skipped[i][ch].  A candidate outside the coder's range
// [2^-24, 2^24] costs nothing to evaluate and gives INT64_MAX.  Every sum is of integers below 2^21, at most 2^31 of them: no order of
// the adds changes it, so the device form, the host form and any batch give the same numbers.
//
// A channel of an image is cut into tiles of TILE pixels.  Pass 1, one unit = (image, channel, tile): part[unit][k] for every
// candidate k and part[unit][n_cand] = the skipped pixels of the tile.  Pass 2, one lane per (image, channel, column): the tiles of
// the column added up.  Nothing is added into memory that another unit or lane owns: no atomics.
#ifndef IREC_RES_FIT_CORE_H_
#define IREC_RES_FIT_CORE_H_

#include <stdint.h>

#include "irec_res_core.h"

namespace irec_res_fit {

constexpr int32_t MAX_CANDIDATES = IREC_RES_FIT_MAX_CANDIDATES;
constexpr int64_t COST_ENTRIES = IREC_RES_COST_ENTRIES;
constexpr int64_t TILE = 4096;                     // pixels of one channel per unit (16 per lane of a 256-lane workgroup)
constexpr int64_t NO_BITS = 0x7fffffffffffffffll;  // INT64_MAX: the column of a candidate that the coder would refuse

struct FitCall {
  const uint8_t *pixels; const float *loc; const float *scales; const uint32_t *cost;
  int32_t N, C, n_cand; int64_t plane, tiles;      // plane = height * width, tiles = ceil(plane / TILE)
  int64_t *bits, *skipped;                          // [N][C][n_cand], [N][C]
  int64_t *part;                                    // workspace [N C tiles][n_cand + 1]
};
IREC_REC_HD inline int64_t tiles_of(int64_t plane) { return (plane + TILE - 1) / TILE; }
IREC_REC_HD inline int64_t workspace_bytes(int64_t N, int64_t C, int64_t plane, int64_t n_cand) { return N * C * tiles_of(plane) * (n_cand + 1) * 8; }

// the units of 2^-16 bit of one pixel
IREC_REC_HD inline uint32_t pixel_units(const uint32_t *cost, int32_t m, int32_t x, double inv) {
  return cost[irec_res::cum(m, inv, x + 1) - irec_res::cum(m, inv, x)];
}

// pass 1 as a plain loop: unit u = (i C + ch) tiles + tile
inline void tile_unit_host(const FitCall &c, int64_t u) {
  const int64_t pair = u / c.tiles, tile = u % c.tiles, ch = pair % c.C;
  const int64_t e0 = tile * TILE, e1 = e0 + TILE < c.plane ? e0 + TILE : c.plane;
  const uint8_t *x = c.pixels + pair * c.plane;
  const float *loc = c.loc + pair * c.plane;
  int64_t *out = c.part + u * (c.n_cand + 1);
  int64_t skipped = 0;
  for (int64_t e = e0; e < e1; ++e) skipped += irec_res::is_finite(loc[e]) ? 0 : 1;
  out[c.n_cand] = skipped;
  for (int32_t k = 0; k < c.n_cand; ++k) {
    const float s = c.scales[ch * c.n_cand + k];
    int64_t sum = 0;
    if (irec_res::scale_ok(s)) {
      const double inv = irec_res::model_inv(s);
      for (int64_t e = e0; e < e1; ++e)
        if (irec_res::is_finite(loc[e])) sum += pixel_units(c.cost, irec_res::loc_to_m(loc[e]), x[e], inv);
    }
    out[k] = sum;
  }
}

// pass 2, lane < N C (n_cand + 1): column k of pair = lane / (n_cand + 1); the last column is the skipped count
IREC_REC_HD inline void finish_lane(const FitCall &c, int64_t lane) {
  const int64_t cols = c.n_cand + 1, pair = lane / cols, k = lane % cols, ch = pair % c.C;
  int64_t sum = 0;
  for (int64_t t = 0; t < c.tiles; ++t) sum += c.part[(pair * c.tiles + t) * cols + k];
  if (k == c.n_cand) c.skipped[pair] = sum;
  else c.bits[pair * c.n_cand + k] = irec_res::scale_ok(c.scales[ch * c.n_cand + k]) ? sum : NO_BITS;
}

// a whole call over host memory; par as in irec_res_core.h
template <class Par>
inline void scale_bits_host(const FitCall &c, Par &&par) {
  par((int64_t)c.N * c.C * c.tiles, [&c](int64_t lo, int64_t hi) { for (int64_t u = lo; u < hi; ++u) tile_unit_host(c, u); });
  const int64_t lanes = (int64_t)c.N * c.C * (c.n_cand + 1);
  for (int64_t l = 0; l < lanes; ++l) finish_lane(c, l);
}

} // namespace irec_res_fit
#endif // IREC_RES_FIT_CORE_H_
