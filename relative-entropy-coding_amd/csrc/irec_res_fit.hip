// irec_res_fit.hip -- the coded cost of a batch under candidate likelihood scales, on the device and on the host (include/irec.h:
// irec_res_scale_bits*, irec_res_cost_table): what a fitter of the .res coder's scale searches over.  The sums and their layout are
// csrc/irec_res_fit_core.h; the host entry point at the end of this file runs that header's plain loops, the kernels here the same
// per-pixel function, and every sum is of integers: the two forms agree bit for bit.
//
//   res_fit_tiles_kernel   one 256-lane workgroup per (image, channel, tile of TILE pixels).  A lane keeps its 16 pixels (x, m) in
//                          16 registers; the candidates are the outer, wave-uniform loop (inv is a scalar of the wave): lane sum in 32
//                          bits (16 x < 2^21), wave reduction by shuffles in 64, one LDS word per (wave, candidate), ONE barrier,
//                          then lane k adds the four waves of candidate k and stores part[unit][k].
//   res_fit_finish_kernel  one lane per (image, channel, column): the tiles added up; INT64_MAX for a refused candidate.
// No atomics: every store goes into a word that only its lane owns.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <exception>
#include <vector>

#include "irec_call.h"
#include "irec_res_fit_core.h"

namespace irec {
namespace {
constexpr int FIT_NT = 256, FIT_WAVES = FIT_NT / 64, FIT_PER_LANE = (int)(irec_res_fit::TILE / FIT_NT);
static_assert(irec_res_fit::TILE % FIT_NT == 0 && irec_res_fit::MAX_CANDIDATES + 1 <= FIT_NT, "a lane per column in the last step");
constexpr int32_t SKIP = -1;                        // a pixel is ((m + 2048) << 8) | x in one register; this one is left out (past the
                                                    // tile's end, or a loc that is not finite)

__global__ __launch_bounds__(FIT_NT) void res_fit_tiles_kernel(irec_res_fit::FitCall c) {
  __shared__ int64_t wave_sum[FIT_WAVES][irec_res_fit::MAX_CANDIDATES + 1];
  const int t = threadIdx.x, wave = t >> 6;
  const int64_t u = blockIdx.x, pair = u / c.tiles, tile = u % c.tiles, ch = pair % c.C;
  const int64_t e0 = tile * irec_res_fit::TILE, e1 = e0 + irec_res_fit::TILE < c.plane ? e0 + irec_res_fit::TILE : c.plane;
  const uint8_t *x = c.pixels + pair * c.plane;
  const float *loc = c.loc + pair * c.plane;
  int32_t px[FIT_PER_LANE];
  uint32_t skipped = 0;
#pragma unroll
  for (int j = 0; j < FIT_PER_LANE; ++j) {
    const int64_t e = e0 + (int64_t)j * FIT_NT + t;
    px[j] = SKIP;
    if (e < e1) {
      const float l = loc[e];
      if (irec_res::is_finite(l)) px[j] = ((irec_res::loc_to_m(l) + 2048) << 8) | (int32_t)x[e]; else ++skipped;
    }
  }
  for (int32_t k = 0; k <= c.n_cand; ++k) {
    uint32_t lane_sum = 0;
    if (k == c.n_cand) lane_sum = skipped;                                       // the last column: the pixels left out
    else {
      const float s = c.scales[ch * c.n_cand + k];
      if (irec_res::scale_ok(s)) {
        const double inv = irec_res::model_inv(s);
#pragma unroll                                                                   // (whole: px stays in registers)
        for (int j = 0; j < FIT_PER_LANE; ++j)
          if (px[j] != SKIP) lane_sum += irec_res_fit::pixel_units(c.cost, (px[j] >> 8) - 2048, px[j] & 255, inv);
      }
    }
    uint64_t sum = lane_sum;
    for (int d = 32; d > 0; d >>= 1) sum += (uint64_t)__shfl_down((unsigned long long)sum, d, 64);
    if ((t & 63) == 0) wave_sum[wave][k] = (int64_t)sum;
  }
  __syncthreads();
  if (t <= c.n_cand) {
    int64_t sum = 0;
    for (int w = 0; w < FIT_WAVES; ++w) sum += wave_sum[w][t];
    c.part[u * (c.n_cand + 1) + t] = sum;
  }
}

__global__ __launch_bounds__(FIT_NT) void res_fit_finish_kernel(irec_res_fit::FitCall c) {
  const int64_t lane = (int64_t)blockIdx.x * FIT_NT + threadIdx.x;
  if (lane < (int64_t)c.N * c.C * (c.n_cand + 1)) irec_res_fit::finish_lane(c, lane);
}

// the call, or false: shapes as the .res entry points take them, 1 .. 64 candidates, a grid of units below 2^31
bool fit_shape_ok(int32_t N, uint32_t height, uint32_t width, uint32_t channels, int32_t n_cand, int64_t *plane, int64_t *tiles) {
  if (N < 0 || height < 1 || width < 1 || channels < 1 || height > 65535 || width > 65535 || channels > 65535 || n_cand < 1 ||
      n_cand > irec_res_fit::MAX_CANDIDATES)
    return false;
  *plane = (int64_t)height * width;
  *tiles = irec_res_fit::tiles_of(*plane);
  return *plane * channels < ((int64_t)1 << 31) && (int64_t)N * channels * *tiles < ((int64_t)1 << 31);
}
bool make_fit_call(irec_res_fit::FitCall &c, const uint8_t *pixels, const float *loc, const float *scales, const uint32_t *cost, int32_t N,
                   uint32_t height, uint32_t width, uint32_t channels, int32_t n_cand, int64_t *bits, int64_t *skipped) {
  int64_t plane = 0, tiles = 0;
  if (!fit_shape_ok(N, height, width, channels, n_cand, &plane, &tiles) || !scales || !cost || (N > 0 && (!pixels || !loc || !bits || !skipped)))
    return false;
  c = irec_res_fit::FitCall{pixels, loc, scales, cost, N, (int32_t)channels, n_cand, plane, tiles, bits, skipped, nullptr};
  return true;
}

} // namespace
} // namespace irec

extern "C" {

irec_status irec_res_cost_table(uint32_t *cost) {
  if (!cost) return irec::set_last_error(IREC_E_INVALID, "irec_res_cost_table", "null table");
  cost[0] = 0;
  for (int64_t n = 1; n < irec_res_fit::COST_ENTRIES; ++n) cost[n] = (uint32_t)std::rint((16.0 - std::log2((double)n)) * 65536.0);
  return IREC_OK;
}

size_t irec_res_scale_bits_workspace_bytes(int32_t n_images, uint32_t height, uint32_t width, uint32_t channels, int32_t n_candidates) {
  int64_t plane = 0, tiles = 0;
  if (!irec::fit_shape_ok(n_images, height, width, channels, n_candidates, &plane, &tiles)) return 0;
  return (size_t)(irec_res_fit::workspace_bytes(n_images, channels, plane, n_candidates) + 256);
}

irec_status irec_res_scale_bits_device(const uint8_t *pixels, const float *loc, const float *scales, const uint32_t *cost, int32_t n_images,
                                       uint32_t height, uint32_t width, uint32_t channels, int32_t n_candidates, int64_t *bits,
                                       int64_t *skipped, void *workspace, size_t workspace_bytes, void *hip_stream) {
  using namespace irec;
  irec_res_fit::FitCall c;
  if (!make_fit_call(c, pixels, loc, scales, cost, n_images, height, width, channels, n_candidates, bits, skipped))
    return set_last_error(IREC_E_INVALID, "irec_res_scale_bits_device", "bad arguments (1 .. 64 candidates)");
  if (irec_status e = check_workspace(irec_res_scale_bits_workspace_bytes(n_images, height, width, channels, n_candidates), workspace, workspace_bytes,
                                      "irec_res_scale_bits_device", "irec_res_scale_bits_workspace_bytes"))
    return e;
  if (n_images == 0) return IREC_OK;
  c.part = (int64_t *)workspace;
  hipStream_t st = (hipStream_t)hip_stream;
  hipLaunchKernelGGL(res_fit_tiles_kernel, dim3((unsigned)((int64_t)c.N * c.C * c.tiles)), dim3(FIT_NT), 0, st, c);
  IREC_HIP_AS("res_fit_tiles_kernel", hipGetLastError());
  const int64_t lanes = (int64_t)c.N * c.C * (c.n_cand + 1);
  hipLaunchKernelGGL(res_fit_finish_kernel, dim3((unsigned)((lanes + FIT_NT - 1) / FIT_NT)), dim3(FIT_NT), 0, st, c);
  IREC_HIP_AS("res_fit_finish_kernel", hipGetLastError());
  return IREC_OK;
}

irec_status irec_res_scale_bits(const uint8_t *pixels, const float *loc, const float *scales, const uint32_t *cost, int32_t n_images,
                                uint32_t height, uint32_t width, uint32_t channels, int32_t n_candidates, int64_t *bits, int64_t *skipped,
                                int32_t n_threads) try {
  using namespace irec;
  irec_res_fit::FitCall c;
  if (!make_fit_call(c, pixels, loc, scales, cost, n_images, height, width, channels, n_candidates, bits, skipped))
    return set_last_error(IREC_E_INVALID, "irec_res_scale_bits", "bad arguments (1 .. 64 candidates)");
  if (n_images == 0) return IREC_OK;
  std::vector<int64_t> ws((size_t)(irec_res_fit::workspace_bytes(n_images, channels, c.plane, n_candidates) / 8 + 1));
  c.part = ws.data();
  irec_res_fit::scale_bits_host(c, Chunks{n_threads, 1});   // (a unit is a tile under every candidate: worth a thread of its own)
  return IREC_OK;
} catch (const std::exception &e) { return irec::set_last_error(IREC_E_INVALID, "irec_res_scale_bits", e.what()); }

} // extern "C"
