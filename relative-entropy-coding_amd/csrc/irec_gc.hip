// irec_gc.hip -- the SEQUENTIAL iREC coder of the reference on the device: GaussianCoder.encode_block / decode_block with an
// ImportanceSampler (rec/coding/coder.py:493-584 over rec/coding/importance_sampling.py:9-103), gfx950 only: alpha = inf (the arg-max
// of the importance weights) and 1 <= alpha < inf (the Gumbel-max over alpha * w + g, importance_sampling.py:67-72).
//
// Arithmetic contract: DESIGN.md §3 "sequential importance coder".  float32, correctly rounded + - * / sqrt in the reference's
// operator order, no contraction; the weight of a sample is the float64 sum of its float32 terms IN DIM ORDER, rounded once.
// That order is kept by construction: one lane owns one (block, sample) pair and walks the dims serially -- no weight is ever
// reduced across lanes; the only cross-lane step is the arg-max over a block's samples.
//
// The standard-normal proposals are DATA the kernels read (like the quantile table of the beam coder): built on the host by
// irec_normal_table_build, tab[(t * D + d) * S_pad + s] = element s * D + d of tf.random.normal after set_seed(seed + t).
// Lanes that own consecutive samples read consecutive floats.
//
// Finite alpha: the perturbation g[j * S_pad + s] of step j (irec_gumbel_table_build: -logf(-logf(z)) of a stateless NORMAL draw, NaN
// for two samples in three, as the reference has it) is DATA too.  The lane that owns sample s reads g[j][s] once its weight is
// complete and offers v = alpha * w + g (one float32 multiply, one float32 add) to the same arg-max: strict ">", so a NaN is never
// chosen, +inf can win, the first of equals wins.  Adjacent lanes read adjacent floats; no LDS and no barrier is added.  The text
// of the encoders is irec_gc_encode.inc, compiled twice: the alpha = inf kernels keep their names and their code
// (scripts/isa_identity.py), the perturbed ones are gc_gumbel_encode_kernel / gc_gumbel_encode_wide_kernel.
//
// Blocks of at most GC_MAX_DIM = 1024 dims (gc_importance_encode_kernel; wider ones: gc_importance_encode_wide_kernel below).
// Shape: one workgroup per block at a time, blockDim = S rounded up to a wave (64 .. 1024 lanes; beyond 1024 samples a lane owns
// several).  The block's (mu_q, sigma_q, mu_p, sigma_p) stay in LDS for all of its K steps.  Per step:
//   (A) lanes over dims:    ts, tl / ts, c of the step's standardised target into LDS
//   (B) lanes over samples: w[s] over d = 0 .. D-1 (constants as LDS broadcasts, table rows coalesced)
//   (C) arg-max over the workgroup (DPP within a wave, LDS across waves): greatest w, first s on ties, a NaN never
//   (D) lanes over dims:    the conditional update with A[d] = sqrt(a[d]) * x[j][d]
#include <cfloat>

#include "irec_device.h"
#include "irec_kernels.h"

namespace irec {

namespace {

constexpr float GC_HL2PI = 0.918938533204672742f;   // float32(0.5 * ln(2 pi))

__device__ __forceinline__ int64_t gc_index(const GcArgs &A, int64_t base, int32_t pos, int d) {
  return base + (A.perm ? (int64_t)A.perm[pos + d] : (int64_t)(pos + d));
}
__device__ __forceinline__ int gc_table_of(const GcArgs &A, int D) {
  int q = -1;
#pragma unroll
  for (int i = 3; i >= 0; --i)
    if (A.tab[i] && A.tab_dim[i] == D) q = i;
  return q;
}
__device__ __forceinline__ bool gc_row_coded(const GcArgs &A, int K) {
  return K >= 0 && K <= A.max_K && K <= A.steps && K <= A.K_limit;
}

} // namespace

// ---- blocks of more than GC_MAX_DIM dims -----------------------------------------------------------------------------------------
// The same coder, op for op, for any D >= 1: one workgroup of GC_WIDE_THREADS = 1024 lanes codes one block at a time.  The block's
// (mu_q, sigma_q, mu_p, sigma_p) live in a slab of the caller's workspace (four float arrays of D rounded up to 1024, one slab per
// resident workgroup) instead of LDS.  In EVERY phase that touches the slab -- the load, (A) and (D) -- a lane reads and writes the
// dims tid + k * 1024 and no others, so no lane ever depends on another lane's global stores.
//
// A step walks the block in chunks of 1024 dims, in increasing order.  Per chunk:
//   (A)  lane tid: ts, tl / ts, c of dim chunk_base + tid into LDS
//   (B1) tiles of TD = GC_TILE_FLOATS / S_pad dims (256 at S_pad = 32): all 1024 lanes compute the float32 terms lt - lp of the tile's
//        TD x S_pad (dim, sample) pairs into a 32 KB LDS tile; the tile of the table is one contiguous run of floats, read linearly
//   (B2) after a barrier lane s < S adds its column of the tile to its own float64 accumulator, dim by dim in order (adjacent lanes
//        read adjacent floats); a barrier follows before the tile is overwritten
// No partial sum is ever formed: the accumulator of a sample sees its D terms one at a time, d = 0, 1, ... -- the contract of
// DESIGN.md §3, and the reason wide and narrow blocks, host and device agree bit for bit.  The tile form spreads the IEEE divisions
// of a step over 1024 lanes and leaves only the float64 add chain serial (at S = 21 the plain walk keeps 21 lanes busy).
//
// THE SWITCH: S_pad > GC_TILE_SPAD_MAX = 1024 (a 32 KB tile would hold fewer than 8 dims; with that many samples all lanes are busy
// anyway) takes the PLAIN walk: samples in groups of 1024, lane tid owns sample g * 1024 + tid of group g and walks the chunk's
// constants as the narrow kernel walks a block's; (A) is computed again for every group (same operations, same bits).
// IREC_GC_WIDE_TILE=0 compiles the tile form out (the plain walk at every S): the A/B of scripts/bench_gc_importance_wide.py.
// Measured (profiles/gc_importance/bench_wide.json): one 8192-dim block at S = 21, 12.6 ms tiled against 139.8 ms plain
// (the host loop: 106.9 ms); three blocks of <= 3000 dims at S = 256, 7.2 ms against 20.5 ms.  The tile form is the default.
#ifndef IREC_GC_WIDE_TILE
#define IREC_GC_WIDE_TILE 1
#endif
constexpr int GC_TILE_FLOATS = 8192;      // 32 KB
constexpr int GC_TILE_SPAD_MAX = 1024;    // GC_TILE_FLOATS / 8

// the encoders: irec_gc_encode.inc, once per selection rule
#define GC_GUMBEL 0
#define GC_NARROW_KERNEL gc_importance_encode_kernel
#define GC_WIDE_KERNEL gc_importance_encode_wide_kernel
#define GC_KERNEL_PARAMS GcArgs A
#include "irec_gc_encode.inc"
#undef GC_GUMBEL
#undef GC_NARROW_KERNEL
#undef GC_WIDE_KERNEL
#undef GC_KERNEL_PARAMS

#define GC_GUMBEL 1
#define GC_NARROW_KERNEL gc_gumbel_encode_kernel
#define GC_WIDE_KERNEL gc_gumbel_encode_wide_kernel
#define GC_KERNEL_PARAMS GcArgs A, const float *gum, float alpha
#include "irec_gc_encode.inc"
#undef GC_GUMBEL
#undef GC_NARROW_KERNEL
#undef GC_WIDE_KERNEL
#undef GC_KERNEL_PARAMS

// GaussianCoder.decode_block (coder.py:561-584): the p recursion alone, every dim on its own.
__global__ __launch_bounds__(256) void gc_importance_decode_kernel(GcArgs A) {
  const int tid = threadIdx.x, nt = blockDim.x;
  for (int64_t blk = blockIdx.x; blk < A.n_blocks; blk += gridDim.x) {
    const int D = A.block_dim[blk];
    const int K = A.K[blk];
    const int q = D >= 1 ? gc_table_of(A, D) : -1;
    const int n_steps = K < 1 ? 1 : K;
    const int32_t *idx = A.indices + blk * (int64_t)A.max_K;
    bool ok = q >= 0 && gc_row_coded(A, K);
    if (ok)
      for (int t = 0; t < n_steps; ++t) ok = ok && (uint32_t)idx[t] < (uint32_t)A.S;
    const float *tab = ok ? A.tab[q] : nullptr;
    const int64_t base = A.block_base[blk];
    const int32_t pos = A.block_pos[blk];
    const size_t S_pad = (size_t)A.S_pad;
    for (int d = tid; d < D; d += nt) {
      const int64_t ix = gc_index(A, base, pos, d);
      float mp = A.p_loc[ix];
      if (!ok) { A.out_sample[ix] = mp; continue; }   // not decodable: p_loc, and no table row is addressed
      float sp = A.p_scale[ix];
      for (int t = 0; t < n_steps - 1; ++t) {
        const float x = tab[((size_t)t * (size_t)D + (size_t)d) * S_pad + (size_t)idx[t]];
        const float cv = sp * sp, a = A.rho[K - 1 - t] * cv;
        const float av = sqrtf(a) * x + 0.0f;
        mp = mp + av;
        sp = sqrtf(cv - a);
      }
      const float x = tab[((size_t)(n_steps - 1) * (size_t)D + (size_t)d) * S_pad + (size_t)idx[n_steps - 1]];
      A.out_sample[ix] = sp * x + mp;
    }
  }
}

int gc_encode_threads(int S) { const int r = (S + 63) / 64 * 64; return r < 64 ? 64 : r > 1024 ? 1024 : r; }

hipError_t launch_gc_importance_encode(const GcArgs &A, int grid, hipStream_t st) {
  hipLaunchKernelGGL(gc_importance_encode_kernel, dim3(grid), dim3(gc_encode_threads(A.S)), 0, st, A);
  return hipGetLastError();
}

hipError_t launch_gc_importance_encode_wide(const GcArgs &A, int grid, hipStream_t st) {
  hipLaunchKernelGGL(gc_importance_encode_wide_kernel, dim3(grid), dim3(GC_WIDE_THREADS), 0, st, A);
  return hipGetLastError();
}

// the perturbed encoders: gum = the call's Gumbel table (device, [steps][S_pad]), alpha finite and >= 1; grids as above
hipError_t launch_gc_gumbel_encode(const GcArgs &A, const float *gum, float alpha, int grid, hipStream_t st) {
  hipLaunchKernelGGL(gc_gumbel_encode_kernel, dim3(grid), dim3(gc_encode_threads(A.S)), 0, st, A, gum, alpha);
  return hipGetLastError();
}

hipError_t launch_gc_gumbel_encode_wide(const GcArgs &A, const float *gum, float alpha, int grid, hipStream_t st) {
  hipLaunchKernelGGL(gc_gumbel_encode_wide_kernel, dim3(grid), dim3(GC_WIDE_THREADS), 0, st, A, gum, alpha);
  return hipGetLastError();
}

hipError_t launch_gc_importance_decode(const GcArgs &A, int grid, hipStream_t st) {
  hipLaunchKernelGGL(gc_importance_decode_kernel, dim3(grid), dim3(256), 0, st, A);
  return hipGetLastError();
}

} // namespace irec
