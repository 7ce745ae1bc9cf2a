// irec_gc_encode.inc -- the two encoders of irec_gc.hip (which has their description), compiled twice from this one text:
//   GC_GUMBEL 0   alpha = inf: gc_importance_encode_kernel / gc_importance_encode_wide_kernel(GcArgs A), the arg-max of the weights
//   GC_GUMBEL 1   1 <= alpha < inf: gc_gumbel_encode_kernel / gc_gumbel_encode_wide_kernel(GcArgs A, const float *gum, float alpha), the
//                 arg-max of alpha * w + gum[step * S_pad + s] -- one float32 multiply, one float32 add, one more load per sample a lane owns
// Textual inclusion, not a template over a shared body: a body that takes GcArgs as a function argument reads the kernel arguments through a
// private copy, and the alpha = inf kernels came out with another schedule (1128 -> 1113 instructions, 87 -> 92 VGPRs in the narrow one).
// This way their token stream is what it was, and scripts/isa_identity.py finds them unchanged.
__global__ __launch_bounds__(1024) void GC_NARROW_KERNEL(GC_KERNEL_PARAMS) {
  __shared__ float s_mq[GC_MAX_DIM], s_sq[GC_MAX_DIM], s_mp[GC_MAX_DIM], s_sp[GC_MAX_DIM];
  __shared__ float s_ts[GC_MAX_DIM], s_tt[GC_MAX_DIM], s_c[GC_MAX_DIM];
  __shared__ unsigned long long s_best[16];
  const int tid = threadIdx.x, nt = blockDim.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), nw = nt >> 6;
  for (int64_t blk = blockIdx.x; blk < A.n_blocks; blk += gridDim.x) {   // (every exit below is uniform over the workgroup)
    const int D = A.block_dim[blk];
    const int K = A.out_K[blk];                 // ceil(KL / Omega), left there by the block-KL kernel of the same call
    const int q = (D >= 1 && D <= GC_MAX_DIM) ? gc_table_of(A, D) : -1;
    if (q < 0) {
      if (tid == 0) A.out_K[blk] = -1;          // dim not covered
      continue;
    }
    if (!gc_row_coded(A, K)) continue;          // not coded: out_K says how many partitions the block needs
    const float *tab = A.tab[q];
    const int64_t base = A.block_base[blk];
    const int32_t pos = A.block_pos[blk];
    const size_t S_pad = (size_t)A.S_pad;
    for (int d = tid; d < D; d += nt) {
      const int64_t ix = gc_index(A, base, pos, d);
      s_mq[d] = A.q_loc[ix]; s_sq[d] = A.q_scale[ix]; s_mp[d] = A.p_loc[ix]; s_sp[d] = A.p_scale[ix];
    }
    const int n_steps = K < 1 ? 1 : K;          // len(indices) = max(K, 1), coder.py:548-557
    for (int t = 0; t < n_steps; ++t) {
      const bool last = t == n_steps - 1;
      const float rho = last ? 0.0f : A.rho[K - 1 - t];   // get_auxiliary_ratio(i), i = K-1 .. 1 (coder.py:505-506)
      // (A) the step's target, standardised w.r.t. its coder (importance_sampling.py:40-41)
      for (int d = tid; d < D; d += nt) {
        const float mq = s_mq[d], sq = s_sq[d], mp = s_mp[d], sp = s_sp[d];
        float tl, ts;
        if (last) {
          tl = (mq - mp) / sp;
          ts = sq / sp;
        } else {
          const float cv = sp * sp, tv = sq * sq, a = rho * cv;
          const float ta_loc = (mq - mp) * a / cv;                                          // coder.py:147-154
          const float ta_scale = sqrtf(tv * (a * a) / (cv * cv) + a * (cv - a) / cv);
          const float pa_scale = sqrtf(a);                                                  // coder.py:141-144
          tl = (ta_loc - 0.0f) / pa_scale;
          ts = ta_scale / pa_scale;
        }
        s_ts[d] = ts;
        s_tt[d] = tl / ts;
        s_c[d] = GC_HL2PI + (float)det_log((double)ts);
      }
      __syncthreads();
      // (B) importance weights, one lane per sample, dims in order
      const float *row = tab + (size_t)t * (size_t)D * S_pad;
      float best = -FLT_MAX;
      int best_s = 0;
      for (int s = tid; s < A.S; s += nt) {
        const float *col = row + s;
        double acc = 0.0;
#pragma unroll 4
        for (int d = 0; d < D; ++d) {
          const float x = col[(size_t)d * S_pad];
          const float e = x / s_ts[d] - s_tt[d];
          const float lt = -0.5f * (e * e) - s_c[d];
          const float lp = -0.5f * (x * x) - GC_HL2PI;
          acc = acc + (double)(lt - lp);
        }
#if GC_GUMBEL
        const float w = alpha * (float)acc + gum[(size_t)t * S_pad + (size_t)s];   // Gumbel-max (importance_sampling.py:67-72)
#else
        const float w = (float)acc;
#endif
        if (w > best) { best = w; best_s = s; }
      }
      // (C) greatest weight, lowest sample index on ties; a lane without a candidate holds (-FLT_MAX, 0), the accumulator's start
      unsigned long long pk = ((unsigned long long)score_key(best) << 32) | (unsigned long long)(0xFFFFFFFFu - (uint32_t)best_s);
      pk = wave_max_u64(pk);
      if (lane == 0) s_best[wave] = pk;
      __syncthreads();
      pk = s_best[0];
      for (int w = 1; w < nw; ++w) { const unsigned long long o = s_best[w]; pk = o > pk ? o : pk; }
      const int j = (int)(0xFFFFFFFFu - (uint32_t)pk);
      if (tid == 0) A.out_indices[blk * (int64_t)A.max_K + t] = j;
      // (D) the chosen sample: the next step's distributions (coder.py:157-171), or the block's sample
      for (int d = tid; d < D; d += nt) {
        const float x = row[(size_t)d * S_pad + (size_t)j];
        const float mq = s_mq[d], sq = s_sq[d], mp = s_mp[d], sp = s_sp[d];
        if (last) {
          A.out_sample[gc_index(A, base, pos, d)] = sp * x + mp;
        } else {
          const float cv = sp * sp, tv = sq * sq, a = rho * cv;
          const float av = sqrtf(a) * x + 0.0f;                                             // pa.scale * x + pa.loc
          s_mq[d] = mp + (av * tv * cv + (mq - mp) * (cv - a) * cv) / (tv * a + cv * (cv - a));
          s_sq[d] = sqrtf(tv * cv * (cv - a) / (a * tv + cv * (cv - a)));
          s_mp[d] = mp + av;
          s_sp[d] = sqrtf(cv - a);
        }
      }
      // (every lane rewrites only the dims it read in (A) and (D); the barrier after (A) of the next step -- or of the next
      //  block -- separates this step's reads of s_best from the next write)
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(GC_WIDE_THREADS) void GC_WIDE_KERNEL(GC_KERNEL_PARAMS) {
  __shared__ float s_ts[GC_WIDE_THREADS], s_tt[GC_WIDE_THREADS], s_c[GC_WIDE_THREADS];
#if IREC_GC_WIDE_TILE
  __shared__ float s_tile[GC_TILE_FLOATS];
#endif
  __shared__ unsigned long long s_best[GC_WIDE_THREADS / 64];
  constexpr int NT = GC_WIDE_THREADS;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const size_t S_pad = (size_t)A.S_pad;
  float *const w_mq = A.slab + (size_t)blockIdx.x * 4 * (size_t)A.slab_dim;   // this workgroup's slab
  float *const w_sq = w_mq + A.slab_dim, *const w_mp = w_sq + A.slab_dim, *const w_sp = w_mp + A.slab_dim;
#if IREC_GC_WIDE_TILE
  const bool tiled = A.S_pad <= GC_TILE_SPAD_MAX;
  const int TD = tiled ? GC_TILE_FLOATS / A.S_pad : 0;          // dims of a tile (>= 8)
  const int e_q = NT / A.S_pad, e_r = NT % A.S_pad;             // a lane's next tile element lies NT floats on: e_q dims, e_r samples
#else
  const bool tiled = false;
#endif
  const int n_groups = (A.S + NT - 1) / NT;                     // (1 whenever the tile form applies)
  for (int64_t blk = blockIdx.x; blk < A.n_blocks; blk += gridDim.x) {   // (every exit below is uniform over the workgroup)
    const int D = A.block_dim[blk];
    const int K = A.out_K[blk];                 // ceil(KL / Omega), left there by the block-KL kernel of the same call
    const int q = (D >= 1 && D <= A.slab_dim) ? gc_table_of(A, D) : -1;
    if (q < 0) {
      __syncthreads();                          // (every lane has read out_K[blk])
      if (tid == 0) A.out_K[blk] = -1;          // dim not covered
      continue;
    }
    if (!gc_row_coded(A, K)) continue;          // not coded: out_K says how many partitions the block needs
    const float *tab = A.tab[q];
    const int64_t base = A.block_base[blk];
    const int32_t pos = A.block_pos[blk];
    for (int d = tid; d < D; d += NT) {
      const int64_t ix = gc_index(A, base, pos, d);
      w_mq[d] = A.q_loc[ix]; w_sq[d] = A.q_scale[ix]; w_mp[d] = A.p_loc[ix]; w_sp[d] = A.p_scale[ix];
    }
    const int n_steps = K < 1 ? 1 : K;          // len(indices) = max(K, 1), coder.py:548-557
    for (int t = 0; t < n_steps; ++t) {
      const bool last = t == n_steps - 1;
      const float rho = last ? 0.0f : A.rho[K - 1 - t];   // get_auxiliary_ratio(i), i = K-1 .. 1 (coder.py:505-506)
      const float *row = tab + (size_t)t * (size_t)D * S_pad;
      float best = -FLT_MAX;
      int best_s = 0;
      for (int g = 0; g < n_groups; ++g) {
        const int s = g * NT + tid;             // the sample whose weight this lane accumulates
        double acc = 0.0;
        for (int cb = 0; cb < D; cb += NT) {    // chunks of 1024 dims, in increasing order
          const int CD = D - cb < NT ? D - cb : NT;
          // (A) the step's target, standardised w.r.t. its coder (importance_sampling.py:40-41)
          if (tid < CD) {
            const int d = cb + tid;
            const float mq = w_mq[d], sq = w_sq[d], mp = w_mp[d], sp = w_sp[d];
            float tl, ts;
            if (last) {
              tl = (mq - mp) / sp;
              ts = sq / sp;
            } else {
              const float cv = sp * sp, tv = sq * sq, a = rho * cv;
              const float ta_loc = (mq - mp) * a / cv;                                          // coder.py:147-154
              const float ta_scale = sqrtf(tv * (a * a) / (cv * cv) + a * (cv - a) / cv);
              const float pa_scale = sqrtf(a);                                                  // coder.py:141-144
              tl = (ta_loc - 0.0f) / pa_scale;
              ts = ta_scale / pa_scale;
            }
            s_ts[tid] = ts;
            s_tt[tid] = tl / ts;
            s_c[tid] = GC_HL2PI + (float)det_log((double)ts);
          }
          __syncthreads();
#if IREC_GC_WIDE_TILE
          if (tiled) {
            for (int t0 = 0; t0 < CD; t0 += TD) {
              const int nd = CD - t0 < TD ? CD - t0 : TD, n = nd * A.S_pad;       // n <= GC_TILE_FLOATS
              const float *src = row + (size_t)(cb + t0) * S_pad;                 // the tile of the table: n contiguous floats
              // (B1) the float32 terms of the tile (the zero padding of a row included: never read below)
              int dl = t0 + tid / A.S_pad, sl = tid % A.S_pad;
              for (int e = tid; e < n; e += NT) {
                const float x = src[e];
                const float u = x / s_ts[dl] - s_tt[dl];
                const float lt = -0.5f * (u * u) - s_c[dl];
                const float lp = -0.5f * (x * x) - GC_HL2PI;
                s_tile[e] = lt - lp;
                dl += e_q; sl += e_r;
                if (sl >= A.S_pad) { sl -= A.S_pad; ++dl; }
              }
              __syncthreads();
              // (B2) the ordered float64 sums: one lane per sample, the tile's dims in order
              if (s < A.S) {
                const float *colp = s_tile + s;
#pragma unroll 8
                for (int i = 0; i < nd; ++i) acc = acc + (double)colp[(size_t)i * S_pad];
              }
              __syncthreads();
            }
          } else
#endif
          {
            // (B) the plain walk: one lane per sample over the chunk's dims in order
            if (s < A.S) {
              const float *col = row + (size_t)cb * S_pad + s;
#pragma unroll 4
              for (int i = 0; i < CD; ++i) {
                const float x = col[(size_t)i * S_pad];
                const float u = x / s_ts[i] - s_tt[i];
                const float lt = -0.5f * (u * u) - s_c[i];
                const float lp = -0.5f * (x * x) - GC_HL2PI;
                acc = acc + (double)(lt - lp);
              }
            }
            __syncthreads();                    // the chunk's constants are read: the next (A) may overwrite them
          }
        }
        if (s < A.S) {
#if GC_GUMBEL
          const float w = alpha * (float)acc + gum[(size_t)t * S_pad + (size_t)s];   // Gumbel-max (importance_sampling.py:67-72)
#else
          const float w = (float)acc;
#endif
          if (w > best) { best = w; best_s = s; }
        }
      }
      // (C) greatest weight, lowest sample index on ties; a lane without a candidate holds (-FLT_MAX, 0), the accumulator's start
      unsigned long long pk = ((unsigned long long)score_key(best) << 32) | (unsigned long long)(0xFFFFFFFFu - (uint32_t)best_s);
      pk = wave_max_u64(pk);
      if (lane == 0) s_best[wave] = pk;
      __syncthreads();
      pk = s_best[0];
#pragma unroll
      for (int w = 1; w < NT / 64; ++w) { const unsigned long long o = s_best[w]; pk = o > pk ? o : pk; }
      const int j = (int)(0xFFFFFFFFu - (uint32_t)pk);
      if (tid == 0) A.out_indices[blk * (int64_t)A.max_K + t] = j;
      // (D) the chosen sample: the next step's distributions (coder.py:157-171), or the block's sample
      for (int d = tid; d < D; d += NT) {
        const float x = row[(size_t)d * S_pad + (size_t)j];
        const float mq = w_mq[d], sq = w_sq[d], mp = w_mp[d], sp = w_sp[d];
        if (last) {
          A.out_sample[gc_index(A, base, pos, d)] = sp * x + mp;
        } else {
          const float cv = sp * sp, tv = sq * sq, a = rho * cv;
          const float av = sqrtf(a) * x + 0.0f;                                             // pa.scale * x + pa.loc
          w_mq[d] = mp + (av * tv * cv + (mq - mp) * (cv - a) * cv) / (tv * a + cv * (cv - a));
          w_sq[d] = sqrtf(tv * cv * (cv - a) / (a * tv + cv * (cv - a)));
          w_mp[d] = mp + av;
          w_sp[d] = sqrtf(cv - a);
        }
      }
      // (the slab: lane tid alone touches the dims tid + k * 1024, in program order.  s_best: the next write is a step -- at least
      //  one barrier -- away)
    }
    __syncthreads();
  }
}
