// irec_chunk.h -- the chunked encoder, for blocks of more than 1024 dims: encode_chunk_kernel, the shape table that picks its build and
// the launcher template.  Included by the two translation units that instantiate it: irec_chunk.hip (one team per block: the product
// builds) and irec_chunk_gang.hip (the GANG builds: several teams per block).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include "irec_device.h"
#include "irec_kernels.h"
#include "irec_fast_common.h"
#include "irec_team_common.h"

#ifndef IREC_GANG_ABLATE
#define IREC_GANG_ABLATE 0   // diagnostics (make variant_gang): phases of a gang step removed -- 1 sample loops, 2 update, 4 reduction, 8 selection,
                             // 32 gang barriers; the outputs are wrong, the time that remains is the point (scripts/gang_latency.py --ablate)
#endif
namespace irec {

// ======================================================================================================
//  encode_chunk_kernel: blocks of MORE than 1024 dims on the team encoder's tables (round 4).
//
//  Coder.__init__ takes any block_size, None included (rec/coding/coder.py:29-36,415-419: the whole latent tensor as ONE
//  block -- the reference's default), and the register-resident encoders (irec_team.hip, irec_ten.hip) hold 1024 dims per block.  Until now such
//  blocks went to encode_generic_kernel (5-10 k latents/s).  Here a team walks the block in CHUNKS of 1024 dims (four dim
//  groups, one per wave, exactly the lane ownership of the canonical tree) twice per step:
//    scoring   per chunk: the step's constants from the slab's statistics and cumulative variance (the IEEE chain of
//              coder.py:141-154), G and the C_b terms of the live beams from the beams in the slab, then every sample x beam
//              over the chunk -- three table copies, copy bits of choice_table_rows, as in encode_team_kernel -- into the
//              per-group partials; a combine adds the chunk's group sums to the RUNNING score of every candidate in
//              increasing group order, which is the specification's order ("group sums are added in increasing
//              group order"), so the bits are encode_generic_kernel's;
//    update    per chunk: the selected parents and proposal rows -> new beams into the slab's other buffer.
//  A (chunk, dim group) is read and written by ONE wave in both phases: no cross-wave traffic through global memory, the
//  only shared state is the team's LDS (partials, running scores / keys, selection).  Two teams per CU at 256 VGPRs for up to 20
//  beams; one team (beam passes of 10 / 16) for 30 / 32 beam slots, whose partials take the LDS of two.
//  Slab of a team: stats [3][Dpad] | cvar [2][Dpad] (by step parity) | sa [Dpad] | beams [2][NB][Dpad] | bp [max_K][NB].
//
//  Gangs (GANG builds, round 5): a call of FEWER blocks than team slots -- block_size = None on one image's latents: one block of 8192
//  dims would keep one team of one CU busy for 21 ms while 255 CUs idle.  G = A.coop_W teams, each on a CU of its own where the grid allows,
//  code a block together: G = GC chunk owners x SP sample stripes; member m owns the chunks m % GC, + GC, ... (statistics, step constants,
//  update: nothing of a chunk ever leaves its member but its group sums; the SP stripes of a chunk repeat that work, each in its own slab)
//  and scores the sample-chunks m / GC, + SP, ... of them.  Per step: every member writes the group sums of its chunks and samples to the
//  block's exchange in HBM; gang barrier;
//  member m forms the canonical sums -- all group sums of a candidate in increasing group order: the same float32 chain the
//  one-team form adds chunk by chunk -- of the candidates m, m + G, ..., and publishes their sort keys; gang barrier; every member reads
//  all keys and runs the same selection.  The bits are the one-team form's (and the generic kernel's); the K of the block comes the same
//  way from the group sums of its KL.  Members wait for each other: all n_blocks * G teams must be resident (one static hand-out slot
//  each), a member that waits 100 ms for partners that are not poisons the block's counter and the block is reported not coded (-2).
// ======================================================================================================
constexpr int CHUNK_MAX_DIM = 1 << 22;   // (= the bound of irec_beam_encode's max_block_dim; the host caps the scratch slabs of huge blocks)
__host__ __device__ inline size_t chunk_ws_bytes(int NB, int dpad, int max_K) {
  return (size_t)(6 + 2 * NB) * dpad * 4 + ((((size_t)(max_K > 0 ? max_K : 1) * NB * 4) + 255) & ~(size_t)255);
}
__host__ __device__ inline size_t chunk_lds_one(int NB, int NBP, int S) {   // part [4][S][NBP] (of ONE beam pass) | run / keys [S][NB] | TeamLds | barrier
  return team_part_bytes(NBP, S) + team_key_bytes(NB, S) + team_small_bytes(NB) + 16;
}
__host__ __device__ inline size_t chunk_lds_total(int NB, int NBP, int S, int teams) { return T3_BYTES + (size_t)teams * chunk_lds_one(NB, NBP, S); }

// NB beam slots; NBP beams per scoring PASS (the G of NBP beams is what a wave holds in registers: NB = 30 scores a chunk in three passes
// of 10 beams, NB = 32 in two of 16 -- the chunk's step constants are formed once, its rows are re-read per pass); TEAMS per workgroup.
// Round 5: the steady-state scoring is the team encoder's software pipeline (the look-ups of the next dim slot in flight under the
// current slot's fma, accumulators in register pairs, reduce_scatter_20 where 20 values are reduced together); any D; steps beyond the
// proposal tables draw their rows in the kernel (plain scoring form), so no block of a chunked call is left to a second pass;
// the partials are those of ONE pass (combined into the running scores pass by pass), so three teams of 10-beam passes -- 12 waves
// per CU at 168 VGPRs, the register budget G of 10 beams fits without a spill -- find room next to the table copies; up to 60 beam slots
// (passes of 10, two teams: 32 < B <= 60 of blocks beyond 1024 dims no longer falls to the generic kernel).
template <int NB, int NBP, int TEAMS, bool GANG = false>
__global__ __launch_bounds__(TEAMS * TEAM_NT, 1) void encode_chunk_kernel(EncArgs A) {
  using TeamLds = TeamLdsT<NB>;
  constexpr int TEAM_MB = team_mb(NB);
  constexpr size_t TEAM_SMALL_BYTES = (sizeof(TeamLds) + 15) & ~(size_t)15;
  constexpr int NT = TEAM_NT;
  constexpr int SPC = NBP <= 10 ? 20 / NBP : 1;    // samples per reduce-scatter
  constexpr int RW = NBP * SPC;                    // accumulators reduced together
  static_assert(NB % NBP == 0 && (NBP == 10 || NBP == 16 || NBP == 20) && NB <= 60, "chunked encoder: passes of 10, 16 or 20 beams, at most 60 beam slots (6-bit back-pointers)");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int S = A.S, B = A.B;
  const int lane = threadIdx.x & 63;
  const int wave_wg = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int team = wave_wg / TEAM_NW, g = wave_wg % TEAM_NW;                    // wave g of a team owns dim group g of every chunk
  const int tid = (int)threadIdx.x - team * NT;
  char *tbase = smem + T3_BYTES + (size_t)team * chunk_lds_one(NB, NBP, S);
  float *part_s = reinterpret_cast<float *>(tbase);                             // [4][S][NBP] of the beam pass being scored
  float *run_s = reinterpret_cast<float *>(tbase + team_part_bytes(NBP, S));    // [S * Bcur] running scores, then the sort keys
  uint32_t *key_s = reinterpret_cast<uint32_t *>(run_s);
  TeamLds *sm = reinterpret_cast<TeamLds *>(tbase + team_part_bytes(NBP, S) + team_key_bytes(NB, S));
  uint32_t *bar_word = reinterpret_cast<uint32_t *>(tbase + team_part_bytes(NBP, S) + team_key_bytes(NB, S) + TEAM_SMALL_BYTES);
  double *gpart = sm->gpart;
  int32_t *sel_s = sm->sel_s, *sel_b = sm->sel_b;
  int32_t *hsum = &sm->hsum[0][0];
  uint32_t *beta4 = &sm->beta4[0][0];
  int32_t *misc = sm->misc;
  float *cpart_s = &sm->cpart[0][0];
  float *Cb_s = sm->Cb;
  const uint16_t *dlog_s = A.dlog4r;
  const int rs_p = rsn_owner<RW>(lane), rs_c = rsn_owner<NBP>(lane);
  const int rs_p20 = RW == 20 ? rs20_owner(lane) : -1;
  double *kl_tot = reinterpret_cast<double *>(sm->wb);                          // running KL total of the prologue (wb is idle then)

  if ((uint32_t)(uintptr_t)(__attribute__((address_space(3))) char *)smem != 0u) __builtin_trap(); // see lds_abs_f32
  commit_table_stamps(A);
  {
    float *l3 = reinterpret_cast<float *>(smem);
    for (int k = (int)threadIdx.x; k < (int)IREC_PM1; k += TEAMS * NT) {
      const float v = A.lut2[k];
      l3[k] = v; l3[k + IREC_PM1] = v; l3[k + 2 * IREC_PM1] = v;
    }
    if (tid == 0) *bar_word = 0u;
  }
  __syncthreads();
  TeamBarrier tsync{bar_word, 0u, (uint32_t)TEAM_NW};

  const int Dpad = A.max_dim_pad;
  char *slab = A.ws + ((size_t)blockIdx.x * TEAMS + team) * A.ws_per_wg;
  float *stats_g = reinterpret_cast<float *>(slab);                 // [3][Dpad]: mq - mp, sq^2, sp^2
  float *cvar_g = stats_g + (size_t)3 * Dpad;                       // [2][Dpad]: cumulative variance, by step parity
  float *sa_g = cvar_g + (size_t)2 * Dpad;                          // [Dpad]: this step's sample scale
  float *beams_g = sa_g + Dpad;                                     // [2][NB][Dpad]
  int32_t *bp = reinterpret_cast<int32_t *>(beams_g + (size_t)2 * NB * Dpad);   // [max_K][NB]

  const int64_t n_static = (int64_t)TEAMS * (int64_t)gridDim.x < A.n_blocks ? (int64_t)TEAMS * (int64_t)gridDim.x : A.n_blocks;
  bool first_block = true;
  int steal = 0;
  // GANG: the G = A.coop_W teams in hand-out slots [blk * G, blk * G + G) code block blk together -- member gm owns the chunks gm, gm + G, ...
  // of it (see "gangs" above the kernel); a team takes its one slot of the static round and leaves
  // The G members are GC chunk owners x SP sample stripes: member gm owns the chunks gc = gm % GC, gc + GC, ... and scores the samples of
  // sample-chunk sp = gm / GC, sp + SP, ... of them (statistics, step constants, G and the update of a chunk are repeated by its SP stripes,
  // each in its own slab; the group sums of a candidate still come from ONE member each).
  constexpr int ABL = GANG ? IREC_GANG_ABLATE : 0;
  const int G = GANG ? A.coop_W : 1;
  const int GC = GANG ? A.gang_chunks : 1, SP = GANG ? G / GC : 1;
  uint32_t gang_epoch = 0u;
  for (;;) {
    tsync();
    if (tid == 0) {
      int64_t r;
      if constexpr (GANG) {
        const int64_t slot = (int64_t)team * (int64_t)gridDim.x + (int64_t)blockIdx.x;
        r = first_block && slot < A.n_blocks * (int64_t)G ? slot / G : A.n_blocks;
        misc[2] = (int32_t)(slot % G);
      } else if (first_block) {
        r = (int64_t)team * (int64_t)gridDim.x + (int64_t)blockIdx.x;
        r = r < n_static ? xcd_static_row(r, n_static, (int)gridDim.x) : A.n_blocks;
      } else r = xcd_pull_row(A, n_static, A.n_blocks, steal);
      misc[0] = (int32_t)r;
    }
    first_block = false;
    tsync();
    const int64_t blk = misc[0];
    if (blk >= A.n_blocks) break; // every wave of the team reaches this
    const int gm = GANG ? misc[2] : 0;
    const int gc = gm % GC, sp = gm / GC;
    if (GANG && A.coop_test_orphan && gm != 0) break;   // IREC_FLAG_TEST_SPLIT_ORPHAN: member 0 waits alone, gives up, reports -2
    const int D = A.block_dim[blk];
    const int64_t base = A.block_base[blk];
    const int32_t pos = A.block_pos[blk];
    const uint16_t *tab = nullptr;
#pragma unroll
    for (int q = 0; q < 4; ++q)
      if (A.tab_dim[q] == D) tab = A.tab[q];
    if (D < 1 || D > Dpad || tab == nullptr) { // host promised D <= max_block_dim and listed dims
      if (tid == 0) A.out_K[blk] = -1;
      continue;
    }
    const int Dp = (D + 3) & ~3;            // row stride of the proposal table
    const int NC = (D + 1023) >> 10;        // chunks of 1024 dims
    auto groups_of = [&](int c) { const int left = D - (c << 10); return left >= 1024 ? 4 : (left + 255) >> 8; };
    // ---- gang exchange of this block (GANG only; layout: gang_xch_bytes, irec_kernels.h) ----
    const int NGt = (D + 255) >> 8;                                // dim groups of the block: the terms of every canonical sum, in order
    const int NGm = 4 * ((Dpad + 1023) >> 10);                     // row stride of the exchange (groups of the call's largest block)
    const int NCAND = S * NB;
    float *gx_part = nullptr, *gx_cpart = nullptr;
    unsigned long long *gx_kl = nullptr;
    uint32_t *gx_keys = nullptr;
    unsigned int *gang_ctr = nullptr;
    if constexpr (GANG) {
      char *xb = A.gang_xch + (size_t)blk * A.gang_stride;
      gx_part = reinterpret_cast<float *>(xb);                     // [S * NB][NGm]: group sums of every candidate, candidate-major
      gx_cpart = gx_part + (size_t)NCAND * NGm;                    // [NB][NGm]: group sums of the C_b terms
      gx_kl = reinterpret_cast<unsigned long long *>(gx_cpart + (size_t)NB * NGm);   // [NGm] doubles: group sums of the KL
      gx_keys = reinterpret_cast<uint32_t *>(gx_kl + NGm);         // [S * NB] sort keys of the step
      gang_ctr = reinterpret_cast<unsigned int *>(A.coop_xch) + (size_t)blk * (COOP_KEYS * 2);   // first word of the block's exchange granules in the
                                                                                             // workspace head: zeroed by the call's preparation kernel
    }
    // Barrier of the gang: a monotonic arrival counter in HBM.  Everything handed over travels as agent-scope (sc1) stores that have
    // drained before the arrival (s_waitcnt vmcnt(0) in every wave, then the team barrier, then one arrival) and is read back by agent-scope loads.  A member
    // that has waited COOP_GIVE_UP_TICKS for partners that are not resident POISONS the counter (bit 31, by compare-and-swap against an
    // incomplete count, so that either every member passes a barrier or none does) and the block is reported as not coded (out_K = -2).
    auto gsync = [&]() -> bool {
      if constexpr ((ABL & 32) != 0) { tsync(); return true; }
      gang_epoch += (uint32_t)G;
      // every wave drains its stores before the team barrier: the release fence in there is workgroup-scoped and need not wait for
      // vector-memory stores to be acknowledged (the waves of a workgroup share their L1), but the partners of the gang sit on other CUs
      // and must find the sums in place once the arrival below is visible.
      // Why this is enough on gfx950, and why it is asm and not the memory model (round 6, scripts/microbench/litmus.hip, profiles/r06r/):
      //   * everything handed over is written by agent-scope stores (global_store .. sc1: written through to the memory side that all XCDs
      //     share) and read by agent-scope loads (global_load .. sc1: not served from a stale L1 / L2 line);
      //   * vmcnt counts a store down when the memory side has ACKNOWLEDGED it, so after s_waitcnt vmcnt(0) the wave's data is where every
      //     agent-scope load finds it; the team barrier then orders the four waves' drains before thread 0's arrival (LDS counter);
      //   * the arrival itself is a relaxed agent-scope RMW on one word: whoever sees it, sees it after the acknowledgements.
      //   The memory model says the same with an agent-scope release fence in every wave and an acquire fence behind the wait; that form
      //   passes the litmus too (form 2m) and costs 3 x the hand-off (47 against 16 us for 16 KB under light load, 76 against 58 under
      //   heavy): buffer_wbl2 + buffer_inv sc1 write back and invalidate the whole L2 for data that never was in it.
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      tsync();
      if (tid == 0) {
        int32_t bad = 0;
        __hip_atomic_fetch_add(gang_ctr, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
        for (uint32_t turn = 1;; ++turn) {
          const uint32_t v = __hip_atomic_load(gang_ctr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          if (v >> 31) { bad = 1; break; }
          if ((int32_t)(v - gang_epoch) >= 0) break;
          __builtin_amdgcn_s_sleep(2);
          if ((turn & 63u) == 0u && __builtin_amdgcn_s_memrealtime() - t0 > COOP_GIVE_UP_TICKS) {
            uint32_t expect = v;
            if (__hip_atomic_compare_exchange_strong(gang_ctr, &expect, v | 0x80000000u, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) {
              __hip_atomic_store(A.coop_err, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
              bad = 1; break;
            }
          }
        }
        misc[6] = bad;
      }
      tsync();
      return misc[6] == 0;
    };
    auto ld_f32 = [](const float *p_) { return __uint_as_float(__hip_atomic_load(reinterpret_cast<const uint32_t *>(p_), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)); };
    auto st_f32x2 = [](float *p_, float a_, float b_) {   // (8-byte aligned)
      __hip_atomic_store(reinterpret_cast<unsigned long long *>(p_), (unsigned long long)__float_as_uint(a_) | ((unsigned long long)__float_as_uint(b_) << 32),
                         __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    };
    // Canonical sums of `nrows` exchange rows (NGt terms each, increasing group order), staged through the partial buffer: all threads
    // fetch a range of groups of up to NT rows, one thread per row adds the range onto its running value in order.
    // src(i): the row's base; sink(i, v): what to do with its sum.
    auto gang_reduce = [&](int nrows, auto src, auto sink) {
      float *stage = part_s;
      const int CAP = 4 * S * NBP;
      const int TI = NT < CAP ? NT : CAP;
      for (int r0 = 0; r0 < nrows; r0 += TI) {
        const int nr = nrows - r0 < TI ? nrows - r0 : TI;
        int GR = CAP / nr;
        if (GR > NGt) GR = NGt;
        float v = 0.f;
        for (int g0 = 0; g0 < NGt; g0 += GR) {
          const int ng = NGt - g0 < GR ? NGt - g0 : GR;
          for (int e = tid; e < nr * ng; e += NT) { const int i = e / ng, gi = e - i * ng; stage[e] = ld_f32(src(r0 + i) + g0 + gi); }
          tsync();
          if (tid < nr) {
            const float *p_ = stage + tid * ng;
            int gi = 0;
            if (g0 == 0) { v = p_[0]; gi = 1; }
            for (; gi < ng; ++gi) v = v + p_[gi];
          }
          tsync();
        }
        if (tid < nr) sink(r0 + tid, v);
      }
      tsync();
    };
    bool gang_lost = false;

    // ---- statistics (split == gather through perm) and the block's KL, groups in increasing order ----
    for (int c = gc; c < NC; c += GC) {
      const int ngc = groups_of(c);
      const int d0 = (c << 10) + g * 256 + lane * 4;
      double klacc = 0.0;
      if (g < ngc) {
        float st3[3][4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          st3[0][i] = 0.f; st3[1][i] = 1.f; st3[2][i] = 1.f;
          if (d0 + i < D) {
            const int64_t ixi = src_index(A, base, pos, d0 + i);
            const float mq_ = A.q_loc[ixi], sq_ = A.q_scale[ixi], mp_ = A.p_loc[ixi], sp_ = A.p_scale[ixi];
            klacc = klacc + kl_dim(mq_, sq_, mp_, sp_);
            st3[0][i] = mq_ - mp_; st3[1][i] = sq_ * sq_; st3[2][i] = sp_ * sp_;
          }
        }
#pragma unroll
        for (int k = 0; k < 3; ++k)
          *reinterpret_cast<float4 *>(stats_g + (size_t)k * Dpad + d0) = make_float4(st3[k][0], st3[k][1], st3[k][2], st3[k][3]);
        *reinterpret_cast<float4 *>(cvar_g + d0) = make_float4(0.f, 0.f, 0.f, 0.f);
      }
      const double gs = wave_tree_sum(klacc);
      if constexpr (GANG) {
        if (g < ngc && lane == 0 && sp == 0) __hip_atomic_store(gx_kl + c * 4 + g, (unsigned long long)__double_as_longlong(gs), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        continue;
      }
      if (g < ngc && lane == 0) gpart[g] = gs;
      tsync();
      if (tid == 0) {
        double tot = c == 0 ? gpart[0] : *kl_tot + gpart[0];
        for (int gg = 1; gg < ngc; ++gg) tot = tot + gpart[gg];
        *kl_tot = tot;
      }
      tsync();
    }
    if constexpr (GANG) {   // the group sums of every member, added in group order by every member
      if (!gsync()) { if (tid == 0) A.out_K[blk] = -2; continue; }
      double *stage = reinterpret_cast<double *>(part_s);
      const int CAPD = 2 * S * NBP;
      double tot = 0.0;
      for (int g0 = 0; g0 < NGt; g0 += CAPD) {
        const int ng = NGt - g0 < CAPD ? NGt - g0 : CAPD;
        for (int e = tid; e < ng; e += NT) stage[e] = __longlong_as_double((long long)__hip_atomic_load(gx_kl + g0 + e, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
        tsync();
        if (tid == 0) {
          int gi = 0;
          if (g0 == 0) { tot = stage[0]; gi = 1; }
          for (; gi < ng; ++gi) tot = tot + stage[gi];
        }
        tsync();
      }
      if (tid == 0) *kl_tot = tot;
    }
    if (tid == 0) {
      const int32_t K = num_aux((float)*kl_tot, A.omega);
      misc[1] = K;
      if (gm == 0) A.out_K[blk] = K;
      hsum[0] = 0;
      beta4[0] = 0u; // hash of the empty path is 1 = g^0
    }
    tsync();
    const int K = misc[1];
    if (K > A.max_K || K > A.K_limit) continue;
    // (steps beyond the table window -- K grows with the dims: 2 200 partitions for a 301 056-dim block -- draw their rows in the kernel, below)
    if (K == 0) { // nothing to code: sample = p.loc
      for (int c = gc; sp == 0 && c < NC; c += GC) {
        const int d0 = (c << 10) + g * 256 + lane * 4;
#pragma unroll
        for (int i = 0; i < 4; ++i)
          if (g < groups_of(c) && d0 + i < D) { const int64_t ixo = src_index(A, base, pos, d0 + i); A.out_sample[ixo] = 0.f + A.p_loc[ixo]; }
      }
      continue;
    }

    int cur = 0, Bcur = 1;
    uint32_t bv_cur = 0u;                                            // lane j: 4 * dlog(hash(path of beam j))
    for (int t = 0; t < K; ++t) {
      const bool fused = t >= A.K_tab;                               // beyond the proposal tables: the rows are drawn here
      const uint16_t *tab_tu = tab + (size_t)(fused ? 0 : t) * S * Dp; // this step's rows (fused: never read)
      const StepSeed ss = make_step_seed(A.seed + t);
      // Row of sample s_ for the quad at dim q0 (a multiple of 4) of a step beyond the tables: the int32 draw of get_pseudo_random_sample
      // itself (beam_search_coder.py:38-43) mapped to discrete logs, copy bit 0 -- the table's format, random banks (8.9 instead of
      // 13.7 look-ups/clk/CU, and a Philox block per quad and sample on the VALU: the regime of blocks no window can hold).
      auto fused_row = [&](int s_, uint32_t q0) {
        uint32_t rm1[4];
        draw_rm1_x4(ss, (uint64_t)s_ * (uint64_t)D + (uint64_t)q0, rm1);   // ((s_ * D + q0) & 3 is wave-uniform: q0 % 4 == 0)
        uint32_t a_[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) a_[i] = (uint32_t)dlog_s[rm1[i]] >> 2;
        return make_uint2(a_[0] | (a_[1] << 16), a_[2] | (a_[3] << 16));
      };
      const float rho = A.rho[K - 1 - t];
      const int N = S * Bcur;
      // ---------------- scoring, chunk by chunk (beam_search_coder.py:67-84) ----------------
      for (int c = gc; c < NC; c += GC) {
        const int ngc = groups_of(c);
        const int d0 = (c << 10) + g * 256 + lane * 4;
        const bool mine = g < ngc;                                    // (wave-uniform) this dim group exists in the chunk
        // the step's constants of my four dims (coder.py:141-154), from the statistics and the cumulative variance in the slab
        float sa[4] = {0.f, 0.f, 0.f, 0.f}, cH[4] = {0.f, 0.f, 0.f, 0.f}, m[4] = {0.f, 0.f, 0.f, 0.f}, cA[4] = {0.f, 0.f, 0.f, 0.f}, cBv[4] = {0.f, 0.f, 0.f, 0.f};
        if (mine) {
          float cn[4];
          {
            const float4 q0 = *reinterpret_cast<const float4 *>(stats_g + d0);
            const float4 q1 = *reinterpret_cast<const float4 *>(stats_g + (size_t)Dpad + d0);
            const float4 q2 = *reinterpret_cast<const float4 *>(stats_g + (size_t)2 * Dpad + d0);
            const float4 qc = *reinterpret_cast<const float4 *>(cvar_g + (size_t)(t & 1) * Dpad + d0);
            const float dmu_[4] = {q0.x, q0.y, q0.z, q0.w}, vq_[4] = {q1.x, q1.y, q1.z, q1.w}, vp_[4] = {q2.x, q2.y, q2.z, q2.w};
            const float c_[4] = {qc.x, qc.y, qc.z, qc.w};
#pragma unroll
            for (int i = 0; i < 4; ++i) {
              const bool ok = d0 + i < D;
              const StepConst sc = step_constants(rho, dmu_[i], vq_[i], vp_[i], c_[i]);
              sa[i] = ok ? sc.sa : 0.f; cH[i] = ok ? sc.H : 0.f;
              m[i] = ok ? sc.m : 0.f; cA[i] = ok ? sc.A : 0.f; cBv[i] = ok ? sc.Bv : 0.f;
              cn[i] = c_[i] + sc.a;                                    // cumulative_auxiliary_variance += auxiliary_var (:109)
              __builtin_amdgcn_sched_barrier(0);
            }
            *reinterpret_cast<float4 *>(cvar_g + (size_t)((t + 1) & 1) * Dpad + d0) = make_float4(cn[0], cn[1], cn[2], cn[3]);
            *reinterpret_cast<float4 *>(sa_g + d0) = make_float4(sa[0], sa[1], sa[2], sa[3]);
          }
        }
        const uint32_t tab_lo = (uint32_t)(d0 < Dp ? d0 : Dp - 4);   // lanes past the row's end: its last quad (zero coefficients)
        const uint16_t *tab_t = tab_tu + tab_lo;
#pragma unroll 1
        for (int bp0 = 0; bp0 < NB; bp0 += NBP) {                    // beam passes (one for NB = NBP)
          const int nlive = Bcur - bp0 < NBP ? Bcur - bp0 : NBP;     // live beams of this pass
          if (nlive <= 0) break;                                     // (uniform over the team)
          if (mine) {
            // G and the C_b terms of the pass's live beams (dead slots: G = 0, never read)
            float G[NBP][4];
            {
              float cacc[rsn_room(NBP)];
#pragma unroll
              for (int b = 0; b < rsn_room(NBP); ++b) cacc[b] = 0.f;
              const float *bold = beams_g + ((size_t)cur * NB + bp0) * Dpad + d0;
              float4 bq[NBP];
#pragma unroll
              for (int b = 0; b < NBP; ++b) {
                bq[b] = make_float4(0.f, 0.f, 0.f, 0.f);
                if (t && b < nlive) bq[b] = *reinterpret_cast<const float4 *>(bold + (size_t)b * Dpad);   // (wave-uniform)
              }
#pragma unroll
              for (int b = 0; b < NBP; ++b) {
                const float bv4[4] = {bq[b].x, bq[b].y, bq[b].z, bq[b].w};
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                  G[b][i] = b < nlive ? beam_G(bv4[i], m[i], cA[i], cBv[i], sa[i]) : 0.f;
                  if (b < nlive) cacc[b] = beam_C_term(cacc[b], bv4[i], m[i], cA[i], cBv[i]);
                }
              }
              const float ctot = reduce_scatter_n<NBP>(cacc, lane);
              if ((lane & 1) == 0 && rs_c >= 0 && rs_c < nlive) cpart_s[g * TEAM_MB + bp0 + rs_c] = ctot;
            }
            uint32_t bet[NBP];
#pragma unroll
            for (int b = 0; b < NBP; ++b) bet[b] = (uint32_t)__builtin_amdgcn_readlane((int)bv_cur, bp0 + b < Bcur ? bp0 + b : 0);
            if (nlive == NBP && Bcur > 1 && !fused) {
              // ---- steady state, software pipelined by dim slot (as encode_team_kernel's scoring loop): the NBP look-ups of the NEXT slot are
              // issued before the current slot's values are consumed; values in register pairs (v_pk_fma_f32); rows two sample-chunks ahead
              typedef float f2 __attribute__((ext_vector_type(2)));
              constexpr int NP = NBP / 2, NQ = 4 * SPC;
              const int n_sch = (S + SPC - 1) / SPC;
              auto row = [&](int s_) {
                uint2 r = make_uint2(0u, 0u);
                if (s_ < S) r = *reinterpret_cast<const uint2 *>(tab_tu + ((uint32_t)s_ * (uint32_t)Dp + tab_lo));
                return r;
              };
              uint2 ap_cur[SPC], ap_nxt[SPC];
#pragma unroll
              for (int cc = 0; cc < SPC; ++cc) { ap_cur[cc] = row(sp * SPC + cc); ap_nxt[cc] = row((sp + SP) * SPC + cc); }
#define CHUNK_AL(CC, I) ((((I) & 2) ? (((I) & 1) ? (ap_cur[CC].y >> 16) : (ap_cur[CC].y & 0xFFFFu)) : (((I) & 1) ? (ap_cur[CC].x >> 16) : (ap_cur[CC].x & 0xFFFFu))) << 2)
#define CHUNK_ISSUE(Z, AD) do { _Pragma("unroll") for (int k = 0; k < NP; ++k) { Z[k].x = lds_abs_f32((AD) + bet[2 * k]); Z[k].y = lds_abs_f32((AD) + bet[2 * k + 1]); } \
                                __builtin_amdgcn_sched_barrier(0); } while (0)
#define CHUNK_CONSUME(Z, I, ACC) do { _Pragma("unroll") for (int k = 0; k < NP; ++k) asm volatile("" : "+v"(Z[k])); \
                                f2 t2_[NP]; \
                                _Pragma("unroll") for (int k = 0; k < NP; ++k) { \
                                  const f2 h2 = {cH[I], cH[I]}, g2 = {G[2 * k][I], G[2 * k + 1][I]}; \
                                  t2_[k] = __builtin_elementwise_fma(h2, Z[k], g2); } \
                                _Pragma("unroll") for (int k = 0; k < NP; ++k) ACC[k] = __builtin_elementwise_fma(t2_[k], Z[k], ACC[k]); \
                                _Pragma("unroll") for (int k = 0; k < NP; ++k) asm volatile("" : "+v"(ACC[k])); \
                                __builtin_amdgcn_sched_barrier(0); } while (0)
              f2 zz[2][NP];
              CHUNK_ISSUE(zz[0], CHUNK_AL(0, 0));
              for (int ch = sp; ch < ((ABL & 1) ? 0 : n_sch); ch += SP) {          // (my stripe of the sample-chunks; SP = 1 but in gangs)
                f2 acc2[SPC][NP];
#pragma unroll
                for (int cc = 0; cc < SPC; ++cc)
#pragma unroll
                  for (int k = 0; k < NP; ++k) acc2[cc][k] = (f2){0.f, 0.f};
                uint2 ap_new[SPC];
#pragma unroll
                for (int cc = 0; cc < SPC; ++cc) ap_new[cc] = row((ch + 2 * SP) * SPC + cc);
#pragma unroll
                for (int q = 0; q < NQ; ++q) {
                  if (q + 1 < NQ) CHUNK_ISSUE(zz[(q + 1) & 1], CHUNK_AL((q + 1) >> 2, (q + 1) & 3));
                  else {
#pragma unroll
                    for (int cc = 0; cc < SPC; ++cc) { ap_cur[cc] = ap_nxt[cc]; ap_nxt[cc] = ap_new[cc]; }
                    CHUNK_ISSUE(zz[0], CHUNK_AL(0, 0));
                  }
                  CHUNK_CONSUME(zz[q & 1], q & 3, acc2[q >> 2]);
                }
                float tot;
                int own;
                if constexpr (RW == 20) {
                  rs_f2 a20[10];
#pragma unroll
                  for (int cc = 0; cc < SPC; ++cc)
#pragma unroll
                    for (int k = 0; k < NP; ++k) a20[cc * NP + k] = acc2[cc][k];
                  tot = reduce_scatter_20(a20, lane);
                  own = rs_p20;
                } else {
                  float acc[rsn_room(RW)];
#pragma unroll
                  for (int cc = 0; cc < SPC; ++cc)
#pragma unroll
                    for (int k = 0; k < NP; ++k) { acc[cc * NBP + 2 * k] = acc2[cc][k].x; acc[cc * NBP + 2 * k + 1] = acc2[cc][k].y; }
                  tot = reduce_scatter_n<RW>(acc, lane);
                  own = rs_p;
                }
                const int cc = own / NBP, b = own - cc * NBP;          // own < 0: unused slot
                const int s_ = ch * SPC + cc;
                if (own >= 0 && (lane & 1) == 0 && s_ < S) part_s[((size_t)g * S + s_) * NBP + b] = tot;
              }
#pragma unroll
              for (int k = 0; k < NP; ++k) asm volatile("" : "+v"(zz[0][k])); // drain the look-ups issued past the last sample
#undef CHUNK_AL
#undef CHUNK_ISSUE
#undef CHUNK_CONSUME
            } else {
              // ---- the first step (one beam) and passes that are not full: a dim slot's look-ups issued together, then consumed
              const int nchunks = (S + SPC - 1) / SPC;
              uint2 alp_next[SPC];
#pragma unroll
              for (int cc = 0; cc < SPC; ++cc) {
                alp_next[cc] = make_uint2(0u, 0u);
                const int s0 = sp * SPC + cc;
                if (s0 < S) alp_next[cc] = fused ? fused_row(s0, tab_lo) : *reinterpret_cast<const uint2 *>(tab_t + (size_t)s0 * Dp);
              }
              for (int ch = sp; ch < ((ABL & 1) ? 0 : nchunks); ch += SP) {
                float acc[rsn_room(RW)];
#pragma unroll
                for (int p_ = 0; p_ < rsn_room(RW); ++p_) acc[p_] = 0.f;
                uint2 alp[SPC];
#pragma unroll
                for (int cc = 0; cc < SPC; ++cc) {
                  alp[cc] = alp_next[cc];
                  const int sn = (ch + SP) * SPC + cc;
                  if (sn < S) alp_next[cc] = fused ? fused_row(sn, tab_lo) : *reinterpret_cast<const uint2 *>(tab_t + (size_t)sn * Dp);
                }
#pragma unroll
                for (int cc = 0; cc < SPC; ++cc) {
                  const int s_ = ch * SPC + cc;
                  if (s_ < S) { // wave-uniform
                    const uint2 ap = alp[cc];
                    const uint32_t al[4] = {(ap.x & 0xFFFFu) << 2, (ap.x >> 16) << 2, (ap.y & 0xFFFFu) << 2, (ap.y >> 16) << 2};
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                      float z[NBP];
#pragma unroll
                      for (int b = 0; b < NBP; ++b) z[b] = lds_abs_f32(al[i] + bet[b]);   // 4 * (dlog r + 10006 c + dlog h): no wrap
#pragma unroll
                      for (int b = 0; b < NBP; ++b) acc[cc * NBP + b] = proposal_term(acc[cc * NBP + b], z[b], cH[i], G[b][i]);
                      __builtin_amdgcn_sched_barrier(0);
                    }
                  }
                }
                const float tot = reduce_scatter_n<RW>(acc, lane);
                const int cc = rs_p / NBP, b = rs_p - cc * NBP;         // rs_p < 0: unused slot
                const int s_ = ch * SPC + cc;
                if (rs_p >= 0 && (lane & 1) == 0 && s_ < S && b < nlive) part_s[((size_t)g * S + s_) * NBP + b] = tot;
              }
            }
          }
          tsync();
          if constexpr (GANG) {   // the pass's group sums of this chunk: to the gang's exchange, four groups of a candidate side by side
            for (int f = tid; f < S * nlive; f += NT) {
              const int s_ = f / nlive, bl = f - s_ * nlive;
              if ((s_ / SPC) % SP != sp) continue;                     // (another stripe's sample)
              float *row = gx_part + (size_t)(s_ * Bcur + bp0 + bl) * NGm + c * 4;
              float v4[4];
#pragma unroll
              for (int gg = 0; gg < 4; ++gg) v4[gg] = gg < ngc ? part_s[((size_t)gg * S + s_) * NBP + bl] : 0.f;
              st_f32x2(row, v4[0], v4[1]); st_f32x2(row + 2, v4[2], v4[3]);
            }
            if (tid < nlive && sp == 0) {
              const int b = bp0 + tid;
              float *row = gx_cpart + (size_t)b * NGm + c * 4;
              float v4[4];
#pragma unroll
              for (int gg = 0; gg < 4; ++gg) v4[gg] = gg < ngc ? cpart_s[gg * TEAM_MB + b] : 0.f;
              st_f32x2(row, v4[0], v4[1]); st_f32x2(row + 2, v4[2], v4[3]);
            }
            tsync();   // partials free for the next pass / chunk
            continue;
          }
          // the pass's group sums of this chunk onto the running scores / C_b of its beams, increasing group order
          for (int f = tid; f < S * nlive; f += NT) {
            const int s_ = f / nlive, bl = f - s_ * nlive;
            const int fr = s_ * Bcur + bp0 + bl;                       // flat candidate index of (sample, beam)
            float v = part_s[((size_t)0 * S + s_) * NBP + bl];
            if (c > 0) v = run_s[fr] + v;
            for (int gg = 1; gg < ngc; ++gg) v = v + part_s[((size_t)gg * S + s_) * NBP + bl];
            run_s[fr] = v;
          }
          if (tid < nlive) {
            const int b = bp0 + tid;
            float cb = cpart_s[b];
            if (c > 0) cb = Cb_s[b] + cb;
            for (int gg = 1; gg < ngc; ++gg) cb = cb + cpart_s[gg * TEAM_MB + b];
            Cb_s[b] = cb;
          }
          tsync();   // partials free for the next pass / chunk; running sums and C_b published
        }
      }
      if constexpr (GANG) {
        // every group sum of the step is out: C_b of every beam by every member, the scores of the candidates gm, gm + G, ... by member gm
        // (the terms of each in increasing group order: the canonical sums), their sort keys to the exchange, all keys back
        if (!gsync()) { gang_lost = true; break; }
        const int n_mine = gm < N ? (N - gm + G - 1) / G : 0;
        const bool cb_all = n_mine >= Bcur;                       // (else: only the C_b of my candidates' beams)
        const int n_cb = cb_all ? Bcur : n_mine;
        auto cb_of = [&](int i) { return cb_all ? i : (gm + i * G) % Bcur; };
        if constexpr ((ABL & 4) == 0)
        gang_reduce(n_cb + n_mine,
                    [&](int i) { return i < n_cb ? gx_cpart + (size_t)cb_of(i) * NGm : gx_part + (size_t)(gm + (i - n_cb) * G) * NGm; },
                    [&](int i, float v) { if (i < n_cb) Cb_s[cb_of(i)] = v; else run_s[i - n_cb] = v; });
        for (int i = tid; i < n_mine; i += NT) {
          const int f = gm + i * G;
          __hip_atomic_store(gx_keys + f, score_key(run_s[i] + Cb_s[f % Bcur]), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        if (!gsync()) { gang_lost = true; break; }
        for (int f = tid; f < N; f += NT) key_s[f] = __hip_atomic_load(gx_keys + f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      } else {
        for (int f = tid; f < N; f += NT) {
          const int s_ = f / Bcur, b = f - s_ * Bcur;
          key_s[f] = score_key(run_s[f] + Cb_s[b]);
        }
      }
      const int Bnew = B < N ? B : N;
      // top-B (beam_search_coder.py:85-89); the selection's first barrier orders the key writes
      if constexpr ((ABL & 8) != 0) {
        tsync();
        if (tid < Bnew) { sel_s[tid] = tid % S; sel_b[tid] = tid % Bcur; sm->sel_bo[tid] = beta4[cur * TEAM_MB + tid % Bcur];
                          hsum[(cur ^ 1) * TEAM_MB + tid] = 0; bp[(size_t)t * NB + tid] = ((tid % S) << 6) | (tid % Bcur); }
        tsync();
      } else
      select_topB_sync<NT>(key_s, N, Bnew, Bcur, sm, tid, tsync, nullptr, [&](int j, int32_t sp_, int32_t bp_, uint32_t) {
        const int32_t nh = (int32_t)((uint32_t)hsum[cur * TEAM_MB + bp_] + (uint32_t)sp_ * (uint32_t)(69 + t));
        hsum[(cur ^ 1) * TEAM_MB + j] = nh;
        sm->sel_bo[j] = beta4[cur * TEAM_MB + bp_];
        bp[(size_t)t * NB + j] = (sp_ << 6) | bp_;
      });
      // ---------------- new beams, chunk by chunk (beam_search_coder.py:92-93) ----------------
      const bool last = (t == K - 1);
      uint32_t bv_new;
      {
        const int32_t nh = hsum[(cur ^ 1) * TEAM_MB + (lane < Bnew ? lane : 0)];
        bv_new = dlog_s[hash_from_sum(nh) - 1u];
      }
      const int Bupd = last ? 1 : ((ABL & 2) ? 0 : Bnew);     // beams[0] is all that leaves the block (:118-122)
      const int32_t v_sp = sel_s[lane < Bnew ? lane : 0], v_bp = sel_b[lane < Bnew ? lane : 0];
      const uint32_t v_bo = sm->sel_bo[lane < Bnew ? lane : 0];
      for (int c = gc; c < NC; c += GC) {
        const int d0 = (c << 10) + g * 256 + lane * 4;
        if (g >= groups_of(c)) continue;     // wave-uniform
        const uint32_t tab_lo = (uint32_t)(d0 < Dp ? d0 : Dp - 4);
        const uint16_t *tab_t = tab_tu + tab_lo;
        const float4 sq = *reinterpret_cast<const float4 *>(sa_g + d0);
        const float sa_t[4] = {sq.x, sq.y, sq.z, sq.w};
        const float *bold = beams_g + (size_t)cur * NB * Dpad + d0;
        float *bnew = beams_g + (size_t)(cur ^ 1) * NB * Dpad + d0;
        constexpr int UB = 5;                // beams per load batch
#pragma unroll 1
        for (int j0 = 0; j0 < Bupd; j0 += UB) {
          uint2 apv[UB];
          float4 obv4[UB];
          uint32_t bet_old[UB];
#pragma unroll
          for (int u = 0; u < UB; ++u) {
            const int j = j0 + u;
            apv[u] = make_uint2(0u, 0u); obv4[u] = make_float4(0.f, 0.f, 0.f, 0.f); bet_old[u] = 0u;
            if (j < Bupd) { // wave-uniform
              const int32_t sp_ = __builtin_amdgcn_readlane(v_sp, j);
              const int32_t bp_ = __builtin_amdgcn_readlane(v_bp, j);
              bet_old[u] = (uint32_t)__builtin_amdgcn_readlane((int)v_bo, j);
              apv[u] = fused ? fused_row(sp_, tab_lo) : *reinterpret_cast<const uint2 *>(tab_t + (size_t)sp_ * Dp);
              if (t) obv4[u] = *reinterpret_cast<const float4 *>(bold + (size_t)bp_ * Dpad);
            }
          }
#pragma unroll
          for (int u = 0; u < UB; ++u) {
            const int j = j0 + u;
            if (j < Bupd) { // wave-uniform
              const uint32_t al[4] = {(apv[u].x & 0xFFFFu) << 2, (apv[u].x >> 16) << 2, (apv[u].y & 0xFFFFu) << 2, (apv[u].y >> 16) << 2};
              const float obv[4] = {obv4[u].x, obv4[u].y, obv4[u].z, obv4[u].w};
              float nb[4];
#pragma unroll
              for (int i = 0; i < 4; ++i) {
                const float y = sa_t[i] * lds_abs_f32(al[i] + bet_old[u]);   // dist.quantile(.), :48-49
                nb[i] = obv[i] + y;                                          // combined_samples[best_ind_aux, best_ind_beam], :81,92-93
              }
              if (last) {
#pragma unroll
                for (int i = 0; i < 4; ++i)
                  if (d0 + i < D && sp == 0) { // beams[0] + coding_dist.loc, :122
                    const int64_t ixo = src_index(A, base, pos, d0 + i);
                    A.out_sample[ixo] = nb[i] + A.p_loc[ixo];
                  }
              } else {
                *reinterpret_cast<float4 *>(bnew + (size_t)j * Dpad) = make_float4(nb[0], nb[1], nb[2], nb[3]);
              }
            }
          }
        }
      }
      if (tid < Bnew) beta4[(cur ^ 1) * TEAM_MB + tid] = bv_new;   // (wave 0: read by its own next selection)
      bv_cur = bv_new;
      cur ^= 1;
      Bcur = Bnew;
    }
    // ---- index path of beam 0 (beam_search_coder.py:118-121) ----
    tsync();
    if (gang_lost) {                           // partners not resident: the block is not coded (the caller codes the call again, IREC_FLAG_NO_SPLIT)
      if (tid == 0) A.out_K[blk] = -2;
      continue;
    }
    if (tid == 0 && gm == 0) {
      int j = 0;
      for (int t = K - 1; t >= 0; --t) {
        const int32_t v = __builtin_nontemporal_load(&bp[(size_t)t * NB + j]);
        A.out_indices[blk * (int64_t)A.max_K + t] = v >> 6;
        j = v & 63;
      }
    }
  }
}

// ---- chunked encoder (blocks of more than 1024 dims) ----
// The build that serves B beams and S samples: beam slots, beams per scoring pass, teams per workgroup -- the first of the candidates
// whose LDS fits next to the table copies (three teams only with passes of 10 beams: 168 VGPRs hold the G of ten, not of twenty).
struct ChunkShape { int nb, nbp, teams; };
static int chunk_nb(int B) { return B <= 10 ? 10 : B <= 20 ? 20 : B <= 30 ? 30 : B <= 32 ? 32 : B <= 40 ? 40 : B <= 50 ? 50 : B <= 60 ? 60 : 0; }
static ChunkShape chunk_shape(int B, int S) {
  // (round 6: {20, 20, 2} -- passes of twenty beams on two teams -- could never be chosen: wherever its LDS fits (S <= 49), that of {20, 10, 3}
  //  before it in the list does too (S <= 52); the planner enumeration of tests/test_kernel_coverage.py found it, the build is gone)
  static const ChunkShape cand[] = {{10, 10, 3}, {10, 10, 2}, {10, 10, 1}, {20, 10, 3}, {20, 10, 1},
                                    {30, 10, 3}, {30, 10, 2}, {30, 10, 1}, {32, 16, 2}, {32, 16, 1},
                                    {40, 10, 2}, {40, 10, 1}, {50, 10, 2}, {50, 10, 1}, {60, 10, 2}, {60, 10, 1}};
  const int nb = chunk_nb(B);
  if (!nb || (int64_t)S * nb > 4096) return ChunkShape{0, 0, 0};
  for (const ChunkShape &c : cand)
    if (c.nb == nb && chunk_lds_total(c.nb, c.nbp, S, c.teams) <= FAST_LDS_LIMIT) return c;
  return ChunkShape{0, 0, 0};
}
template <int NB, int NBP, int TEAMS, bool GANG = false>
static hipError_t launch_chunk_t(const EncArgs &A, int grid, hipStream_t st) {
  const size_t lds = chunk_lds_total(NB, NBP, A.S, TEAMS);
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(encode_chunk_kernel<NB, NBP, TEAMS, GANG>),
                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL((encode_chunk_kernel<NB, NBP, TEAMS, GANG>), dim3(grid), dim3(TEAMS * TEAM_NT), lds, st, A);
  return hipGetLastError();
}

} // namespace irec
