// irec_team.hip -- the default gfx950 encoder: independent TEAMS of waves inside one workgroup per CU, all of them looking
// up ONE shared set of three quantile-table copies in LDS.
//
// Hot path (reference file:line): BeamSearchCoder.encode_block rec/coding/beam_search_coder.py:53-122, as in
// irec_kernels.hip; the arithmetic specification and therefore every emitted bit are the same.
//
// What is different is how the look-up  z = quantile((r * hash) mod 10007 / 10007) = lut2[(dlog r + dlog hash) mod 10006]
// reaches the LDS (scripts/microbench/gather_rates.hip):
//   * a random 4-byte gather costs a 32-lane group as many LDS cycles as the busiest of the 32 banks has distinct
//     addresses (3.5 on average) -- the 8.9 look-ups/clk/CU ceiling the one-table encoders sit under;
//   * here the table is stored THREE times back to back (120 KB, shared by every team of the CU).  Entry
//     e = alpha' + beta with alpha' = dlog r + 10006 c, c in {0, 1}, beta = dlog hash never leaves the three copies, so
//     the address is ONE add (no "mod 10006"), and bank(e) = (dlog r + 22 c + beta) mod 32: the copy bit c moves a
//     lane by 22 banks whatever the beam.  c is chosen once per call for every (step, sample, 32-lane group, dim
//     slot) by the call's preparation kernel (choice_table_rows, irec_prep.hip) -- an exact min-max assignment on two 16-rings of banks -- and travels inside the
//     proposal table the block kernel streams anyway.  Busiest bank: 2.15 addresses instead of 3.5.
//   * one workgroup owns the CU; its teams code blocks independently (own block counter pulls, own LDS scratch, own
//     scratch slab) and synchronise with team barriers (an LDS counter), never with s_barrier, so one team's serial
//     phases (top-B, beam update) overlap the other teams' scoring.
// Around the steady-state scoring loop (r02i, DESIGN.md §4 "Outside the steady state"): the first step (one beam) reduces RW
// SAMPLES per reduce-scatter instead of one; the last step forms beam 0 only; the loop's 20-value reduce-scatter runs on the
// accumulator pairs with bank-masked DPP adds (reduce_scatter_20, irec_fast_common.h); rows are fetched a chunk ahead.
// Shapes (team_shape() at the end of the file): B <= 10: three 4-wave teams (two if the LDS is short); B <= 20: three 4-wave
// teams at 168 VGPRs -- the BASELINE workload (two at 256 VGPRs for calls of one to two blocks per CU); 20 < B <= 32, or
// B <= 20 with more samples than one scoring pass holds: ONE team whose waves split the beams into stripes (12 waves x 10
// beams, 8 x 16, 8 x 10) and that scores the samples in passes.
// The LDS geometry (team_s_pass, team_lds_total, ...) is in irec_team_common.h; blocks of more than 1024 dims take encode_chunk_kernel
// (irec_chunk.h), which walks them on the same tables.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <stdint.h>
#include <stdio.h>
#include <type_traits>

#include "irec_device.h"
#include "irec_kernels.h"
#include "irec_fast_common.h"
#include "irec_team_common.h"

#ifndef IREC_PK_ADDR
#define IREC_PK_ADDR 1          // scoring loop: look-up addresses of a beam pair by one v_pk_add_f32 (0: two v_add_u32; A/B builds)
#endif
namespace irec {

// Diagnostic build (-DIREC_TEAM_STAMPS, scripts/gpu_stamps.sh): per-wave cycle sums per phase, written once at exit.
#ifdef IREC_TEAM_STAMPS
#define TSTAMP(slot) do { const unsigned long long now_ = __builtin_amdgcn_s_memtime(); st_acc[slot] += now_ - st_prev; st_prev = now_; } while (0)
#else
#define TSTAMP(slot) do { } while (0)
#endif

// Lane swaps (irec_kernels.h): first dim of the quad that lane `lane` of dim group g holds at step t of a block of table slot q
__device__ __forceinline__ int swapped_quad_dim(const EncArgs &A, int q, int t, int g, int lane) {
  int l = lane;
  if (A.lane_swaps && t < SWAP_STEPS) {
    const uint32_t msk = (uint32_t)__builtin_amdgcn_readfirstlane((int)swap_masks_of(A.ws_head)[(q * SWAP_STEPS + t) * 4 + g]);
    l ^= (int)((msk >> (lane & 31)) & 1u) << 5;
  }
  return g * 256 + l * 4;
}

// LDS carve (bytes): lut2 x 3 [120080] | team 0: part [4][S][NB] f32 | sort keys [S*NB] | TeamLds | barrier | team 1: same
// BS = beam stripes: with BS == 2 a team has 8 waves, wave w serves dim group / sample stripe (w & 3) and the beams
// [NBW * (w >> 2), + NBW), NBW = NB / BS: half the G registers per lane (128-VGPR budget, 16 waves per CU).
// PASSES: a multi-team build that scores the S samples of a step in several passes and may keep its sort keys in the slab
// (the single-team builds always can): S beyond what a team's share of the LDS holds -- the reference's sweep reaches
// S = int(e^9) = 8103 (examples/lossless/data_aggregation.py:5-7).
// ONE: the build of one-beam calls (B = 1 of the reference's sweep): every step takes the wide path, which is therefore the
// pipelined form (rows a half batch ahead, two samples per v_pk_fma_f32) -- in the other builds only step 0 comes there and
// the extra row buffers cost registers everywhere else (r03e A/B: B = 32 -14 %, B = 30 -2 %, B = 10 -3 % with it).
// SHARE: the build of calls whose rows beyond one per CU are shared between teams (A.coop_W > 1, below) -- its own instantiation:
// the exchange code costs the two-team builds their spill-free register allocation (r04: <20,2,1> 80 -> 400 B of scratch with it).
// MARGIN (round 5): the build behind irec_beam_encode_ex / IREC_FLAG_MARGINS -- after every selection wave 0 also takes the gap between
// the last candidate kept and the best one rejected (margin_step, irec_fast_common.h) and the block leaves four floats in
// A.out_margin; one team barrier more per step.  Instantiated in its own translation unit (irec_team_margin.hip) for the shapes the
// BASELINE configurations run; every other call with margins takes the generic kernel.  Same indices and samples, bit for bit.
template <int NB, int TEAMS, int BS, bool PASSES = false, bool ONE = false, bool SHARE = false, bool MARGIN = false>
__global__ __launch_bounds__(TEAMS * BS * TEAM_NT, 1) void encode_team_kernel(EncArgs A) {
  using TeamLds = TeamLdsT<NB>;
  constexpr int TEAM_MB = team_mb(NB);
  constexpr size_t TEAM_SMALL_BYTES = (sizeof(TeamLds) + 15) & ~(size_t)15;
  constexpr bool MULTI_PASS = TEAMS == 1 || PASSES;
  constexpr bool SHORT = TEAMS * BS >= 3 && NB / BS == 20;   // 12 waves per CU x 20 beams per wave: the 168-VGPR builds
  constexpr int NW = TEAM_NW;                    // waves per beam stripe (dim groups x sample stripes)
  constexpr int NWT = TEAM_NW * BS, NT = 64 * NWT; // waves / threads per team
  constexpr int NBW = NB / BS;                   // beams per wave
  static_assert(NB % BS == 0, "beam stripes must divide the beam count");
  // 20 accumulators are reduced together (one sample x 20 beams, or two samples x 10 beams) by the 20-value
  // reduce-scatter: 22 exchange+add pairs instead of the 31 of a zero-padded 32-wide one, and 12 registers fewer
  static_assert(NBW == 10 || NBW == 16 || NBW == 18 || NBW == 20, "the team encoder is built for 10, 16, 18 or 20 beams per wave");
  static_assert(NB <= TEAM_MB && NB <= 64, "beam indices are lane indices and 6-bit back-pointers");
  constexpr int CMAX = TEAMS == 1 ? 2048 : 1024;    // candidates one combine round covers (host: SP * NB <= CMAX)
  constexpr int SPC = BS >= 2 ? 1 : 20 / NBW;   // samples per chunk (beam-striped builds: one, to fit 128 VGPRs)
  constexpr int RW = NBW * SPC;                  // accumulators reduced together
  constexpr int ACC_ROOM = rsn_room(RW);
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int S = A.S, B = A.B;
  const int lane = threadIdx.x & 63;
  const int wave_wg = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)); // wave-uniform by construction
  const int team = wave_wg / NWT, wave_t = wave_wg % NWT;
  const int wave = wave_t & 3, bs = wave_t >> 2;                                // quad position, beam stripe
  const int b_lo = bs * NBW;                                                    // first beam of my stripe
  const int tid = (int)threadIdx.x - team * NT;                                 // index inside the team
  // samples scored per pass: only the single-team builds take more than one pass (the host checked that the others fit
  // S in one -- then the pass loop below folds away)
  const int PS = NB == 10 ? team_row(NB, B) : NB;                              // beam slots per sample row (1 for a one-beam call)
  const int SP = MULTI_PASS ? team_s_pass(NB, S, TEAMS, CMAX, PASSES, PS) : S;
  const bool keys_lds = !MULTI_PASS || team_keys_in_lds(NB, S, TEAMS, PASSES, PS); // (compile-time true for the one-pass multi-team builds)
  constexpr bool KEYS_ALIAS = TEAMS >= 3 && NB == 20 && !PASSES;               // team_keys_alias()
  const size_t key_lds_bytes = (keys_lds && !KEYS_ALIAS) ? team_key_bytes(PS, S) : 0;
  char *tbase = smem + T3_BYTES + (size_t)team * team_lds_one(NB, S, SP, TEAMS, PASSES, PS);
  float *part_s = reinterpret_cast<float *>(tbase);                             // [4][SP][PS] per-group partial scores
  TeamLds *sm = reinterpret_cast<TeamLds *>(tbase + team_part_bytes(PS, SP) + key_lds_bytes);
  uint32_t *bar_word = reinterpret_cast<uint32_t *>(tbase + team_part_bytes(PS, SP) + key_lds_bytes + TEAM_SMALL_BYTES);
  double *gpart = sm->gpart;
  int32_t *sel_s = sm->sel_s, *sel_b = sm->sel_b;
  int32_t *hsum = &sm->hsum[0][0];
  uint32_t *beta4 = &sm->beta4[0][0];
  int32_t *misc = sm->misc;
  float *cpart_s = &sm->cpart[0][0];
  const uint16_t *dlog_s = A.dlog4r;                                            // [10006] 4*dlog(j+1), global (L2)
  const int rs_p = rsn_owner<RW>(lane);                                         // accumulator whose total reduce_scatter_n<20> leaves here
  const int rs_p20 = RW == 20 ? rs20_owner(lane) : -1;                          // same for the scoring loop's reduce_scatter_20
  const int rs_c = rsn_owner<NBW>(lane);                                        // same for the NBW C_b partials of the update

  if ((uint32_t)(uintptr_t)(__attribute__((address_space(3))) char *)smem != 0u) __builtin_trap(); // see lds_abs_f32
  commit_table_stamps(A);
  constexpr bool CAN_SHARE = SHARE && TEAMS >= 2 && BS == 1 && !PASSES && !ONE;
  const int Wsh = (CAN_SHARE && A.coop_W > 1) ? A.coop_W : 1;
  const int64_t n_whole = Wsh > 1 ? (A.tsplit_first < A.n_blocks ? A.tsplit_first : A.n_blocks) : A.n_blocks;
  const int64_t n_slots = n_whole + (A.n_blocks - n_whole) * Wsh;
  const int64_t n_static = (int64_t)TEAMS * (int64_t)gridDim.x < n_slots ? (int64_t)TEAMS * (int64_t)gridDim.x : n_slots;
  // Cost-ordered hand-out (round 4; A.row_cost: distinct keys (K * dims) << 10 | row from the call's preparation kernel, set by the host only
  // when the static round deals every slot): slot u < lo = min(grid, n_whole) is the row of ascending cost rank u, slot lo + k the row
  // of rank n_blocks - 1 - k / W -- a workgroup's first team gets a cheap row, its other teams (or the teams that share a row) the
  // costliest ones, longest first.  Every workgroup ranks the rows itself, once, in the LDS the table copies are about to fill
  // (one row per thread, n compares each: ~2 us): no second kernel, no grid-wide wait.
  constexpr bool CAN_PLACE = NB == 20 && TEAMS == 2 && BS == 1 && !PASSES && !ONE;   // (team_placeable(): the builds the host asks it of)
  // (n_static == n_slots: the static round deals every slot, which the ranking below assumes -- the host only sets row_cost then
  //  (irec_host.cpp); should a later change break that, the rows are dealt as listed instead of the slots beyond the static round being lost)
  const bool placed = CAN_PLACE && A.row_cost != nullptr && n_static == n_slots;
  const int64_t lo_rank = (int64_t)gridDim.x < n_whole ? (int64_t)gridDim.x : n_whole;
  int32_t placed_row = -1;
  if (placed) {
    uint32_t *cs = reinterpret_cast<uint32_t *>(smem);
    const int n = (int)A.n_blocks;
    for (int k = (int)threadIdx.x; k < n; k += TEAMS * NT) cs[k] = A.row_cost[k];
    if ((int)threadIdx.x < TEAMS) cs[n + (int)threadIdx.x] = 0xFFFFFFFFu;
    int want[TEAMS];
#pragma unroll
    for (int tm = 0; tm < TEAMS; ++tm) {
      const int64_t u = (int64_t)tm * (int64_t)gridDim.x + (int64_t)blockIdx.x;
      want[tm] = u >= n_static ? -1 : u < lo_rank ? (int)u : n - 1 - (int)((u - lo_rank) / (u < n_whole ? 1 : Wsh));
    }
    __syncthreads();
    for (int i = (int)threadIdx.x; i < n; i += TEAMS * NT) {
      const uint32_t ci = cs[i];
      int rk = 0;
#pragma unroll 8
      for (int j = 0; j < n; ++j) rk += cs[j] < ci ? 1 : 0;
#pragma unroll
      for (int tm = 0; tm < TEAMS; ++tm)
        if (rk == want[tm]) cs[n + tm] = (uint32_t)i;
    }
    __syncthreads();
    placed_row = (int32_t)cs[n + team];
    __syncthreads();   // (the table copies overwrite the keys)
  }
  {
    float *l3 = reinterpret_cast<float *>(smem);
    for (int k = (int)threadIdx.x; k < (int)IREC_PM1; k += TEAMS * NT) {
      const float v = A.lut2[k];
      l3[k] = v; l3[k + IREC_PM1] = v; l3[k + 2 * IREC_PM1] = v;
    }
    if (tid == 0) *bar_word = 0u;
  }
  __syncthreads(); // the only workgroup-wide barrier: from here on the teams never wait for each other
  TeamBarrier tsync{bar_word, 0u, (uint32_t)NWT};

  char *slab = A.ws + ((size_t)blockIdx.x * TEAMS + team) * A.ws_per_wg;
  const size_t key_glb_bytes = keys_lds ? 0 : ((team_key_bytes(PS, S) + 255) & ~(size_t)255);   // sort keys at the slab's end
  uint32_t *key_s = KEYS_ALIAS ? reinterpret_cast<uint32_t *>(tbase)                            // over partial group 0
                    : keys_lds ? reinterpret_cast<uint32_t *>(tbase + team_part_bytes(PS, SP))     // [S*PS] sort keys
                               : reinterpret_cast<uint32_t *>(slab + A.ws_per_wg - key_glb_bytes);
  int32_t *bp = reinterpret_cast<int32_t *>(slab);                                            // [max_K][NB]
  float *beams_g = reinterpret_cast<float *>(slab + A.ws_per_wg - key_glb_bytes - (size_t)2 * NB * FAST_MAX_DIM * 4); // [2][NB][1024]
  float *stats_g = beams_g - 3 * FAST_MAX_DIM;  // [3][1024]: mq - mp, sq^2, sp^2 of the block, coalesced
  float *park_g = stats_g - 2 * FAST_MAX_DIM;   // [2][1024]: c (cumulative variance) and sa of the PARK builds
  // Three-team builds have 168 VGPRs: the cumulative variance and the sample scale (needed only by the update) are parked
  // in the slab across the scoring loop instead of being spilled inside it
  constexpr bool PARK = SHORT;
  // Lane swaps (irec_kernels.h): in the builds that park their per-dim state in the slab every value a lane holds for its dims makes a
  // round trip through the slab once per step, so the lane -> quad map may differ from step to step at no cost: lane l of dim group g
  // holds quad l ^ 32 where bit l & 31 of the step's mask (A.lane_swaps) is set.  The first level of every lane tree adds lanes
  // l and l ^ 32 (commutative bit for bit), so no total moves; the preparation kernel picks the masks that spread the look-ups best.
  constexpr bool SWAP = PARK && !SHARE && !MARGIN;
  constexpr bool LATE_G = false;   // (tried: new beams wait in G's registers and G is formed after the batches -- the
                                   //  register allocator then shuffles eight registers through scratch per beam: 844 B)

#ifdef IREC_TEAM_STAMPS
  unsigned long long st_acc[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  unsigned long long st_prev = __builtin_amdgcn_s_memtime();
  const unsigned long long st_t0 = st_prev, st_r0 = __builtin_amdgcn_s_memrealtime();   // shader clock = d(memtime) / d(memrealtime) x 100 MHz
#endif
  // Block hand-out: the first block of team k of workgroup w is k * gridDim.x + w -- a call of fewer blocks than resident
  // teams (a mid-size batch: 38 images x 9 blocks) puts ONE block on every CU before any CU gets a second one, instead of
  // three on the first third of the CUs; later blocks come from the atomic counter, which starts behind the static ones.
  // Both rounds deal the rows of a tensor to one XCD (irec_fast_common.h: xcd_static_row / xcd_pull_row).
  // Shared blocks (round 4; calls of one to two blocks per CU): the rows from A.tsplit_first on are coded by A.coop_W teams EACH --
  // anywhere on the chip -- that split the row's SAMPLES: team q of a row scores the samples of stripe q, publishes their sort
  // keys as tagged granules (the split encoder's exchange, irec_kernels.hip), sweeps its partners' and then runs the same
  // selection and the same update as they do, on its own slab: nothing but keys is shared.  A 342-block call then loads a CU
  // with one whole block and a fraction of another instead of two whole ones.  Hand-out slots: one per whole row, coop_W per
  // shared row; the host sizes coop_W so that the static round deals every slot (all partners resident at once).
  bool first_block = true;
  int steal = 0;
  for (;;) {
    tsync();
    if (tid == 0) {
      int64_t r;
      if (first_block) {
        r = (int64_t)team * (int64_t)gridDim.x + (int64_t)blockIdx.x;
        r = r < n_static ? (placed ? r : xcd_static_row(r, n_static, (int)gridDim.x)) : n_slots;
      } else r = placed ? n_slots : xcd_pull_row(A, n_static, n_slots, steal);
      misc[0] = (int32_t)r;
      misc[6] = 0;                          // (shared rows: a partner gave up)
    }
    first_block = false;
    tsync();
    const int64_t slot = misc[0];
    TSTAMP(0);
    if (slot >= n_slots) break; // every wave of the team reaches this; the other team drains on its own
    int64_t blk = slot < n_whole ? slot : n_whole + (slot - n_whole) / Wsh;
    const int64_t xrow = slot < n_whole ? 0 : (slot - n_whole) / Wsh;        // exchange slot of a shared row
    const int qsh = slot < n_whole ? 0 : (int)((slot - n_whole) % Wsh);      // my sample stripe of a shared row
    const int Wrow = slot < n_whole ? 1 : Wsh;                               // teams that code this row
    if (placed) {
      blk = placed_row;
      if (blk < 0 || blk >= A.n_blocks) __builtin_trap();   // (the cost keys are distinct: their ranks are a permutation of the rows)
    }
    if (Wrow > 1 && A.coop_test_orphan && qsh != 0) continue;                // test hook: team 0 of a shared row is left waiting
    const int D = A.block_dim[blk];
    const int64_t base = A.block_base[blk];
    const int32_t pos = A.block_pos[blk];
    const uint16_t *tab = nullptr;
    int tab_q = 0;                          // (SWAP builds: the slot's masks)
#pragma unroll
    for (int q = 0; q < 4; ++q)
      if (A.tab_dim[q] == D) { tab = A.tab[q]; tab_q = q; }
    if (D < 1 || D > FAST_MAX_DIM || tab == nullptr) { // host promised D <= 1024 and listed dims
      if (tid == 0 && qsh == 0) A.out_K[blk] = -1;
      continue;
    }
    const int Dp = (D + 3) & ~3;            // row stride of the proposal table
    const int NG = (D + 255) >> 8;          // 1..4 dim groups
    const int NSW = NW / NG;                // sample stripes
    const bool active = wave < NG * NSW;
    const int g = wave % NG, sw = wave / NG;
    const int NSWe = NSW * Wrow, swe = sw * Wrow + qsh;   // ... of the row over all the teams that code it: my samples are swe, swe + NSWe, ...
    // first dim of my quad (SWAP builds: d0 and valid[] move with the step's mask; everywhere else they never change)
    std::conditional_t<SWAP, int, const int> d0 = g * 256 + lane * 4;
    if constexpr (SWAP) d0 = swapped_quad_dim(A, tab_q, 0, g, lane);

    // ---- my 4 dims (split == gather through perm) and the block's KL ----
    float c[4];
    bool valid[4];
    // the wave that reads a dim group's statistics keeps them in registers; only the other waves of the group (sample /
    // beam stripes of short blocks and of the striped builds) re-read them from the slab every step
    float own_dmu[4], own_vq[4], own_vp[4];
    const bool own_stats = active && sw == 0 && bs == 0 && TEAMS < 3 && !SHORT;   // (168-VGPR builds: the slab keeps them)
    double klacc = 0.0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int d = d0 + i;
      valid[i] = d < D;
      c[i] = 0.f;
      // (the element's index is looked up again when the sample is written: four 64-bit indices per lane are not worth
      // holding, or spilling, across the whole step loop)
      const int64_t ixi = valid[i] ? src_index(A, base, pos, d) : src_index(A, base, pos, 0);
      float st3[3] = {0.f, 1.f, 1.f};
      if (valid[i] && active && sw == 0 && bs == 0) { // one wave per dim group does the float64 KL and publishes the statistics
        const float mq_ = A.q_loc[ixi], sq_ = A.q_scale[ixi], mp_ = A.p_loc[ixi], sp_ = A.p_scale[ixi];
        klacc = klacc + kl_dim(mq_, sq_, mp_, sp_);
        st3[0] = mq_ - mp_; st3[1] = sq_ * sq_; st3[2] = sp_ * sp_;
      }
      own_dmu[i] = st3[0]; own_vq[i] = st3[1]; own_vp[i] = st3[2];
      if (active && sw == 0 && bs == 0 && (NSW > 1 || BS > 1 || TEAMS >= 3)) { // somebody else (or a later step) needs them
        stats_g[d0 + i] = st3[0]; stats_g[FAST_MAX_DIM + d0 + i] = st3[1]; stats_g[2 * FAST_MAX_DIM + d0 + i] = st3[2];
      }
    }
    {
      const double gs = wave_tree_sum(klacc);
      if (sw == 0 && bs == 0 && active && lane == 0) gpart[g] = gs;
      tsync();
      if (tid == 0) {
        double tot = gpart[0];
        for (int gg = 1; gg < NG; ++gg) tot = tot + gpart[gg];
        const int32_t K = num_aux((float)tot, A.omega);
        misc[1] = K;
        if (qsh == 0) A.out_K[blk] = K;
        hsum[0] = 0;
        beta4[0] = 0u; // hash of the empty path is 1 = g^0
        if constexpr (MARGIN) { if (qsh == 0) margin_write(A.out_margin, blk, MarginAcc()); }   // (a block that is not coded here keeps "no comparison")
      }
      tsync();
    }
    const int K = misc[1];
    MarginAcc macc;
    if (K > A.max_K || K > A.K_limit) continue;
    if (K > A.K_tab) { // beyond the table window: the fused-Philox pass codes it
      if (tid == 0 && qsh == 0) atomicAdd(A.defer_count, 1u);
      continue;
    }
    if (K == 0) { // nothing to code: sample = p.loc
      if (active && sw == 0 && bs == 0 && qsh == 0) {
#pragma unroll
        for (int i = 0; i < 4; ++i)
          if (valid[i]) { const int64_t ixo = src_index(A, base, pos, d0 + i); A.out_sample[ixo] = 0.f + A.p_loc[ixo]; }
      }
      continue;
    }

    float sa[4], cH[4];
    float G[NBW][4];
    auto step_consts = [&](int t_next, float (&m)[4], float (&cA)[4], float (&cBv)[4]) {
      const float rho = A.rho[K - 1 - t_next];
      float dmu_[4], vq_[4], vp_[4];
      if (own_stats) { // wave-uniform
#pragma unroll
        for (int i = 0; i < 4; ++i) { dmu_[i] = own_dmu[i]; vq_[i] = own_vq[i]; vp_[i] = own_vp[i]; }
      } else {
        const float4 q0 = *reinterpret_cast<const float4 *>(stats_g + d0);
        const float4 q1 = *reinterpret_cast<const float4 *>(stats_g + FAST_MAX_DIM + d0);
        const float4 q2 = *reinterpret_cast<const float4 *>(stats_g + 2 * FAST_MAX_DIM + d0);
        dmu_[0] = q0.x; dmu_[1] = q0.y; dmu_[2] = q0.z; dmu_[3] = q0.w;
        vq_[0] = q1.x; vq_[1] = q1.y; vq_[2] = q1.z; vq_[3] = q1.w;
        vp_[0] = q2.x; vp_[1] = q2.y; vp_[2] = q2.z; vp_[3] = q2.w;
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const StepConst sc = step_constants(rho, dmu_[i], vq_[i], vp_[i], c[i]);
        sa[i] = valid[i] ? sc.sa : 0.f; cH[i] = valid[i] ? sc.H : 0.f;
        m[i] = valid[i] ? sc.m : 0.f; cA[i] = valid[i] ? sc.A : 0.f; cBv[i] = valid[i] ? sc.Bv : 0.f;
        c[i] = c[i] + sc.a; // cumulative_auxiliary_variance += auxiliary_var (:109)
        __builtin_amdgcn_sched_barrier(0); // one dim at a time: the division sequences are register hungry
      }
    };
    auto park = [&]() {     // (waves of the same dim group write the same bits)
      if (PARK && active) {
        *reinterpret_cast<float4 *>(park_g + d0) = make_float4(c[0], c[1], c[2], c[3]);
        *reinterpret_cast<float4 *>(park_g + FAST_MAX_DIM + d0) = make_float4(sa[0], sa[1], sa[2], sa[3]);
      }
    };
    auto unpark = [&]() {
      if (PARK && active) {
        asm volatile("" ::: "memory");   // a real reload: the values are dead between park() and here
        const float4 pc = *reinterpret_cast<const float4 *>(park_g + d0);
        const float4 ps = *reinterpret_cast<const float4 *>(park_g + FAST_MAX_DIM + d0);
        c[0] = pc.x; c[1] = pc.y; c[2] = pc.z; c[3] = pc.w;
        sa[0] = ps.x; sa[1] = ps.y; sa[2] = ps.z; sa[3] = ps.w;
      }
    };
    // ---- prologue: step 0 has one (all-zero) beam ----
    {
      float m[4], cA[4], cBv[4];
      step_consts(0, m, cA, cBv);
      park();
      float cacc = 0.f;
#pragma unroll
      for (int b = 0; b < NBW; ++b)
#pragma unroll
        for (int i = 0; i < 4; ++i) G[b][i] = 0.f;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        if (bs == 0) G[0][i] = beam_G(0.f, m[i], cA[i], cBv[i], sa[i]);
        cacc = beam_C_term(cacc, 0.f, m[i], cA[i], cBv[i]);
      }
      const float cg = wave_tree_sum(cacc);
      if (active && sw == 0 && bs == 0 && lane == 0) cpart_s[g * TEAM_MB + 0] = cg;
      // (visibility of the C_b partials: the barrier after scoring)
    }

    TSTAMP(1);
    bool abandoned = false;
    int cur = 0, Bcur = 1;
    // 4 * dlog(hash) of the live beams, lane j = beam j: every wave carries its own copy from the update into the next step's
    // scoring (r04: the table look-up behind it is a GLOBAL load; it used to sit inside the one-wave selection, a round trip
    // to the L2 on the path every wave of the team waits on)
    uint32_t bv_cur = 0u;                                            // hash of the empty path is 1 = g^0
    for (int t = 0; t < K; ++t) {
#ifdef IREC_TEAM_STAMPS
      st_acc[11] += 1ull;                                            // (diagnostic build: block-steps of this wave)
#endif
      const uint16_t *tab_tu = tab + (size_t)t * S * Dp;             // uniform base of this step's rows
      // my quad inside a row (32-bit offsets: one VGPR).  Lanes past the padded row end (all their dims invalid, zero
      // coefficients) read the row's LAST quad: finite z, and the same addresses as the last real lane of their 32-lane
      // group -- the LDS serves identical addresses as one broadcast, so they add no bank conflict to the look-ups
      const uint32_t tab_lo = (uint32_t)(d0 < Dp ? d0 : Dp - 4);
      const uint16_t *tab_t = tab_tu + tab_lo;   // (SWAP builds: the update moves it to the next step's quad)
      uint32_t bet[NBW];
      {
#pragma unroll
        for (int b = 0; b < NBW; ++b) bet[b] = (uint32_t)__builtin_amdgcn_readlane((int)bv_cur, b_lo + b);
      }
      const int nlive = Bcur - b_lo < 0 ? 0 : (Bcur - b_lo < NBW ? Bcur - b_lo : NBW);   // live beams of my stripe

      const int N = S * Bcur;
      for (int s_base = 0; s_base < S; s_base += SP) {
      const int s_end = s_base + SP < S ? s_base + SP : S;
      const int Sp = s_end - s_base;                                // samples of this pass
      // ---------------- scoring: samples [s_base, s_end) x Bcur candidates (beam_search_coder.py:80-84) ----------------
#ifdef IREC_ABLATE_SCORING
      if (false) {
#else
      // Steady state: every beam of my stripe alive -- or at least half of them (B = 50 on the 60-beam build: the third stripe
      // holds beams 40..49): the dead ones are scored as PHANTOM beams (G = 0, the address of beam 0: finite values that no
      // candidate ever reads) rather than sending the whole stripe down the beam-by-beam path below.
      if (active && Bcur > 1 && (nlive == NBW || 2 * nlive >= NBW)) {
        // Steady state, software pipelined by dim slot: the NBW gathers of the NEXT slot (of this sample, of the chunk's
        // next sample, or of the next chunk's first sample) are issued before the current slot's values are consumed, so
        // the wave always has look-ups in flight -- also under the fma chain and the reduce-scatter.  A wave can have at
        // most 15 LDS operations outstanding, so by the time the next slot's are issued the current slot's have landed
        // (or the compiler's wait counts see to it).  Empty volatile asm statements pin the order (pure arithmetic would
        // otherwise drift across the scheduling barriers).  A chunk is SPC samples (20 accumulators, one reduce-scatter).
        const int n_mine = Sp > swe ? (Sp - swe + NSWe - 1) / NSWe : 0; // my samples of the pass: s_base + swe, + NSWe, ...
        const int n_chunks = (n_mine + SPC - 1) / SPC;
        auto row = [&](int m) {                                     // proposal row of my m-th sample; zero row past the end:
          uint2 r = make_uint2(0u, 0u);                             // entry 0 is a valid address, its results are dropped
          if (m < n_mine) r = *reinterpret_cast<const uint2 *>(tab_tu + ((uint32_t)(s_base + m * NSWe + swe) * (uint32_t)Dp + tab_lo));
          return r;
        };
        // proposal rows stay packed (4 x uint16 per sample in two registers); the byte address of a dim slot's entry in copy 0
        // is unpacked when its look-ups are issued (one live temporary instead of four registers per sample)
        uint2 ap_cur[SPC], ap_nxt[SPC];
#pragma unroll
        for (int cc = 0; cc < SPC; ++cc) { ap_cur[cc] = row(cc); ap_nxt[cc] = row(SPC + cc); }
#define IREC_AL(CC, I) ((((I) & 2) ? (((I) & 1) ? (ap_cur[CC].y >> 16) : (ap_cur[CC].y & 0xFFFFu)) : (((I) & 1) ? (ap_cur[CC].x >> 16) : (ap_cur[CC].x & 0xFFFFu))) << 2)
        // values travel in register pairs so that the two fma of two beams stay one v_pk_fma_f32 each
        typedef float f2 __attribute__((ext_vector_type(2)));
        constexpr int NP = NBW / 2;
        constexpr int NQ = 4 * SPC;                                 // dim slots per chunk (even: buffers alternate cleanly)
        static_assert(NBW % 2 == 0, "beams are processed in pairs");
        // Pipeline granule: a whole dim slot (NP beam pairs per look-up buffer), or HALF a slot for the three-team
        // 20-beam build (5 pairs per buffer: 20 instead of 40 look-up registers -- three waves per SIMD hide what the
        // shallower pipeline exposes).
        constexpr int NH = SHORT ? 2 : 1;                           // granules per dim slot
        constexpr int HP = NP / NH;                                 // beam pairs per granule
        constexpr int NQH = NQ * NH;                                // granules per chunk
        static_assert(NP % NH == 0 && NQH % 2 == 0, "granules must tile the slots and alternate buffers cleanly");
        f2 zz[2][HP];
#if IREC_PK_ADDR
        // round 6: the two addresses of a beam pair come out of ONE v_pk_add_f32 on their bit patterns -- byte addresses below 2^23 read as
        // float32 are denormals, denormals are preserved (the arithmetic contract needs them), and the sum of two such numbers is exact and
        // carries the integer sum in its bits: half the address instructions (irec_ten.hip has the same)
        f2 betf[NP];
#pragma unroll
        for (int k = 0; k < NP; ++k) betf[k] = (f2){__uint_as_float(bet[2 * k]), __uint_as_float(bet[2 * k + 1])};
#define IREC_ISSUE(Z, AD, K0) do { const float adf_ = __uint_as_float(AD); const f2 ad2_ = {adf_, adf_}; \
                               _Pragma("unroll") for (int k = 0; k < HP; ++k) { const f2 a2_ = ad2_ + betf[(K0) + k]; \
                                 Z[k].x = lds_abs_f32(__float_as_uint(a2_.x)); Z[k].y = lds_abs_f32(__float_as_uint(a2_.y)); } \
                               __builtin_amdgcn_sched_barrier(0); } while (0)
#else
#define IREC_ISSUE(Z, AD, K0) do { _Pragma("unroll") for (int k = 0; k < HP; ++k) { Z[k].x = lds_abs_f32((AD) + bet[2 * ((K0) + k)]); Z[k].y = lds_abs_f32((AD) + bet[2 * ((K0) + k) + 1]); } \
                               __builtin_amdgcn_sched_barrier(0); } while (0)
#endif
#define IREC_CONSUME(Z, I, ACC, K0) do { _Pragma("unroll") for (int k = 0; k < HP; ++k) asm volatile("" : "+v"(Z[k])); \
                                f2 t2_[HP]; \
                                _Pragma("unroll") for (int k = 0; k < HP; ++k) { \
                                  const f2 h2 = {cH[I], cH[I]}, g2 = {G[2 * ((K0) + k)][I], G[2 * ((K0) + k) + 1][I]}; \
                                  t2_[k] = __builtin_elementwise_fma(h2, Z[k], g2); } /* inner fma of every pair first: */ \
                                _Pragma("unroll") for (int k = 0; k < HP; ++k) /* no dependent back-to-back issue */ \
                                  ACC[(K0) + k] = __builtin_elementwise_fma(t2_[k], Z[k], ACC[(K0) + k]); \
                                _Pragma("unroll") for (int k = 0; k < HP; ++k) asm volatile("" : "+v"(ACC[(K0) + k])); \
                                __builtin_amdgcn_sched_barrier(0); } while (0)
        if constexpr (PARK) { // every G of the wave in a register HERE: a spilled one is reloaded once per step, not per sample
#pragma unroll
          for (int b = 0; b < NBW; ++b)
#pragma unroll
            for (int i = 0; i < 4; ++i) asm volatile("" : "+v"(G[b][i]));
        }
        IREC_ISSUE(zz[0], IREC_AL(0, 0), 0);
        for (int ch = 0; ch < n_chunks; ++ch) {
          if constexpr (BS >= 2) {
            // One team, BS waves per SIMD (the stripes' waves of one dim group share a SIMD): the SIMD's arbiter favours its
            // oldest wave, which then reaches the pass's barrier a third of the pass early and leaves the SIMD to two waves,
            // then one (r03g stamps: 20-28 % of every wave's time is that wait).  The favoured stripe rotates instead.
            if ((((ch >> 2) + bs) % BS) == 0) __builtin_amdgcn_s_setprio(1);   // (every four chunks)
            else __builtin_amdgcn_s_setprio(0);
          }
          f2 acc2[SPC][NP];
#pragma unroll
          for (int cc = 0; cc < SPC; ++cc)
#pragma unroll
            for (int k = 0; k < NP; ++k) acc2[cc][k] = (f2){0.f, 0.f};
          uint2 ap_new[SPC];                                        // rows of the chunk after next: a whole chunk of lead
#pragma unroll
          for (int cc = 0; cc < SPC; ++cc) ap_new[cc] = row((ch + 2) * SPC + cc);
#pragma unroll
          for (int qh = 0; qh < NQH; ++qh) {
            constexpr int dummy_ = 0; (void)dummy_;
            const int q = qh / NH, h = qh % NH;                     // dim slot of the chunk, granule of the slot
            if (qh + 1 < NQH) {
              const int qn = (qh + 1) / NH, hn = (qh + 1) % NH;
              IREC_ISSUE(zz[(qh + 1) & 1], IREC_AL(qn >> 2, qn & 3), hn * HP);
            } else {
              // next chunk's rows
#pragma unroll
              for (int cc = 0; cc < SPC; ++cc) { ap_cur[cc] = ap_nxt[cc]; ap_nxt[cc] = ap_new[cc]; }
              IREC_ISSUE(zz[0], IREC_AL(0, 0), 0);
            }
            IREC_CONSUME(zz[qh & 1], q & 3, acc2[q >> 2], h * HP);
          }
          float tot;
          int own;                                                  // value of the chunk whose total this lane ends up with
          if constexpr (RW == 20) {               // the accumulator pairs go in as they are
            rs_f2 a20[10];
#pragma unroll
            for (int cc = 0; cc < SPC; ++cc)
#pragma unroll
              for (int k = 0; k < NP; ++k) a20[cc * NP + k] = acc2[cc][k];
            tot = reduce_scatter_20(a20, lane);
            own = rs_p20;
          } else {
            float acc[ACC_ROOM];
#pragma unroll
            for (int cc = 0; cc < SPC; ++cc)
#pragma unroll
              for (int k = 0; k < NP; ++k) { acc[cc * NBW + 2 * k] = acc2[cc][k].x; acc[cc * NBW + 2 * k + 1] = acc2[cc][k].y; }
            tot = reduce_scatter_n<RW>(acc, lane);
            own = rs_p;
          }
          const int cc = own / NBW, b = own - cc * NBW;            // own < 0: unused slot
          const int m = ch * SPC + cc;                              // my m-th sample
          if (own >= 0 && (lane & 1) == 0 && m < n_mine && b < nlive) part_s[((size_t)g * SP + m * NSWe + swe) * PS + b_lo + b] = tot;
        }
        if constexpr (BS >= 2) __builtin_amdgcn_s_setprio(0);
#pragma unroll
        for (int k = 0; k < HP; ++k) asm volatile("" : "+v"(zz[0][k])); // drain the look-ups issued past the last sample
#undef IREC_ISSUE
#undef IREC_CONSUME
#undef IREC_AL
      } else if (active && Bcur == 1 && bs == 0) {
        // First step (beam_search_coder.py:97-106): ONE beam, so a sample is a single candidate.  Scored beam-wise it would
        // pay a whole reduce-scatter (86 instructions) for 4 look-ups; here RW SAMPLES share one -- a sample sits where a
        // beam sits in the steady state, every total still comes out of the same lane chain and lane tree.  36 samples: two
        // rounds instead of 36 (r02i: step 0 cost half a full step's instructions for a twentieth of its look-ups).
        const int n_mine = Sp > swe ? (Sp - swe + NSWe - 1) / NSWe : 0; // my samples of the pass: s_base + swe, + NSWe, ...
        const uint32_t bet0 = bet[0];
        if constexpr (ONE) {   // (the one-beam builds: every step comes here)
        // two half batches of rows (even sizes: samples go through the fma in pairs), 20 registers as the steady state's
        constexpr int HA = ((RW / 2) + 1) & ~1, HBb = RW - HA;
        static_assert(RW % 2 == 0 && HBb >= 2 && HBb % 2 == 0, "half batches of sample pairs");
        // round 3 (one-beam calls live here for EVERY step): the rows of the next half batch are in flight under the current
        // one's look-ups (they used to be fetched and waited for batch by batch), and two samples share each v_pk_fma_f32
        typedef float f2w __attribute__((ext_vector_type(2)));
        // Row of my m-th sample: a wave-uniform base (scalar arithmetic) plus my quad's byte offset -- no vector address
        // arithmetic per row; past my last sample the LAST row is read again (its totals are dropped at the store).
        const uint32_t lane_off = tab_lo * 2u;
        auto rows = [&](int m_first, auto &ap) {
          constexpr int H = (int)(sizeof(ap) / sizeof(ap[0]));
#pragma unroll
          for (int k = 0; k < H; ++k) {
            int m = m_first + k;
            m = m < n_mine ? m : n_mine - 1;
            const char *rowp = reinterpret_cast<const char *>(tab_tu) + (size_t)((uint32_t)(s_base + m * NSWe + swe) * (uint32_t)Dp) * 2u;
            ap[k] = *reinterpret_cast<const uint2 *>(rowp + lane_off);
          }
        };
        auto half = [&](const auto &ap, f2w *acc2) {
          constexpr int H = (int)(sizeof(ap) / sizeof(ap[0]));
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            float z[H];
#pragma unroll
            for (int k = 0; k < H; ++k) {
              const uint32_t w = (i & 2) ? ap[k].y : ap[k].x;
              const uint32_t e = __builtin_amdgcn_ubfe(w, (i & 1) ? 16u : 0u, 16u);   // v_bfe_u32, then one v_lshl_add_u32 (an
              z[k] = lds_abs_f32((e << 2) + bet0);                  // `& 0xFFFF` is folded into shift + mask + add: three)
            }
            const f2w h2 = {cH[i], cH[i]}, g2 = {G[0][i], G[0][i]};
#pragma unroll
            for (int k = 0; k < H / 2; ++k) {
              const f2w z2 = {z[2 * k], z[2 * k + 1]};
              acc2[k] = __builtin_elementwise_fma(__builtin_elementwise_fma(h2, z2, g2), z2, acc2[k]);   // proposal_term, two samples
            }
            __builtin_amdgcn_sched_barrier(0);
          }
        };
        uint2 apA[HA], apB[HBb];
        rows(0, apA);
        for (int m0 = 0; m0 < n_mine; m0 += RW) {
          f2w acc2[RW / 2];
#pragma unroll
          for (int p = 0; p < RW / 2; ++p) acc2[p] = (f2w){0.f, 0.f};
          rows(m0 + HA, apB);
          half(apA, &acc2[0]);
          rows(m0 + RW, apA);                                       // first half of the next round
          half(apB, &acc2[HA / 2]);
          float tot;
          int own;
          if constexpr (RW == 20) {
            rs_f2 a20[10];
#pragma unroll
            for (int k = 0; k < 10; ++k) a20[k] = acc2[k];
            tot = reduce_scatter_20(a20, lane);
            own = rs_p20;
          } else {
            float acc[ACC_ROOM];
#pragma unroll
            for (int k = 0; k < RW / 2; ++k) { acc[2 * k] = acc2[k].x; acc[2 * k + 1] = acc2[k].y; }
            tot = reduce_scatter_n<RW>(acc, lane);
            own = rs_p;
          }
          const int m = m0 + own;                                   // own < 0: unused slot
          if (own >= 0 && (lane & 1) == 0 && m < n_mine) part_s[((size_t)g * SP + m * NSWe + swe) * PS] = tot;
        }
        } else {   // the round-2 form (builds of more than one beam: only their first step comes here)
          constexpr int HB = RW / 2;                                  // rows fetched together (20 registers, as the steady state's)
          static_assert(RW % 2 == 0, "half batches");
          for (int m0 = 0; m0 < n_mine; m0 += RW) {
            float acc[ACC_ROOM];
#pragma unroll
            for (int p = 0; p < RW; ++p) acc[p] = 0.f;
#pragma unroll
            for (int h = 0; h < 2; ++h) {
              uint2 ap[HB];
#pragma unroll
              for (int k = 0; k < HB; ++k) {
                const int m = m0 + h * HB + k;                        // past my last sample: entry 0, the total is dropped
                ap[k] = make_uint2(0u, 0u);
                if (m < n_mine) ap[k] = *reinterpret_cast<const uint2 *>(tab_tu + ((uint32_t)(s_base + m * NSWe + swe) * (uint32_t)Dp + tab_lo));
              }
#pragma unroll
              for (int i = 0; i < 4; ++i) {
                float z[HB];
#pragma unroll
                for (int k = 0; k < HB; ++k) {
                  const uint32_t w = (i & 2) ? ap[k].y : ap[k].x;
                  z[k] = lds_abs_f32((((i & 1) ? (w >> 16) : (w & 0xFFFFu)) << 2) + bet0);
                }
#pragma unroll
                for (int k = 0; k < HB; ++k) acc[h * HB + k] = proposal_term(acc[h * HB + k], z[k], cH[i], G[0][i]);
                __builtin_amdgcn_sched_barrier(0);
              }
            }
            const float tot = reduce_scatter_n<RW>(acc, lane);
            const int m = m0 + rs_p;                                  // rs_p < 0: unused slot
            if (rs_p >= 0 && (lane & 1) == 0 && m < n_mine) part_s[((size_t)g * SP + m * NSWe + swe) * PS] = tot;
          }
        }
      } else if (active && nlive > 0) {
#endif
        const int s_per_stripe = (Sp + NSWe - 1) / NSWe;
        const int nchunks = (s_per_stripe + SPC - 1) / SPC;
        // proposal rows (4 x uint16: dlog(r) + 10006 c of my dims) are fetched one chunk ahead
        uint2 alp_next[SPC];
#pragma unroll
        for (int cc = 0; cc < SPC; ++cc) {
          const int s0 = cc * NSWe + swe;   // sample index inside the pass
          alp_next[cc] = make_uint2(0u, 0u);
          if (s0 < Sp) alp_next[cc] = *reinterpret_cast<const uint2 *>(tab_t + (size_t)(s_base + s0) * Dp);
        }
        for (int ch = 0; ch < nchunks; ++ch) {
          float acc[ACC_ROOM];
#pragma unroll
          for (int p = 0; p < RW; ++p) acc[p] = 0.f;
          uint2 alp[SPC];
#pragma unroll
          for (int cc = 0; cc < SPC; ++cc) {
            alp[cc] = alp_next[cc];
            const int sn = ((ch + 1) * SPC + cc) * NSWe + swe;
            if (sn < Sp) alp_next[cc] = *reinterpret_cast<const uint2 *>(tab_t + (size_t)(s_base + sn) * Dp);
          }
#pragma unroll
          for (int cc = 0; cc < SPC; ++cc) {
            const int s = (ch * SPC + cc) * NSWe + swe;   // sample index inside the pass
            if (s < Sp) { // wave-uniform
              const uint2 ap = alp[cc];
              // byte address of entry alpha' in copy 0 (the table starts at LDS address 0)
              const uint32_t al[4] = {(ap.x & 0xFFFFu) << 2, (ap.x >> 16) << 2, (ap.y & 0xFFFFu) << 2, (ap.y >> 16) << 2};
              if (nlive == NBW) {
                // steady state: all my beams alive -> branch-free; the NBW gathers of one dim are issued back to back
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                  float z[NBW];
#pragma unroll
                  for (int b = 0; b < NBW; ++b) z[b] = lds_abs_f32(al[i] + bet[b]); // 4*(dlog r + 10006 c + dlog h): no wrap
#pragma unroll
                  for (int b = 0; b < NBW; ++b) acc[cc * NBW + b] = proposal_term(acc[cc * NBW + b], z[b], cH[i], G[b][i]);
                  __builtin_amdgcn_sched_barrier(0); // one dim's NBW gathers in flight at a time (VGPR budget)
                }
              } else {
#pragma unroll
                for (int b = 0; b < NBW; ++b) {
                  if (b < nlive) { // wave-uniform
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                      const float z = lds_abs_f32(al[i] + bet[b]);
                      acc[cc * NBW + b] = proposal_term(acc[cc * NBW + b], z, cH[i], G[b][i]);
                    }
                  }
                }
              }
            }
          }
          const float tot = reduce_scatter_n<RW>(acc, lane);
          const int cc = rs_p / NBW, b = rs_p - cc * NBW;   // rs_p < 0: unused slot
          const int s = (ch * SPC + cc) * NSWe + swe;
          if (rs_p >= 0 && (lane & 1) == 0 && s < Sp && b < nlive) part_s[((size_t)g * SP + s) * PS + b_lo + b] = tot;
        }
      }
      TSTAMP(2);
      tsync();
      TSTAMP(3);
      // ---------------- combine dim groups in order, add C_b, build sort keys ----------------
      {
        constexpr int MK = (CMAX + NT - 1) / NT;
        const int Np = Sp * Bcur, f_base = s_base * Bcur; // this pass's candidates: flat indices f_base + [0, Np)
        {
          // every partial of my candidates (and of their beams' C_b) is fetched before the first is used: one LDS
          // latency instead of 4 per key
          float pr[MK][4], cbv[MK][4];
          const int gstride = SP * PS;
#pragma unroll
          for (int q = 0; q < MK; ++q) {
            const int f = q * NT + tid, fs = f < Np ? f : 0;
            const int s = Bcur == NB ? fs / NB : fs / Bcur, b = fs - s * Bcur;   // s: sample index inside the pass
#pragma unroll
            for (int gg = 0; gg < 4; ++gg) pr[q][gg] = part_s[(gg < NG ? gg : 0) * gstride + s * PS + b];
#pragma unroll
            for (int gg = 0; gg < 4; ++gg) cbv[q][gg] = cpart_s[(gg < NG ? gg : 0) * TEAM_MB + b];
          }
          if (KEYS_ALIAS && Bcur != NB) { // key f and partial f belong to different candidates: all reads before any write
#pragma unroll
            for (int q = 0; q < MK; ++q)
#pragma unroll
              for (int gg = 0; gg < 4; ++gg) asm volatile("" : "+v"(pr[q][gg]));
            tsync();
          }
          // shared rows: a candidate is MINE when its sample lies in my stripe; the others' keys come out of the exchange
          unsigned long long *xg = nullptr;
          if (CAN_SHARE && Wrow > 1)
            xg = reinterpret_cast<unsigned long long *>(A.coop_xch) + ((size_t)(t & 1) * COOP_MAX_BLOCKS + (size_t)xrow) * COOP_KEYS;
          const unsigned long long tag64 = (unsigned long long)(uint32_t)(t + 1) << 32;
          uint32_t foreign = 0u;                        // bit q: candidate q * NT + tid is a partner's
#pragma unroll
          for (int q = 0; q < MK; ++q) {
            float sc = pr[q][0];
            if (NG > 1) sc = sc + pr[q][1];
            if (NG > 2) sc = sc + pr[q][2];
            if (NG > 3) sc = sc + pr[q][3];
            float cb = cbv[q][0];                       // C_b: its dim-group partials in order, as the scores'
            if (NG > 1) cb = cb + cbv[q][1];
            if (NG > 2) cb = cb + cbv[q][2];
            if (NG > 3) cb = cb + cbv[q][3];
            const int f = q * NT + tid;
            if (f < Np) {
              bool mine = true;
              if (CAN_SHARE && Wrow > 1) {
                const int s_ = Bcur == NB ? f / NB : f / Bcur;
                mine = ((s_ % NSWe) % Wrow) == qsh;
              }
              if (mine) {
                const uint32_t key = score_key(sc + cb);
                key_s[f_base + f] = key;
                if (CAN_SHARE && Wrow > 1) __hip_atomic_store(&xg[f], tag64 | (unsigned long long)key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
              } else foreign |= 1u << q;
            }
          }
          if (CAN_SHARE && Wrow > 1) {
            // sweep the partners' granules until each carries this step's tag (tags start at 1; the preparation kernel zeroed the row's
            // granules; buffer t & 1 last held tag t - 1).  Give-up as in the split encoder: sticky error flag, COOP_GIVE_UP_TICKS (100 ms).
            const uint32_t tag = (uint32_t)(t + 1);
            const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();          // 100 MHz
            int32_t bad = 0;
            for (uint32_t turn = 1; foreign != 0u; ++turn) {
              unsigned long long gq[MK];
#pragma unroll
              for (int q = 0; q < MK; ++q)
                gq[q] = (foreign >> q) & 1u ? __hip_atomic_load(&xg[q * NT + tid], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0ull;
#pragma unroll
              for (int q = 0; q < MK; ++q)
                if (((foreign >> q) & 1u) && (uint32_t)(gq[q] >> 32) == tag) { key_s[f_base + q * NT + tid] = (uint32_t)gq[q]; foreign &= ~(1u << q); }
              if (foreign == 0u || (turn & 63u) != 0u) continue;
              if (__hip_atomic_load(A.coop_err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u) { bad = 1; break; }
              if (__builtin_amdgcn_s_memrealtime() - t0 > COOP_GIVE_UP_TICKS) { // the partners are not resident -- give up, loudly
                __hip_atomic_store(A.coop_err, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                bad = 1; break;
              }
            }
            if (bad) misc[6] = 1;
          }
        }
      }
      if (s_end < S) tsync(); // the next pass overwrites the partials
      } // sample passes
      if (CAN_SHARE && Wrow > 1) {   // every team of the row sees the (sticky) flag: nobody waits for anybody any more
        tsync();
        if (misc[6]) { abandoned = true; break; }
      }
      const int Bnew = B < N ? B : N;
      TSTAMP(4);
#ifdef IREC_ABLATE_SELECT
      tsync();
      if (tid < Bnew) { sel_s[tid] = tid % S; sel_b[tid] = tid % Bcur; sm->sel_bo[tid] = beta4[cur * TEAM_MB + tid % Bcur];
                        hsum[(cur ^ 1) * TEAM_MB + tid] = 0; beta4[(cur ^ 1) * TEAM_MB + tid] = 0u; }
      tsync();
#else
      // top-B (beam_search_coder.py:85-89); the thread that records new beam j also extends its hash / back-pointer
      // (:94-95) and notes its parent's table offset, so one barrier publishes everything the update needs
      constexpr bool QUICK_SEL = TEAMS <= 2 && !MULTI_PASS;   // (fast_common.h, select_topB_sync: not the 168-VGPR builds)
      if constexpr (QUICK_SEL) __builtin_assume(N <= 1024);   // (host: one pass holds S * NB <= CMAX = 1024 candidates -- the
                                                                //  selection's other paths fold away: -500 cycles per step, scripts/microbench/select_rates.hip)
      select_topB_sync<NT, QUICK_SEL>(key_s, N, Bnew, Bcur, sm, tid, tsync, nullptr, [&](int j, int32_t sp_, int32_t bp_, uint32_t key_) {
        const int32_t nh = (int32_t)((uint32_t)hsum[cur * TEAM_MB + bp_] + (uint32_t)sp_ * (uint32_t)(69 + t));
        hsum[(cur ^ 1) * TEAM_MB + j] = nh;                    // (its discrete log: looked up by every wave in the update, below)
        sm->sel_bo[j] = beta4[cur * TEAM_MB + bp_];
        bp[(size_t)t * NB + j] = (sp_ << 6) | bp_;
        if constexpr (MARGIN) margin_stash(sm, j, key_);
      });
      if constexpr (MARGIN) {   // how close was it?  (wave 0; the barrier keeps the next step's partials off the keys meanwhile)
        if (tid < 64) margin_step(key_s, N, Bnew, Bcur, sm, lane, t == K - 1, macc);
        tsync();
      }
#endif
      TSTAMP(5);
      // ---------------- gather the surviving beams (beam_search_coder.py:92-93), prepare the next step ----------------
      const bool last = (t == K - 1);
      __builtin_amdgcn_s_setprio(2); // serial phase: ahead of the other team's scoring waves
      // new beams' table offsets: lane j looks up dlog(hash(path_j)) -- a global load, consumed at the end of the update
      if constexpr (SWAP) {
        // words of park_g, stats_g and the beams that ANOTHER lane of this wave stored (the last update, at this step's map) are loaded
        // below at the next step's: the stores have left the wave before the first such load is issued
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      }
      uint32_t bv_new;
      {
        const int32_t nh = hsum[(cur ^ 1) * TEAM_MB + (lane < Bnew ? lane : 0)];
        bv_new = dlog_s[hash_from_sum(nh) - 1u];
      }
#ifdef IREC_ABLATE_UPDATE
      if (false) {
#else
      if (active) {
#endif
        if constexpr (SWAP) {
          // the whole update runs at the NEXT step's map: parents, new beams and their look-ups, c and sa out of the slab, the next
          // step's constants, G and the C_b terms.  (The last step keeps its map: the sample leaves from it.)
          if (!last && A.lane_swaps) {
            d0 = swapped_quad_dim(A, tab_q, t + 1, g, lane);
#pragma unroll
            for (int i = 0; i < 4; ++i) valid[i] = d0 + i < D;
            tab_t = tab_tu + (uint32_t)(d0 < Dp ? d0 : Dp - 4);
          }
        }
        unpark();
        const float sa_t[4] = {sa[0], sa[1], sa[2], sa[3]};   // this step's sample scale
        const float *bold = beams_g + ((size_t)cur * NB) * FAST_MAX_DIM + d0;
        float *bnew = beams_g + ((size_t)(cur ^ 1) * NB) * FAST_MAX_DIM + d0;
        // G is dead from the end of scoring until it is rebuilt below: every entry is redefined here
#pragma unroll
        for (int j = 0; j < NBW; ++j)
#pragma unroll
          for (int i = 0; i < 4; ++i) G[j][i] = 0.f;
        float m[4], cA[4], cBv[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) { m[i] = 0.f; cA[i] = 0.f; cBv[i] = 0.f; }
        float cacc[rsn_room(NBW)];
#pragma unroll
        for (int j = 0; j < rsn_room(NBW); ++j) cacc[j] = 0.f;
        constexpr int UB = (TEAMS >= 3 || BS >= 2) ? 5 : NBW;              // beams per load batch: all at once (G's registers are free) unless registers are short
        // the last step keeps ONE beam: beams[0] is all that leaves the block (beam_search_coder.py:118-122), so the parents,
        // rows and look-ups of the other new beams are not fetched at all
        const int Bupd = last ? 1 : Bnew;
        // lane j fetches the selection of new beam j and the offset of its parent: two LDS round trips for all beams
        const int32_t v_sp = sel_s[lane < Bnew ? lane : 0], v_bp = sel_b[lane < Bnew ? lane : 0];
        const uint32_t v_bo = sm->sel_bo[lane < Bnew ? lane : 0];
#pragma unroll
        for (int j0 = 0; j0 < NBW; j0 += UB) {
          // ---- issue the batch's global reads (proposal rows, old beams) back to back ----
          uint2 apv[UB];
          float4 obv4[UB];
          uint32_t bet_old[UB];
#pragma unroll
          for (int u = 0; u < UB; ++u) {
            const int jj = j0 + u, j = b_lo + jj;  // jj: slot in my stripe, j: new beam
            apv[u] = make_uint2(0u, 0u);
            obv4[u] = make_float4(0.f, 0.f, 0.f, 0.f);
            bet_old[u] = 0u;
            if (jj < NBW && j < Bupd) { // wave-uniform
              const int32_t sp_ = __builtin_amdgcn_readlane(v_sp, j);
              const int32_t bp_ = __builtin_amdgcn_readlane(v_bp, j);
              bet_old[u] = (uint32_t)__builtin_amdgcn_readlane((int)v_bo, j);
              apv[u] = *reinterpret_cast<const uint2 *>(tab_t + (size_t)sp_ * Dp);
#ifndef IREC_ABLATE_SLAB
              if (t) obv4[u] = *reinterpret_cast<const float4 *>(bold + (size_t)bp_ * FAST_MAX_DIM);
#endif
            }
          }
          if (j0 == 0 && !last) { step_consts(t + 1, m, cA, cBv); park(); } // next step's constants, under the loads' latency
          if (j0 == 0) TSTAMP(9);   // (diagnostic build: selection fetch + first load batch issued + step constants)
          // ---- new beams, their G and C terms ----
          // look-ups of YB beams are issued back to back, then consumed: UB / YB LDS latencies per batch instead of UB
          constexpr int YB = 5;
          float zy[YB][4];
#pragma unroll
          for (int u = 0; u < UB; ++u) {
            if (u % YB == 0) {
#pragma unroll
              for (int v = 0; v < YB; ++v) {
                const int uu = u + v < UB ? u + v : UB - 1;
                const uint32_t al[4] = {(apv[uu].x & 0xFFFFu) << 2, (apv[uu].x >> 16) << 2, (apv[uu].y & 0xFFFFu) << 2, (apv[uu].y >> 16) << 2};
#pragma unroll
                for (int i = 0; i < 4; ++i) zy[v][i] = lds_abs_f32(al[i] + bet_old[uu]); // entry 0 for beams that do not exist
              }
            }
            const int jj = j0 + u, j = b_lo + jj;
            if (jj < NBW && j < Bupd) { // wave-uniform
              const float obv[4] = {obv4[u].x, obv4[u].y, obv4[u].z, obv4[u].w};
              float nb[4];
#pragma unroll
              for (int i = 0; i < 4; ++i) {
                const float y = sa_t[i] * zy[u % YB][i];                    // dist.quantile(.), :48-49
                nb[i] = obv[i] + y;                                         // combined_samples[best_ind_aux, best_ind_beam], :81,92-93
              }
              if (last) {
                if (j == 0 && sw == 0 && qsh == 0) {
#pragma unroll
                  for (int i = 0; i < 4; ++i)
                    if (valid[i]) { // beams[0] + coding_dist.loc, :122
                      const int64_t ixo = src_index(A, base, pos, d0 + i);
                      A.out_sample[ixo] = nb[i] + A.p_loc[ixo];
                    }
                }
              } else {
#ifndef IREC_ABLATE_SLAB
                if (sw == 0) *reinterpret_cast<float4 *>(bnew + (size_t)j * FAST_MAX_DIM) = make_float4(nb[0], nb[1], nb[2], nb[3]);
#endif
                if constexpr (LATE_G) {
                  // 168-VGPR builds: the new beam waits in G's own registers; G and the C terms are formed below, once the
                  // batch temporaries (parent beams, proposal rows, look-ups) are dead -- same operations on the same values
#pragma unroll
                  for (int i = 0; i < 4; ++i) G[jj][i] = nb[i];
                } else {
#pragma unroll
                  for (int i = 0; i < 4; ++i) {
                    G[jj][i] = beam_G(nb[i], m[i], cA[i], cBv[i], sa[i]);
                    cacc[jj] = beam_C_term(cacc[jj], nb[i], m[i], cA[i], cBv[i]);
                  }
                }
              }
            }
          }
          __builtin_amdgcn_sched_barrier(0);
        }
        if constexpr (LATE_G) {
          if (!last) {
#pragma unroll
            for (int jj = 0; jj < NBW; ++jj) {
              if (b_lo + jj < Bnew) { // wave-uniform; beams that do not exist keep G = 0
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                  const float nbv = G[jj][i];
                  G[jj][i] = beam_G(nbv, m[i], cA[i], cBv[i], sa[i]);
                  cacc[jj] = beam_C_term(cacc[jj], nbv, m[i], cA[i], cBv[i]);
                }
              }
              __builtin_amdgcn_sched_barrier(0); // one beam at a time (the scheduler would interleave all twenty)
            }
          }
        }
        TSTAMP(10);                 // (diagnostic build: the load batches -- new beams, G, C)
        if (!last) {
          const float ctot = reduce_scatter_n<NBW>(cacc, lane);
          if (sw == 0 && (lane & 1) == 0 && rs_c >= 0 && b_lo + rs_c < Bnew) cpart_s[g * TEAM_MB + b_lo + rs_c] = ctot;
        }
      }
      TSTAMP(6);
      __builtin_amdgcn_s_setprio(0);
      // (wave 0 keeps the LDS copy for the parent look-up of the next selection, which it runs itself: same wave, program order)
      if (tid < Bnew) beta4[(cur ^ 1) * TEAM_MB + tid] = bv_new;
      bv_cur = bv_new;
      // no barrier here: the new C_b partials, hashes and beams are first read behind the next step's barriers
      cur ^= 1;
      Bcur = Bnew;
    }
    // ---- index path of beam 0 (beam_search_coder.py:118-121) ----
    tsync();
    if (abandoned) {                          // a shared row whose partners were not all resident: not coded (the host codes the call again)
      if (tid == 0 && qsh == 0) A.out_K[blk] = -2;
      continue;
    }
    if (tid == 0 && qsh == 0) {
      int j = 0;
      for (int t = K - 1; t >= 0; --t) {
        const int32_t v = __builtin_nontemporal_load(&bp[(size_t)t * NB + j]);
        A.out_indices[blk * (int64_t)A.max_K + t] = v >> 6;
        j = v & 63;
      }
      if constexpr (MARGIN) margin_write(A.out_margin, blk, macc);
    }
    TSTAMP(8);
  }
#ifdef IREC_TEAM_STAMPS
  if (A.dbg && lane == 0)
    for (int k = 0; k < 12; ++k) A.dbg[((size_t)blockIdx.x * (TEAMS * BS * 4) + wave_wg) * 16 + k] = st_acc[k];
  if (A.dbg && lane == 0) {
    A.dbg[((size_t)blockIdx.x * (TEAMS * BS * 4) + wave_wg) * 16 + 12] = __builtin_amdgcn_s_memtime() - st_t0;
    A.dbg[((size_t)blockIdx.x * (TEAMS * BS * 4) + wave_wg) * 16 + 13] = __builtin_amdgcn_s_memrealtime() - st_r0;
  }
#endif
}

// ======================================================================================================
//  launchers
// ======================================================================================================
// teams per workgroup / beam stripes per team.  Defaults: B <= 20: 3 x 1 where the LDS allows (else 2 x 1, or 1 x 2 with
// sample passes); B <= 30: 1 x 3.  Diagnostic overrides for B <= 20 travel in irec_params.flags (IREC_FLAG_SHAPE_*, no
// environment variable is read on the product path): cfg 20 = exactly two teams (also where three would be the default),
// 3 = three 4-wave teams (168 VGPRs), 12 = one 8-wave beam-striped team.  (Round 6: the one-team and the 2 x 2 shapes, which lost
// at every size, are gone with their builds <20,1,1> and <20,2,2>.)
static int team_cfg(int shape_override) {
  switch (shape_override) {
    case 2: return 20;
    case 3: return 3;
    case 5: return 12;
    default: return 2;
  }
}
// shape of the workgroup that serves B beams: beams per build, teams per workgroup, beam stripes per team
struct TeamShape { int nb, teams, bs; bool passes; bool one = false; };
static TeamShape team_shape(int B, int S, int ovr) {
  const int cfg = team_cfg(ovr);
  // 10 beams: G is 40 registers per lane, three teams fit the register file (168 VGPRs) and, for small S, the LDS: +9 %
  if (B == 1 && cfg == 2) {   // one beam: its own build (pipelined wide path), three teams, packed rows
    return TeamShape{10, 3, 1, team_s_pass(10, S, 3, 1024, false, 1) != S, true};
  }
  if (B <= 10) {
    const int ps = team_row(10, B);
    if (cfg == 3 || (cfg == 2 && team_s_pass(10, S, 3, 1024, false, ps) == S)) return TeamShape{10, 3, 1, false};
    if (cfg != 2 || team_s_pass(10, S, 2, 1024, false, ps) == S) return TeamShape{10, 2, 1, false};
    return TeamShape{10, 3, 1, true};   // more samples than one pass of two teams holds (S > 102): three teams, sample passes
  }
  if (B <= 20) {
    if (cfg == 20) return TeamShape{20, 2, 1, false};
    if (cfg == 12) return TeamShape{20, 1, 2, false};
    // three 4-wave teams (168 VGPRs: half-slot look-up pipeline, statistics / variance / scale parked in the slab, sort keys
    // over the partial scores) wherever their LDS fits next to the table copies -- S <= 38, the BASELINE workload: a third
    // team scores while another is in a serial phase (r02c: 13.2 ms against 13.7 ms of two teams)
    if (team_s_pass(20, S, 3, 1024) == S) return TeamShape{20, 3, 1, false};
    // more samples than two teams can hold in one pass (e.g. Omega = 5: S = 148): one 8-wave team with two beam stripes
    // and sample passes
    if (team_s_pass(20, S, 2, 1024) != S) return TeamShape{20, 1, 2, false};
    return TeamShape{20, 2, 1, false};
  }
  if (B <= 30) return TeamShape{30, 1, 3, false};   // one 12-wave team: three stripes of 10 beams (the B = 30 stress configuration)
  if (B <= 32) return TeamShape{32, 1, 2, false};   // one 8-wave team: two stripes of 16 beams
  // round 3: B = 50 of the reference's sweep (examples/lossless/data_aggregation.py:7).  One 12-wave team, three stripes of
  // 20 beams at 168 VGPRs (the three-team build's register diet: half-slot pipeline, parked state); a stripe that is at least
  // half alive scores its missing beams as phantoms
  // round 4: stripes of 18 beams for 48 < B <= 54 at S >= 128 -- B = 50 of the sweep then scores 54 beam slots instead of 60
  // (its third stripe holds 14 live beams and 4 phantoms instead of 10 and 10): -3 % time from S = 148 on (10.06 against
  // 9.71 look-ups/clk/CU at S = 1808), but its full-slot look-up pipeline at 168 VGPRs (416 B of scratch) loses 10-26 % to the
  // 60-beam build's half-slot diet below S ~ 100; stripes of 16 for B <= 48 lose at every S (B = 40 on the 60-beam build
  // leaves its third stripe idle anyway) and are not built (profiles/archive/r04g/).
  if (cfg != 3 && B > 48 && B <= 54 && S >= 128) return TeamShape{54, 1, 3, false};
  if (B <= 60) return TeamShape{60, 1, 3, false};
  return TeamShape{0, 0, 0, false};
}

template <int NB, int TEAMS, int BS, bool PASSES = false, bool ONE = false, bool SHARE = false, bool MARGIN = false>
static hipError_t launch_team_t(const EncArgs &A, int grid, hipStream_t st) {
  const int ps = team_row(NB, A.B);
  const int sp = (TEAMS == 1 || PASSES) ? team_s_pass(NB, A.S, TEAMS, TEAMS == 1 ? 2048 : 1024, PASSES, ps) : A.S;
  const size_t lds = team_lds_total(NB, A.S, sp, TEAMS, PASSES, ps);
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(encode_team_kernel<NB, TEAMS, BS, PASSES, ONE, SHARE, MARGIN>),
                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL((encode_team_kernel<NB, TEAMS, BS, PASSES, ONE, SHARE, MARGIN>), dim3(grid), dim3(TEAMS * BS * TEAM_NT), lds, st, A);
  return hipGetLastError();
}

// One source, two objects: irec_team.o holds the product builds below `#else`; irec_team_margin.hip includes this file with its
// macro set and gets the margin builds instead, so that their five instantiations compile beside the product's.
#ifdef IREC_TEAM_MARGIN_TU
// ---- margin builds (irec_beam_encode_ex, IREC_FLAG_MARGINS): the shapes the BASELINE configurations run ----
static int team_margin_key(int B, int S, int ovr) {
  const TeamShape sh = team_shape(B, S, ovr);
  if (!sh.nb || sh.passes || sh.one) return 0;
  const int key = sh.nb * 100 + sh.teams * 10 + sh.bs;
  return (key == 2031 || key == 2021 || key == 1031 || key == 1021 || key == 3013) ? key : 0;
}
bool team_margin_build(int B, int S, int shape_override) { return team_margin_key(B, S, shape_override) != 0; }
hipError_t launch_encode_team_margin(const EncArgs &A, int grid, hipStream_t st) {
  if (A.out_margin == nullptr || A.coop_W > 1) return hipErrorInvalidValue;   // (no rows are shared under IREC_FLAG_MARGINS)
  switch (team_margin_key(A.B, A.S, A.shape_override)) {
    case 2031: return launch_team_t<20, 3, 1, false, false, false, true>(A, grid, st);
    case 2021: return launch_team_t<20, 2, 1, false, false, false, true>(A, grid, st);
    case 1031: return launch_team_t<10, 3, 1, false, false, false, true>(A, grid, st);
    case 1021: return launch_team_t<10, 2, 1, false, false, false, true>(A, grid, st);
    case 3013: return launch_team_t<30, 1, 3, false, false, false, true>(A, grid, st);
    default: return hipErrorInvalidValue;
  }
}

} // namespace irec
#else
// ---- product builds: what the planner asks about the shape of a call (irec_kernels.h), and the launcher ----
int team_count_for(int B, int S, int ovr) { return team_shape(B, S, ovr).teams; }
int team_shareable(int B, int S, int ovr) {
  const TeamShape sh = team_shape(B, S, ovr);
  return (sh.nb && sh.teams >= 2 && sh.bs == 1 && !sh.passes && !sh.one && (int64_t)S * sh.nb <= COOP_KEYS) ? sh.teams : 0;
}
bool team_takes_swaps(int B, int S, int ovr) {   // the builds that apply EncArgs::lane_swaps (SWAP in encode_team_kernel; the host
  const TeamShape sh = team_shape(B, S, ovr);    // leaves the masks out of shared-row and margin calls, whose builds do not)
  return sh.nb != 0 && sh.teams * sh.bs >= 3 && sh.nb / sh.bs == 20;
}
bool team_placeable(int B, int S, int ovr) {   // the builds that can deal their rows by cost (CAN_PLACE in encode_team_kernel)
  const TeamShape sh = team_shape(B, S, ovr);
  return sh.nb == 20 && sh.teams == 2 && sh.bs == 1 && !sh.passes && !sh.one;
}
int team_waves_for(int B, int S, int ovr) { const TeamShape sh = team_shape(B, S, ovr); return sh.teams * sh.bs * TEAM_NW; }
size_t team_ws_extra_for(int B, int S, int ovr) { // scratch-slab bytes on top of fast_ws_for(): the sort keys when they do not fit the LDS
  const TeamShape sh = team_shape(B, S, ovr);
  const int ps = sh.nb ? team_row(sh.nb, B) : 0;
  return (sh.nb && !team_keys_in_lds(sh.nb, S, sh.teams, sh.passes, ps)) ? ((team_key_bytes(ps, S) + 255) & ~(size_t)255) : 0;
}
size_t team_ws_bytes_for(int B, int S, int ovr, int max_K) {
  const TeamShape sh = team_shape(B, S, ovr);
  return sh.nb ? fast_ws_bytes(sh.nb, max_K) + team_ws_extra_for(B, S, ovr) : 0;
}
// teams per workgroup of encode_ten_kernel (irec_ten.hip) when a plain call of this shape takes it, else 0
int team_ten_teams(int B, int S, int ovr) {
  const TeamShape sh = team_shape(B, S, ovr);
  if (!(sh.nb == 10 && sh.bs == 1 && !sh.passes && !sh.one && (sh.teams == 2 || sh.teams == 3) && ten_applies(B, S))) return 0;
  return sh.teams;   // (r06f: FOUR teams at 128 VGPRs hold the scoring loop without a spill and LOSE 12 %: 4096 latents 8.6 -> 9.7 ms)
}
const char *team_kernel_name(int B, int S, int ovr) {
  static thread_local char buf[64];
  const TeamShape sh = team_shape(B, S, ovr);
  snprintf(buf, sizeof buf, "encode_team_kernel<%d,%d,%d%s%s>", sh.nb, sh.teams, sh.bs, sh.passes ? ",passes" : "", sh.one ? ",one" : "");
  return buf;
}

size_t team_lds_for(int B, int S, int ovr) {
  const TeamShape sh = team_shape(B, S, ovr);
  if (!sh.nb) return (size_t)-1;
  if ((int64_t)S * sh.nb >= (1 << 24)) return (size_t)-1;
  const int ps = team_row(sh.nb, B);
  const int sp = team_s_pass(sh.nb, S, sh.teams, sh.teams == 1 ? 2048 : 1024, sh.passes, ps);
  if (sp < 1 || (sp < S && (sp < 16 || (sh.teams > 1 && !sh.passes)))) return (size_t)-1;   // does not fit (one-pass builds: in one
                                                                             // pass), or only in slivers: the one-table encoder takes it
  const size_t b = team_lds_total(sh.nb, S, sp, sh.teams, sh.passes, ps);
  return b <= FAST_LDS_LIMIT ? b : (size_t)-1;
}

hipError_t launch_encode_team(const EncArgs &A, int grid, hipStream_t st) {
  const TeamShape sh = team_shape(A.B, A.S, A.shape_override);
  const int key = sh.nb * 100 + sh.teams * 10 + sh.bs + (sh.passes ? 10000 : 0) + (sh.one ? 100000 : 0);
  if (A.coop_W > 1) {   // rows shared between teams (host: team_share_width -> team_shareable builds only)
    switch (key) {
      case 1021: return launch_team_t<10, 2, 1, false, false, true>(A, grid, st);
      case 2021: return launch_team_t<20, 2, 1, false, false, true>(A, grid, st);
      case 2031: return launch_team_t<20, 3, 1, false, false, true>(A, grid, st);
      default: return hipErrorInvalidValue;
    }
  }
  if ((key == 1031 || key == 1021) && !A.no_ten && ten_applies(A.B, A.S)) return launch_encode_ten(A, team_ten_teams(A.B, A.S, A.shape_override), grid, st);   // (irec_ten.hip)
  switch (key) {
    case 101031: return launch_team_t<10, 3, 1, false, true>(A, grid, st);
    case 111031: return launch_team_t<10, 3, 1, true, true>(A, grid, st);
    case 11031: return launch_team_t<10, 3, 1, true>(A, grid, st);
    case 6013: return launch_team_t<60, 1, 3>(A, grid, st);
    case 5413: return launch_team_t<54, 1, 3>(A, grid, st);
    case 1021: return launch_team_t<10, 2, 1>(A, grid, st);
    case 1031: return launch_team_t<10, 3, 1>(A, grid, st);
    case 2021: return launch_team_t<20, 2, 1>(A, grid, st);
    case 2031: return launch_team_t<20, 3, 1>(A, grid, st);
    case 2012: return launch_team_t<20, 1, 2>(A, grid, st);
    case 3013: return launch_team_t<30, 1, 3>(A, grid, st);
    case 3212: return launch_team_t<32, 1, 2>(A, grid, st);
    default: return hipErrorInvalidValue;
  }
}

} // namespace irec

// The product builds of the chunked encoder are compiled in THIS unit, not in one of their own.  Their kernels share no code path with
// encode_team_kernel, but the compiler's view of the geometry helpers of irec_team_common.h does depend on them: the helpers are internal
// to the device module, so interprocedural constant propagation gives their arguments the ranges it sees at ALL call sites of the module
// (with the chunk kernels: `ps` of team_key_bytes in [1, 61); without them the merge of the team kernels' own call sites gives up and the
// range is gone), and with other ranges every encode_team_kernel build comes out with other instructions (a sign extension where a zero
// extension was, one key-size computation no longer shared, another schedule after it).  The headline kernel's code is not to move with
// its neighbours: scripts/isa_identity.py against the previous build is the check for any change to this arrangement.
#include "irec_chunk.hip"
#endif   // IREC_TEAM_MARGIN_TU
