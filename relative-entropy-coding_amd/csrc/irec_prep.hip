// irec_prep.hip -- the call's preparation kernel (irec_kernels.h, "The call's preparation kernel"): one launch per call that clears the
// books and the exchange granules, builds the proposal tables with their bank-spreading copy bits (choice_table_rows) that the team
// encoders (irec_team.hip, irec_ten.hip, irec_chunk.h) and the one-beam encoder (irec_lone.hip) stream, and writes the cost key of every
// row for the cost-ordered hand-out of encode_team_kernel.  alpha_choice_kernel builds the tables alone.  swap_mask_kernel, launched in front
// of the preparation kernel by the calls that take them, picks the lane-swap masks (irec_kernels.h, "Lane swaps") the copy bits are assigned for.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <stdint.h>

#include "irec_device.h"
#include "irec_kernels.h"
#include "irec_fast_common.h"

namespace irec {

// ======================================================================================================
//  proposal table with copy bits: tab[t][s][d] = dlog_g(r[s, d]) + 10006 * c   (uint16, row stride = D rounded up to 4)
//
//  The int32 draw of get_pseudo_random_sample (beam_search_coder.py:38-43) depends only on (seed + t, S, D): it is
//  evaluated once per call.  The block kernel's lane l of dim group g reads the quad d = 256 g + 4 l .. +3 of a row and
//  issues, per dim slot i and beam, one ds_read_b32 whose 32-lane groups are the quads [32 m, 32 m + 32) of the row.
//  For every such group and slot the 32 look-ups are spread over the banks by choosing c per lane: lane with
//  a = dlog mod 32 lands on bank a (c = 0) or a + 22 (c = 1), plus the beam's common rotation.  Since gcd(22, 32) = 2
//  the banks form two rings of 16 (p -> p + 1 is bank -> bank + 22) and a lane is an edge between neighbours; the
//  assignment minimising the busiest bank is found exactly: for L = 1, 2, ... and every x_0, push as many edges as
//  node p still takes (x_p = min(n_p, L - n_{p-1} + x_{p-1})) and test the closing node.
//  One half-wave per (t, s, m); choice bits never change any emitted value (all three table copies are identical).
// ======================================================================================================
// Round 4 (second half): ONE launch builds every table of the call (a latent's 1000-dim and residual-dim tables used to be
// two launches of 56 + 21 us at the default 32-step window); the rank of a look-up among those of its bank is the value an
// LDS atomic returns (any order serves: the x lowest ranks stay) instead of 32 ballots per slot; the four draws of a quad come
// from one Philox block (two where S * D is not a multiple of 4); the ring search starts at the average load and keeps one
// running value instead of three 16-entry arrays -- 82 VGPRs instead of 256 + 65 AGPRs, so several workgroups share a CU.
#ifndef IREC_CHOICE_WPE
#define IREC_CHOICE_WPE 2   // waves per SIMD the table-building kernels are compiled for
#endif
// Exact min-max assignment on one 16-ring of banks: n[p] look-ups have node p as their c = 0 bank and node p + 1 as their c = 1 bank.
// Returns the smallest L for which no node takes more than L, and in x0 how many of node 0's look-ups stay (the others follow from it).
__device__ __forceinline__ int ring_min_busiest(const int (&n)[16], int tot, int &x0f) {
  int Lf = 32;                       // (L = 32 with every look-up at c = 0 is always feasible)
  x0f = n[0];
  bool done = false;
  for (int L = tot > 16 ? (tot + 15) >> 4 : 1; L < 32 && !done; ++L)
    for (int x0 = 0; x0 <= n[0] && !done; ++x0) {
      int xp = x0;
      bool ok = true;
#pragma unroll
      for (int p = 1; p < 16; ++p) {
        const int ub = L - n[p - 1] + xp;
        ok = ok && ub >= 0;
        xp = n[p] < ub ? n[p] : (ub < 0 ? 0 : ub);
      }
      if (ok && x0 + n[15] - xp <= L) { done = true; Lf = L; x0f = x0; }
    }
  return Lf;
}
// 32-lane groups of a row of NQ quads (with lane swaps both groups of a dim group exist as soon as one does: quads move between them)
__host__ __device__ inline int choice_groups(int NQ, bool swaps) { return swaps ? ((NQ + 63) >> 6) << 1 : (NQ + 31) >> 5; }
// rows with copy bits: workgroup `wg` of `n_wg` (256 threads: 8 half-waves); skip bit q set: table q is in place already
__device__ __forceinline__ void choice_table_rows(int64_t seed, int32_t S, int32_t K_tab, const uint16_t *__restrict__ dlog4r,
                                                  const ChoiceJobs &jobs, uint32_t skip, int64_t wg, int64_t n_wg) {
  __shared__ uint32_t n_s[8][4][32]; // [half-wave][slot][bank] look-ups whose c = 0 bank this is
  __shared__ uint8_t x_s[8][4][32];  // how many of them stay (c = 0)
  const int hwl = threadIdx.x >> 5, j = threadIdx.x & 31;
  const int64_t n_hw = jobs.hw_end[jobs.n - 1];
  for (int64_t hw0 = wg * 8; hw0 < n_hw; hw0 += n_wg * 8) {
    const int64_t hwg = hw0 + hwl;
    int q = 0;
    while (q + 1 < jobs.n && hwg >= jobs.hw_end[q]) ++q;
    const int64_t hw = hwg - (q ? jobs.hw_end[q - 1] : 0);
    // (a table in place that was built for exactly this key is left alone)
    const bool hw_ok = hwg < n_hw && !((skip >> q) & 1u) && !(jobs.keep[q] && *jobs.keep[q]);
    const int D = jobs.D[q];
    const int Dp = (D + 3) & ~3;
    const int NQ = Dp >> 2;             // quads per row
    const int NM = choice_groups(NQ, jobs.swap != nullptr);   // 32-lane groups per row
    const int64_t row = hw_ok ? hw / NM : 0;           // t * S + s
    const int m = hw_ok ? (int)(hw - row * NM) : 0;
    const int t = (int)(row / S), s = (int)(row - (int64_t)t * S);
    // lane swaps: lane j of group m holds quad 32 m + j, or that of the other group of its dim group where bit j of the mask is set
    uint32_t msk = 0u;
    if (jobs.swap != nullptr && hw_ok && t < SWAP_STEPS) msk = jobs.swap[(q * SWAP_STEPS + t) * 4 + (m >> 1)];
    const int quad = 32 * (m ^ (int)((msk >> j) & 1u)) + j;
    const bool q_ok = hw_ok && quad < NQ;
    uint32_t al[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int i = 0; i < 4; ++i) n_s[hwl][i][j] = 0u;
    if (q_ok) {
      const StepSeed ss = make_step_seed(seed + t);
      uint32_t rm1[4];
      draw_rm1_x4(ss, (uint64_t)s * (uint64_t)D + (uint64_t)(4 * quad), rm1);   // (draws past the row's end are not used)
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (4 * quad + i < D) al[i] = (uint32_t)dlog4r[rm1[i]] >> 2;
    }
    __syncthreads();
    // rank of every look-up among those of its group with the same c = 0 bank, and the per-bank counts
    uint32_t rank[4] = {0u, 0u, 0u, 0u};
    if (q_ok) {
#pragma unroll
      for (int i = 0; i < 4; ++i) rank[i] = atomicAdd(&n_s[hwl][i][al[i] & 31u], 1u);
    }
    __syncthreads();
    if (j < 8 && hw_ok) { // 4 slots x 2 rings per half-wave
      const int slot = j >> 1, ring = j & 1;
      int n[16];
      int tot = 0;
#pragma unroll
      for (int p = 0; p < 16; ++p) { n[p] = (int)n_s[hwl][slot][(ring + 22 * p) & 31]; tot += n[p]; }
      int x0f;
      const int Lf = ring_min_busiest(n, tot, x0f);
      int xp = x0f;
      x_s[hwl][slot][ring] = (uint8_t)xp;
#pragma unroll
      for (int p = 1; p < 16; ++p) {
        const int ub = Lf - n[p - 1] + xp;
        xp = n[p] < ub ? n[p] : (ub < 0 ? 0 : ub);
        x_s[hwl][slot][(ring + 22 * p) & 31] = (uint8_t)xp;
      }
    }
    __syncthreads();
    if (q_ok) {
      uint32_t v[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) v[i] = al[i] + (rank[i] < (uint32_t)x_s[hwl][i][al[i] & 31u] ? 0u : IREC_PM1);
      *reinterpret_cast<uint2 *>(jobs.tab[q] + (row * Dp + 4 * quad)) = make_uint2(v[0] | (v[1] << 16), v[2] | (v[3] << 16));
    }
    __syncthreads(); // n_s / x_s are reused by the next round
  }
}
__global__ __launch_bounds__(256, IREC_CHOICE_WPE) void alpha_choice_kernel(int64_t seed, int32_t S, int32_t K_tab,
                                                           const uint16_t *__restrict__ dlog4r, ChoiceJobs jobs) {
  choice_table_rows(seed, S, K_tab, dlog4r, jobs, 0u, (int64_t)blockIdx.x, (int64_t)gridDim.x);
}

// ======================================================================================================
//  lane-swap masks (irec_kernels.h, "Lane swaps"): one workgroup per (table, step, dim group)
//
//  The step's S * 4 look-up instructions of the dim group are charged L(lanes 0-31) + L(lanes 32-63), L the busiest
//  bank of the exact assignment above (0 for an empty group).  Greedy, two passes over the 32 bits: flip a bit, keep the flip if the
//  step's sum drops.  Quads past the row's end are not counted, as in choice_table_rows.
// ======================================================================================================
__device__ __forceinline__ uint32_t tables_in_place(const uint32_t *head, const TableStamps &ts) {   // bit q: slot q's stamp is the call's key
  uint32_t skip = 0u;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    bool same = ts.reuse != 0 && ts.w[q][0] != 0u;
#pragma unroll
    for (int k = 0; k < WS_STAMP_WORDS; ++k) same = same && __builtin_nontemporal_load(head + WS_STAMP_WORD + q * WS_STAMP_WORDS + k) == ts.w[q][k];
    skip |= same ? (1u << q) : 0u;
  }
  return skip;
}
// 1024 threads: thread (instruction, 32-lane group h, ring) keeps the 16 counts of its ring of banks (a column of cnt_s) and solves that
// ring alone; the two rings of a group sit in neighbouring lanes.  (One thread per instruction with all four rings took 930 us a call.)
__global__ __launch_bounds__(1024) void swap_mask_kernel(PrepArgs P, uint32_t *masks, int32_t mode, int32_t steps) {
  __shared__ uint8_t bank_s[64][256];      // [quad of the dim group][instruction s * 4 + slot]: c = 0 bank, 0xFF = no such quad
  __shared__ uint8_t cnt_s[16][1024];      // [node of the ring][thread]: look-ups of the thread's group whose c = 0 bank the node is
  __shared__ int32_t sum_s[3];
  const int tid = (int)threadIdx.x;
  const int unit = (int)blockIdx.x;        // (q * steps + t) * 4 + g
  const int g = unit & 3, t = (unit >> 2) % steps, q = (unit >> 2) / steps;
  if (q >= P.jobs.n) return;
  if ((tables_in_place(P.head, P.ts) >> q) & 1u) return;   // the table stays, and so do its masks
  uint32_t *out = masks + (q * SWAP_STEPS + t) * 4 + g;
  const int D = P.jobs.D[q], S = P.S;
  const int NQ = (((D + 3) & ~3) >> 2) - 64 * g;           // quads of this dim group (<= 0: none)
  if (mode != 1 || NQ <= 0 || S > SWAP_MAX_S) {
    if (tid == 0) *out = (mode == 2 && NQ > 0) ? 0xFFFFFFFFu : 0u;
    return;
  }
  const StepSeed ss = make_step_seed(P.seed + t);
  for (int item = tid; item < S * 64; item += 1024) {
    const int s = item >> 6, ql = item & 63, quad = 64 * g + ql;
    uint32_t b[4] = {0xFFu, 0xFFu, 0xFFu, 0xFFu};
    if (ql < NQ) {
      uint32_t rm1[4];
      draw_rm1_x4(ss, (uint64_t)s * (uint64_t)D + (uint64_t)(4 * quad), rm1);
#pragma unroll
      for (int i = 0; i < 4; ++i) b[i] = 4 * quad + i < D ? ((uint32_t)P.dlog4r[rm1[i]] >> 2) & 31u : 0u;   // (dims past D: entry 0)
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) bank_s[ql][s * 4 + i] = (uint8_t)b[i];
  }
#pragma unroll
  for (int p = 0; p < 16; ++p) cnt_s[p][tid] = 0;
  if (tid < 3) sum_s[tid] = 0;
  __syncthreads();
  const int ins = tid >> 2, h = (tid >> 1) & 1, ring = tid & 1;
  const bool mine = ins < S * 4;           // my look-up instruction
  // bank b of my ring is its node p with (ring + 22 p) mod 32 = b: p = 3 (b - ring) / 2 mod 16
  auto move = [&](uint32_t b, int d) { if (b != 0xFFu && (int)(b & 1u) == ring) cnt_s[(3 * ((b - (uint32_t)ring) >> 1)) & 15][tid] += (uint8_t)d; };
  if (mine)
    for (int ql = 32 * h; ql < 32 * h + 32; ++ql) move(bank_s[ql][ins], 1);
  auto cost = [&]() {                      // of my group, in the lane of its ring 0; every lane of the wave comes here
    int L = 0;
    if (mine) {
      int n[16], tot = 0, x0;
#pragma unroll
      for (int p = 0; p < 16; ++p) { n[p] = (int)cnt_s[p][tid]; tot += n[p]; }
      L = tot ? ring_min_busiest(n, tot, x0) : 0;
    }
    const int Lo = __shfl_xor(L, 1, 64);
    int c = ring == 0 ? (L > Lo ? L : Lo) : 0;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) c += __shfl_xor(c, off, 64);
    return c;                              // the wave's sum
  };
  auto flip = [&](int j, uint32_t m) {     // quads j and j + 32 trade groups (m: the mask before the flip)
    const int h0 = (int)((m >> j) & 1u);   // where quad j is now
    move(bank_s[j][ins], h == h0 ? -1 : 1);
    move(bank_s[j + 32][ins], h == h0 ? 1 : -1);
  };
  // three counters in turn: the one of the round after next is cleared while this round's is summed (its last reader passed a barrier since)
  {
    const int c = cost();
    if ((tid & 63) == 0) atomicAdd(&sum_s[0], c);
  }
  __syncthreads();
  int best = sum_s[0];
  uint32_t m = 0u;
  const int nj = NQ < 32 ? NQ : 32;        // (a bit whose two quads both lie past the row's end moves nothing)
  int round = 1;
  for (int pass = 0; pass < 2; ++pass)
    for (int j = 0; j < nj; ++j, ++round) {
      if (tid == 0) sum_s[(round + 1) % 3] = 0;
      if (mine) flip(j, m);
      const int c = cost();
      if ((tid & 63) == 0) atomicAdd(&sum_s[round % 3], c);
      __syncthreads();
      const int tot = sum_s[round % 3];
      if (tot < best) { best = tot; m ^= 1u << j; }
      else if (mine) flip(j, m ^ (1u << j));   // back
    }
  if (tid == 0) *out = m;
}
hipError_t launch_swap_masks(const PrepArgs &P, uint32_t *masks, int mode, hipStream_t st) {
  if (P.jobs.n < 1 || masks == nullptr) return hipErrorInvalidValue;
  const int steps = P.K_tab < SWAP_STEPS ? P.K_tab : SWAP_STEPS;
  hipLaunchKernelGGL(swap_mask_kernel, dim3((unsigned)(P.jobs.n * steps * 4)), dim3(1024), 0, st, P, masks, (int32_t)mode, (int32_t)steps);
  return hipGetLastError();
}

// cost key of one row by one 256-thread workgroup: the row's KL summed in any order -- it places the row, it does not code it.
// (Two halves: all gathers of the call's statistics -- four dims per thread -- are issued before the first is used.)
struct CostRow { float v[4][4]; bool ok[4]; bool okD; int D; };
__device__ __forceinline__ void cost_row_issue(const EncArgs &A, int64_t blk, int t, CostRow &c) {
  c.D = A.block_dim[blk];
  const int64_t base = A.block_base[blk];
  const int32_t pos = A.block_pos[blk];
  c.okD = c.D >= 1 && c.D <= FAST_MAX_DIM;
  int64_t ix[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) { const int d = t + 256 * i; c.ok[i] = c.okD && d < c.D; ix[i] = c.ok[i] ? src_index(A, base, pos, d) : 0; }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    c.v[i][0] = c.v[i][1] = c.v[i][2] = c.v[i][3] = 1.f;
    if (c.ok[i]) { c.v[i][0] = A.q_loc[ix[i]]; c.v[i][1] = A.q_scale[ix[i]]; c.v[i][2] = A.p_loc[ix[i]]; c.v[i][3] = A.p_scale[ix[i]]; }
  }
}
__device__ __forceinline__ void cost_row_finish(const PrepArgs &P, const EncArgs &A, int64_t blk, int t, const CostRow &c) {
  __shared__ double part[4];
  double acc = 0.0;
#pragma unroll
  for (int i = 0; i < 4; ++i)
    if (c.ok[i]) acc = acc + kl_dim(c.v[i][0], c.v[i][1], c.v[i][2], c.v[i][3]);
  const double ws = wave_tree_sum(acc);
  if ((t & 63) == 0) part[t >> 6] = ws;
  __syncthreads();
  if (t == 0) {
    const double tot = ((part[0] + part[1]) + part[2]) + part[3];
    int32_t K = c.okD ? num_aux((float)tot, A.omega) : 0;
    K = K < 0 ? 0 : (K > (1 << 20) ? (1 << 20) : K);
    const uint32_t cst = (uint32_t)K * (uint32_t)(c.okD ? c.D : 0);
    P.cost[blk] = ((cst < (1u << 22) ? cst : (1u << 22) - 1u) << 10) | (uint32_t)blk;   // distinct keys: ties go to the lower row
  }
}

// ======================================================================================================
//  the call's preparation kernel (irec_kernels.h, "The call's preparation kernel"): books, exchange granules, row costs, tables
// ======================================================================================================
__global__ __launch_bounds__(256, IREC_CHOICE_WPE) void prep_kernel(PrepArgs P, EncArgs A) {
  const int t = (int)threadIdx.x;
  uint32_t *p = P.head;
  int wg = (int)blockIdx.x;
  if (wg == 0) { // ---- books
    for (int w = t; w < (int)(WS_COUNTER_BYTES / 4); w += 256) {
      const bool book = (w >= WS_KEEP_WORD && w < WS_KEEP_WORD + 4) || (w >= WS_STAMP_WORD && w < WS_STAMP_WORD + 4 * WS_STAMP_WORDS) ||
                        (w >= WS_PENDING_WORD && w < WS_PENDING_WORD + 4 * WS_STAMP_WORDS);
      if (!book) p[w] = 0u;
    }
    if (t < 4) {   // one thread owns a slot's words
      uint32_t *stamp = p + WS_STAMP_WORD + t * WS_STAMP_WORDS, *pend = p + WS_PENDING_WORD + t * WS_STAMP_WORDS;
      bool same = P.ts.reuse != 0 && P.ts.w[t][0] != 0u;
#pragma unroll
      for (int k = 0; k < WS_STAMP_WORDS; ++k) same = same && stamp[k] == P.ts.w[t][k];
      p[WS_KEEP_WORD + t] = same ? 1u : 0u;
#pragma unroll
      for (int k = 0; k < WS_STAMP_WORDS; ++k) pend[k] = P.ts.w[t][k];
      if (!same) {   // not this call's table: no word of the slot may pass for the key's until the encode kernel commits it
#pragma unroll
        for (int k = 0; k < WS_STAMP_WORDS; ++k) stamp[k] = ~P.ts.w[t][k];
      }
    }
    return;
  }
  wg -= 1;
  if (wg < P.n_granule) { // ---- exchange granules of shared block `wg`, both parities (16 KB): the step tags of the split encoder
                          // start at 1, so no granule of an earlier call on this workspace -- or whatever the memory held -- passes for one of this call's
    uint4 *x = reinterpret_cast<uint4 *>(reinterpret_cast<char *>(p) + WS_COUNTER_BYTES);
#pragma unroll
    for (int par = 0; par < 2; ++par) {
      uint4 *xb = x + ((size_t)par * COOP_MAX_BLOCKS + (size_t)wg) * (COOP_KEYS * 8 / 16);
      for (int k = t; k < COOP_KEYS * 8 / 16; k += 256) xb[k] = make_uint4(0u, 0u, 0u, 0u);
    }
    return;
  }
  wg -= P.n_granule;
  if (wg < P.n_table_wgs) {
    // ---- proposal tables: which slots are in place?  (read-only; see irec_kernels.h for why the race with workgroup 0 is benign)
    const uint32_t skip = tables_in_place(p, P.ts);
    if (P.table_kind == 1) choice_table_rows(P.seed, P.S, P.K_tab, P.dlog4r, P.jobs, skip, (int64_t)wg, (int64_t)P.n_table_wgs);
    else if (P.table_kind == 2) {
      // plain rows: the workgroups are dealt to the tables in proportion to their rows (jobs.hw_end counts 1024-entry units)
      int q = 0;
      while (q + 1 < P.jobs.n && (int64_t)wg >= P.jobs.hw_end[q]) ++q;
      const int64_t first = q ? P.jobs.hw_end[q - 1] : 0;
      if (!((skip >> q) & 1u)) plain_table_rows(P.seed, P.S, P.jobs.D[q], P.K_tab, P.dlog4r, P.jobs.tab[q], (int64_t)wg - first, P.jobs.hw_end[q] - first);
    }
    return;
  }
  wg -= P.n_table_wgs;
  // ---- cost key of row `wg`, a workgroup each, BEHIND the table workgroups (profiles/r06end/).  The key is three dependent gathers away
  // (descriptors -> permutation -> statistics, 5 000 random lines per row through the vector L1) and costs the launch 4 us (17 against 13)
  // here; in front of the tables, as in round 4, the cost workgroups held those back as well (18.5 us at 302 rows, 29 at 512:
  // prep_cost_first.log).  Also measured: the row riding on table workgroup `wg` with its gathers issued first (25 us: they did not overlap
  // with the table work, prep_cost_riding.log); a wave per row, four rows per workgroup (30 us, prep_cost_wave_per_row.log).
  if (wg < P.n_cost) {
    CostRow cr;
    cost_row_issue(A, wg, t, cr);
    cost_row_finish(P, A, wg, t, cr);
  }
}

// workgroups that build the call's tables (kind 1: 8 half-waves per workgroup, at most 4096 workgroups, grid-stride; kind 2: per table
// one workgroup per 1024 entries, at most 1024 per table, grid-stride inside the table); fills jobs->D / hw_end / n (jobs->swap: set before)
int64_t prep_table_wgs(int kind, int32_t S, int32_t K_tab, int n, const int32_t *dims, ChoiceJobs *jobs) {
  int64_t end = 0;
  for (int q = 0; q < n; ++q) {
    if (kind == 1) end += (int64_t)K_tab * S * choice_groups((dims[q] + 3) >> 2, jobs->swap != nullptr);   // half-waves: one per (step, sample, 32-quad group)
    else {
      const int64_t total = (int64_t)K_tab * S * ((dims[q] + 3) & ~3);
      end += std::min<int64_t>((total + 1023) / 1024, 1024);
    }
    jobs->D[q] = dims[q]; jobs->hw_end[q] = end;
  }
  jobs->n = n;
  if (kind == 1) { const int64_t want = (end + 7) / 8; return want < 4096 ? want : 4096; }
  return end;
}
hipError_t launch_prep(const PrepArgs &P, const EncArgs &A, hipStream_t st) {
  const int64_t grid = 1 + (int64_t)P.n_granule + P.n_table_wgs + P.n_cost;
  hipLaunchKernelGGL(prep_kernel, dim3((unsigned)grid), dim3(256), 0, st, P, A);
  return hipGetLastError();
}
hipError_t launch_alpha_choice_all(int64_t seed, int32_t S, int32_t K_tab, const uint16_t *dlog4r, int n, const int32_t *dims,
                                   uint16_t *const *tabs, const uint32_t *const *keeps, hipStream_t st) {
  if (n < 1 || n > 4) return hipErrorInvalidValue;
  ChoiceJobs jobs{};
  const int64_t grid = prep_table_wgs(1, S, K_tab, n, dims, &jobs);
  for (int q = 0; q < n; ++q) { jobs.tab[q] = tabs[q]; jobs.keep[q] = keeps ? keeps[q] : nullptr; }
  hipLaunchKernelGGL(alpha_choice_kernel, dim3(grid > 0 ? (unsigned)grid : 1u), dim3(256), 0, st, seed, S, K_tab, dlog4r, jobs);
  return hipGetLastError();
}
hipError_t launch_alpha_choice(int64_t seed, int32_t S, int32_t D, int32_t K_tab, const uint16_t *dlog4r, uint16_t *tab,
                               const uint32_t *keep, hipStream_t st) {
  return launch_alpha_choice_all(seed, S, K_tab, dlog4r, 1, &D, &tab, &keep, st);
}

} // namespace irec
