// irec_team_common.h -- pieces shared by the team encoders (irec_team.hip, irec_ten.hip, irec_chunk.h): team size, the three
// quantile-table copies at the start of the LDS, the team barrier, and the LDS geometry of a team (partial scores, sort keys, sample
// passes) that encode_team_kernel and encode_chunk_kernel both carve their share of the LDS by.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "irec_device.h"
#include "irec_kernels.h"
#include "irec_fast_common.h"   // SmallLdsT

namespace irec {

constexpr int TEAM_NW = 4;                       // waves per team
constexpr int TEAM_NT = TEAM_NW * 64;            // threads per team
constexpr uint32_t T3_FLOATS = 3u * IREC_PM1;    // three copies of lut2
constexpr size_t T3_BYTES = ((size_t)T3_FLOATS * 4 + 15) & ~(size_t)15;


// Barrier of the 4 waves of one team: a monotonic LDS counter.  LDS operations of one wave execute in program order and
// the LDS serves one instruction at a time, so a wave's earlier writes are in place before its add lands; the fences
// order the global slab traffic (vmcnt) the way __syncthreads would.
struct TeamBarrier {
  uint32_t *cnt;
  uint32_t epoch;
  uint32_t n_waves;
  __device__ __forceinline__ void operator()() {
    epoch += n_waves;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    if ((threadIdx.x & 63) == 0) __hip_atomic_fetch_add(cnt, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    for (;;) {
      const uint32_t v = (uint32_t)__builtin_amdgcn_readfirstlane((int)__hip_atomic_load(cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP));
      if ((int32_t)(v - epoch) >= 0) break; // every wave of the team has arrived
      __builtin_amdgcn_s_sleep(1);   // (64 clocks between two polls; 0 / 2 / 4: neutral within 0.3 %, r05l)
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
  }
};

// ---- LDS geometry of a team ----
// beams a team serves at most (sizes its small LDS arrays): 32 for the builds of up to 32 beams -- the three-team 20-beam
// build has no LDS to spare -- and 64 (with room for 512 selection survivors) for the 60-beam build
__host__ __device__ constexpr int team_mb(int NB) { return NB <= 32 ? 32 : 64; }
template <int NB> using TeamLdsT = SmallLdsT<(NB <= 32 ? 32 : 64), (NB <= 32 ? 32 : 64), (NB <= 32 ? 64 : 512)>;
__host__ __device__ inline size_t team_small_bytes(int NB) {
  return NB <= 32 ? ((sizeof(TeamLdsT<32>) + 15) & ~(size_t)15) : ((sizeof(TeamLdsT<64>) + 15) & ~(size_t)15);
}
// Sample passes.  The per-group partial scores of SP samples sit in LDS at a time ([4][SP][NB] f32); a step scores S in
// ceil(S / SP) passes, each followed by the group combine into the sort keys ([S*NB] u32, all of them resident).  Every
// BASELINE configuration with B <= 20 takes one pass; the 30-beam stress configuration (S = 148) takes four of 37.
// (`ps` below: beam slots per sample in the partial-score rows and the key array -- NB, or 1 when the call has ONE beam
//  (B = 1 of the reference's sweep: a 10-beam layout would spend ten times the LDS per sample and ten times the passes))
__host__ __device__ inline int team_row(int NB, int B) { return (NB == 10 && B == 1) ? 1 : NB; }
__host__ __device__ inline size_t team_key_bytes(int ps, int S) { return (((size_t)S * ps * 4) + 15) & ~(size_t)15; }
// Keys in LDS unless they alone would leave room for fewer than 16 samples of partials (single-team builds only: 12 090
// candidates of B = 30, S = 403 are 48 KB); then they live in the team's scratch slab (L2) and the selection scans them there.
// (`passes`: a multi-team build that scores S in passes -- round 3, B <= 10 with more samples than one pass holds; the
//  other multi-team builds take S in one pass and keep their keys in LDS by construction)
__host__ __device__ inline bool team_keys_in_lds(int NB, int S, int teams, bool passes, int ps = 0) {
  if (ps <= 0) ps = NB;
  const long long avail = (long long)((FAST_LDS_LIMIT - T3_BYTES) / (size_t)teams) - (long long)team_key_bytes(ps, S) -
                          (long long)team_small_bytes(NB) - 32;
  return (teams > 1 && !passes) || avail / (4LL * ps * 4) >= (S < 16 ? S : 16);
}
// Three 20-beam teams only fit the 160 KB next to the table copies if the sort keys are written over group 0 of the partial
// scores (key f = s * Bcur + b lands on partial s * NB + b: the same word when Bcur == NB, which every step but the first
// has; otherwise a barrier separates the partial reads from the key writes).
__host__ __device__ inline bool team_keys_alias(int NB, int teams) { return teams >= 3 && NB == 20; }
__host__ __device__ inline int team_s_pass(int NB, int S, int teams, int cmax, bool passes = false, int ps = 0) {
  if (ps <= 0) ps = NB;
  const long long avail = (long long)((FAST_LDS_LIMIT - T3_BYTES) / (size_t)teams) -
                          ((team_keys_in_lds(NB, S, teams, passes, ps) && !(team_keys_alias(NB, teams) && !passes)) ? (long long)team_key_bytes(ps, S) : 0) -
                          (long long)team_small_bytes(NB) - 32;
  long long fit = avail / (4LL * ps * 4);           // samples whose partials fit
  if (fit > cmax / ps) fit = cmax / ps;             // and whose candidates one combine round covers
  if (fit < 1) return 0;
  if (fit >= S) return S;
  const int n_pass = (int)((S + fit - 1) / fit);
  return (S + n_pass - 1) / n_pass;                 // balanced passes
}
__host__ __device__ inline size_t team_part_bytes(int ps, int SP) { return (((size_t)4 * SP * ps * 4) + 15) & ~(size_t)15; }
__host__ __device__ inline size_t team_lds_one(int NB, int S, int SP, int teams, bool passes = false, int ps = 0) {
  if (ps <= 0) ps = NB;
  return team_part_bytes(ps, SP) + ((team_keys_in_lds(NB, S, teams, passes, ps) && !(team_keys_alias(NB, teams) && !passes)) ? team_key_bytes(ps, S) : 0) +
         team_small_bytes(NB) + 16;
}
__host__ __device__ inline size_t team_lds_total(int NB, int S, int SP, int teams, bool passes = false, int ps = 0) {
  return T3_BYTES + (size_t)teams * team_lds_one(NB, S, SP, teams, passes, ps);
}

} // namespace irec
