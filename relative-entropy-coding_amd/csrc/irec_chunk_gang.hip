// irec_chunk_gang.hip -- the GANG builds of encode_chunk_kernel (irec_chunk.h, "Gangs"): calls of few blocks of more than 1024 dims, each
// coded by several teams.  A translation unit of its own, so that the ten instantiations compile beside the product's instead of behind them.
#include "irec_chunk.h"

namespace irec {

// Gang builds (A.coop_W > 1): the three-team shape of passes of ten beams where its LDS fits (B <= 30), else the one-team
// shape of the beam count -- a gang spreads its members over the CUs, so teams per workgroup only bound how many members a call may have.
static ChunkShape chunk_gang_shape(int B, int S) {
  const ChunkShape c = chunk_shape(B, S);
  if (!c.teams) return c;
  if (c.nb <= 30 && c.nbp == 10 && c.teams == 3) return c;
  return ChunkShape{c.nb, c.nb == 32 ? 16 : 10, 1};            // (the last candidate of every beam count: fits where any does)
}
int chunk_gang_teams(int B, int S) { return chunk_gang_shape(B, S).teams; }
int chunk_gang_nb(int B, int S) { return chunk_gang_shape(B, S).nb; }
size_t chunk_gang_lds_for(int B, int S) { const ChunkShape c = chunk_gang_shape(B, S); return chunk_lds_total(c.nb, c.nbp, S, c.teams); }
const char *chunk_gang_kernel_name(int B, int S) {
  static thread_local char buf[56];
  const ChunkShape c = chunk_gang_shape(B, S);
  snprintf(buf, sizeof buf, "encode_chunk_kernel<%d,%d,%d,gang>", c.nb, c.nbp, c.teams);
  return buf;
}
hipError_t launch_encode_chunk_gang(const EncArgs &A, int grid, hipStream_t st) {
  const ChunkShape c = chunk_gang_shape(A.B, A.S);
  if (!c.teams || A.max_dim_pad <= FAST_MAX_DIM || A.max_dim_pad > CHUNK_MAX_DIM) return hipErrorInvalidValue;
  if (A.coop_W < 2 || A.gang_chunks < 1 || A.coop_W % A.gang_chunks != 0 || !A.gang_xch || A.n_blocks > GANG_MAX_BLOCKS ||
      A.n_blocks * (int64_t)A.coop_W > (int64_t)grid * c.teams)
    return hipErrorInvalidValue;
  switch (c.nb * 1000 + c.nbp * 10 + c.teams) {
    case 10103: return launch_chunk_t<10, 10, 3, true>(A, grid, st);
    case 20103: return launch_chunk_t<20, 10, 3, true>(A, grid, st);
    case 30103: return launch_chunk_t<30, 10, 3, true>(A, grid, st);
    case 10101: return launch_chunk_t<10, 10, 1, true>(A, grid, st);
    case 20101: return launch_chunk_t<20, 10, 1, true>(A, grid, st);
    case 30101: return launch_chunk_t<30, 10, 1, true>(A, grid, st);
    case 32161: return launch_chunk_t<32, 16, 1, true>(A, grid, st);
    case 40101: return launch_chunk_t<40, 10, 1, true>(A, grid, st);
    case 50101: return launch_chunk_t<50, 10, 1, true>(A, grid, st);
    case 60101: return launch_chunk_t<60, 10, 1, true>(A, grid, st);
    default: return hipErrorInvalidValue;
  }
}

} // namespace irec
