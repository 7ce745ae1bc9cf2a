// irec_chunk.hip -- the product builds of encode_chunk_kernel (irec_chunk.h): one team codes a block of more than 1024 dims.  The shape
// queries the planner asks and the launcher.  Not an object of its own: irec_team.hip includes it at its end and says why.
#include "irec_chunk.h"

namespace irec {

int chunk_teams(int B, int S) { return chunk_shape(B, S).teams; }
bool chunk_applies(int B, int S, int max_dim) {
  return max_dim > FAST_MAX_DIM && max_dim <= CHUNK_MAX_DIM && chunk_shape(B, S).teams != 0;
}
size_t chunk_lds_for(int B, int S) { const ChunkShape c = chunk_shape(B, S); return chunk_lds_total(c.nb, c.nbp, S, c.teams); }
size_t chunk_ws_for(int B, int dpad, int max_K) { return chunk_ws_bytes(chunk_nb(B) ? chunk_nb(B) : 60, dpad, max_K); }
const char *chunk_kernel_name(int B, int S) {
  static thread_local char buf[48];
  const ChunkShape c = chunk_shape(B, S);
  snprintf(buf, sizeof buf, "encode_chunk_kernel<%d,%d,%d>", c.nb, c.nbp, c.teams);
  return buf;
}
hipError_t launch_encode_chunk(const EncArgs &A, int grid, hipStream_t st) {
  if (!chunk_applies(A.B, A.S, A.max_dim_pad)) return hipErrorInvalidValue;
  if (A.coop_W > 1) return launch_encode_chunk_gang(A, grid, st);
  const ChunkShape c = chunk_shape(A.B, A.S);
  switch (c.nb * 1000 + c.nbp * 10 + c.teams) {
    case 10103: return launch_chunk_t<10, 10, 3>(A, grid, st);
    case 10102: return launch_chunk_t<10, 10, 2>(A, grid, st);
    case 10101: return launch_chunk_t<10, 10, 1>(A, grid, st);
    case 20103: return launch_chunk_t<20, 10, 3>(A, grid, st);
    case 20101: return launch_chunk_t<20, 10, 1>(A, grid, st);
    case 30103: return launch_chunk_t<30, 10, 3>(A, grid, st);
    case 30102: return launch_chunk_t<30, 10, 2>(A, grid, st);
    case 30101: return launch_chunk_t<30, 10, 1>(A, grid, st);
    case 32162: return launch_chunk_t<32, 16, 2>(A, grid, st);
    case 32161: return launch_chunk_t<32, 16, 1>(A, grid, st);
    case 40102: return launch_chunk_t<40, 10, 2>(A, grid, st);
    case 40101: return launch_chunk_t<40, 10, 1>(A, grid, st);
    case 50102: return launch_chunk_t<50, 10, 2>(A, grid, st);
    case 50101: return launch_chunk_t<50, 10, 1>(A, grid, st);
    case 60102: return launch_chunk_t<60, 10, 2>(A, grid, st);
    case 60101: return launch_chunk_t<60, 10, 1>(A, grid, st);
    default: return hipErrorInvalidValue;
  }
}

} // namespace irec
