// The tiled kernel (pgemm_tile.h), candidates 0-5 with the fused BN-backward
// epilogue of kind 2 (RES, bf16 mask), one or two targets: compiled here,
// launched by pgemm.hip.
#include "pgemm_tile.h"

namespace artsbir {

template void pg_launch_cfg<false, 2, false>(int, const PgArgs&, long long, hipStream_t);
template void pg_launch_cfg<false, 2, true>(int, const PgArgs&, long long, hipStream_t);

}  // namespace artsbir
