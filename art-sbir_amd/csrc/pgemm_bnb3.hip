// The tiled kernel (pgemm_tile.h), candidates 0-5 with the fused BN-backward
// epilogue of kind 3 (RES, mask as bits), one or two targets: compiled here,
// launched by pgemm.hip.
#include "pgemm_tile.h"

namespace artsbir {

template void pg_launch_cfg<false, 3, false>(int, const PgArgs&, long long, hipStream_t);
template void pg_launch_cfg<false, 3, true>(int, const PgArgs&, long long, hipStream_t);

}  // namespace artsbir
