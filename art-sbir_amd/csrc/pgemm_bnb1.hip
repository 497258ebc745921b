// The tiled kernel (pgemm_tile.h), candidates 0-5 with the fused BN-backward
// epilogue of kind 1 (ACT): compiled here, launched by pgemm.hip.
#include "pgemm_tile.h"

namespace artsbir {

template void pg_launch_cfg<true, 1, false>(int, const PgArgs&, long long, hipStream_t);
template void pg_launch_cfg<false, 1, false>(int, const PgArgs&, long long, hipStream_t);

}  // namespace artsbir
