// The tiled kernel (pgemm_tile.h) with the epilogue operands prefetched into
// registers: candidates 11-13.
#include "pgemm.h"
#include "pgemm_tile.h"

namespace artsbir {

// PF variants (candidates 11 / 12 / 13 = tile shapes 1 / 2 / 3 with the
// epilogue operands prefetched into registers)
template <int BK, bool TWO>
static void pg_launch_pf(int base, const PgArgs& a, long long tiles, hipStream_t st) {
  const dim3 g((unsigned)tiles);
  switch (base) {
    case 1: hipLaunchKernelGGL((pgemm_kernel<256, 128, 4, 2, 3, false, BK, TWO, true>), g, dim3(512), 0, st, a); break;
    case 2: hipLaunchKernelGGL((pgemm_kernel<256, 64, 4, 2, 3, false, BK, TWO, true>), g, dim3(512), 0, st, a); break;
    default: hipLaunchKernelGGL((pgemm_kernel<128, 128, 2, 2, 2, false, BK, TWO, true>), g, dim3(256), 0, st, a); break;
  }
}

bool pg_pf_launch(int c, const PgArgs& a, bool multi, hipStream_t st) {
  const int base = c - 10;
  if (multi || base < 1 || base > 3) return false;
  if (a.bnb == 2 || (a.bnb == 1 && (a.bnb_nt != 1 || a.res_mode)) || (a.bnb == 3 && !a.res_mode)) return false;
  // plain: the data gradient with a residual, or the gated GEMM (res_mode 3, column sums in stats)
  if (!a.bnb && (!a.res_mode || (a.stats && a.res_mode != 3))) return false;
  const PgCfg& g = kCfgs[base];
  const long long tiles = ((a.M + g.bpx - 1) / g.bpx) * ((a.Cout + g.bch - 1) / g.bch);
  if (tiles > 0x7fffffffLL) return false;
  if (a.bnb == 1) pg_launch_pf<1, false>(base, a, tiles, st);
  else if (a.bnb == 3 && a.bnb_nt == 2) pg_launch_pf<3, true>(base, a, tiles, st);
  else if (a.bnb == 3) pg_launch_pf<3, false>(base, a, tiles, st);
  else pg_launch_pf<0, false>(base, a, tiles, st);
  static const char* names[2][3] = {{"pgemm_kernel<256,128,pf>", "pgemm_kernel<256,64,pf>", "pgemm_kernel<128,128,pf>"},
                                    {"pgemm_kernel<256,128,bnb,pf>", "pgemm_kernel<256,64,bnb,pf>",
                                     "pgemm_kernel<128,128,bnb,pf>"}};
  set_last_kernel(names[a.bnb ? 1 : 0][base - 1]);
  return true;
}

}  // namespace artsbir
