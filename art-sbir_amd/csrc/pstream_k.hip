// The persistent streaming kernel (pstream_kernel.h) past candidate 10: the
// compile-time fused BN-backward epilogue (14), 32-k stages (15) and the
// two-operand fold (10 / 14 / 17, and with its weight-gradient operands).
#include "pgemm.h"
#include "pstream_kernel.h"

namespace artsbir {

template <int BK, bool TWO>
static void pstream_launch_k(int bch, const PgArgs& a, int grid, int ntl, hipStream_t st) {
  constexpr bool ONLY64 = TWO || BK == 1;  // 128-channel blocks would spill there
  if (ONLY64 || bch == 64)
    hipLaunchKernelGGL((pstream_kernel<64, 4, 2, 3, false, true, false, BK, TWO>), dim3(grid), dim3(768), 0, st, a, ntl);
  else if constexpr (!ONLY64)
    hipLaunchKernelGGL((pstream_kernel<128, 4, 2, 3, false, true, false, BK, TWO>), dim3(grid), dim3(768), 0, st, a,
                       ntl);
}

// candidate 15: the persistent streaming kernel with 32-k stages (six in the
// LDS the 64-k form holds three in; plain and forward-statistics epilogues,
// C % 64 == 0, 64- / 128-channel blocks)
bool pstream_k32_launch(const PgArgs& a, bool multi, hipStream_t st) {
  if (multi || a.bnb || a.Cout <= 32) return false;
  const int bch = a.Cout <= 64 ? 64 : 128;
  const long long nt = ((a.M + 255) / 256) * ((a.Cout + bch - 1) / bch);
  if (nt > 0x7fffffffLL) return false;
  const int grid = (int)(nt < 256 ? nt : 256), ntl = (int)nt;
  set_last_kernel(bch == 64 ? "pstream_kernel<64,k32>" : "pstream_kernel<128,k32>");
  if (a.stats) {
    if (bch == 64)
      hipLaunchKernelGGL((pstream_kernel<64, 4, 2, 6, false, false, true, 0, false, 32>), dim3(grid), dim3(768), 0, st, a,
                         ntl);
    else hipLaunchKernelGGL((pstream_kernel<128, 4, 2, 6, false, false, true, 0, false, 32>), dim3(grid), dim3(768), 0,
                            st, a, ntl);
  } else {
    if (bch == 64)
      hipLaunchKernelGGL((pstream_kernel<64, 4, 2, 6, false, false, false, 0, false, 32>), dim3(grid), dim3(768), 0, st,
                         a, ntl);
    else hipLaunchKernelGGL((pstream_kernel<128, 4, 2, 6, false, false, false, 0, false, 32>), dim3(grid), dim3(768), 0,
                            st, a, ntl);
  }
  return true;
}

// candidate 14: the persistent streaming kernel with the specialised fused
// BN-backward epilogue (the kinds pg_launch_bnb takes, channel blocks 64 / 128)
bool pstream_bnb_launch(const PgArgs& a, bool multi, hipStream_t st) {
  if (!a.bnb || multi || a.Cout < 64) return false;
  if (a.bnb == 1 && (a.bnb_nt != 1 || a.res_mode)) return false;
  if (a.bnb != 1 && !a.res_mode) return false;
  const int bch = (a.Cout <= 64 || a.bnb == 1 || a.bnb_nt == 2) ? 64 : 128;  // see pstream_launch_k
  const long long nt = ((a.M + 255) / 256) * ((a.Cout + bch - 1) / bch);
  if (nt > 0x7fffffffLL) return false;
  const int grid = (int)(nt < 256 ? nt : 256), ntl = (int)nt;
  set_last_kernel(bch == 64 ? "pstream_kernel<64,bnbk>" : "pstream_kernel<128,bnbk>");
  if (a.bnb == 1) pstream_launch_k<1, false>(bch, a, grid, ntl, st);
  else if (a.bnb == 3 && a.bnb_nt == 2) pstream_launch_k<3, true>(bch, a, grid, ntl, st);
  else if (a.bnb == 3) pstream_launch_k<3, false>(bch, a, grid, ntl, st);
  else if (a.bnb_nt == 2) pstream_launch_k<2, true>(bch, a, grid, ntl, st);
  else pstream_launch_k<2, false>(bch, a, grid, ntl, st);
  return true;
}

// The streaming candidates of the folded BatchNorm-backward data gradient
// (pg_fold_launch, which has checked what all its candidates share): 10 / 14
// plain / ACT on 64- or 128-channel blocks, 17 either on 32-channel blocks
bool pstream_fold_launch(const PgArgs& a, int c, hipStream_t st) {
  const bool k1 = a.bnb == 1;
  switch (c) {
    case 10:
    case 14: {
      if ((c == 14) != k1 || !pg_fold_ok(a, 256, 64) || a.Cout < 64) return false;
      const int bch = (k1 || a.Cout <= 64) ? 64 : 128;  // the ACT epilogue: 64-channel blocks (pstream_launch_k)
      const long long nt = pg_ntiles(a, 256, bch);
      if (nt > 0x7fffffffLL) return false;
      const int grid = (int)(nt < 256 ? nt : 256);
      if (k1)
        hipLaunchKernelGGL((pstream_kernel<64, 4, 2, 3, false, true, false, 1, false, 64, true>), dim3(grid), dim3(768), 0,
                           st, a, (int)nt);
      else if (bch == 64)
        hipLaunchKernelGGL((pstream_kernel<64, 4, 2, 3, false, false, false, 0, false, 64, true>), dim3(grid), dim3(768),
                           0, st, a, (int)nt);
      else
        hipLaunchKernelGGL((pstream_kernel<128, 4, 2, 3, false, false, false, 0, false, 64, true>), dim3(grid), dim3(768),
                           0, st, a, (int)nt);
      set_last_kernel(k1 ? "pstream_kernel<64,bnbk,fold>" : bch == 64 ? "pstream_kernel<64,fold>" : "pstream_kernel<128,fold>");
      return true;
    }
    case 17: {  // the persistent streaming kernel with 32-channel blocks (four tiles per pixel panel)
      if (!pg_fold_ok(a, 256, 64) || a.Cout < 32 || a.Cout % 32) return false;
      const long long nt = pg_ntiles(a, 256, 32);
      if (nt > 0x7fffffffLL) return false;
      const int grid = (int)(nt < 256 ? nt : 256);
      if (k1)
        hipLaunchKernelGGL((pstream_kernel<32, 8, 1, 4, false, true, false, 1, false, 64, true>), dim3(grid), dim3(768), 0,
                           st, a, (int)nt);
      else
        hipLaunchKernelGGL((pstream_kernel<32, 8, 1, 4, false, false, false, 0, false, 64, true>), dim3(grid), dim3(768),
                           0, st, a, (int)nt);
      set_last_kernel(k1 ? "pstream_kernel<32,bnbk,fold>" : "pstream_kernel<32,fold>");
      return true;
    }
    default:
      return false;
  }
}

// The fold data gradient together with its weight-gradient operands (a.wg_p,
// a.wg_gram): the persistent streaming kernel whose loader waves accumulate
// g^T x and x^T x from the stages they stream (pstream_wg_loader).  Layers with
// 64 input channels under a 256-channel output (K = 320: layer 1's conv3 and
// downsample conv), contiguous NHWC operands, whole 256-pixel tiles.
bool pg_fold_wg_launch(const PgArgs& a, hipStream_t st) {
  if (!a.x2 || !a.wg_p || !a.wg_gram || !a.bias || a.relu || a.stats || a.res_mode) return false;
  if (a.bnb && (a.bnb != 1 || a.bnb_nt != 1)) return false;
  if (a.Cout != 64 || a.K != 320 || a.C1 != 256 || a.C != a.K) return false;
  bool multi;
  if (!pg_supported(a, multi) || multi || !pg_fold_ok(a, 256, 64)) return false;
  if (a.M % 256 || (a.seg_m > 0 && a.seg_m % 256)) return false;
  if (a.sW != a.C1 || a.sH != (long long)a.W * a.sW || a.sN != (long long)a.H * a.sH) return false;
  if (a.sW2 != a.Cout || a.sH2 != (long long)a.W * a.sW2 || a.sN2 != (long long)a.H * a.sH2) return false;
  const long long nt = a.M / 256;
  if (nt > 0x7fffffffLL) return false;
  const int grid = (int)(nt < 256 ? nt : 256);
  if (a.bnb == 1) {
    hipLaunchKernelGGL((pstream_kernel<64, 4, 2, 3, false, true, false, 1, false, 64, true, 320>), dim3(grid),
                       dim3(768), 0, st, a, (int)nt);
    set_last_kernel("pstream_kernel<64,bnbk,fold,wg>");
  } else {
    hipLaunchKernelGGL((pstream_kernel<64, 4, 2, 3, false, false, false, 0, false, 64, true, 320>), dim3(grid),
                       dim3(768), 0, st, a, (int)nt);
    set_last_kernel("pstream_kernel<64,fold,wg>");
  }
  return true;
}

}  // namespace artsbir
