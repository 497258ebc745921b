// Candidate 10 of the conv GEMM (pgemm.h lists the candidates): the persistent
// streaming kernel with the plain, BN-statistics and run-time BN-backward
// epilogues.
#include "pgemm.h"
#include "pstream_kernel.h"

namespace artsbir {

template <bool MULTI, bool BNB, bool FWDS>
static void pstream_launch(int bch, const PgArgs& a, int grid, int ntl, hipStream_t st) {
  if (bch == 32)
    hipLaunchKernelGGL((pstream_kernel<32, 8, 1, 4, MULTI, BNB, FWDS>), dim3(grid), dim3(768), 0, st, a, ntl);
  else if (bch == 64)
    hipLaunchKernelGGL((pstream_kernel<64, 4, 2, 3, MULTI, BNB, FWDS>), dim3(grid), dim3(768), 0, st, a, ntl);
  else hipLaunchKernelGGL((pstream_kernel<128, 4, 2, 3, MULTI, BNB, FWDS>), dim3(grid), dim3(768), 0, st, a, ntl);
}

// candidate 10: the plain, BN-statistics and run-time BN-backward epilogues
bool pstream_plain_launch(const PgArgs& a, bool multi, hipStream_t st) {
  const int bch = a.Cout <= 32 ? 32 : a.Cout <= 64 ? 64 : 128;
  const long long nt = ((a.M + 255) / 256) * ((a.Cout + bch - 1) / bch);
  if (nt > 0x7fffffffLL) return false;
  const int grid = (int)(nt < 256 ? nt : 256);
  const int ntl = (int)nt;
  static const char* pnames[2][3] = {{"pstream_kernel<32>", "pstream_kernel<64>", "pstream_kernel<128>"},
                                     {"pstream_kernel<32,bnb>", "pstream_kernel<64,bnb>", "pstream_kernel<128,bnb>"}};
  set_last_kernel(pnames[a.bnb ? 1 : 0][bch == 32 ? 0 : bch == 64 ? 1 : 2]);
  if (a.bnb) {
    if (multi) pstream_launch<true, true, false>(bch, a, grid, ntl, st);
    else pstream_launch<false, true, false>(bch, a, grid, ntl, st);
  } else if (a.stats) {
    if (multi) pstream_launch<true, false, true>(bch, a, grid, ntl, st);
    else pstream_launch<false, false, true>(bch, a, grid, ntl, st);
  } else {
    if (multi) pstream_launch<true, false, false>(bch, a, grid, ntl, st);
    else pstream_launch<false, false, false>(bch, a, grid, ntl, st);
  }
  return true;
}

}  // namespace artsbir
