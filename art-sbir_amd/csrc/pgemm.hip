// The dispatcher of the conv GEMM candidates (pgemm.h lists them) and the
// tiled kernel's plain tile shapes, candidates 0-5.  The kernel families:
// pgemm_tile.h (the tiled kernel; pgemm_bnb1/2/3.hip, pgemm_pf.hip and
// pgemm_glb.hip hold its other launcher groups), pstream.hip / pstream_k.hip,
// conv3x3.hip, pp256.hip, rstream.hip.
#include <string>

#include "../../include/artsbir.h"
#include "pgemm.h"
#include "pgemm_tile.h"

namespace artsbir {

// the tuner's candidates in trial order (tune::fastest keeps the first of equal
// times); -2 is the register-staged kernel of gemm.hip
const std::vector<int>& pgemm_tune_candidates() {
  static const std::vector<int> cands = {-2, 0,  1,  2,  3,  4,  5,  10, 11, 12, 13,
                                         14, 15, 16, 18, 19, 20, 21, 22, 24, 25, 26};
  return cands;
}

// candidates 0-5, plain: compiled here (the others: pgemm_bnb1/2/3.hip)
template void pg_launch_cfg<true, 0, false>(int, const PgArgs&, long long, hipStream_t);
template void pg_launch_cfg<false, 0, false>(int, const PgArgs&, long long, hipStream_t);

// the fused-epilogue variant of a launch: ACT (kind 1, one target, no
// residual) or RES (kinds 2/3, residual present, one or two targets)
template <bool MULTI>
static bool pg_launch_bnb(int c, const PgArgs& a, long long tiles, hipStream_t st) {
  if (a.bnb == 1) {
    if (a.bnb_nt != 1 || a.res_mode) return false;
    pg_launch_cfg<MULTI, 1, false>(c, a, tiles, st);
    return true;
  }
  if (MULTI || !a.res_mode) return false;  // RES dgrads: 1x1 convs over >= 64 channels, residual added
  if (a.bnb == 3) {
    if (a.bnb_nt == 2) pg_launch_cfg<false, 3, true>(c, a, tiles, st);
    else pg_launch_cfg<false, 3, false>(c, a, tiles, st);
  } else {
    if (a.bnb_nt == 2) pg_launch_cfg<false, 2, true>(c, a, tiles, st);
    else pg_launch_cfg<false, 2, false>(c, a, tiles, st);
  }
  return true;
}

// the candidates: pgemm.h
bool pgemm_launch_cfg(const PgArgs& a, int c, hipStream_t st) {
  if (a.x2 || a.w_sstride) return c == 22 ? pp256_launch(a, false, st) : pg_fold_launch(a, c, st);
  const bool act = a.bias != nullptr || a.relu != 0;  // bias / ReLU epilogue: pgemm_kernel and pstream only
  if (act && (a.stats || a.bnb)) return false;
  // res_mode 3 (gated data gradient, pg_epilogue_k only): the plain pgemm_kernel tiles
  if (c == 22 || c == 23) return pp256_launch(a, c == 23, st);  // pp256.hip: every epilogue it supports
  if (c == 26) return rstream_launch(a, st);                      // rstream.hip: RES-kind 1x1 dgrads
  if (a.res_mode == 3 && (c < 0 || (c >= kNumCfg && c != 16 && (c < 11 || c > 13)) || a.bnb || a.R * a.S != 1))
    return false;
  if (c == 20) return !act && sconv_launch(a, st);
  if (c == 21) return hconv_launch(a, st);  // bias / ReLU epilogue supported
  if (act && c >= 11 && c <= 13) return false;
  bool multi;
  if (!pg_supported(a, multi)) return false;
  if (c >= 11 && c <= 13) return pg_pf_launch(c, a, multi, st);
  if (c == 14) return pstream_bnb_launch(a, multi, st);
  if (c == 15) return pstream_k32_launch(a, multi, st);
  if (c == 24 || c == 25) {  // 10 / 15 with the forward-statistics epilogue's stores non-temporal
    if (!a.stats || a.bnb || a.bias || a.relu) return false;
    PgArgs b = a;
    b.nts = 1;
    if (!pgemm_launch_cfg(b, c == 24 ? 10 : 15, st)) return false;
    const std::string base = artsbir_last_kernel();
    static const char* nt_names[] = {"pstream_kernel<32,nt>", "pstream_kernel<64,nt>", "pstream_kernel<128,nt>",
                                     "pstream_kernel<64,k32,nt>", "pstream_kernel<128,k32,nt>"};
    const char* nm = base == "pstream_kernel<32>"       ? nt_names[0]
                     : base == "pstream_kernel<64>"     ? nt_names[1]
                     : base == "pstream_kernel<128>"    ? nt_names[2]
                     : base == "pstream_kernel<64,k32>" ? nt_names[3]
                                                        : nt_names[4];
    set_last_kernel(nm);
    return true;
  }
  if (c == 16) return pg_glb_launch(a, multi, st);
  if (c == 18) return pg_glb2_launch(a, multi, st);
  if (c == 19) return pg_k32w8_launch(a, multi, st);
  if (c == 10) return pstream_plain_launch(a, multi, st);
  if (c < 0 || c >= kNumCfg) return false;
  if (c == 5 && multi) return false;
  const PgCfg& g = kCfgs[c];
  const long long tiles = ((a.M + g.bpx - 1) / g.bpx) * ((a.Cout + g.bch - 1) / g.bch);
  if (tiles > 0x7fffffffLL) return false;
  static const char* names[2][kNumCfg] = {
      {"pgemm_kernel<256,256>", "pgemm_kernel<256,128>", "pgemm_kernel<256,64>", "pgemm_kernel<128,128>",
       "pgemm_kernel<256,32>", "pgemm_kernel<256,256,k32>"},
      {"pgemm_kernel<256,256,bnb>", "pgemm_kernel<256,128,bnb>", "pgemm_kernel<256,64,bnb>",
       "pgemm_kernel<128,128,bnb>", "pgemm_kernel<256,32,bnb>", "pgemm_kernel<256,256,k32,bnb>"}};
  if (a.bnb) {
    if (!(multi ? pg_launch_bnb<true>(c, a, tiles, st) : pg_launch_bnb<false>(c, a, tiles, st))) return false;
  } else {
    if (multi) pg_launch_cfg<true, 0, false>(c, a, tiles, st);
    else pg_launch_cfg<false, 0, false>(c, a, tiles, st);
  }
  set_last_kernel(names[a.bnb ? 1 : 0][c]);
  return true;
}

// static choice (no tuning): streaming kernel for many tiles, else best-scored tile
int pgemm_default_cfg(const PgArgs& a) {
  if (sconv_ok(a) && !a.bias && !a.relu && a.res_mode != 3) return 20;
  bool multi;
  if (!pg_supported(a, multi)) return -1;
  const int bch = a.Cout <= 32 ? 32 : a.Cout <= 64 ? 64 : 128;
  if (((a.M + 255) / 256) * ((a.Cout + bch - 1) / bch) >= 4 * 256 && a.res_mode != 3) return 10;
  int best = -1;
  float best_score = -1.f;
  for (int c = 0; c < 5; ++c) {
    const PgCfg& g = kCfgs[c];
    const long long tiles = ((a.M + g.bpx - 1) / g.bpx) * ((a.Cout + g.bch - 1) / g.bch);
    const double util = (double)a.M * a.Cout / ((double)tiles * g.bpx * g.bch);
    const int per_cu = (160 * 1024) / g.lds;
    const long long slots = 256LL * (per_cu < 1 ? 1 : per_cu);
    const long long waves = (tiles + slots - 1) / slots;
    const double fill = (double)tiles / (double)(waves * slots);
    const float score = (float)(g.factor * util * fill);
    if (score > best_score) { best_score = score; best = c; }
  }
  return best;
}

}  // namespace artsbir
