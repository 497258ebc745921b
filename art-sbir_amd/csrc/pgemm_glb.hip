// The tiled kernel (pgemm_tile.h) with the epilogue operands read from global
// memory (GLB: candidates 16, 18, 19) and the two-operand fold.
#include "pgemm.h"
#include "pgemm_tile.h"

namespace artsbir {

// candidate 16: the fused BN-backward data gradient (or a plain one with a
// residual / gate operand) on a 128 x 128 tile (4 waves) with 32-k stages
// (3-stage ring, 48 KB) and its epilogue operands read from global memory
// (GLB): three workgroups per CU
bool pg_glb_launch(const PgArgs& a, bool multi, hipStream_t st) {
  if (multi) return false;
  if (!a.bnb) {  // plain epilogue with a residual or gate operand (res_mode 1-3), read from global memory
    if (!a.res_mode || a.bias || a.relu) return false;
    const long long tiles = ((a.M + 127) / 128) * ((a.Cout + 127) / 128);
    if (tiles > 0x7fffffffLL) return false;
    hipLaunchKernelGGL((pgemm_kernel<128, 128, 2, 2, 3, false, 0, false, false, 32, true>), dim3((unsigned)tiles),
                       dim3(256), 0, st, a);
    set_last_kernel("pgemm_kernel<128,128,k32,glb>");
    return true;
  }
  if (a.bnb == 1 && (a.bnb_nt != 1 || a.res_mode)) return false;
  if (a.bnb != 1 && !a.res_mode) return false;
  const long long tiles = ((a.M + 127) / 128) * ((a.Cout + 127) / 128);
  if (tiles > 0x7fffffffLL) return false;
  const dim3 g((unsigned)tiles);
#define PG_GLB(BKV, TWOV) \
  hipLaunchKernelGGL((pgemm_kernel<128, 128, 2, 2, 3, false, BKV, TWOV, false, 32, true>), g, dim3(256), 0, st, a)
  if (a.bnb == 1) PG_GLB(1, false);
  else if (a.bnb == 3 && a.bnb_nt == 2) PG_GLB(3, true);
  else if (a.bnb == 3) PG_GLB(3, false);
  else if (a.bnb_nt == 2) PG_GLB(2, true);
  else PG_GLB(2, false);
#undef PG_GLB
  set_last_kernel("pgemm_kernel<128,128,k32,glb,bnb>");
  return true;
}

// candidate 18: the fused BN-backward RES dgrad with the mask as bits (kind 3,
// one target) on a 256 x 128 tile of 8 waves, 32-k stages in a 3-stage ring
// (72 KB), epilogue operands from global memory: two workgroups (16 waves) per
// CU at 128 VGPRs (the other kinds spill there)
bool pg_glb2_launch(const PgArgs& a, bool multi, hipStream_t st) {
  if (multi || a.bnb != 3 || a.bnb_nt != 1 || !a.res_mode) return false;
  const long long tiles = ((a.M + 255) / 256) * ((a.Cout + 127) / 128);
  if (tiles > 0x7fffffffLL) return false;
  hipLaunchKernelGGL((pgemm_kernel<256, 128, 4, 2, 3, false, 3, false, false, 32, true>), dim3((unsigned)tiles),
                     dim3(512), 0, st, a);
  set_last_kernel("pgemm_kernel<256,128,k32,glb,bnb>");
  return true;
}

// candidate 19: the plain / statistics / bias-ReLU-residual epilogues on the
// 256 x 128 8-wave tile with a 3-stage ring of 32-k stages and operands read
// from global memory (72 KB of LDS): two workgroups per CU at 128 VGPRs
bool pg_k32w8_launch(const PgArgs& a, bool multi, hipStream_t st) {
  if (multi || a.bnb || a.res_mode == 3) return false;
  const long long tiles = ((a.M + 255) / 256) * ((a.Cout + 127) / 128);
  if (tiles > 0x7fffffffLL) return false;
  hipLaunchKernelGGL((pgemm_kernel<256, 128, 4, 2, 3, false, 0, false, false, 32, true>), dim3((unsigned)tiles),
                     dim3(512), 0, st, a);
  set_last_kernel("pgemm_kernel<256,128,k32,glb>");
  return true;
}

// The y-side fold of the block's first conv with the fused BN-backward reduction
// of the previous block's output (artsbir_conv1x1_dgrad_fold_y: residual added,
// kinds 2 / 3, one or two targets): candidates 16 (128 x 128 GLB), 18 (256 x 128
// GLB, kind 3 with one target: the 8-wave tile's 128 VGPRs) and 22 (pp256)
static bool pg_fold_res_launch(const PgArgs& a, int c, hipStream_t st) {
  if (!a.res_mode) return false;
  const bool two = a.bnb_nt == 2;
  switch (c) {
    case 16: {
      if (!pg_fold_ok(a, 128, 32) || pg_ntiles(a, 128, 128) > 0x7fffffffLL) return false;
      const dim3 g((unsigned)pg_ntiles(a, 128, 128));
#define PG_FGLB(BKV, TWOV) \
  hipLaunchKernelGGL((pgemm_kernel<128, 128, 2, 2, 3, false, BKV, TWOV, false, 32, true, true>), g, dim3(256), 0, st, a)
      if (a.bnb == 3 && two) PG_FGLB(3, true);
      else if (a.bnb == 3) PG_FGLB(3, false);
      else if (two) PG_FGLB(2, true);
      else PG_FGLB(2, false);
#undef PG_FGLB
      set_last_kernel("pgemm_kernel<128,128,k32,glb,bnb,fold>");
      return true;
    }
    case 18: {
      if (a.bnb != 3 || two || !pg_fold_ok(a, 256, 32) || pg_ntiles(a, 256, 128) > 0x7fffffffLL) return false;
      hipLaunchKernelGGL((pgemm_kernel<256, 128, 4, 2, 3, false, 3, false, false, 32, true, true>),
                         dim3((unsigned)pg_ntiles(a, 256, 128)), dim3(512), 0, st, a);
      set_last_kernel("pgemm_kernel<256,128,k32,glb,bnb,fold>");
      return true;
    }
    default:
      return false;
  }
}

// The folded BatchNorm-backward data gradient (a.x2: artsbir_conv1x1_dgrad_fold):
// the candidates instantiated with the two-operand loader — 2 (256 x 64), 16 (the
// 128 x 128 GLB tile, plain or ACT epilogue), 19 (256 x 128 GLB, plain), 10 / 14
// (the persistent streaming kernel, plain / ACT, 64- or 128-channel blocks) and 22
// (pp256, in pp256_launch); epilogue: per-segment bias (+ the kind-1 mask and
// BN-backward reduction of the BatchNorm before the conv's input)
bool pg_fold_launch(const PgArgs& a, int c, hipStream_t st) {
  if (!a.x2 || !a.bias || a.relu || a.stats || a.res_mode == 3) return false;
  if (a.bnb == 1 && (a.bnb_nt != 1 || a.res_mode)) return false;
  bool multi;
  if (!pg_supported(a, multi) || multi) return false;
  if (a.bnb == 2 || a.bnb == 3) return pg_fold_res_launch(a, c, st);
  const bool k1 = a.bnb == 1;
  switch (c) {
    case 2: {
      if (!pg_fold_ok(a, 256, 64) || pg_ntiles(a, 256, 64) > 0x7fffffffLL) return false;
      const dim3 g((unsigned)pg_ntiles(a, 256, 64));
      if (k1) hipLaunchKernelGGL((pgemm_kernel<256, 64, 4, 2, 3, false, 1, false, false, 64, false, true>), g, dim3(512), 0, st, a);
      else hipLaunchKernelGGL((pgemm_kernel<256, 64, 4, 2, 3, false, 0, false, false, 64, false, true>), g, dim3(512), 0, st, a);
      set_last_kernel(k1 ? "pgemm_kernel<256,64,bnb,fold>" : "pgemm_kernel<256,64,fold>");
      return true;
    }
    case 16: {
      if (!pg_fold_ok(a, 128, 32) || pg_ntiles(a, 128, 128) > 0x7fffffffLL) return false;
      const dim3 g((unsigned)pg_ntiles(a, 128, 128));
      if (k1) hipLaunchKernelGGL((pgemm_kernel<128, 128, 2, 2, 3, false, 1, false, false, 32, true, true>), g, dim3(256), 0, st, a);
      else hipLaunchKernelGGL((pgemm_kernel<128, 128, 2, 2, 3, false, 0, false, false, 32, true, true>), g, dim3(256), 0, st, a);
      set_last_kernel(k1 ? "pgemm_kernel<128,128,k32,glb,bnb,fold>" : "pgemm_kernel<128,128,k32,glb,fold>");
      return true;
    }
    case 19: {
      if (k1 || !pg_fold_ok(a, 256, 32) || pg_ntiles(a, 256, 128) > 0x7fffffffLL) return false;
      hipLaunchKernelGGL((pgemm_kernel<256, 128, 4, 2, 3, false, 0, false, false, 32, true, true>),
                         dim3((unsigned)pg_ntiles(a, 256, 128)), dim3(512), 0, st, a);
      set_last_kernel("pgemm_kernel<256,128,k32,glb,fold>");
      return true;
    }
    case 10:
    case 14:
    case 17:
      return pstream_fold_launch(a, c, st);
    default:
      return false;
  }
}

}  // namespace artsbir
