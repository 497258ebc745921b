// Pipelined implicit-GEMM convolution (bf16 in, f32 accumulate, bf16 out) for
// gfx950: conv forward and conv data-gradient of the encoder
// (models.py:198-221 Bottleneck convs, models.py:310-316 stem).
//
// Structure (cdna_hip_programming.md §5, "glds" rows):
//  * the output tile is computed transposed, out^T[channel][pixel], so that an
//    MFMA accumulator lane holds 4 consecutive channels of one pixel; with the
//    channel order inside the tile permuted (below) a lane holds 8 consecutive
//    channels across two 16-row MFMA tiles and the epilogue stores 16-B bf16
//    vectors straight from registers (no LDS staging, BN statistics from the
//    f32 accumulators);
//  * both operands are staged by LDS-DMA (buffer_load ... lds, 16 B per lane):
//    one wave instruction fills 8 rows x 128 B (8 lanes per row = one full
//    128-B line of k), the LDS image of a row is its 8 k-chunks in slot order
//    chunk ^ (row & 7) (the XOR swizzle is applied to the per-lane SOURCE
//    address; the LDS destination stays lane-linear), which makes the MFMA
//    fragment reads (16 rows x one chunk per ds_read_b128) conflict-free;
//  * an NSTAGE ring of LDS stages, one raw s_barrier per K-step, counted
//    s_waitcnt vmcnt so that NSTAGE-2 stages stay in flight across the barrier;
//  * implicit im2col: per pixel row a tap-validity mask; out-of-range (padding,
//    tails) source offsets are 0x80000000, which the buffer unit turns into
//    zeros written to LDS.
//
// The tiled kernel and its tile-shape switch live in this header because
// several units instantiate them, one per launcher group: pgemm.hip (candidates
// 0-5, plain), pgemm_bnb1/2/3.hip (0-5 with the fused BN-backward epilogue of
// kind 1 / 2 / 3), pgemm_pf.hip (11-13) and pgemm_glb.hip (16, 18, 19, the fold).
#pragma once
#include "pgemm_dev.h"

namespace artsbir {

// BK (0 / 1 / 2 / 3, see pg_epilogue_k) and TWO select the fused epilogue.
// PF: epilogue operands prefetched into registers before the main loop
// (epi_prefetch) instead of staged through LDS after it
// KS: k per stage.  64: LDS rows of 128 B (8 chunks, slot = chunk ^ (row & 7),
// 8 rows per DMA instruction).  32: rows of 64 B (4 chunks, slot = chunk ^
// ((row >> 2) & 2), 16 rows per DMA instruction; conflict-free for the
// ds_read_b128 lane groups {0-3,12-15,20-27}, {4-11,16-19,28-31}, ... of
// MI355X_MICROARCH §LDS — the earlier chunk ^ ((row >> 2) & 3) put rows r and
// r+4 of one group on the same banks, 2-way) — half the bytes per stage, so
// the same LDS holds twice the stages and more of them are in flight (C % 64
// == 0 only)
// GLB (fused BN-backward only): the epilogue reads y, residual, mask and BN
// constants straight from global memory (no LDS staging, no parameter table),
// so the LDS is the stage ring alone and several workgroups share a CU: one's
// epilogue streams while another's main loop runs
// X2 (1x1 only): the BatchNorm-backward fold of artsbir_conv1x1_dgrad_fold — the
// reduction runs over two operands (k < C1 from x, the rest from x2), the
// weights and the bias are those of the tile's BN segment
template <int BPX, int BCH, int WPX, int WCH, int NSTAGE, bool MULTI, int BK, bool TWO, bool PF = false, int KS = 64,
          bool GLB = false, bool X2 = false>
__global__ void __launch_bounds__(64 * WPX * WCH, GLB ? (WPX * WCH == 8 ? 4 : 3) : 1) pgemm_kernel(PgArgs a) {
  constexpr bool BNB = BK != 0;
  static_assert(!GLB || !PF, "GLB: operands from global memory, not prefetched into registers");
  static_assert(!PF || BK != 2, "PF: the bf16 mask operand of kind 2 is not prefetched");
  static_assert(KS == 64 || (KS == 32 && !MULTI), "32-k stages: uniform taps only");
  constexpr int ROWB = 2 * KS, RPI = 1024 / ROWB, CPR = ROWB / 16;
  constexpr int NW = WPX * WCH;
  constexpr int PXB = BPX * ROWB, CHB = BCH * ROWB, STAGE = PXB + CHB;
  constexpr int IPX = BPX / (RPI * NW);
  constexpr int ICH_TOT = BCH / RPI;
  constexpr int ICH = (ICH_TOT + NW - 1) / NW;
  constexpr int WTPX = BPX / WPX, WTCH = BCH / WCH;
  constexpr int NTP = WTPX / 16, MTC = WTCH / 16;
  constexpr int LPS_HI = IPX + ICH;                            // loads per stage, waves with ICH weight loads
  constexpr int LPS_LO = IPX + ICH_TOT / NW;                   // ... waves with one fewer
  static_assert(IPX >= 1 && IPX * RPI * NW == BPX, "pixel loader");
  static_assert(MTC % 2 == 0 && WTCH % 32 == 0, "channel pairs");
  // stage ring | BN statistics accumulator | (BNB) BN constants | (BNB) mask bits
  constexpr int XTRA = (BNB && !GLB) ? pg_prm_bytes<BCH>() + BPX * (BCH / 8) : 0;
  __shared__ __attribute__((aligned(16))) char smem[NSTAGE * STAGE + pg_red_bytes<BCH>() + XTRA];
  float* red = reinterpret_cast<float*>(smem + NSTAGE * STAGE);
  int* red_cnt = reinterpret_cast<int*>(smem + NSTAGE * STAGE + 6 * BCH * 4);
  float* prm = reinterpret_cast<float*>(smem + NSTAGE * STAGE + pg_red_bytes<BCH>());
  unsigned char* sbits = reinterpret_cast<unsigned char*>(smem + NSTAGE * STAGE + pg_red_bytes<BCH>() +
                                                          pg_prm_bytes<BCH>());

  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wpx = wid % WPX, wch = wid / WPX;
  const int ntc = (a.Cout + BCH - 1) / BCH;
  const long long ntp = (a.M + BPX - 1) / BPX;
  const long long lid = pg_xcd_remap(blockIdx.x, ntp * ntc);
  const long long bpx = (lid / ntc) * BPX;
  const int bch = (int)(lid % ntc) * BCH;
  const long long seg0 = a.seg_m > 0 ? bpx / a.seg_m : 0;
  if constexpr (BNB && !GLB) pg_prm_fill<BCH, 64 * NW>(a, prm, bpx, bch, seg0);  // published by the main loop's barriers
  const int HoWo = a.Ho * a.Wo;
  const long long img0 = bpx / HoWo;
  const __amdgpu_buffer_rsrc_t xr =
      pg_rsrc(reinterpret_cast<const bf16*>(a.x) + img0 * a.sN, (a.x_elems - img0 * a.sN) * 2);
  const __amdgpu_buffer_rsrc_t xr2 =
      X2 ? pg_rsrc(reinterpret_cast<const bf16*>(a.x2) + img0 * a.sN2, (a.x2_elems - img0 * a.sN2) * 2) : xr;
  const __amdgpu_buffer_rsrc_t wr =
      pg_rsrc(reinterpret_cast<const bf16*>(a.w) + (X2 ? seg0 * a.w_sstride : 0), (long long)a.Cout * a.K * 2);

  // ---- loader decode: this lane fills slot (lane & 7) of row (lane >> 3)
  // of each 8-row wave instruction, with k-chunk csrc = slot ^ (row & 7)
  const int lrow = lane / CPR, lslot = lane % CPR;
  const int csrc = KS == 64 ? (lslot ^ lrow) : (lslot ^ ((lrow >> 2) & 2));
  int rowoff[IPX];
  unsigned rmask[IPX];
  // X2: the row offsets into the second operand replace rowoff[] once, at the
  // first stage past C1 (1x1, stride 1: the pixel itself) — not held beside
  // them through the first operand's stages (the 8-wave tile's 128 VGPRs)
  auto rowoff_x2 = [&](int u) {
    const int row = (u * NW + wid) * RPI + lrow;
    const long long gm = bpx + row;
    const long long gmc = gm < a.M ? gm : bpx;
    const long long img = gmc / HoWo;
    const int rem = (int)(gmc - img * HoWo);
    const int oh = rem / a.Wo, ow = rem - (rem / a.Wo) * a.Wo;
    return (int)(((img - img0) * a.sN2 + (long long)oh * a.sH2 + (long long)ow * a.sW2) * 2);
  };
#pragma unroll
  for (int u = 0; u < IPX; ++u) {
    const int row = (u * NW + wid) * RPI + lrow;
    const long long gm = bpx + row;
    const bool valid = gm < a.M;
    const long long gmc = valid ? gm : bpx;
    const long long img = gmc / HoWo;
    const int rem = (int)(gmc - img * HoWo);
    const int oh = rem / a.Wo, ow = rem - (rem / a.Wo) * a.Wo;
    const int ih0 = oh * a.stride - a.pad, iw0 = ow * a.stride - a.pad;
    rowoff[u] = (int)(((img - img0) * a.sN + (long long)ih0 * a.sH + (long long)iw0 * a.sW) * 2);
    unsigned msk = 0;
    for (int r = 0; r < a.R; ++r)
      for (int s = 0; s < a.S; ++s) {
        const bool ok = valid && ih0 + r >= 0 && ih0 + r < a.H && iw0 + s >= 0 && iw0 + s < a.W;
        msk |= (ok ? 1u : 0u) << (r * a.S + s);
      }
    rmask[u] = msk;
  }
  unsigned woff[ICH];
#pragma unroll
  for (int u = 0; u < ICH; ++u) {
    const int g = u * NW + wid;
    const int ch = bch + pg_perm(g * RPI + lrow);
    woff[u] = (g < ICH_TOT && ch < a.Cout) ? (unsigned)(ch * a.K * 2 + csrc * 16) : PG_OOB;
  }
  const bool lps_hi = (ICH - 1) * NW + wid < ICH_TOT;

  int u_ci = 0, u_s = 0, u_r = 0;  // uniform-tap walk (C % 64 == 0)
  bool on2 = false;                 // X2: rowoff[] holds the second operand's offsets
  auto issue = [&](int kt, int buf) {
    char* pxs = smem + buf * STAGE;
    char* chs = pxs + PXB;
    int rs, tapoff;
    bool kval;
    bool src2 = false;  // X2: this stage's k lie in the second operand
    if constexpr (!MULTI) {
      rs = u_r * a.S + u_s;
      int ci = u_ci;
      if constexpr (X2) {
        src2 = u_ci >= a.C1;
        if (src2) {
          ci -= a.C1;
          if (!on2) {
            on2 = true;
#pragma unroll
            for (int u = 0; u < IPX; ++u) rowoff[u] = rowoff_x2(u);
          }
        }
      }
      tapoff = (u_r * (int)a.sH + u_s * (int)a.sW + ci + csrc * 8) * 2;
      kval = true;
      u_ci += KS;
      if (u_ci == a.C) {
        u_ci = 0;
        if (++u_s == a.S) { u_s = 0; ++u_r; }
      }
    } else {
      const int cpt = a.C >> 3;  // 16-B chunks per tap: 1, 2 or 4
      const int sub = csrc / cpt;
      const int ci = (csrc - sub * cpt) * 8;
      rs = kt * (64 / a.C) + sub;
      kval = rs < a.R * a.S;
      const int r = rs / a.S, s = rs - (rs / a.S) * a.S;
      tapoff = (r * (int)a.sH + s * (int)a.sW + ci) * 2;
    }
#pragma unroll
    for (int u = 0; u < IPX; ++u) {
      const bool ok = kval && ((rmask[u] >> (rs & 31)) & 1u);
      if constexpr (X2) {
        glds16(src2 ? xr2 : xr, pxs + (u * NW + wid) * 1024, ok ? (unsigned)(rowoff[u] + tapoff) : PG_OOB);
      } else {
        glds16(xr, pxs + (u * NW + wid) * 1024, ok ? (unsigned)(rowoff[u] + tapoff) : PG_OOB);
      }
    }
    const bool wk = kt * KS + csrc * 8 < a.K;
#pragma unroll
    for (int u = 0; u < ICH; ++u) {
      if (u * NW + wid < ICH_TOT)
        glds16(wr, chs + (u * NW + wid) * 1024, (wk && woff[u] != PG_OOB) ? woff[u] + kt * ROWB : PG_OOB);
    }
  };

  f32x4 acc[MTC][NTP];
#pragma unroll
  for (int i = 0; i < MTC; ++i)
#pragma unroll
    for (int j = 0; j < NTP; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int fr = lane & 15, fq = lane >> 4;
  auto compute = [&](int buf) {
    const char* pxs = smem + buf * STAGE;
    const char* chs = pxs + PXB;
#pragma unroll
    for (int kk = 0; kk < KS / 32; ++kk) {
      const int so = (KS == 64 ? ((kk * 4 + fq) ^ (fr & 7)) : (fq ^ ((fr >> 2) & 2))) << 4;
      uint4 af[MTC], bv[NTP];
#pragma unroll
      for (int i = 0; i < MTC; ++i) af[i] = *reinterpret_cast<const uint4*>(chs + (wch * WTCH + i * 16 + fr) * ROWB + so);
#pragma unroll
      for (int j = 0; j < NTP; ++j) bv[j] = *reinterpret_cast<const uint4*>(pxs + (wpx * WTPX + j * 16 + fr) * ROWB + so);
      PG_PRIO_ON();
#pragma unroll
      for (int i = 0; i < MTC; ++i)
#pragma unroll
        for (int j = 0; j < NTP; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(*reinterpret_cast<const bf16x8*>(&af[i]),
                                                              *reinterpret_cast<const bf16x8*>(&bv[j]), acc[i][j], 0,
                                                              0, 0);
      PG_PRIO_OFF();
    }
  };

  const bool sums = BNB || a.stats != nullptr;
  if (sums) {
    for (int i = tid; i < 6 * BCH; i += 64 * NW) red[i] = 0.f;
    if (tid == 0) *red_cnt = 0;
  }
  EpiRegs<MTC / 2, NTP> er;
  if constexpr (PF) epi_prefetch<BK, TWO, MTC, NTP, WTPX, WTCH>(a, er, bpx, bch, wpx, wch, fr, fq);
  const int nk = (a.K + KS - 1) / KS;
#pragma unroll
  for (int s = 0; s < NSTAGE - 1; ++s)
    if (s < nk) issue(s, s);
  for (int kt = 0; kt < nk; ++kt) {
    int ahead = nk - 1 - kt;
    if (ahead > NSTAGE - 2) ahead = NSTAGE - 2;
    if (lps_hi) wait_stages<LPS_HI, NSTAGE>(ahead);
    else wait_stages<LPS_LO, NSTAGE>(ahead);
    // retire this wave's LDS reads of the slot the next issue overwrites
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    if (kt + NSTAGE - 1 < nk) issue(kt + NSTAGE - 1, (kt + NSTAGE - 1) % NSTAGE);
    compute(kt % NSTAGE);
  }

  // ---- epilogue operands into the (now free) stage ring by LDS-DMA: slot 0
  // y_0, then the residual, y_1 and the bf16 mask as far as the ring holds them
  constexpr int OPB = BPX * BCH * 2;            // bytes of one staged operand
  constexpr int NOP = (NSTAGE * STAGE) / OPB;   // operands that fit
  constexpr bool RESK = BK == 2 || BK == 3;
  constexpr bool S_RES = RESK && NOP >= 2;
  constexpr bool S_Y1 = TWO && NOP >= 2 + (S_RES ? 1 : 0);
  constexpr bool S_MK = BK == 2 && NOP >= 2 + (S_RES ? 1 : 0) + (S_Y1 ? 1 : 0);
  static_assert(!BNB || NOP >= 1, "y_0 must fit the stage ring");
  EpiStage sg{nullptr, nullptr, nullptr, nullptr, nullptr, BNB ? prm : nullptr, seg0};
  if constexpr (PF) {
    const int slot = (int)(blockIdx.x % ARTSBIR_NSLOT);
    pg_epilogue_k<BK, TWO, false, false, false, BCH, MTC, NTP, WTPX, WTCH, true>(a, acc, bpx, bch, wpx, wch, fr, fq,
                                                                                red, sg, &er);
    if (sums) stats_flush<BCH>(red, red_cnt, NW - 1, a, bch, slot, lane, bpx, BPX);
    return;
  }
  if constexpr (GLB) {
    const int slot = (int)(blockIdx.x % ARTSBIR_NSLOT);
    if constexpr (NW >= 8) {  // channel pairs outside (the 8-wave tile: 128 VGPRs)
      EpiStage sgg{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, seg0};
      pg_epilogue_k<BK, TWO, false, false, false, BCH, MTC, NTP, WTPX, WTCH, false, 1, true, X2, NW >= 8>(
          a, acc, bpx, bch, wpx, wch, fr, fq, red, sgg);
    } else {
      // the 8-wave 256 x 128 tile runs at 128 VGPRs (two workgroups per CU):
      // statistics reduced per (tile, pair) there, carried in registers otherwise
      // statistics carried in registers across the pixel tiles; the BN constants
      // from an LDS table where the registers allow (4 waves: 168 VGPRs), else
      // from the L1-resident parameter vectors (8 waves: 128 VGPRs)
      constexpr bool SP = true, TBL = NW < 8;
      float* tprm = reinterpret_cast<float*>(smem);  // the stage ring is free after the main loop
      if constexpr (BNB && TBL) {
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __syncthreads();  // every wave is done reading the stages
        pg_prm_fill<BCH, 64 * NW>(a, tprm, bpx, bch, seg0);
        __syncthreads();
      }
      pg_epilogue_glb<BK, TWO, BCH, MTC, NTP, WTPX, WTCH, X2, SP, TBL>(a, acc, bpx, bch, wpx, wch, fr, fq, red,
                                                                       tprm, seg0);
    }
    if (sums) stats_flush<BCH>(red, red_cnt, NW - 1, a, bch, slot, lane, bpx, BPX);
    return;
  }
  if constexpr (BNB) {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __syncthreads();  // every wave is done reading the stages
    const long long rows = a.M;
    int n = 0;
    sg.y0 = smem;
    stage_operand<BPX, BCH, NW>(a.bnb_y[0], rows, a.ldy, smem, bpx, bch, a, false, wid, lane);
    ++n;
    if constexpr (S_RES) {
      sg.res = smem + n * OPB;
      stage_operand<BPX, BCH, NW>(a.res, a.res_mode == 2 ? rows / 4 : rows, a.ldy, smem + n * OPB, bpx, bch, a,
                                  a.res_mode == 2, wid, lane);
      ++n;
    }
    if constexpr (S_Y1) {
      sg.y1 = smem + n * OPB;
      stage_operand<BPX, BCH, NW>(a.bnb_y[1], rows, a.ldy, smem + n * OPB, bpx, bch, a, false, wid, lane);
      ++n;
    }
    if constexpr (S_MK) {
      sg.mk = smem + n * OPB;
      stage_operand<BPX, BCH, NW>(a.bnb_mask, rows, a.ldy, smem + n * OPB, bpx, bch, a, false, wid, lane);
      ++n;
    }
    if constexpr (BK == 3) {
      sg.bits = sbits;
      stage_bits<BPX, BCH, NW>(a.bnb_mask, sbits, bpx, bch, a, wid, lane);
    }
    vm_wait<0>();
    __syncthreads();  // every wave's DMA has landed
  } else if (a.res_mode) {  // plain data gradient with a residual: stage it
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __syncthreads();
    sg.res = smem;
    stage_operand<BPX, BCH, NW>(a.res, a.res_mode == 2 ? a.M / 4 : a.M, a.ldy, smem, bpx, bch, a, a.res_mode == 2,
                                wid, lane);
    vm_wait<0>();
    __syncthreads();
  }
  const int slot = (int)(blockIdx.x % ARTSBIR_NSLOT);
  pg_epilogue_k<BK, TWO, S_RES, S_Y1, S_MK, BCH, MTC, NTP, WTPX, WTCH, false, 2, false, X2>(a, acc, bpx, bch, wpx, wch,
                                                                                            fr, fq, red, sg);
  if (sums) stats_flush<BCH>(red, red_cnt, NW - 1, a, bch, slot, lane, bpx, BPX);
}

// candidates 0-5 (the tile shapes of kCfgs) with one epilogue
template <bool MULTI, int BK, bool TWO>
void pg_launch_cfg(int c, const PgArgs& a, long long tiles, hipStream_t st) {
  const dim3 g((unsigned)tiles);
  switch (c) {
    case 0: hipLaunchKernelGGL((pgemm_kernel<256, 256, 4, 2, 2, MULTI, BK, TWO>), g, dim3(512), 0, st, a); break;
    case 1: hipLaunchKernelGGL((pgemm_kernel<256, 128, 4, 2, 3, MULTI, BK, TWO>), g, dim3(512), 0, st, a); break;
    case 2: hipLaunchKernelGGL((pgemm_kernel<256, 64, 4, 2, 3, MULTI, BK, TWO>), g, dim3(512), 0, st, a); break;
    case 3: hipLaunchKernelGGL((pgemm_kernel<128, 128, 2, 2, 2, MULTI, BK, TWO>), g, dim3(256), 0, st, a); break;
    case 4: hipLaunchKernelGGL((pgemm_kernel<256, 32, 8, 1, 4, MULTI, BK, TWO>), g, dim3(512), 0, st, a); break;
    default:
      if constexpr (!MULTI)
        hipLaunchKernelGGL((pgemm_kernel<256, 256, 4, 2, 4, false, BK, TWO, false, 32>), g, dim3(512), 0, st, a);
      break;
  }
}
// its instantiations are compiled once each, 11 or 12 kernels to a unit
#define PG_LAUNCH_CFG_IN_UNIT(MULTI, BK, TWO) \
  extern template void pg_launch_cfg<MULTI, BK, TWO>(int, const PgArgs&, long long, hipStream_t)
PG_LAUNCH_CFG_IN_UNIT(true, 0, false);   // pgemm.hip
PG_LAUNCH_CFG_IN_UNIT(false, 0, false);
PG_LAUNCH_CFG_IN_UNIT(true, 1, false);   // pgemm_bnb1.hip
PG_LAUNCH_CFG_IN_UNIT(false, 1, false);
PG_LAUNCH_CFG_IN_UNIT(false, 2, false);  // pgemm_bnb2.hip
PG_LAUNCH_CFG_IN_UNIT(false, 2, true);
PG_LAUNCH_CFG_IN_UNIT(false, 3, false);  // pgemm_bnb3.hip
PG_LAUNCH_CFG_IN_UNIT(false, 3, true);
#undef PG_LAUNCH_CFG_IN_UNIT

}  // namespace artsbir
