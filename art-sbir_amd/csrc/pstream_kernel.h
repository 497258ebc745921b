// The persistent streaming implicit-GEMM kernel; pstream.hip (candidate 10) and
// pstream_k.hip (14, 15, 17, the fold) instantiate it.
#pragma once
#include "pgemm_dev.h"

namespace artsbir {


// ---------------------------------------------------------------------------
// Persistent producer/consumer variant for layers with many 256-pixel tiles
// (stem, layer1-3, low K).  4 loader waves only issue LDS-DMA, so their vmcnt
// counts exactly their own loads; 8 compute waves only read LDS, run MFMAs and
// store.  One s_barrier per stage hands a landed stage to the compute waves
// and the slot they just drained back to the loaders.  The stage sequence runs
// across tile boundaries: the next tile's loads are in flight while this
// tile's epilogue stores drain, which is what the low-K layers (1-5 K-steps
// per tile) need to stream at HBM rate.
// ---------------------------------------------------------------------------
// FWDS: forward with BN statistics (carried across tiles, pg_epilogue_fwd)
// BK > 0: the fused BN-backward epilogue specialised at compile time
// (pg_epilogue_k, kinds as pgemm_kernel's, TWO targets), its operands and BN
// constants read from global memory in batches of two pixel tiles while the
// loader waves already stream the next tile's stages
// KS: k per stage as in pgemm_kernel (32: 64-B LDS rows, twice the stages in
// the same LDS, uniform taps only)
// X2: the two-operand / per-segment-weight fold of pgemm_kernel (1x1 only)
// WGK > 0: the fold (X2) with its weight-gradient operands accumulated by the
// loader waves (pstream_wg_loader, K = WGK, 64 output channels)

template <int BCH, int WPX, int WCH, int NSTAGE, bool MULTI, bool BNB, bool FWDS, int BK = 0, bool TWO = false,
          int KS = 64, bool X2 = false, int WGK = 0>
__global__ void __launch_bounds__(768) pstream_kernel(PgArgs a, int ntiles) {
  constexpr int BPX = 256, NWC = 8, NWL = 4;
  static_assert(WPX * WCH == NWC, "compute waves");
  static_assert(KS == 64 || (KS == 32 && !MULTI), "32-k stages: uniform taps only");
  constexpr int ROWB = 2 * KS, RPI = 1024 / ROWB, CPR = ROWB / 16;
  constexpr int PXB = BPX * ROWB, CHB = BCH * ROWB, STAGE = PXB + CHB;
  constexpr int LPX = BPX / (RPI * NWL);
  constexpr int LCH = BCH / (RPI * NWL);
  constexpr int LPS = LPX + LCH;
  constexpr int WTPX = BPX / WPX, WTCH = BCH / WCH;
  constexpr int NTP = WTPX / 16, MTC = WTCH / 16;
  static_assert(LCH >= 1 && MTC % 2 == 0, "shape");
  __shared__ __attribute__((aligned(16))) char smem[NSTAGE * STAGE + pg_red_bytes<BCH>()];
  float* red = reinterpret_cast<float*>(smem + NSTAGE * STAGE);
  int* red_cnt = reinterpret_cast<int*>(smem + NSTAGE * STAGE + 6 * BCH * 4);

  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int ntc = (a.Cout + BCH - 1) / BCH;
  const int G = gridDim.x;
  const int bslot = (G % 8 == 0) ? (int)(blockIdx.x % 8) * (G / 8) + (int)(blockIdx.x / 8) : (int)blockIdx.x;
  const int my_tiles = bslot < ntiles ? (ntiles - 1 - bslot) / G + 1 : 0;
  const int nk = (a.K + KS - 1) / KS;
  const int total = my_tiles * nk;
  const int HoWo = a.Ho * a.Wo;

  if (wid >= NWC) {
    // ------------------------------------------------------------ loaders
    if constexpr (WGK > 0) {
      static_assert(X2 && !MULTI && KS == 64 && !FWDS, "WGK: the fold's 64-k stages");
      pstream_wg_loader<BCH, NSTAGE, LPX, LCH, STAGE, PXB, WGK>(a, smem, wid - NWC, lane, G, bslot, nk, total);
      return;
    }
    const int lw = wid - NWC;
    const int lrow = lane / CPR, lslot = lane % CPR;
    const int csrc = KS == 64 ? (lslot ^ lrow) : (lslot ^ ((lrow >> 2) & 2));
    __amdgpu_buffer_rsrc_t wr = pg_rsrc(a.w, (long long)a.Cout * a.K * 2);
    __amdgpu_buffer_rsrc_t xr = wr, xr2 = wr;
    int rowoff[LPX], rowoff2[X2 ? LPX : 1];
    unsigned rmask[LPX];
    unsigned woff[LCH];
    int u_ci = 0, u_s = 0, u_r = 0;
    auto start_tile = [&](int i) {
      const long long t = (long long)i * G + bslot;
      const long long bpx = (t / ntc) * BPX;
      const int bch = (int)(t % ntc) * BCH;
      const long long img0 = bpx / HoWo;
      xr = pg_rsrc(reinterpret_cast<const bf16*>(a.x) + img0 * a.sN, (a.x_elems - img0 * a.sN) * 2);
      if constexpr (X2) {
        xr2 = pg_rsrc(reinterpret_cast<const bf16*>(a.x2) + img0 * a.sN2, (a.x2_elems - img0 * a.sN2) * 2);
        const long long sg = a.seg_m > 0 ? bpx / a.seg_m : 0;
        wr = pg_rsrc(reinterpret_cast<const bf16*>(a.w) + sg * a.w_sstride, (long long)a.Cout * a.K * 2);
      }
#pragma unroll
      for (int u = 0; u < LPX; ++u) {
        const int row = (u * NWL + lw) * RPI + lrow;
        const long long gm = bpx + row;
        const bool valid = gm < a.M;
        const long long gmc = valid ? gm : bpx;
        const long long img = gmc / HoWo;
        const int rem = (int)(gmc - img * HoWo);
        const int oh = rem / a.Wo, ow = rem - (rem / a.Wo) * a.Wo;
        const int ih0 = oh * a.stride - a.pad, iw0 = ow * a.stride - a.pad;
        rowoff[u] = (int)(((img - img0) * a.sN + (long long)ih0 * a.sH + (long long)iw0 * a.sW) * 2);
        if constexpr (X2)
          rowoff2[u] = (int)(((img - img0) * a.sN2 + (long long)oh * a.sH2 + (long long)ow * a.sW2) * 2);
        unsigned msk = 0;
        for (int r = 0; r < a.R; ++r)
          for (int s = 0; s < a.S; ++s) {
            const bool ok = valid && ih0 + r >= 0 && ih0 + r < a.H && iw0 + s >= 0 && iw0 + s < a.W;
            msk |= (ok ? 1u : 0u) << (r * a.S + s);
          }
        rmask[u] = msk;
      }
#pragma unroll
      for (int u = 0; u < LCH; ++u) {
        const int ch = bch + pg_perm((u * NWL + lw) * RPI + lrow);
        woff[u] = ch < a.Cout ? (unsigned)(ch * a.K * 2 + csrc * 16) : PG_OOB;
      }
      u_ci = 0; u_s = 0; u_r = 0;
    };
    auto issue = [&](int sidx) {
      const int i = sidx / nk, kt = sidx - i * nk;
      if (kt == 0) start_tile(i);
      char* pxs = smem + (sidx % NSTAGE) * STAGE;
      char* chs = pxs + PXB;
      int rs, tapoff;
      bool kval;
      bool src2 = false;
      if constexpr (!MULTI) {
        rs = u_r * a.S + u_s;
        int ci = u_ci;
        if constexpr (X2) {
          src2 = u_ci >= a.C1;
          if (src2) ci -= a.C1;
        }
        tapoff = (u_r * (int)a.sH + u_s * (int)a.sW + ci + csrc * 8) * 2;
        kval = true;
        u_ci += KS;
        if (u_ci == a.C) {
          u_ci = 0;
          if (++u_s == a.S) { u_s = 0; ++u_r; }
        }
      } else {
        const int cpt = a.C >> 3;
        const int sub = csrc / cpt;
        const int ci = (csrc - sub * cpt) * 8;
        rs = kt * (64 / a.C) + sub;
        kval = rs < a.R * a.S;
        const int r = rs / a.S, s = rs - (rs / a.S) * a.S;
        tapoff = (r * (int)a.sH + s * (int)a.sW + ci) * 2;
      }
#pragma unroll
      for (int u = 0; u < LPX; ++u) {
        const bool ok = kval && ((rmask[u] >> (rs & 31)) & 1u);
        if constexpr (X2) {
          if (src2) glds16(xr2, pxs + (u * NWL + lw) * 1024, ok ? (unsigned)(rowoff2[u] + tapoff) : PG_OOB);
          else glds16(xr, pxs + (u * NWL + lw) * 1024, ok ? (unsigned)(rowoff[u] + tapoff) : PG_OOB);
        } else {
          glds16(xr, pxs + (u * NWL + lw) * 1024, ok ? (unsigned)(rowoff[u] + tapoff) : PG_OOB);
        }
      }
      const bool wk = kt * KS + csrc * 8 < a.K;
#pragma unroll
      for (int u = 0; u < LCH; ++u)
        glds16(wr, chs + (u * NWL + lw) * 1024, (wk && woff[u] != PG_OOB) ? woff[u] + kt * ROWB : PG_OOB);
    };
    for (int s = 0; s < NSTAGE - 1; ++s)
      if (s < total) issue(s);
    if (total > 0) {
      int ahead = total - 1;
      if (ahead > NSTAGE - 2) ahead = NSTAGE - 2;
      wait_stages<LPS, NSTAGE>(ahead);
    }
    for (int s = 0; s < total; ++s) {
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
      asm volatile("" ::: "memory");
      if (s + NSTAGE - 1 < total) issue(s + NSTAGE - 1);
      if (s + 1 < total) {
        int ahead = total - 2 - s;
        if (ahead > NSTAGE - 2) ahead = NSTAGE - 2;
        wait_stages<LPS, NSTAGE>(ahead);
      }
    }
    return;
  }

  // -------------------------------------------------------------- compute
  const bool sums = !FWDS && (BNB || a.stats != nullptr);
  if (sums) {  // ordered before any use by the first stage barrier
    for (int i = tid; i < 6 * BCH; i += 64 * NWC) red[i] = 0.f;
    if (tid == 0) *red_cnt = 0;
  }
  const int wpx = wid % WPX, wch = wid / WPX;
  const int fr = lane & 15, fq = lane >> 4;
  f32x4 acc[MTC][NTP];
#pragma unroll
  for (int i = 0; i < MTC; ++i)
#pragma unroll
    for (int j = 0; j < NTP; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  WaveStats<MTC / 2> ws;  // forward statistics carried across tiles (pg_epilogue_fwd)
  wstats_zero(ws);
  ws.seg = -1;
  ws.bch = -1;
  const int wslot = (int)((blockIdx.x * NWC + wid) % ARTSBIR_NSLOT);
  for (int s = 0; s < total; ++s) {
    // retire this wave's LDS reads of the slot the next issue overwrites
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    {
      const char* pxs = smem + (s % NSTAGE) * STAGE;
      const char* chs = pxs + PXB;
#pragma unroll
      for (int kk = 0; kk < KS / 32; ++kk) {
        const int so = (KS == 64 ? ((kk * 4 + fq) ^ (fr & 7)) : (fq ^ ((fr >> 2) & 2))) << 4;
        uint4 af[MTC], bv[NTP];
#pragma unroll
        for (int i = 0; i < MTC; ++i)
          af[i] = *reinterpret_cast<const uint4*>(chs + (wch * WTCH + i * 16 + fr) * ROWB + so);
#pragma unroll
        for (int j = 0; j < NTP; ++j)
          bv[j] = *reinterpret_cast<const uint4*>(pxs + (wpx * WTPX + j * 16 + fr) * ROWB + so);
        PG_PRIO_ON();
#pragma unroll
        for (int i = 0; i < MTC; ++i)
#pragma unroll
          for (int j = 0; j < NTP; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(*reinterpret_cast<const bf16x8*>(&af[i]),
                                                                *reinterpret_cast<const bf16x8*>(&bv[j]), acc[i][j],
                                                                0, 0, 0);
        PG_PRIO_OFF();
      }
    }
    const int ti = s / nk;
    if (s - ti * nk != nk - 1) continue;
    // ---- epilogue of tile ti
    const long long t = (long long)ti * G + bslot;
    const long long bpx = (t / ntc) * BPX;
    const int bch = (int)(t % ntc) * BCH;
    const int slot = (int)(t % ARTSBIR_NSLOT);
    if constexpr (FWDS) {
      pg_epilogue_fwd<BCH, MTC, NTP, WTPX, WTCH>(a, acc, bpx, bch, wpx, wch, fr, fq, ws, wslot);
    } else if constexpr (BK != 0) {
      const EpiStage sg{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, a.seg_m > 0 ? bpx / a.seg_m : 0};
      pg_epilogue_k<BK, TWO, false, false, false, BCH, MTC, NTP, WTPX, WTCH, false, 2, true, X2>(a, acc, bpx, bch, wpx,
                                                                                              wch, fr, fq, red, sg);
      if (sums) stats_flush<BCH>(red, red_cnt, NWC * (ti + 1) - 1, a, bch, slot, lane, bpx, BPX);
    } else {
      pg_epilogue<BNB, BCH, MTC, NTP, WTPX, WTCH, 1>(a, acc, bpx, bch, wpx, wch, fr, fq, red);
      // the flushing wave zeroes red before it reaches the next stage barrier,
      // and no wave adds for tile ti+1 before passing that barrier
      if (sums) stats_flush<BCH>(red, red_cnt, NWC * (ti + 1) - 1, a, bch, slot, lane, bpx, BPX);
    }
#pragma unroll
    for (int i = 0; i < MTC; ++i)
#pragma unroll
      for (int j = 0; j < NTP; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  if constexpr (FWDS) wstats_flush<MTC / 2, WTCH>(ws, a, wch, fr, fq, wslot);
}

}  // namespace artsbir
