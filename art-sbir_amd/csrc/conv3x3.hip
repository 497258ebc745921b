// The two direct 3x3 convolutions for few channels: sconv_kernel (candidate 20)
// and hconv_kernel (candidate 21); pgemm.h lists the candidates.  They share
// the LDS image of the filters (sc_sw).
#include <cstdio>

#include "pgemm.h"
#include "pgemm_dev.h"

namespace artsbir {

// ---------------------------------------------------------------------------
// Direct 3x3 convolution for few channels (C in {8, 32, 64} in, Cout in
// {32, 64} out): the stem (models.py:310-317, 112x112) and the layer-1 3x3
// convolutions, forward and data gradient.  Their im2col rows are short
// (K = 72..576), so the LDS-staged im2col of pgemm spends its time gathering:
// here the pixel operand is read STRAIGHT from global memory into the MFMA B
// fragments — lane (fr, fq) of a 16-pixel tile loads 16 B (8 channels) of its
// own input pixel, so for C = 32 one wave instruction reads one contiguous
// 1 KB run of 16 pixels x 64 B (coalesced; the 9 tap re-reads hit L1/L2) —
// while the whole filter bank sits in LDS (read as A fragments, XOR-swizzled
// conflict-free).  Padding and tails come back as zeros from the buffer unit.
// Output tile = 256 consecutive pixels x all Cout channels, 4 waves x 64
// pixels; the epilogue (BN statistics, BN-backward fusion, segments) is
// pgemm's.
// ---------------------------------------------------------------------------
// LDS image of the filters: block kk (32 k = 4 chunks of 16 B) holds COUT rows
// of 64 B; row rho carries channel pg_perm(rho), chunk c at slot c ^ sw(rho).
__device__ __forceinline__ int sc_sw(int rho) { return (rho ^ (rho >> 1)) & 3; }

template <int C, int COUT, int STRIDE, bool BNB>
__global__ void __launch_bounds__(256) sconv_kernel(PgArgs a, int ntiles) {
  constexpr int K = 9 * C;
  constexpr int NKK = (K + 31) / 32;  // 32-k MFMA steps
  constexpr int CPT = C / 8;          // 16-B chunks per tap
  constexpr int MTC = COUT / 16, NTP = 4, WTPX = 64, BPX = 256, BCH = COUT;
  constexpr int PF = 2;                // k-steps of B fragments in flight ahead
  constexpr int WB = NKK * COUT * 64;  // filter image bytes
  __shared__ __attribute__((aligned(16))) char smem[WB + pg_red_bytes<BCH>()];
  float* red = reinterpret_cast<float*>(smem + WB);
  int* red_cnt = reinterpret_cast<int*>(smem + WB + 6 * BCH * 4);
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int fr = lane & 15, fq = lane >> 4;
  const bool sums = a.stats != nullptr || a.bnb != 0;
  if (sums) {
    for (int i = tid; i < 6 * BCH; i += 256) red[i] = 0.f;
    if (tid == 0) *red_cnt = 0;
  }
  // ---- filters -> LDS once per (persistent) block (zero past K)
  for (int i = tid; i < NKK * COUT * 4; i += 256) {
    const int kk = i / (COUT * 4), rem = i - kk * COUT * 4;
    const int rho = rem >> 2, c = rem & 3;
    const int k = kk * 32 + c * 8;
    uint4 v = make_uint4(0, 0, 0, 0);
    if (k < K) v = *reinterpret_cast<const uint4*>(reinterpret_cast<const bf16*>(a.w) + (long long)pg_perm(rho) * K + k);
    *reinterpret_cast<uint4*>(smem + (kk * COUT + rho) * 64 + ((c ^ sc_sw(rho)) << 4)) = v;
  }
  const int HoWo = a.Ho * a.Wo;
  const int G = gridDim.x;
  int ti = 0;
  for (int tile = blockIdx.x; tile < ntiles; tile += G, ++ti) {
    // filter image visible (first tile); the previous tile's statistics flush
    // is complete before any wave adds this tile's sums
    __syncthreads();
    const long long bpx = (long long)tile * BPX;
    // ---- per pixel tile: input origin and tap validity of this lane's pixel
    const long long img0 = bpx / HoWo;
    const __amdgpu_buffer_rsrc_t xr =
        pg_rsrc(reinterpret_cast<const bf16*>(a.x) + img0 * a.sN, (a.x_elems - img0 * a.sN) * 2);
    const long long wpx0 = bpx + wid * WTPX;
    int boff[NTP];
    unsigned vmask[NTP];
#pragma unroll
    for (int j = 0; j < NTP; ++j) {
      const long long px = wpx0 + j * 16 + fr;
      const bool valid = px < a.M;
      const long long pc = valid ? px : bpx;
      const long long n = pc / HoWo;
      const int rem = (int)(pc - n * HoWo);
      const int oh = rem / a.Wo, ow = rem - (rem / a.Wo) * a.Wo;
      const int ih0 = oh * STRIDE - 1, iw0 = ow * STRIDE - 1;
      boff[j] = (int)(((n - img0) * a.sN + (long long)ih0 * a.sH + (long long)iw0 * a.sW) * 2);
      unsigned m = 0;
#pragma unroll
      for (int t = 0; t < 9; ++t) {
        const int r = t / 3, s = t % 3;
        const bool ok = valid && ih0 + r >= 0 && ih0 + r < a.H && iw0 + s >= 0 && iw0 + s < a.W;
        m |= (ok ? 1u : 0u) << t;
      }
      vmask[j] = m;
    }
    // B fragment of k-step kk, pixel tile j: 16 B of the lane's own input pixel
    auto bload = [&](int kk, int j) -> uint4 {
      const int kc = kk * 4 + fq;  // 16-B chunk of the im2col row
      const int t = kc / CPT, cc = kc - (kc / CPT) * CPT;
      const int r = t / 3, s = t - (t / 3) * 3;
      const bool ok = kc < 9 * CPT && ((vmask[j] >> t) & 1u);
      const unsigned off = (unsigned)(boff[j] + ((r * (int)a.sH + s * (int)a.sW) * 2) + cc * 16);
      const u32x4v v = __builtin_amdgcn_raw_buffer_load_b128(xr, ok ? (int)off : (int)PG_OOB, 0, 0);
      return make_uint4(v[0], v[1], v[2], v[3]);
    };
    f32x4 acc[MTC][NTP];
#pragma unroll
    for (int i = 0; i < MTC; ++i)
#pragma unroll
      for (int j = 0; j < NTP; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    // ring of PF + 1 k-steps of B fragments (fully unrolled: static indices)
    uint4 bf[PF + 1][NTP];
#pragma unroll
    for (int q = 0; q < PF; ++q)
      if (q < NKK) {
#pragma unroll
        for (int j = 0; j < NTP; ++j) bf[q][j] = bload(q, j);
      }
#pragma unroll
    for (int kk = 0; kk < NKK; ++kk) {
      if (kk + PF < NKK) {
#pragma unroll
        for (int j = 0; j < NTP; ++j) bf[(kk + PF) % (PF + 1)][j] = bload(kk + PF, j);
      }
      uint4 af[MTC];
#pragma unroll
      for (int i = 0; i < MTC; ++i) {
        const int rho = i * 16 + fr;
        af[i] = *reinterpret_cast<const uint4*>(smem + (kk * COUT + rho) * 64 + ((fq ^ sc_sw(rho)) << 4));
      }
#pragma unroll
      for (int i = 0; i < MTC; ++i)
#pragma unroll
        for (int j = 0; j < NTP; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(*reinterpret_cast<const bf16x8*>(&af[i]),
                                                              *reinterpret_cast<const bf16x8*>(&bf[kk % (PF + 1)][j]),
                                                              acc[i][j], 0, 0, 0);
    }
    const int slot = tile % ARTSBIR_NSLOT;
    pg_epilogue<BNB, BCH, MTC, NTP, WTPX, COUT, 1>(a, acc, bpx, 0, wid, 0, fr, fq, red);
    if (sums) stats_flush<BCH>(red, red_cnt, 4 * (ti + 1) - 1, a, 0, slot, lane, bpx, BPX);
  }
}

// shapes the direct small-channel kernel takes
bool sconv_ok(const PgArgs& a) {
  if (a.R != 3 || a.S != 3 || a.pad != 1 || a.M <= 0) return false;
  if (a.Cout != 32 && a.Cout != 64) return false;
  if (!((a.stride == 1 && (a.C == 32 || a.C == 64)) || (a.stride == 2 && a.C == 8 && a.Cout == 32))) return false;
  if (a.seg_m > 0 && (a.seg_m % 64 != 0 || a.seg_m < 256 || a.M % a.seg_m != 0)) return false;
  if (a.bnb && a.stats) return false;
  const long long HoWo = (long long)a.Ho * a.Wo;
  // block-relative byte offsets in 31 bits: a 256-pixel tile spans few images
  if (((256 + HoWo - 1) / HoWo + 2) * a.sN * 2 > 0x7fffffffLL) return false;
  return (a.M + 255) / 256 <= 0x7fffffffLL / 256;
}

// persistent grid: as many blocks as fit on the 256 CUs at once — by LDS and
// by registers (the runtime's occupancy of the kernel): an LDS-only count put
// 4 blocks per CU where the 150-220-register forms hold 2-3, so the last
// blocks ran their whole tile share after the others had finished
template <int C, int COUT, int ST, bool BNB>
static int sconv_grid(int ntiles) {
  constexpr int K = 9 * C, NKK = (K + 31) / 32;
  constexpr int lds = NKK * COUT * 64 + 2 * 3 * COUT * 4 + 16;
  static const int per_cu = [] {
    int n = (160 * 1024) / lds;
    if (n > 4) n = 4;  // 4 x 256 threads: 16 waves per CU
    int occ = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, sconv_kernel<C, COUT, ST, BNB>, 256, 0) == hipSuccess &&
        occ >= 1 && occ < n)
      n = occ;
    return n;
  }();
  const int g = 256 * per_cu;
  return ntiles < g ? ntiles : g;
}

template <bool BNB>
static bool sconv_dispatch(const PgArgs& a, int ntiles, hipStream_t st) {
  if (a.stride == 1 && a.C == 32 && a.Cout == 32) {
    set_last_kernel(BNB ? "sconv_kernel<32,32,bnb>" : "sconv_kernel<32,32>");
    hipLaunchKernelGGL((sconv_kernel<32, 32, 1, BNB>), dim3(sconv_grid<32, 32, 1, BNB>(ntiles)), dim3(256), 0, st, a, ntiles);
  } else if (a.stride == 1 && a.C == 32 && a.Cout == 64) {
    set_last_kernel(BNB ? "sconv_kernel<32,64,bnb>" : "sconv_kernel<32,64>");
    hipLaunchKernelGGL((sconv_kernel<32, 64, 1, BNB>), dim3(sconv_grid<32, 64, 1, BNB>(ntiles)), dim3(256), 0, st, a, ntiles);
  } else if (a.stride == 1 && a.C == 64 && a.Cout == 32) {
    set_last_kernel(BNB ? "sconv_kernel<64,32,bnb>" : "sconv_kernel<64,32>");
    hipLaunchKernelGGL((sconv_kernel<64, 32, 1, BNB>), dim3(sconv_grid<64, 32, 1, BNB>(ntiles)), dim3(256), 0, st, a, ntiles);
  } else if (a.stride == 1 && a.C == 64 && a.Cout == 64) {
    set_last_kernel(BNB ? "sconv_kernel<64,64,bnb>" : "sconv_kernel<64,64>");
    hipLaunchKernelGGL((sconv_kernel<64, 64, 1, BNB>), dim3(sconv_grid<64, 64, 1, BNB>(ntiles)), dim3(256), 0, st, a, ntiles);
  } else if (a.stride == 2 && a.C == 8 && a.Cout == 32) {
    set_last_kernel(BNB ? "sconv_kernel<8,32,s2,bnb>" : "sconv_kernel<8,32,s2>");
    hipLaunchKernelGGL((sconv_kernel<8, 32, 2, BNB>), dim3(sconv_grid<8, 32, 2, BNB>(ntiles)), dim3(256), 0, st, a, ntiles);
  } else {
    return false;
  }
  return true;
}

// candidate 20: the direct small-channel kernel; false if the shape is not one
bool sconv_launch(const PgArgs& a, hipStream_t st) {
  if (!sconv_ok(a)) return false;
  const int ntiles = (int)((a.M + 255) / 256);
  if (a.bnb) return sconv_dispatch<true>(a, ntiles, st);
  return sconv_dispatch<false>(a, ntiles, st);
}

// ---------------------------------------------------------------------------
// Halo-tiled direct 3x3 convolution (stride 1, pad 1; C in {32, 64} channels
// in, Cout in {32, 64} out): the stem conv2/conv3 (models.py:312-317, 112x112)
// and the layer-1 conv2 (models.py:200-201, 56x56), forward and data gradient
// with the fused BN-backward reduction.
//
// An output tile is TR x TC pixels of one image (all Cout channels): 16 x 16
// where the image splits evenly and three such halos fit the LDS beside the
// filters, else 8 x 16.  Its input halo of (TR+2) x (TC+2) pixels is brought
// into LDS ONCE by LDS-DMA and all nine taps read it there (sconv re-reads every
// input pixel nine times through L1/L2 as fragment-shaped loads); the filter
// bank stays in LDS for the whole persistent block.
//
// Eight compute waves, two per SIMD, as two groups of four that take the
// block's tiles alternately, half a tile apart.  Between two workgroup barriers
// one group runs the MFMAs of tile j while the other runs the epilogue of tile
// j - 1 (BN-backward arithmetic, 16-B stores) and issues the halo DMA of tile
// j + 2, so a SIMD's matrix pipe has work while its other wave stores.  There
// is no loader wave: the four waves of the group in its epilogue half share the
// DMA instructions, and each waits for its own (vmcnt(0)) before the barrier
// that ends its next MFMA half — the barrier after which the other group reads
// that halo.  Three halo buffers: tile j in buffer j % 3; the buffer of tile j
// is refilled (tile j + 3) by the group that read it, after the barrier that
// ends its MFMA half.  Every wave passes n + 1 barriers for the block's n tiles
// (group 1 starts one barrier late; the group without a tile in the last half
// passes one more at the end).
//
// Halo LDS image: 1-KB blocks of PB pixels x CPT 16-B channel chunks, chunk
// major inside a block (lane l of a DMA instruction fills chunk l / PB of
// pixel l % PB, so one instruction reads PB whole pixels = 1 KB of contiguous
// NHWC input).  A B fragment read (16 consecutive halo pixels of one tile row,
// one chunk per lane quad) then hits 16 distinct 16-B bank slots in every
// ds_read_b128 lane group, for every tap offset; the filter reads keep sconv's
// pg_perm / sc_sw image (SQ_LDS_BANK_CONFLICT 0 in every instance).
//
// The BN-backward operand of the epilogue (y of the BN before the ReLU) is
// loaded one tile of the group ahead, after the previous epilogue.  The sums (BN
// statistics, or the BN-backward reduction) stay in registers, one partial per
// lane, across all tiles of a segment; a wave reduces them over its 16 pixel
// lanes and adds them to its replica slot when the segment changes and at the
// end — a few times per launch, not once per tile — so the tile loop has no LDS
// accumulator, no counter and no flush.  (The deterministic mode takes no sums
// from this kernel: it launches it without them.)
//
// With 64 -> 64 channels the filters take 72 KB, which leaves the LDS for three
// 8 x 16 halos and no more: neither a second workgroup per CU, nor a tile whose
// rows are 56 wide (2 x 56 needs 29 KB per halo, 87 KB for three), nor four
// pixel fragments per wave (a 16 x 16 halo is 41 KB) fits.
// ---------------------------------------------------------------------------
#define HC_MAXSEG 4
template <int C>
__device__ __forceinline__ int hc_addr(int q, int c) {
  constexpr int PB = 64 / (C / 8);
  constexpr int PBL = PB == 16 ? 4 : 3;
  return ((q >> PBL) << 10) + c * (PB * 16) + ((q & (PB - 1)) << 4);
}

template <int C, int COUT, int TR, int TC, bool BNB>
struct HcGeom {
  static constexpr int NWG = 4;                    // compute waves per group
  static constexpr int CPT = C / 8, PB = 64 / CPT;
  static constexpr int NKK = 9 * C / 32;
  static constexpr int MTC = COUT / 16, NP = MTC / 2;
  static constexpr int TCB = TC / 16;
  static constexpr int NTP = TR * TCB / NWG;       // MFMA pixel tiles per wave
  static constexpr int HW = TC + 2, NQ = HW * (TR + 2);
  static constexpr int NB = (NQ + PB - 1) / PB;
  static constexpr int HB = NB * 1024;
  static constexpr int WB = NKK * COUT * 64;
  // BN-backward parameters per segment: an LDS table, or, where the table is what
  // would not fit (64 -> 32 at 16 x 16: 159 KB of filters and halos), the lane's
  // own 8 channels in registers, reloaded when the segment changes
  static constexpr int PTAB = BNB ? HC_MAXSEG * 4 * COUT * 4 : 0;
  static constexpr bool PREG = BNB && NP == 1 && WB + 3 * HB + PTAB > 160 * 1024;
  static constexpr int PRM = PREG ? 0 : PTAB;
  static constexpr int LDS = WB + 3 * HB + PRM;
  static constexpr bool FITS = LDS <= 160 * 1024;
};

template <int C, int COUT, int TR, int TC, bool BNB>
__global__ void __launch_bounds__(512) hconv_kernel(PgArgs a, int ntiles) {
  using Gm = HcGeom<C, COUT, TR, TC, BNB>;
  constexpr int NWG = Gm::NWG, PB = Gm::PB, NKK = Gm::NKK, MTC = Gm::MTC, NP = Gm::NP;
  constexpr int TCB = Gm::TCB, NTP = Gm::NTP, HW = Gm::HW, NQ = Gm::NQ, NB = Gm::NB, HB = Gm::HB;
  constexpr int WB = Gm::WB;
  static_assert(C % 32 == 0 && COUT % 32 == 0 && TC % 16 == 0, "tile shape");
  static_assert(NTP * NWG == TR * TCB, "pixel tiles per wave");
  static_assert(Gm::FITS, "LDS");
  __shared__ __attribute__((aligned(16))) char smem[Gm::LDS];
  float* prm = reinterpret_cast<float*>(smem + WB + 3 * HB);  // [seg][istd, mean, mask scale, mask beta][COUT]
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int grp = wid >> 2, wg = wid & 3;
  const int fr = lane & 15, fq = lane >> 4;
  const int G = gridDim.x;
  const int ntw = (a.Wo + TC - 1) / TC, nth = (a.Ho + TR - 1) / TR;
  const int HoWo = a.Ho * a.Wo;
  const bool sums = a.stats != nullptr || BNB;
  const int n = (ntiles - (int)blockIdx.x + G - 1) / G;  // tiles of this block (the grid is at most ntiles)

  // this wave's share of the halo DMA of the block's j-th tile -> buffer j % 3
  auto issue_halo = [&](int j) {
    const int t = blockIdx.x + j * G;
    const int img = t / (nth * ntw), rem = t - img * (nth * ntw);
    const int h0 = (rem / ntw) * TR, w0 = (rem - (rem / ntw) * ntw) * TC;
    const __amdgpu_buffer_rsrc_t xr =
        pg_rsrc(reinterpret_cast<const bf16*>(a.x) + (long long)img * a.sN, (a.x_elems - (long long)img * a.sN) * 2);
    char* hb = smem + WB + (j % 3) * HB;
    const int c = lane / PB, ql = lane - c * PB;
    for (int b = wg; b < NB; b += NWG) {
      const int q = b * PB + ql;
      const int hr = q / HW, hc = q - (q / HW) * HW;
      const int ih = h0 - 1 + hr, iw = w0 - 1 + hc;
      const bool ok = q < NQ && ih >= 0 && ih < a.H && iw >= 0 && iw < a.W;
      glds16(xr, hb + b * 1024, ok ? (unsigned)((ih * (int)a.sH + iw * (int)a.sW) * 2 + c * 16) : PG_OOB);
    }
  };

  if (grp < n) issue_halo(grp);
  if constexpr (BNB && !Gm::PREG) {
    const int nsg = a.seg_m > 0 ? (int)(a.M / a.seg_m) : 1;
    for (int i = tid; i < nsg * 4 * COUT; i += 128 * NWG) {
      const int sg = i / (4 * COUT), r = (i / COUT) & 3, ch = i % COUT;
      const float* src = r == 0 ? a.bnb_istd[0] : r == 1 ? a.bnb_mean[0]
                       : r == 2 ? a.bnb_mbn + 2 * a.Cout : a.bnb_mbn + 3 * a.Cout;
      prm[i] = src[sg * a.bnb_pstride + ch];
    }
  }
  // filters -> LDS (sconv's image: block kk holds COUT rows of 64 B)
  for (int i = tid; i < NKK * COUT * 4; i += 128 * NWG) {
    const int kk = i / (COUT * 4), rem = i - kk * COUT * 4;
    const int rho = rem >> 2, c = rem & 3;
    const uint4 v =
        *reinterpret_cast<const uint4*>(reinterpret_cast<const bf16*>(a.w) + (long long)pg_perm(rho) * a.K + kk * 32 + c * 8);
    *reinterpret_cast<uint4*>(smem + (kk * COUT + rho) * 64 + ((c ^ sc_sw(rho)) << 4)) = v;
  }
  vm_wait<0>();  // the first halos of both groups have landed before barrier 0

  // per MFMA pixel tile m of the block's j-th tile: this lane's output pixel and its halo position
  auto tile_px = [&](int j, long long (&px)[NTP], bool (&pv)[NTP], int (&qb)[NTP]) {
    const int tile = blockIdx.x + j * G;
    const int img = tile / (nth * ntw), rem = tile - img * (nth * ntw);
    const int h0 = (rem / ntw) * TR, w0 = (rem - (rem / ntw) * ntw) * TC;
    const long long pimg = (long long)img * HoWo;
#pragma unroll
    for (int m = 0; m < NTP; ++m) {
      const int mt = wg * NTP + m, row = mt / TCB, cb = mt - (mt / TCB) * TCB;
      const int oh = h0 + row, ow = w0 + cb * 16 + fr;
      pv[m] = oh < a.Ho && ow < a.Wo;
      px[m] = pv[m] ? pimg + oh * a.Wo + ow : pimg;
      qb[m] = row * HW + cb * 16 + fr;
    }
    return pimg;
  };
  // the BN-backward operand of a tile is loaded one tile of the group ahead
  // (issued after the previous epilogue), so its latency runs under the other
  // group's half and this group's MFMAs
  Vec16<bf16> yp[NP][NTP];
  auto load_yp = [&](int j) {
    long long px[NTP];
    bool pv[NTP];
    int qb[NTP];
    tile_px(j, px, pv, qb);
#pragma unroll
    for (int p = 0; p < NP; ++p)
#pragma unroll
      for (int m = 0; m < NTP; ++m)
        yp[p][m] = ld16<bf16>(reinterpret_cast<const bf16*>(a.bnb_y[0]) + px[m] * a.ldy + 32 * p + 8 * fq);
  };
  if constexpr (BNB) {
    if (grp < n) load_yp(grp);
  }
  // the sums carried across the tiles of a segment, and their flush
  float cs1[NP][8], cs2[NP][8];
#pragma unroll
  for (int p = 0; p < NP; ++p)
#pragma unroll
    for (int e = 0; e < 8; ++e) { cs1[p][e] = 0.f; cs2[p][e] = 0.f; }
  long long cseg = -1;
  float preg[4][8];  // PREG: istd, mean, mask scale, mask beta of the lane's channels
  const int slot = (int)((blockIdx.x * (2 * NWG) + wid) % ARTSBIR_NSLOT);
  auto sums_flush = [&]() {
    const long long so = cseg * a.seg_stride + (long long)slot * 2 * a.Cout;
    float* dst = (BNB ? a.bnb_slots[0] : a.stats) + so;
#pragma unroll
    for (int p = 0; p < NP; ++p) {
      const int ch0 = 32 * p + 8 * fq;
#pragma unroll
      for (int e = 0; e < 8; ++e) { cs1[p][e] = dpp_row_sum(cs1[p][e]); cs2[p][e] = dpp_row_sum(cs2[p][e]); }
      if (fr == 15 && !(a.dbg & 1)) {
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          atomicAdd(dst + ch0 + e, cs1[p][e]);
          atomicAdd(dst + a.Cout + ch0 + e, cs2[p][e]);
        }
      }
#pragma unroll
      for (int e = 0; e < 8; ++e) { cs1[p][e] = 0.f; cs2[p][e] = 0.f; }
    }
  };
  auto barrier = [&]() {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
  };

  if (grp == 1) {
    barrier();  // barrier 0: group 0 starts tile 0
    if (2 < n) issue_halo(2);
  }
  for (int j = grp; j < n; j += 2) {
    barrier();  // barrier j: halo j visible
    long long px[NTP];
    bool pv[NTP];
    int qb[NTP];
    const long long pimg = tile_px(j, px, pv, qb);
    const long long wseg = a.seg_m > 0 ? pimg / a.seg_m : 0;
    // ---- MFMAs: filters (A) and halo (B) from LDS
    const char* hb = smem + WB + (j % 3) * HB;
    f32x4 acc[MTC][NTP];
#pragma unroll
    for (int i = 0; i < MTC; ++i)
#pragma unroll
      for (int m = 0; m < NTP; ++m) acc[i][m] = f32x4{0.f, 0.f, 0.f, 0.f};
    constexpr int KPT = C / 32;  // 32-k steps per tap
    // taps fully unrolled where the registers allow (no spills), else by rows
    constexpr int TUN = (NTP <= 2 || (C == 32 && MTC * NTP <= 8)) ? 9 : 3;
#pragma unroll TUN
    for (int t = 0; t < 9; ++t) {
      const int toff = (t / 3) * HW + (t % 3);
      int qa[NTP];
#pragma unroll
      for (int m = 0; m < NTP; ++m) qa[m] = qb[m] + toff;
#pragma unroll
      for (int h = 0; h < KPT; ++h) {
        const int kk = t * KPT + h, c = h * 4 + fq;
        uint4 af[MTC], bv[NTP];
#pragma unroll
        for (int i = 0; i < MTC; ++i) {
          const int rho = i * 16 + fr;
          af[i] = *reinterpret_cast<const uint4*>(smem + (kk * COUT + rho) * 64 + ((fq ^ sc_sw(rho)) << 4));
        }
#pragma unroll
        for (int m = 0; m < NTP; ++m) bv[m] = *reinterpret_cast<const uint4*>(hb + hc_addr<C>(qa[m], c));
#pragma unroll
        for (int i = 0; i < MTC; ++i)
#pragma unroll
          for (int m = 0; m < NTP; ++m)
            acc[i][m] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(*reinterpret_cast<const bf16x8*>(&af[i]),
                                                                *reinterpret_cast<const bf16x8*>(&bv[m]), acc[i][m], 0, 0, 0);
      }
    }
    // this wave's DMAs of halo j + 1 (issued in its previous epilogue half) have
    // landed before the barrier after which the other group reads them
    vm_wait<0>();
    barrier();  // barrier j + 1: buffer j % 3 is free
    if (j + 3 < n) issue_halo(j + 3);
    // ---- epilogue: BN statistics or the fused BN-backward reduction, bf16 stores
    if (sums && wseg != cseg) {
      if (cseg >= 0) sums_flush();
      cseg = wseg;
      if constexpr (Gm::PREG) {
        const long long po = wseg * a.bnb_pstride + 8 * fq;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          preg[0][e] = a.bnb_istd[0][po + e];
          preg[1][e] = a.bnb_mean[0][po + e];
          preg[2][e] = a.bnb_mbn[2 * a.Cout + po + e];
          preg[3][e] = a.bnb_mbn[3 * a.Cout + po + e];
        }
      }
    }
#pragma unroll
    for (int p = 0; p < NP; ++p) {
      const int ch0 = 32 * p + 8 * fq;
      float xa[8], xm[8], ms[8], mh[8];
      if constexpr (Gm::PREG) {
#pragma unroll
        for (int e = 0; e < 8; ++e) { xa[e] = preg[0][e]; xm[e] = preg[1][e]; ms[e] = preg[2][e]; mh[e] = preg[3][e]; }
      } else if constexpr (BNB) {
        const float* pp = prm + wseg * 4 * COUT + ch0;
        loadf8v(pp, xa);
        loadf8v(pp + COUT, xm);
        loadf8v(pp + 2 * COUT, ms);
        loadf8v(pp + 3 * COUT, mh);
      }
#pragma unroll
      for (int m = 0; m < NTP; ++m) {
        float v[8];
#pragma unroll
        for (int r = 0; r < 4; ++r) { v[r] = acc[2 * p][m][r]; v[4 + r] = acc[2 * p + 1][m][r]; }
        if (pv[m]) {
          if constexpr (!BNB) {  // eval-mode conv + folded BN (+ ReLU): bias and activation here
            if (a.bias) {
#pragma unroll
              for (int e = 0; e < 8; ++e) v[e] += a.bias[ch0 + e];
            }
            if (a.relu) {
#pragma unroll
              for (int e = 0; e < 8; ++e) v[e] = fmaxf(v[e], 0.f);
            }
          }
          if constexpr (BNB) {
#pragma unroll
            for (int e = 0; e < 8; ++e) {
              const float yv = to_f(yp[p][m].v[e]);
              v[e] = (yv - xm[e]) * ms[e] + mh[e] > 0.f ? v[e] : 0.f;  // kind 1: target 0 is the ReLU's BN
              cs1[p][e] += v[e];
              cs2[p][e] += v[e] * ((yv - xm[e]) * xa[e]);
            }
          } else if (sums) {
#pragma unroll
            for (int e = 0; e < 8; ++e) { cs1[p][e] += v[e]; cs2[p][e] += v[e] * v[e]; }
          }
          Vec16<bf16> o;
#pragma unroll
          for (int e = 0; e < 8; ++e) o.v[e] = from_f<bf16>(v[e]);
          st16<bf16>(reinterpret_cast<bf16*>(a.y) + px[m] * a.ldy + ch0, o);
        }
      }
    }
    if constexpr (BNB) {
      if (j + 2 < n) load_yp(j + 2);
    }
  }
  // barrier n for the group that took no tile in the last half.  n = 3: group 0 (tiles 0, 2) passed
  // barriers 0 1 2 3 in its loop, group 1 (tile 1) passed 0 before it and 1 2 in it and takes 3 here;
  // n = 4: group 1 (tiles 1, 3) passed 0, then 1 2 3 4, group 0 (tiles 0, 2) passed 0 1 2 3 and takes 4 here
  if (((n + grp) & 1) == 0) barrier();
  if (sums && cseg >= 0) sums_flush();
}

// shapes the halo-tiled kernel takes
static bool hconv_ok(const PgArgs& a) {
  if (a.R != 3 || a.S != 3 || a.pad != 1 || a.stride != 1 || a.M <= 0) return false;
  if ((a.C != 32 && a.C != 64) || (a.Cout != 32 && a.Cout != 64) || a.K != 9 * a.C) return false;
  if (a.res_mode || (a.bnb && (a.bnb != 1 || a.bnb_nt != 1 || a.stats))) return false;
  const long long HoWo = (long long)a.Ho * a.Wo;
  if (a.Ho != a.H || a.Wo != a.W || a.M % HoWo) return false;
  // statistics segments are whole images (a tile never spans two)
  if (a.seg_m > 0 && (a.seg_m % HoWo || a.M % a.seg_m)) return false;
  if (a.bnb && a.seg_m > 0 && a.M / a.seg_m > HC_MAXSEG) return false;
  if (a.sW < a.C || a.sN * 2 > 0x7fffffffLL || (long long)a.H * a.sH * 2 > 0x7fffffffLL) return false;
  const long long nt = (a.M / HoWo) * ((a.Ho + 15) / 16) * ((a.Wo + 15) / 16) * 2;
  return nt < 0x7fffffffLL;
}

// persistent grid: one workgroup of 512 per CU, or as many as the LDS and the registers admit
template <int C, int COUT, int TR, int TC, bool BNB>
static void hconv_go(const PgArgs& a, hipStream_t st) {
  using Gm = HcGeom<C, COUT, TR, TC, BNB>;
  const int ntiles = (int)((a.M / ((long long)a.Ho * a.Wo)) * ((a.Ho + TR - 1) / TR) * ((a.Wo + TC - 1) / TC));
  static const int per_cu = [] {
    int n = (160 * 1024) / Gm::LDS;
    if (n > 4) n = 4;  // 4 x 512 threads: 32 waves per CU
    int occ = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, hconv_kernel<C, COUT, TR, TC, BNB>, 512, 0) == hipSuccess &&
        occ >= 1 && occ < n)
      n = occ;
    return n;
  }();
  const int g = 256 * per_cu < ntiles ? 256 * per_cu : ntiles;
  static const char* nm = nullptr;
  static char buf[64];
  if (!nm) {
    snprintf(buf, sizeof buf, "hconv_kernel<%d,%d,%dx%d%s>", C, COUT, TR, TC, BNB ? ",bnb" : "");
    nm = buf;
  }
  set_last_kernel(nm);
  hipLaunchKernelGGL((hconv_kernel<C, COUT, TR, TC, BNB>), dim3(g), dim3(512), 0, st, a, ntiles);
}

template <int C, int COUT, bool BNB>
static void hconv_tiles(const PgArgs& a, hipStream_t st) {
  // 16 x 16 tiles when the image splits evenly (stem, 112 x 112) and three such halos fit the LDS
  // beside the filters (not 64 -> 64), else 8 x 16
  if constexpr (HcGeom<C, COUT, 16, 16, BNB>::FITS) {
    if (a.Ho % 16 == 0 && a.Wo % 16 == 0) return hconv_go<C, COUT, 16, 16, BNB>(a, st);
  }
  hconv_go<C, COUT, 8, 16, BNB>(a, st);
}

template <bool BNB>
static void hconv_dispatch(const PgArgs& a, hipStream_t st) {
  if (a.C == 32 && a.Cout == 32) hconv_tiles<32, 32, BNB>(a, st);
  else if (a.C == 32) hconv_tiles<32, 64, BNB>(a, st);
  else if (a.Cout == 32) hconv_tiles<64, 32, BNB>(a, st);
  else hconv_tiles<64, 64, BNB>(a, st);
}

// candidate 21: the halo-tiled small-channel kernel
bool hconv_launch(const PgArgs& a, hipStream_t st) {
  if (!hconv_ok(a)) return false;
  if (a.bnb) hconv_dispatch<true>(a, st);
  else hconv_dispatch<false>(a, st);
  return true;
}

}  // namespace artsbir
