// Streaming Bottleneck tail fused with the next block's first 1x1 conv (gfx950).
// Reference: models.py:220-236 (bn3, the downsample BN, out += identity, relu3)
// of one Bottleneck and models.py:198-199 (conv1, bn1's batch statistics) of the
// next, run by autograd as separate modules.
//
//   out[m][k] = relu(bn3(y3[m][k]) + r[m][k]),  r = identity or bnd(yd)
//   y1[m][n]  = sum_k out[m][k] W[n][k],  stats += (sum y1, sum y1^2) per segment
//
// conv1 has K = 4 planes inputs and only N = planes outputs, so the pair
// (block_out, then the conv reading `out` back) is a byte stream read twice with
// a small GEMM behind it.  Here one pass forms `out` in registers in the MFMA's
// pixel-operand layout, stores it (and the ReLU mask bits of the stored values)
// as a by-product and feeds the same registers to the MFMAs; the read-back of
// `out` and one launch per block disappear.  The mirror image of rstream.hip:
//  * the whole W ([N][K], rows permuted so a lane's MFMA outputs are 8
//    consecutive channels: pg_perm; XOR-swizzled 16-B chunks) stays in LDS, read
//    once per workgroup; every wave of the workgroup computes all N outputs of
//    its own 16-pixel blocks (blocks b0 + wave, + BS_NW, ... of a contiguous range);
//  * the operands go from global memory straight into registers, BS_KC k-steps
//    (128 channels: two whole 128-B lines per pixel and tensor, both halves of a
//    line in adjacent requests) per pipeline stage, one stage ahead — a stage's
//    elementwise work, stores and MFMAs run while the next stage's 8 KB per wave
//    are in flight; the pipeline runs over K-chunks, not whole blocks, because a
//    K = 512 block's operands alone are 128 registers per lane;
//  * a lane owns K / 32 eight-channel groups, so the BN parameters (3 floats per
//    channel and BN) cannot live in registers: they are read from an LDS table
//    of the BS_NSEGT segments the workgroup's range can touch;
//  * bn1's sums are carried in registers across a wave's blocks and reduced
//    (DPP) and flushed with global atomics only when the BN segment changes.
#include "common.h"
#include "pgemm.h"
#include "pgemm_dev.h"
#include "../../include/artsbir.h"

namespace artsbir {

constexpr int BS_NW = 8;      // waves per workgroup: one workgroup per CU, two waves per SIMD, <= 256 registers each
constexpr int BS_KC = 4;      // MFMA k-steps (32 channels each) per pipeline stage
constexpr int BS_CHUNK = 64;  // 16-pixel blocks per workgroup (upper bound)
// segments whose BN parameters a workgroup holds: its range of at most
// BS_CHUNK blocks lies within two consecutive segments (bstream_launch sizes
// the ranges so); every segment's table would not fit beside a 128 KB W
constexpr int BS_NSEGT = 2;
// non-temporal stores (bit 0: out, bit 1: y1).  `out` is read again at once, by
// the next block's launch of this kernel as its residual, y1 by act_pool:
// plain stores measured faster for both (profiles/r7_blockconv_bench.txt)
#ifndef ARTSBIR_BS_NT
#define ARTSBIR_BS_NT 0
#endif

// A wave-uniform base p + off held in scalar registers (pg_uniform), as a
// global-memory pointer: through the integer round trip the compiler no longer
// knows the address space, and generic (flat) loads count on both wait counters,
// which turns every counted wait of the load pipeline into a full drain
#define BS_GLOBAL __attribute__((address_space(1)))
template <typename T>
__device__ __forceinline__ BS_GLOBAL T* bs_base(T* p, long long off) {
  return (BS_GLOBAL T*)pg_uniform((long long)(p + off));
}

typedef __attribute__((ext_vector_type(4))) unsigned bs_u4;
template <bool NT>
__device__ __forceinline__ void bs_store(BS_GLOBAL bf16* p, const Vec16<bf16>& v) {
  if constexpr (NT) __builtin_nontemporal_store(*reinterpret_cast<const bs_u4*>(&v), reinterpret_cast<BS_GLOBAL bs_u4*>(p));
  else *reinterpret_cast<BS_GLOBAL bs_u4*>(p) = *reinterpret_cast<const bs_u4*>(&v);
}

struct BsArgs {
  const bf16* y3;
  const bf16* res;    // the identity, or yd when bnd is set
  const bf16* w;      // [N][K]
  const float* bn3;   // [nseg][4][K] parameter blocks (mean, istd, scale, beta)
  const float* bnd;   // the downsample BN's, or null
  bf16* out;
  unsigned char* bits;  // optional
  bf16* y1;
  float* stats;       // [nseg][ARTSBIR_NSLOT][2][N], optional
  int nblk;           // 16-pixel blocks in all
  int seg_blk;        // per BN segment
  int nseg;
  int chunk;          // blocks per workgroup
};

template <int K, int N, bool TWO>
__global__ void __launch_bounds__(BS_NW * 64) bstream_kernel(BsArgs a) {
  constexpr int CPR = K / 8;          // 16-B chunks per W row
  constexpr int NKC = K / (32 * BS_KC);  // pipeline stages per block
  constexpr int NT = N / 16;          // MFMA row tiles (output channels)
  constexpr int NP = N / 32;          // 8-channel output groups per lane
  constexpr int NQ = TWO ? 6 : 3;     // parameter rows: mean, scale, beta (x2)
  static_assert(NKC % 2 == 0, "two operand sets, a whole number of pairs per block");
  __shared__ __attribute__((aligned(16))) char wlds[N * K * 2];
  __shared__ __attribute__((aligned(16))) float prm[BS_NSEGT][NQ][K];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int fr = lane & 15, fq = lane >> 4;
  const int b0 = blockIdx.x * a.chunk;
  const int b1 = b0 + a.chunk < a.nblk ? b0 + a.chunk : a.nblk;
  const int seg0 = b0 / a.seg_blk;

  // ---- W (permuted rows, swizzled chunks) and the BN constants into LDS
  {
    const bf16* wg = a.w;
    for (int i = tid; i < N * CPR; i += BS_NW * 64) {
      const int rho = i / CPR, c = i - rho * CPR;
      const uint4 v = *reinterpret_cast<const uint4*>(wg + (long long)pg_perm(rho) * K + c * 8);
      *reinterpret_cast<uint4*>(wlds + (rho * CPR + (c ^ (rho & 15))) * 16) = v;
    }
    const float* p3 = a.bn3;
    const float* pd = TWO ? a.bnd : a.bn3;
#pragma unroll
    for (int t = 0; t < BS_NSEGT; ++t) {
      const bool on = seg0 + t < a.nseg;
      const long long po = (long long)(on ? seg0 + t : seg0) * 4 * K;
      for (int c = tid; c < K; c += BS_NW * 64) {
        prm[t][0][c] = p3[po + c];
        prm[t][1][c] = p3[po + 2 * K + c];
        prm[t][2][c] = p3[po + 3 * K + c];
        if constexpr (TWO) {
          prm[t][3][c] = pd[po + c];
          prm[t][4][c] = pd[po + 2 * K + c];
          prm[t][5][c] = pd[po + 3 * K + c];
        }
      }
    }
  }
  __syncthreads();

  // the argument fields the loop uses, as locals (the lambdas below must not
  // take the by-value kernel argument by reference: that copies it to scratch)
  const bf16* const y3p = a.y3;
  const bf16* const resp = a.res;
  bf16* const outp = a.out;
  bf16* const y1p = a.y1;
  unsigned char* const bitp = a.bits;
  float* const statp = a.stats;
  const int seg_blk = a.seg_blk;
  const int slot = blockIdx.x % ARTSBIR_NSLOT;
  // the lane's element offsets inside a 16-pixel block: pixel fr, channels 8 fq ..
  const unsigned lof = fr * K + 8 * fq, lob = fr * CPR + fq, lo1 = fr * N + 8 * fq;
  const int lx = fq ^ fr;  // chunk slot of k-step ks in the lane's W rows: (4 ks + fq) ^ fr = (4 ks) ^ lx

  float s1[NP][8], s2[NP][8];
  auto zero_sums = [&]() __attribute__((always_inline)) {
#pragma unroll
    for (int p = 0; p < NP; ++p)
#pragma unroll
      for (int e = 0; e < 8; ++e) { s1[p][e] = 0.f; s2[p][e] = 0.f; }
  };
  zero_sums();
  auto flush = [&](int seg) __attribute__((always_inline)) {
#pragma unroll
    for (int p = 0; p < NP; ++p) {
#pragma unroll
      for (int e = 0; e < 8; ++e) { s1[p][e] = dpp_row_sum(s1[p][e]); s2[p][e] = dpp_row_sum(s2[p][e]); }
      if (statp && fr == 15) {
        // the lane's offset formed here (opaque): hoisted above the block loop the
        // address pair is live through it, one spill at K = 512 with two BNs
        int lo = 8 * fq;
        asm volatile("" : "+v"(lo));
        float* so = statp + ((long long)seg * ARTSBIR_NSLOT + slot) * 2 * N + 32 * p + lo;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          atomicAdd(so + e, s1[p][e]);
          atomicAdd(so + N + e, s2[p][e]);
        }
      }
    }
    zero_sums();
  };

  // one stage's operands of block blk: 128 channels of y3 and of the residual
  // operand for the lane's pixel, as the MFMA pixel fragments (k = 32 s + 8 fq)
  auto load = [&](int blk, int kc, bs_u4 (&yv)[BS_KC], bs_u4 (&rv)[BS_KC]) __attribute__((always_inline)) {
    // wave-uniform block base (pg_uniform: kept in scalar registers) + the lane's
    // 32-bit offset: no 64-bit address pair per tensor in vector registers
    const BS_GLOBAL bf16* yblk = bs_base(y3p, (long long)blk * 16 * K);
    const BS_GLOBAL bf16* rblk = bs_base(resp, (long long)blk * 16 * K);
    const unsigned o = lof + kc * (32 * BS_KC);
#pragma unroll
    for (int s = 0; s < BS_KC; ++s) yv[s] = *reinterpret_cast<const BS_GLOBAL bs_u4*>(yblk + (o + 32 * s));
#pragma unroll
    for (int s = 0; s < BS_KC; ++s) rv[s] = *reinterpret_cast<const BS_GLOBAL bs_u4*>(rblk + (o + 32 * s));
  };
  // the stage: out (stored with its mask bits) and its share of the GEMM
  auto stage = [&](int blk, int kc, int tseg, int wrow, const bs_u4 (&yv)[BS_KC], const bs_u4 (&rv)[BS_KC],
                   f32x4 (&acc)[NT]) __attribute__((always_inline)) {
    BS_GLOBAL bf16* oblk = bs_base(outp, (long long)blk * 16 * K);
    BS_GLOBAL unsigned char* bblk = bs_base(bitp, (long long)blk * 16 * CPR);
#pragma unroll
    for (int s = 0; s < BS_KC; ++s) {
      const int ks = kc * BS_KC + s;
      const int c0 = 32 * ks + 8 * fq;
      const bf16* yb = reinterpret_cast<const bf16*>(&yv[s]);
      const bf16* rb = reinterpret_cast<const bf16*>(&rv[s]);
      float r[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) r[e] = to_f(rb[e]);
      if constexpr (TWO) {
        float m2[8], s2v[8], h2[8];
        loadf8v(&prm[tseg][3][c0], m2);
        loadf8v(&prm[tseg][4][c0], s2v);
        loadf8v(&prm[tseg][5][c0], h2);
#pragma unroll
        for (int e = 0; e < 8; ++e) r[e] = bn_value(r[e], m2[e], s2v[e], h2[e]);
        // the second BN's 24 parameter registers are dead before bn3's are
        // loaded (scheduled together they spill at K = 512)
        __builtin_amdgcn_sched_barrier(0);
      }
      float m[8], sc[8], h[8];
      loadf8v(&prm[tseg][0][c0], m);
      loadf8v(&prm[tseg][1][c0], sc);
      loadf8v(&prm[tseg][2][c0], h);
      Vec16<bf16> ov;
      unsigned mk = 0;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        ov.v[e] = from_f<bf16>(block_out_value(to_f(yb[e]), m[e], sc[e], h[e], r[e]));
        mk |= (to_f(ov.v[e]) > 0.f ? 1u : 0u) << e;  // of the stored value
      }
      bs_store<(ARTSBIR_BS_NT & 1) != 0>(oblk + (lof + 32 * ks), ov);
      if (bitp) bblk[lob + 4 * ks] = (unsigned char)mk;
      // the rounded values are conv1's pixel operand
      const bf16x8 bfrag = *reinterpret_cast<const bf16x8*>(&ov);
      // A fragments four row tiles at a time (all N / 16 at once cost 32 registers at N = 128)
#pragma unroll
      for (int i0 = 0; i0 < NT; i0 += 4) {
        uint4 af[4];
#pragma unroll
        for (int i = 0; i < 4; ++i)
          af[i] = *reinterpret_cast<const uint4*>(wlds + wrow + (16 * (i0 + i) * CPR + ((4 * ks) ^ lx)) * 16);
#pragma unroll
        for (int i = 0; i < 4; ++i)
          acc[i0 + i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(*reinterpret_cast<const bf16x8*>(&af[i]), bfrag,
                                                                acc[i0 + i], 0, 0, 0);
        if (NT > 4) __builtin_amdgcn_sched_barrier(0);
      }
    }
  };
  // y1 of the block and bn1's sums of the f32 accumulators
  auto finish = [&](int blk, const f32x4 (&acc)[NT]) __attribute__((always_inline)) {
    BS_GLOBAL bf16* yblk = bs_base(y1p, (long long)blk * 16 * N);
#pragma unroll
    for (int p = 0; p < NP; ++p) {
      float v[8];
#pragma unroll
      for (int r = 0; r < 4; ++r) { v[r] = acc[2 * p][r]; v[4 + r] = acc[2 * p + 1][r]; }
      Vec16<bf16> ov;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        s1[p][e] += v[e];
        s2[p][e] += v[e] * v[e];
        ov.v[e] = from_f<bf16>(v[e]);
      }
      bs_store<(ARTSBIR_BS_NT & 2) != 0>(yblk + (lo1 + 32 * p), ov);
    }
  };

  // software pipeline over the stages of the wave's blocks (two operand sets)
  bs_u4 ya[BS_KC], ra[BS_KC], yb[BS_KC], rb[BS_KC];
  int blk = b0 + wid;
  int cur = -1, seg = seg0, seg_end = (seg0 + 1) * seg_blk;
  if (blk < b1) load(blk, 0, ya, ra);
  for (; blk < b1; blk += BS_NW) {
    while (blk >= seg_end) { ++seg; seg_end += seg_blk; }
    if (seg != cur) {
      if (cur >= 0) flush(cur);
      cur = seg;
    }
    const int tseg = seg - seg0;
    // the lane's W row offset, opaque per block: the A fragments do not depend
    // on the block, and hoisted out of the loop they would take N K / 256
    // registers per lane (spills at N = 64, where they almost fit)
    int wrow = fr * CPR * 16;
    asm volatile("" : "+v"(wrow));
    f32x4 acc[NT];
#pragma unroll
    for (int i = 0; i < NT; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kp = 0; kp < NKC / 2; ++kp) {
      load(blk, 2 * kp + 1, yb, rb);
      stage(blk, 2 * kp, tseg, wrow, ya, ra, acc);
      if (2 * kp + 2 < NKC) load(blk, 2 * kp + 2, ya, ra);
      else if (blk + BS_NW < b1) load(blk + BS_NW, 0, ya, ra);
      stage(blk, 2 * kp + 1, tseg, wrow, yb, rb, acc);
    }
    finish(blk, acc);
  }
  if (cur >= 0) flush(cur);
}

// The shapes the streaming kernel takes: a static list, each entry measured
// faster than block_out + the tuned conv by more than the pair's own spread
// (profiles/r7_blockconv_bench.txt)
static bool bstream_shape(int K, int N) {
  return (K == 256 && N == 64) || (K == 256 && N == 128) || (K == 512 && N == 128);
}

static int bstream_cus() {
  static const int n = [] {
    int dev = 0, v = 0;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || v <= 0)
      v = 256;
    return v;
  }();
  return n;
}

// false: not this kernel's shape (nothing launched)
static bool bstream_launch(const artsbir_conv_desc* d, const void* y3, const float* bn3, const void* yd,
                           const float* bnd, const void* identity, const void* w, int nseg, void* out,
                           unsigned char* bits, void* y1, float* stats, hipStream_t st) {
  if (d->dtype != ARTSBIR_DT_BF16 || !bstream_shape(d->C, d->Cout)) return false;
  if (d->R != 1 || d->S != 1 || d->stride != 1 || d->pad != 0) return false;
  const long long M = (long long)d->N * d->H * d->W, seg_m = M / nseg;
  // whole 16-pixel blocks per BN segment; block indices in 32 bits
  if (M <= 0 || seg_m % 16 != 0 || M / 16 > 0x3fffffffLL) return false;
  BsArgs a;
  a.y3 = reinterpret_cast<const bf16*>(y3);
  a.res = reinterpret_cast<const bf16*>(yd ? yd : identity);
  a.w = reinterpret_cast<const bf16*>(w);
  a.bn3 = bn3; a.bnd = yd ? bnd : nullptr;
  a.out = reinterpret_cast<bf16*>(out); a.bits = bits;
  a.y1 = reinterpret_cast<bf16*>(y1); a.stats = stats;
  a.nblk = (int)(M / 16); a.seg_blk = (int)(seg_m / 16); a.nseg = nseg;
  // ranges of about BS_CHUNK blocks, their number a multiple of the CU count
  // (one workgroup per CU at a time, equal ranges: whole rounds, no short last
  // one), and no longer than a segment, so a range meets at most BS_NSEGT
  long long wgs = (a.nblk + BS_CHUNK - 1) / BS_CHUNK;
  const int cus = bstream_cus();
  if (wgs > cus) wgs = (wgs + cus - 1) / cus * cus;
  int chunk = (int)((a.nblk + wgs - 1) / wgs);
  if (nseg > BS_NSEGT && chunk > a.seg_blk) chunk = a.seg_blk;
  a.chunk = chunk;
  const dim3 g((unsigned)((a.nblk + chunk - 1) / chunk)), b(BS_NW * 64);
  const bool two = yd != nullptr;
#define BS_GO(KV, NV)                                                                          \
  do {                                                                                         \
    if (two) hipLaunchKernelGGL((bstream_kernel<KV, NV, true>), g, b, 0, st, a);         \
    else hipLaunchKernelGGL((bstream_kernel<KV, NV, false>), g, b, 0, st, a);            \
  } while (0)
  if (d->C == 256 && d->Cout == 64) BS_GO(256, 64);
  else if (d->C == 256) BS_GO(256, 128);
  else BS_GO(512, 128);
#undef BS_GO
  set_last_kernel(two ? "bstream_kernel<two>" : "bstream_kernel<idn>");
  return true;
}

}  // namespace artsbir

using namespace artsbir;

extern "C" int artsbir_block_out_conv1x1_fwd(const artsbir_conv_desc* d, const void* y3, const float* bn3,
                                             const void* yd, const float* bnd, const void* identity, const void* w,
                                             int nseg, void* out, unsigned char* mask_bits, void* y1, float* stats,
                                             void* stream) {
  if (!d) { set_error("block_out_conv1x1_fwd: null descriptor"); return -1; }
  if (d->R != 1 || d->S != 1 || d->stride != 1 || d->pad != 0) {
    set_error("block_out_conv1x1_fwd: the consumer must be a 1x1 stride-1 conv (%dx%d/%d pad %d)", d->R, d->S,
              d->stride, d->pad);
    return -1;
  }
  if (d->C <= 0 || d->C % 8 || d->Cout <= 0 || d->N <= 0 || d->H <= 0 || d->W <= 0) {
    set_error("block_out_conv1x1_fwd: bad shape (C=%d must be a positive multiple of 8)", d->C);
    return -1;
  }
  if (nseg < 1 || d->N % nseg) {
    set_error("block_out_conv1x1_fwd: %d segments do not divide batch %d", nseg, d->N);
    return -1;
  }
  if (!y3 || !bn3 || !w || !out || !y1) { set_error("block_out_conv1x1_fwd: null operand"); return -1; }
  if (!yd && !identity) { set_error("block_out_conv1x1_fwd: need downsample or identity input"); return -1; }
  if (yd && !bnd) { set_error("block_out_conv1x1_fwd: missing BN parameter block"); return -1; }
  if (bstream_launch(d, y3, bn3, yd, bnd, identity, w, nseg, out, mask_bits, y1, stats, (hipStream_t)stream)) {
    ARTSBIR_CHECK_LAUNCH("bstream");
    return 0;
  }
  // any other shape or dtype: the two launches the kernel stands for
  const long long rows = (long long)d->N * d->H * d->W;
  if (artsbir_block_out_mask(d->dtype, y3, bn3, yd, bnd, identity, rows, d->C, nseg, out, mask_bits, stream)) return -1;
  return artsbir_conv2d_fwd_seg(d, out, w, y1, nseg, stats, stream);
}
