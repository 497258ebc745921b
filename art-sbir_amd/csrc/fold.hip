// The BatchNorm backward folded through the 1x1 convolution in front of it
// (gfx950).  Reference chain: models.py:219-220 (Bottleneck conv3 -> bn3) and
// models.py:227-229 (downsample AvgPool -> conv -> BN), differentiated by
// autograd through BatchNorm2d (train) and Conv2d.
//
// In training mode the BN backward maps the masked output gradient g to
//   dy = c1 (g - c2 - xhat c3),   xhat = (y - mean) istd
// (artsbir_bn_bwd_finalize: c1 = gamma istd, c2 = mean g, c3 = mean g xhat), and
// the conv then needs dx = dy W and dW = dy^T x.  With y = x W^T both are linear
// in (g, x), per BN segment s:
//   dx = g (diag(c1) W) + x (W^T diag(b') W) + e,          b' = -c1 c3 istd
//   e  = k W,                                                k = -c1 (c2 - c3 istd mean)
//   dW = diag(c1) g^T x + diag(b') W (x^T x) + k (1^T x)
// so dy never exists: the data gradient is one GEMM over [g | x]
// (artsbir_conv1x1_dgrad_fold below, on the launcher of gemm.hip) with the
// weights this file prepares, and the weight gradient is g^T x, the Gram matrix
// x^T x and the column sums of x per segment, combined here.  That removes the
// BN-backward apply pass (read g, y; write dy) and the data gradient's read of
// dy from the HBM-bound main stream of the step.
#include <cstdlib>

#include "common.h"
#include "conv_launch.h"

namespace artsbir {

// one row ci of segment s: B1[s][ci][co] = c1 W^T[ci][co], A[s][ci][co] = b' W^T[ci][co]
// (the left operand of the Gram-side GEMM), bias[s][ci] = sum_co W^T[ci][co] k[co]
template <typename T>
__global__ void __launch_bounds__(256) fold_prep_kernel(const T* __restrict__ wt, int Co, int Ci,
                                                        const float* __restrict__ coef, const float* __restrict__ prm,
                                                        long long pstride, T* __restrict__ wout, T* __restrict__ amat,
                                                        float* __restrict__ bias) {
  const int ci = blockIdx.x, s = blockIdx.y;
  const float* c1 = coef + (long long)s * 3 * Co;
  const float* c2 = c1 + Co;
  const float* c3 = c2 + Co;
  const float* mean = prm + s * pstride;
  const float* istd = mean + Co;
  const T* wr = wt + (long long)ci * Co;
  T* bo = wout + ((long long)s * Ci + ci) * (Co + Ci);
  T* ao = amat + ((long long)s * Ci + ci) * Co;
  float acc = 0.f;
  for (int c = threadIdx.x; c < Co; c += 256) {
    const float w = to_f(wr[c]);
    const float a1 = c1[c], is = istd[c];
    const float bp = -a1 * c3[c] * is;
    const float k = -a1 * (c2[c] - c3[c] * is * mean[c]);
    bo[c] = from_f<T>(a1 * w);
    ao[c] = from_f<T>(bp * w);
    acc += w * k;
  }
  __shared__ float red[4];
  acc = warp_sum(acc);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) bias[(long long)s * Ci + ci] = (red[0] + red[1]) + (red[2] + red[3]);
}

// The y-side fold (artsbir_bn_fold_bwd_prep_y): the BatchNorm right after the
// conv is folded with its own input y (the conv output, kept for the BN backward)
// instead of the conv input x — dy = c1 g + b' y + k, so
//   dx = g (diag(c1) W) + y (diag(b') W) + k W
// needs no Gram-side GEMM: row ci of segment s is wout[s][ci][co] = c1 W^T[ci][co],
// wout[s][ci][Co + co] = b' W^T[ci][co], bias[s][ci] = sum_co W^T[ci][co] k[co]
template <typename T>
__global__ void __launch_bounds__(256) fold_prep_y_kernel(const T* __restrict__ wt, int Co, int Ci,
                                                          const float* __restrict__ coef, const float* __restrict__ prm,
                                                          long long pstride, T* __restrict__ wout,
                                                          float* __restrict__ bias) {
  const int ci = blockIdx.x, s = blockIdx.y;
  const float* c1 = coef + (long long)s * 3 * Co;
  const float* c2 = c1 + Co;
  const float* c3 = c2 + Co;
  const float* mean = prm + s * pstride;
  const float* istd = mean + Co;
  const T* wr = wt + (long long)ci * Co;
  T* bo = wout + ((long long)s * Ci + ci) * (2 * Co);
  float acc = 0.f;
  for (int c = threadIdx.x; c < Co; c += 256) {
    const float w = to_f(wr[c]);
    const float a1 = c1[c], is = istd[c];
    const float bp = -a1 * c3[c] * is;
    const float k = -a1 * (c2[c] - c3[c] * is * mean[c]);
    bo[c] = from_f<T>(a1 * w);
    bo[Co + c] = from_f<T>(bp * w);
    acc += w * k;
  }
  __shared__ float red[4];
  acc = warp_sum(acc);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) bias[(long long)s * Ci + ci] = (red[0] + red[1]) + (red[2] + red[3]);
}

// dW[co][ci] += sum_s c1_s[co] P_s[co][ci] + b'_s[co] T[co][s Ci + ci] + k_s[co] cs_s[ci]
// with T = W [Gram_0 | Gram_1 | ...] (an f32 GEMM before it) — or, for the y-side
// fold, T_s = y_s^T x_s straight from artsbir_gemm_tn2 (t_co / t_s: the strides of
// T's rows and segments): elementwise, 4 values of one dW row per thread
__global__ void __launch_bounds__(256) fold_wgrad_combine_kernel(const float* __restrict__ P,
                                                                 const float* __restrict__ T, long long t_co,
                                                                 long long t_s, const float* __restrict__ cs,
                                                                 int cs_slots, int Co, int Ci, int nseg,
                                                                 const float* __restrict__ coef,
                                                                 const float* __restrict__ prm, long long pstride,
                                                                 float* __restrict__ dw) {
  const int cq = Ci / 4;
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long long)Co * cq) return;
  const int co = (int)(i / cq), ci = (int)(i - (long long)co * cq) * 4;
  float4 acc = *reinterpret_cast<const float4*>(dw + (long long)co * Ci + ci);
  for (int s = 0; s < nseg; ++s) {
    const float* c = coef + (long long)s * 3 * Co;
    const float* mp = prm + s * pstride;
    const float c1 = c[co], c2 = c[Co + co], c3 = c[2 * Co + co], mean = mp[co], istd = mp[Co + co];
    const float bp = -c1 * c3 * istd, k = -c1 * (c2 - c3 * istd * mean);
    const float4 p = *reinterpret_cast<const float4*>(P + ((long long)s * Co + co) * Ci + ci);
    const float4 t = *reinterpret_cast<const float4*>(T + co * t_co + s * t_s + ci);
    float4 q = make_float4(0.f, 0.f, 0.f, 0.f);  // the column sums' replica rows of segment s
    for (int r = 0; r < cs_slots; ++r) {
      const float4 v = *reinterpret_cast<const float4*>(cs + ((long long)s * cs_slots + r) * Ci + ci);
      q.x += v.x; q.y += v.y; q.z += v.z; q.w += v.w;
    }
    acc.x += c1 * p.x + bp * t.x + k * q.x;
    acc.y += c1 * p.y + bp * t.y + k * q.y;
    acc.z += c1 * p.z + bp * t.z + k * q.z;
    acc.w += c1 * p.w + bp * t.w + k * q.w;
  }
  *reinterpret_cast<float4*>(dw + (long long)co * Ci + ci) = acc;
}

// C[m][n] (ldc) = sum_k A[m][k] B[n][k] for the two small GEMMs of the fold
// (the x-side weights W^T diag(b') W; T = W Gram in the weight gradient), with a
// footprint that lets it share a CU with the other stream's GEMM workgroups: a
// 64 x 64 tile per 4-wave workgroup, 32-k LDS stages double-buffered in 16 KB
// (24 KB with an f32 B) — the 128-160 KB tiles of the pipelined kernels wait for
// a CU the weight gradients have left, which cost these ~20-50 us GEMMs ~150 us
// each in the step.  A bf16 [M][K]; B bf16, or f32 split into two bf16 parts
// (hi + lo, so the f32 Gram matrices keep ~16 significant bits) [N][K]; f32
// accumulation on v_mfma_f32_16x16x32_bf16; output bf16 or f32.  M, N % 64 == 0,
// K % 32 == 0.
__device__ __forceinline__ int fg_slot(int row, int chunk) { return chunk ^ ((row >> 2) & 2); }

template <bool BF32, bool OF32>
__global__ void __launch_bounds__(256) fold_gemm_kernel(const bf16* __restrict__ A, long long lda,
                                                        const void* __restrict__ Bv, long long ldb, void* C,
                                                        long long ldc, int M, int N, int K) {
  constexpr int NB = BF32 ? 2 : 1;  // B parts (hi, lo)
  __shared__ __attribute__((aligned(16))) char smem[2][(1 + NB) * 64 * 64];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int ntn = N / 64;
  const int m0 = (blockIdx.x / ntn) * 64, n0 = (blockIdx.x % ntn) * 64;
  const int wm = (wid >> 1) * 32, wn = (wid & 1) * 32;
  const int lr = tid >> 2, lc = tid & 3;  // loader: row, 16-B chunk of a 64-B row
  f32x4 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  uint4 ra, rb[NB];
  auto load = [&](int k0) {
    ra = *reinterpret_cast<const uint4*>(A + (long long)(m0 + lr) * lda + k0 + lc * 8);
    if constexpr (BF32) {
      const float* bp = reinterpret_cast<const float*>(Bv) + (long long)(n0 + lr) * ldb + k0 + lc * 8;
      const float4 f0 = *reinterpret_cast<const float4*>(bp), f1 = *reinterpret_cast<const float4*>(bp + 4);
      const float f[8] = {f0.x, f0.y, f0.z, f0.w, f1.x, f1.y, f1.z, f1.w};
      bf16 hi[8], lo[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        hi[e] = (bf16)f[e];
        lo[e] = (bf16)(f[e] - (float)hi[e]);
      }
      rb[0] = *reinterpret_cast<const uint4*>(hi);
      rb[NB - 1] = *reinterpret_cast<const uint4*>(lo);
    } else {
      rb[0] = *reinterpret_cast<const uint4*>(reinterpret_cast<const bf16*>(Bv) + (long long)(n0 + lr) * ldb + k0 + lc * 8);
    }
  };
  auto store = [&](int buf) {
    char* s = smem[buf];
    const int o = lr * 64 + (fg_slot(lr, lc) << 4);
    *reinterpret_cast<uint4*>(s + o) = ra;
#pragma unroll
    for (int p = 0; p < NB; ++p) *reinterpret_cast<uint4*>(s + (1 + p) * 4096 + o) = rb[p];
  };
  const int fr = lane & 15, fq = lane >> 4;
  const int nk = K / 32;
  load(0);
  store(0);
  __syncthreads();
  for (int kt = 0; kt < nk; ++kt) {
    const int cur = kt & 1;
    if (kt + 1 < nk) load((kt + 1) * 32);
    const char* s = smem[cur];
    uint4 af[2], bfr[NB][2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int r = wm + 16 * i + fr;
      af[i] = *reinterpret_cast<const uint4*>(s + r * 64 + (fg_slot(r, fq) << 4));
    }
#pragma unroll
    for (int p = 0; p < NB; ++p)
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int r = wn + 16 * j + fr;
        bfr[p][j] = *reinterpret_cast<const uint4*>(s + (1 + p) * 4096 + r * 64 + (fg_slot(r, fq) << 4));
      }
#pragma unroll
    for (int p = 0; p < NB; ++p)
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(*reinterpret_cast<const bf16x8*>(&bfr[p][j]),
                                                              *reinterpret_cast<const bf16x8*>(&af[i]), acc[i][j], 0,
                                                              0, 0);
    if (kt + 1 < nk) store(cur ^ 1);
    __syncthreads();
  }
  // acc[i][j][r]: row m = m0 + wm + 16 i + fr, column n = n0 + wn + 16 j + 4 fq + r
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const long long m = m0 + wm + 16 * i + fr;
      const int n = n0 + wn + 16 * j + 4 * fq;
      if constexpr (OF32) {
        *reinterpret_cast<float4*>(reinterpret_cast<float*>(C) + m * ldc + n) =
            make_float4(acc[i][j][0], acc[i][j][1], acc[i][j][2], acc[i][j][3]);
      } else {
        bf16 o[4] = {(bf16)acc[i][j][0], (bf16)acc[i][j][1], (bf16)acc[i][j][2], (bf16)acc[i][j][3]};
        *reinterpret_cast<uint2*>(reinterpret_cast<bf16*>(C) + m * ldc + n) = *reinterpret_cast<const uint2*>(o);
      }
    }
}

}  // namespace artsbir

using namespace artsbir;

// the fold's small GEMMs on fold_gemm_kernel where the shape allows, else artsbir_gemm_nt
static int fold_gemm(int dtype, bool b_f32, int M, int N, int K, const void* a, long long lda, const void* b,
                     long long ldb, void* c, long long ldc, bool out_f32, hipStream_t st) {
  const bool ok = dtype == ARTSBIR_DT_BF16 && M % 64 == 0 && N % 64 == 0 && K % 32 == 0 && lda % 8 == 0 &&
                  ldb % 8 == 0 && ldc % 4 == 0 && (long long)(M / 64) * (N / 64) < 0x7fffffffLL;
  if (!ok) {
    if (b_f32 && dtype == ARTSBIR_DT_BF16) { set_error("fold_gemm: f32 B needs 64-multiple shapes"); return -1; }
    return artsbir_gemm_nt(dtype, M, N, K, a, lda, b, c, ldc, out_f32 ? 1 : 0, 0, nullptr, nullptr, st);
  }
  const dim3 g((unsigned)((M / 64) * (N / 64)));
  const bf16* A = reinterpret_cast<const bf16*>(a);
  if (b_f32 && out_f32) hipLaunchKernelGGL((fold_gemm_kernel<true, true>), g, dim3(256), 0, st, A, lda, b, ldb, c, ldc, M, N, K);
  else if (b_f32) hipLaunchKernelGGL((fold_gemm_kernel<true, false>), g, dim3(256), 0, st, A, lda, b, ldb, c, ldc, M, N, K);
  else if (out_f32) hipLaunchKernelGGL((fold_gemm_kernel<false, true>), g, dim3(256), 0, st, A, lda, b, ldb, c, ldc, M, N, K);
  else hipLaunchKernelGGL((fold_gemm_kernel<false, false>), g, dim3(256), 0, st, A, lda, b, ldb, c, ldc, M, N, K);
  ARTSBIR_CHECK_LAUNCH("fold_gemm");
  return 0;
}

extern "C" int artsbir_bn_fold_bwd_prep(int dtype, int Co, int Ci, const void* wt, const float* coef,
                                        const float* prm, long long pstride, int nseg, void* wout, float* bias,
                                        void* amat, void* stream) {
  if (Co <= 0 || Ci <= 0 || Co % 8 || Ci % 8 || nseg < 1) {
    set_error("bn_fold_bwd_prep: bad shape Co=%d Ci=%d nseg=%d", Co, Ci, nseg);
    return -1;
  }
  if (!wt || !coef || !prm || !wout || !bias || !amat) { set_error("bn_fold_bwd_prep: null operand"); return -1; }
  hipStream_t st = (hipStream_t)stream;
  const dim3 g((unsigned)Ci, (unsigned)nseg);
  if (dtype == ARTSBIR_DT_BF16)
    hipLaunchKernelGGL(fold_prep_kernel<bf16>, g, dim3(256), 0, st, reinterpret_cast<const bf16*>(wt), Co, Ci, coef, prm,
                       pstride, reinterpret_cast<bf16*>(wout), reinterpret_cast<bf16*>(amat), bias);
  else
    hipLaunchKernelGGL(fold_prep_kernel<float>, g, dim3(256), 0, st, reinterpret_cast<const float*>(wt), Co, Ci, coef,
                       prm, pstride, reinterpret_cast<float*>(wout), reinterpret_cast<float*>(amat), bias);
  ARTSBIR_CHECK_LAUNCH("fold_prep");
  // the x-side weights W^T diag(b') W of every segment in one GEMM: rows s*Ci + ci
  // of A times W^T (as [N = Ci][K = Co]) into columns Co.. of wout's rows
  const size_t es = dtype == ARTSBIR_DT_BF16 ? 2 : 4;
  return fold_gemm(dtype, false, nseg * Ci, Ci, Co, amat, Co, wt, Co, reinterpret_cast<char*>(wout) + Co * es, Co + Ci,
                   false, st);
}

extern "C" int artsbir_bn_fold_wgrad_combine(int dtype, int Co, int Ci, int nseg, const float* P, const float* gram,
                                             const float* colsums, int cs_slots, const void* w, const float* coef,
                                             const float* prm, long long pstride, float* dw, float* workspace,
                                             void* stream) {
  if (Co <= 0 || Ci <= 0 || Co % 8 || Ci % 8 || nseg < 1) { set_error("bn_fold_wgrad_combine: bad shape"); return -1; }
  if (!P || !gram || !colsums || !w || !coef || !prm || !dw || !workspace) {
    set_error("bn_fold_wgrad_combine: null operand");
    return -1;
  }
  hipStream_t st = (hipStream_t)stream;
  // T = W [Gram_0 | ... ] (the Gram matrices are [nseg * Ci][Ci] rows, symmetric):
  // bf16 W against the f32 Gram split into two bf16 parts, f32 out; in the f32
  // mode an f32 GEMM
  float* T = workspace;
  if (dtype == ARTSBIR_DT_BF16 && (Co % 64 || Ci % 64)) {
    // shapes off the 64-tile (small test models): W in f32, one f32 GEMM
    float* wc = workspace;
    T = workspace + (long long)Co * Ci;
    if (artsbir_cast(ARTSBIR_DT_BF16, w, ARTSBIR_DT_F32, wc, (long long)Co * Ci, stream)) return -1;
    if (artsbir_gemm_nt(ARTSBIR_DT_F32, Co, nseg * Ci, Ci, wc, Ci, gram, T, (long long)nseg * Ci, 1, 0, nullptr,
                        nullptr, stream))
      return -1;
  } else if (fold_gemm(dtype, true, Co, nseg * Ci, Ci, w, Ci, gram, Ci, T, (long long)nseg * Ci, true, st)) {
    return -1;
  }
  const long long n = (long long)Co * (Ci / 4);
  hipLaunchKernelGGL(fold_wgrad_combine_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, P, T,
                     (long long)nseg * Ci, (long long)Ci, colsums, cs_slots < 1 ? 1 : cs_slots, Co, Ci, nseg, coef, prm,
                     pstride, dw);
  ARTSBIR_CHECK_LAUNCH("fold_wgrad_combine");
  return 0;
}

extern "C" int artsbir_bn_fold_bwd_prep_y(int dtype, int Co, int Ci, const void* wt, const float* coef,
                                          const float* prm, long long pstride, int nseg, void* wout, float* bias,
                                          void* stream) {
  if (Co <= 0 || Ci <= 0 || Co % 8 || Ci % 8 || nseg < 1) {
    set_error("bn_fold_bwd_prep_y: bad shape Co=%d Ci=%d nseg=%d", Co, Ci, nseg);
    return -1;
  }
  if (!wt || !coef || !prm || !wout || !bias) { set_error("bn_fold_bwd_prep_y: null operand"); return -1; }
  hipStream_t st = (hipStream_t)stream;
  const dim3 g((unsigned)Ci, (unsigned)nseg);
  if (dtype == ARTSBIR_DT_BF16)
    hipLaunchKernelGGL(fold_prep_y_kernel<bf16>, g, dim3(256), 0, st, reinterpret_cast<const bf16*>(wt), Co, Ci, coef,
                       prm, pstride, reinterpret_cast<bf16*>(wout), bias);
  else
    hipLaunchKernelGGL(fold_prep_y_kernel<float>, g, dim3(256), 0, st, reinterpret_cast<const float*>(wt), Co, Ci,
                       coef, prm, pstride, reinterpret_cast<float*>(wout), bias);
  ARTSBIR_CHECK_LAUNCH("fold_prep_y");
  return 0;
}

extern "C" int artsbir_bn_fold_wgrad_combine_y(int Co, int Ci, int nseg, const float* P, const float* Q,
                                               const float* colsums, int cs_slots, const float* coef,
                                               const float* prm, long long pstride, float* dw, void* stream) {
  if (Co <= 0 || Ci <= 0 || Co % 8 || Ci % 8 || nseg < 1) { set_error("bn_fold_wgrad_combine_y: bad shape"); return -1; }
  if (!P || !Q || !colsums || !coef || !prm || !dw) { set_error("bn_fold_wgrad_combine_y: null operand"); return -1; }
  const long long n = (long long)Co * (Ci / 4);
  hipLaunchKernelGGL(fold_wgrad_combine_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     P, Q, (long long)Ci, (long long)Co * Ci, colsums, cs_slots < 1 ? 1 : cs_slots, Co, Ci, nseg, coef,
                     prm, pstride, dw);
  ARTSBIR_CHECK_LAUNCH("fold_wgrad_combine_y");
  return 0;
}

// ---------------------------------------------------------------------------
// Data gradient of a 1x1 convolution with the BatchNorm backward of its output
// folded in (artsbir.h: artsbir_conv1x1_dgrad_fold).  The reference's chain
// conv -> BatchNorm2d (models.py:219-220 conv3 -> bn3, 227-229 downsample conv ->
// BN) is differentiated by autograd as dy = c1 (g - c2 - xhat c3) followed by
// dx = dy W; since y = x W^T the whole chain is linear in (g, x):
//   dx = g (diag(c1) W) + x (W^T diag(b') W) + e,  b' = -c1 c3 istd,
//   e = (-c1 (c2 - c3 istd mean)) W
// per BN segment, so it runs as ONE GEMM over the concatenated reduction
// [g | x] (K = Co + Ci) with per-segment weights (artsbir_bn_fold_bwd_prep) and
// bias — no dy tensor is written or read.
// ---------------------------------------------------------------------------
template <typename T>
__global__ void __launch_bounds__(256) fold_concat_kernel(const T* __restrict__ g, const T* __restrict__ x, T* out,
                                                          long long M, int Co, int C2) {
  constexpr int EPC = 16 / sizeof(T);
  const int cg = (Co + C2) / EPC;  // 16-B chunks per output row
  const long long n = M * cg;
  for (long long i = blockIdx.x * 256LL + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
    const long long m = i / cg;
    const int c = (int)(i - m * cg) * EPC;
    const uint4 v = c < Co ? *reinterpret_cast<const uint4*>(g + m * Co + c)
                           : *reinterpret_cast<const uint4*>(x + m * C2 + (c - Co));
    *reinterpret_cast<uint4*>(out + m * (Co + C2) + c) = v;
  }
}

// One fold launch: dx [N][H][W][Ci] = [g | x2] w_s^T + bias_s (+ residual) for
// the pixels of BN segment s, g with Co channels, x2 with C2 (the conv input x,
// C2 = Ci: artsbir_conv1x1_dgrad_fold; the BN input y, C2 = Co:
// artsbir_conv1x1_dgrad_fold_y), an optional fused BN-backward reduction of the
// gradient it produces
struct FoldOp {
  const artsbir_conv_desc* d;
  const void* g;
  const void* x2;
  int C2;
  const void* w;
  const float* bias;
  void* dx;
  const void* res;
  int res_mode;
  const artsbir_bn_bwd_desc* bnb;
  int nseg;
  long long pstride;
};

static int fold_check(const FoldOp& f) {
  const artsbir_conv_desc* d = f.d;
  if (check_conv(d)) return -1;
  if (d->R != 1 || d->S != 1 || d->stride != 1 || d->pad != 0) { set_error("conv1x1_dgrad_fold: 1x1 stride-1 convolutions only"); return -1; }
  if (!f.g || !f.x2 || !f.w || !f.bias || !f.dx) { set_error("conv1x1_dgrad_fold: null operand"); return -1; }
  if (d->Cout % 8 || d->C % 8 || f.C2 % 8 || f.C2 <= 0) { set_error("conv1x1_dgrad_fold: channels must be multiples of 8"); return -1; }
  if (f.nseg < 1 || d->N % f.nseg) { set_error("conv1x1_dgrad_fold: %d segments do not divide batch %d", f.nseg, d->N); return -1; }
  if (f.res_mode < 0 || f.res_mode > 2 || (f.res_mode && !f.res)) { set_error("conv1x1_dgrad_fold: bad residual"); return -1; }
  if (f.res_mode == 2 && (d->H % 2 || d->W % 2)) { set_error("conv1x1_dgrad_fold: unpool residual needs even H, W"); return -1; }
  if (f.res_mode == 2 && (d->N / f.nseg) * d->H * d->W % 4) { set_error("conv1x1_dgrad_fold: unpool residual segments"); return -1; }
  if (const artsbir_bn_bwd_desc* b = f.bnb) {
    if (b->dtype != d->dtype || b->pool > 1) { set_error("conv1x1_dgrad_fold: bad fused BN backward"); return -1; }
    if (b->kind == 1) {
      if (b->ntarget != 1 || !b->mask_bn || f.res_mode) {
        set_error("conv1x1_dgrad_fold: a kind-1 fused BN backward takes one target and no residual");
        return -1;
      }
    } else if (b->kind == 0 || b->kind == 3) {
      if (b->ntarget < 1 || b->ntarget > 2 || !b->mask || !f.res_mode) {
        set_error("conv1x1_dgrad_fold: a kind-0/3 fused BN backward takes 1-2 targets, a mask and a residual");
        return -1;
      }
      if (b->kind == 3 && (d->dtype != ARTSBIR_DT_BF16 || d->C % 8)) { set_error("conv1x1_dgrad_fold: bit masks need bf16"); return -1; }
    } else {
      set_error("conv1x1_dgrad_fold: fused BN-backward kind %d", b->kind);
      return -1;
    }
  }
  return 0;
}

// the two-operand / per-segment-weight launch arguments of the fold (f passed
// fold_check): the 1x1 data gradient over g, the reduction extended by x2
static ConvArgs fold_conv_args(const FoldOp& f) {
  const int Co = f.d->Cout, Ci = f.d->C, K = Co + f.C2;
  artsbir_conv_desc t = *f.d;
  t.C = Co; t.Cout = Ci;
  ConvArgs a = conv_args_nhwc(&t, f.g, f.w, f.dx);
  a.x2 = f.x2; a.sW2 = f.C2; a.sH2 = (long long)t.W * f.C2; a.sN2 = (long long)t.H * t.W * f.C2; a.x2_elems = a.M * f.C2;
  a.C1 = Co; a.C = K; a.K = K;
  a.bias = f.bias; a.res = f.res; a.res_mode = f.res_mode;
  a.nseg = f.nseg; a.bnb_desc = f.bnb; a.bnb_pstride = f.pstride;
  a.w_sstride = (long long)Ci * K; a.bias_sstride = Ci;
  return a;
}

// segment s's slice of a fold launch (one BN segment, its weights and bias)
static ConvArgs fold_segment(const FoldOp& f, const ConvArgs& a, int s, artsbir_bn_bwd_desc* bs) {
  const int Co = f.d->Cout, Ci = f.d->C;
  const long long seg_m = a.M / f.nseg;
  const long long es = f.d->dtype == ARTSBIR_DT_BF16 ? 2 : 4;
  ConvArgs p = a;
  if (f.bnb) { *bs = bnb_segment(f.bnb, s, seg_m, Ci, f.pstride); p.bnb_desc = bs; }
  p.nseg = 1; p.M = seg_m;
  p.x = reinterpret_cast<const char*>(f.g) + s * seg_m * Co * es; p.x_elems = seg_m * Co;
  p.x2 = reinterpret_cast<const char*>(f.x2) + s * seg_m * f.C2 * es; p.x2_elems = seg_m * f.C2;
  p.w = reinterpret_cast<const char*>(f.w) + s * a.w_sstride * es;
  p.bias = f.bias + s * Ci;
  p.y = reinterpret_cast<char*>(f.dx) + s * seg_m * Ci * es;
  if (f.res_mode) p.res = reinterpret_cast<const char*>(f.res) + s * (f.res_mode == 2 ? seg_m / 4 : seg_m) * Ci * es;
  return p;
}

// the two operands concatenated per pixel into ws, then one plain GEMM per segment
static int fold_concat_gemms(const FoldOp& f, const ConvArgs& a, void* ws, hipStream_t st) {
  const artsbir_conv_desc* d = f.d;
  const int Co = d->Cout, K = Co + f.C2;
  const long long M = (long long)d->N * d->H * d->W, seg_m = M / f.nseg;
  const bool bf = d->dtype == ARTSBIR_DT_BF16;
  const long long es = bf ? 2 : 4;
  {
    const long long n = M * (K * es / 16);
    const unsigned grid = (unsigned)((n + 255) / 256 < 65536 ? (n + 255) / 256 : 65536);
    if (bf)
      hipLaunchKernelGGL(fold_concat_kernel<bf16>, dim3(grid), dim3(256), 0, st, reinterpret_cast<const bf16*>(f.g),
                         reinterpret_cast<const bf16*>(f.x2), reinterpret_cast<bf16*>(ws), M, Co, f.C2);
    else
      hipLaunchKernelGGL(fold_concat_kernel<float>, dim3(grid), dim3(256), 0, st, reinterpret_cast<const float*>(f.g),
                         reinterpret_cast<const float*>(f.x2), reinterpret_cast<float*>(ws), M, Co, f.C2);
    ARTSBIR_CHECK_LAUNCH("fold_concat");
  }
  for (int s = 0; s < f.nseg; ++s) {
    artsbir_bn_bwd_desc bs;
    ConvArgs p = fold_segment(f, a, s, &bs);
    p.x2 = nullptr; p.C1 = 0; p.w_sstride = 0; p.bias_sstride = 0;
    p.x = reinterpret_cast<const char*>(ws) + s * seg_m * K * es; p.x_elems = seg_m * K;
    p.sW = K; p.sH = (long long)d->W * K; p.sN = (long long)d->H * d->W * K;
    if (conv_launch(d->dtype, p, st)) return -1;
  }
  return 0;
}

static int fold_dgrad(const FoldOp& f, hipStream_t st) {
  if (fold_check(f)) return -1;
  const artsbir_conv_desc* d = f.d;
  const ConvArgs a = fold_conv_args(f);
  // one launch over every segment, else one per segment (the tiles of a
  // launch then never straddle two), on the two-operand pipelined kernels
  if (d->dtype == ARTSBIR_DT_BF16) {
    int rc = conv_launch(ARTSBIR_DT_BF16, a, st);
    if (rc <= 0) return rc;
    // no kernel took the whole batch (a tile would straddle two segments): one
    // launch per segment; segment 0 decides, a refusal there drops to the
    // concatenated form below (every segment has the same shape)
    for (int s = 0; s < f.nseg; ++s) {
      artsbir_bn_bwd_desc bs;
      const ConvArgs p = fold_segment(f, a, s, &bs);
      rc = conv_launch(ARTSBIR_DT_BF16, p, st);
      if (rc < 0) return rc;
      if (rc > 0) {
        if (s > 0) { set_error("conv1x1_dgrad_fold: segment %d has no kernel", s); return -1; }
        break;
      }
    }
    if (rc == 0) return 0;
  }
  // f32 (the parity mode) and shapes the pipelined kernels do not take: the two
  // operands concatenated per pixel, then one plain GEMM per segment.  The
  // concatenated operand is stream-ordered scratch (hipMallocAsync / hipFreeAsync
  // on the caller's stream): no process-wide buffer shared across devices or
  // threads, no device-synchronous hipFree in the middle of a step
  const size_t need = (size_t)(a.M * a.K * (d->dtype == ARTSBIR_DT_BF16 ? 2 : 4));
  void* ws = nullptr;
  if (hipMallocAsync(&ws, need, st) != hipSuccess) {
    set_error("conv1x1_dgrad_fold: workspace of %zu bytes", need);
    return -1;
  }
  const int rc = fold_concat_gemms(f, a, ws, st);
  (void)hipFreeAsync(ws, st);
  return rc;
}

extern "C" int artsbir_conv1x1_dgrad_fold(const artsbir_conv_desc* d, const void* g, const void* x, const void* w,
                                          const float* bias, void* dx, const artsbir_bn_bwd_desc* bnb, int nseg,
                                          long long param_stride, void* stream) {
  if (bnb && bnb->kind != 1) { set_error("conv1x1_dgrad_fold: the fused BN backward must be kind 1 with one target"); return -1; }
  const FoldOp f{d, g, x, d ? d->C : 0, w, bias, dx, nullptr, 0, bnb, nseg, param_stride};
  return fold_dgrad(f, (hipStream_t)stream);
}

extern "C" int artsbir_conv1x1_dgrad_fold_y(const artsbir_conv_desc* d, const void* g, const void* y, const void* w,
                                            const float* bias, void* dx, const void* res, int res_mode,
                                            const artsbir_bn_bwd_desc* bnb, int nseg, long long param_stride,
                                            void* stream) {
  const FoldOp f{d, g, y, d ? d->Cout : 0, w, bias, dx, res, res_mode, bnb, nseg, param_stride};
  return fold_dgrad(f, (hipStream_t)stream);
}

// The fold's data gradient and, from the same pass, the operands of its weight
// gradient (artsbir.h: artsbir_conv1x1_dgrad_fold_wg): per segment s
// P[s] += g_s^T x_s ([Co][Ci]) and gram[s] += x_s^T x_s ([Ci][Ci]), f32.  One
// kernel where pg_fold_wg_launch takes the shape; otherwise the data gradient
// (artsbir_conv1x1_dgrad_fold) and one artsbir_gemm_tn2 per segment.
extern "C" int artsbir_conv1x1_dgrad_fold_wg(const artsbir_conv_desc* d, const void* g, const void* x, const void* w,
                                             const float* bias, void* dx, const artsbir_bn_bwd_desc* bnb, int nseg,
                                             long long param_stride, float* P, float* gram, void* stream) {
  if (bnb && bnb->kind != 1) { set_error("conv1x1_dgrad_fold_wg: the fused BN backward must be kind 1"); return -1; }
  const FoldOp f{d, g, x, d ? d->C : 0, w, bias, dx, nullptr, 0, bnb, nseg, param_stride};
  if (fold_check(f)) return -1;
  if (!P || !gram) { set_error("conv1x1_dgrad_fold_wg: null weight-gradient operand"); return -1; }
  const int Co = d->Cout, Ci = d->C;
  const long long M = (long long)d->N * d->H * d->W, seg_m = M / nseg;
  const long long es = d->dtype == ARTSBIR_DT_BF16 ? 2 : 4;
  static const bool off = getenv("ARTSBIR_FOLD_WG") && atoi(getenv("ARTSBIR_FOLD_WG")) == 0;  // measurement switch
  if (d->dtype == ARTSBIR_DT_BF16 && !off) {
    ConvArgs a = fold_conv_args(f);
    a.wg_p = P; a.wg_gram = gram;
    const int rc = conv_launch(ARTSBIR_DT_BF16, a, (hipStream_t)stream);
    if (rc <= 0) return rc;
  }
  if (artsbir_conv1x1_dgrad_fold(d, g, x, w, bias, dx, bnb, nseg, param_stride, stream)) return -1;
  for (int s = 0; s < nseg; ++s) {
    const char* gs = reinterpret_cast<const char*>(g) + s * seg_m * Co * es;
    const char* xs = reinterpret_cast<const char*>(x) + s * seg_m * Ci * es;
    if (artsbir_gemm_tn2(d->dtype, seg_m, Co, Ci, Ci, gs, Co, xs, Ci, xs, Ci, P + (long long)s * Co * Ci,
                         gram + (long long)s * Ci * Ci, stream))
      return -1;
  }
  return 0;
}
