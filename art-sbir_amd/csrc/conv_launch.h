// Host side of the implicit-GEMM launches (gemm.hip), shared with the folded
// BatchNorm backward (fold.hip): the argument structs of the register-staged
// kernels, one builder per operand form, and the launcher that picks a kernel.
#pragma once
#include "common.h"
#include "../../include/artsbir.h"

namespace artsbir {

// Forward / data-gradient implicit GEMM:  Y[m][n] = sum_k Xcol[m][k] * W[n][k]
// (conv_gemm_kernel, gemm.hip; passed to the kernel by value)
struct ConvArgs {
  const void* x = nullptr;
  long long x_elems = 0;              // extent of x (elements) for the bounds check
  long long sN = 0, sH = 0, sW = 0;   // element strides of x (channel stride 1)
  int H = 0, W = 0, C = 0;
  int R = 0, S = 0, stride = 0, pad = 0;
  int Ho = 0, Wo = 0;
  const float* in_scale = nullptr;
  const float* in_shift = nullptr;
  int in_relu = 0;
  const void* w = nullptr;  // [Cout][K], K contiguous
  int Cout = 0, K = 0;
  long long M = 0;
  void* y = nullptr;
  long long ldy = 0;
  int out_f32 = 0;
  int accumulate = 0;
  const float* bias = nullptr;
  float* stats = nullptr;     // [NSLOT][2][Cout] (x nseg)
  const void* res = nullptr;  // epilogue residual (T): mode 1 same index, mode 2 2x2 average-unpool
  int res_mode = 0;
  int relu = 0;               // ReLU on the stored output (after bias and residual)
  // host-side only (the launcher splits / fuses; kernels ignore them)
  int nseg = 1;                     // BN segments (separate reference forward calls) of equal size
  const void* bnb_desc = nullptr;   // artsbir_bn_bwd_desc of a fused BN-backward reduction (dgrad)
  long long bnb_pstride = 0;        // floats between the BN parameters of consecutive segments
  // the folded BatchNorm backward of artsbir_conv1x1_dgrad_fold (PgArgs: same
  // fields); only the pipelined bf16 kernels take it
  const void* x2 = nullptr;
  long long x2_elems = 0, sN2 = 0, sH2 = 0, sW2 = 0;
  int C1 = 0;
  long long w_sstride = 0, bias_sstride = 0;
  float* wg_p = nullptr;  // the fold's weight-gradient operands in the same pass (pg_fold_wg_launch)
  float* wg_gram = nullptr;
};

// Weight gradient:  dW[co][k] += sum_m dY[m][co] * Xcol[m][k]
// (wgrad_kernel, gemm.hip; passed to the kernel by value)
struct WgradArgs {
  const void* dy = nullptr;
  long long dy_elems = 0;
  long long ldd = 0;  // row stride of dY
  const void* x = nullptr;
  long long x_elems = 0;
  long long sN = 0, sH = 0, sW = 0;
  int H = 0, W = 0, C = 0;
  int R = 0, S = 0, stride = 0, pad = 0;
  int Ho = 0, Wo = 0;
  int dense = 0;      // Xcol[m][k] = x[m*ldx + k] (1x1, stride 1, no pad)
  long long ldx = 0;
  const float* in_scale = nullptr;
  const float* in_shift = nullptr;
  int in_relu = 0;
  int Cout = 0, K = 0;
  long long M = 0;
  long long m_per_split = 0;  // multiple of BK (set by the tile launcher)
  float* dw = nullptr;        // [Cout][K] f32
  // dY in two parts along Cout (PwArgs: same fields; the pipelined kernels only)
  const void* dy2 = nullptr;
  long long dy2_elems = 0, ldd2 = 0;
  int Cout1 = 0;
  float* dw2 = nullptr;
};

// y [N][Ho][Wo][Cout] = conv(x [N][H][W][C], w [Cout][R][S][C]) of d, NHWC
inline ConvArgs conv_args_nhwc(const artsbir_conv_desc* d, const void* x, const void* w, void* y) {
  ConvArgs a;
  a.x = x;
  a.sW = d->C;
  a.sH = (long long)d->W * d->C;
  a.sN = (long long)d->H * d->W * d->C;
  a.x_elems = (long long)d->N * a.sN;
  a.H = d->H; a.W = d->W; a.C = d->C;
  a.R = d->R; a.S = d->S; a.stride = d->stride; a.pad = d->pad;
  a.Ho = (d->H + 2 * d->pad - d->R) / d->stride + 1;
  a.Wo = (d->W + 2 * d->pad - d->S) / d->stride + 1;
  a.w = w; a.Cout = d->Cout; a.K = d->R * d->S * d->C;
  a.M = (long long)d->N * a.Ho * a.Wo;
  a.y = y; a.ldy = d->Cout;
  return a;
}

// c [M][N] (ldc, N if <= 0) = a [M][K] (lda) b [N][K]^T: dense rows as "images"
// of one pixel, so row offsets stay relative to the tile
inline ConvArgs conv_args_dense(long long M, int N, int K, const void* a, long long lda, const void* b, void* c,
                                long long ldc) {
  ConvArgs p;
  p.x = a; p.sN = lda;
  p.x_elems = (M - 1) * lda + K;
  p.H = 1; p.W = 1; p.C = K;
  p.R = 1; p.S = 1; p.stride = 1; p.Ho = 1; p.Wo = 1;
  p.w = b; p.Cout = N; p.K = K; p.M = M;
  p.y = c; p.ldy = ldc > 0 ? ldc : N;
  return p;
}

// dw [Cout][R][S][C] += dy [N][Ho][Wo][Cout]^T Xcol(x [N][H][W][C]) of d
inline WgradArgs wgrad_args_nhwc(const artsbir_conv_desc* d, const void* dy, const void* x, float* dw) {
  WgradArgs a;
  a.Ho = (d->H + 2 * d->pad - d->R) / d->stride + 1;
  a.Wo = (d->W + 2 * d->pad - d->S) / d->stride + 1;
  a.dy = dy; a.ldd = d->Cout;
  a.M = (long long)d->N * a.Ho * a.Wo;
  a.dy_elems = a.M * d->Cout;
  a.x = x;
  a.sW = d->C; a.sH = (long long)d->W * d->C; a.sN = (long long)d->H * d->W * d->C;
  a.x_elems = (long long)d->N * a.sN;
  a.H = d->H; a.W = d->W; a.C = d->C;
  a.R = d->R; a.S = d->S; a.stride = d->stride; a.pad = d->pad;
  a.ldx = d->C;
  a.Cout = d->Cout; a.K = d->R * d->S * d->C;
  a.dw = dw;
  return a;
}

// dw [N][K] += dy [M][N] (ldd)^T x [M][K] (ldx)
inline WgradArgs wgrad_args_dense(long long M, int N, int K, const void* dy, long long ldd, const void* x,
                                  long long ldx, float* dw) {
  WgradArgs a;
  a.dy = dy; a.ldd = ldd; a.dy_elems = (M - 1) * ldd + N;
  a.x = x; a.x_elems = (M - 1) * ldx + K;
  a.H = 1; a.W = 1; a.C = K;
  a.R = 1; a.S = 1; a.stride = 1; a.Ho = 1; a.Wo = 1;
  a.dense = 1; a.ldx = ldx;
  a.Cout = N; a.K = K; a.M = M; a.dw = dw;
  return a;
}

// the segment s slice of a fused BN-backward descriptor over [seg_m][C] pixels
// per segment (its tensors, mask and BN parameters advanced by whole segments)
inline artsbir_bn_bwd_desc bnb_segment(const artsbir_bn_bwd_desc* bd, int s, long long seg_m, int C,
                                       long long pstride) {
  artsbir_bn_bwd_desc d = *bd;
  const long long es = bd->dtype == ARTSBIR_DT_BF16 ? 2 : 4;
  d.nseg = 1;
  if (bd->mask_bn) d.mask_bn = bd->mask_bn + s * pstride;
  if (bd->mask)  // kind 3: one mask byte per 8 channels; kind 0: the block output
    d.mask = reinterpret_cast<const char*>(bd->mask) + (bd->kind == 3 ? s * seg_m * (C / 8) : s * seg_m * C * es);
  for (int t = 0; t < bd->ntarget; ++t) {
    d.y[t] = reinterpret_cast<const char*>(bd->y[t]) + s * seg_m * C * es;
    d.mean[t] = bd->mean[t] + s * pstride;
    d.istd[t] = bd->istd[t] + s * pstride;
    d.slots[t] = bd->slots[t] + (long long)s * ARTSBIR_NSLOT * 2 * C;
  }
  return d;
}

// the shape checks every convolution entry point starts with (-1 with the error set)
int check_conv(const artsbir_conv_desc* d);

// Launches a: 0 launched, -1 error (artsbir_last_error), 1 a two-operand fold no
// pipelined kernel took (the caller falls back)
int conv_launch(int dtype, const ConvArgs& a, hipStream_t st);

}  // namespace artsbir
