// In-batch negative mining for the triplet step: for every anchor the hardest or
// semi-hardest of the 2*B gallery-side embeddings of the batch (the B positives
// then the B negatives), the gather of the selected rows and the deterministic
// scatter of their gradient.
//
// d(i, c) is the loss's own key in the difference form, f32 from the f32 rows:
//   metric 0   || A[i] - C[c] + eps ||_2       (triplet_rows_kernel, loss_optim.hip)
//   metric 1   1 - cos with the clamps of cosine_fwd_kernel (heads.hip)
// One wave computes a pair: lane l sums the columns l, l + 64, ... in order and the
// 64 partial sums meet in warp_sum's butterfly, so the value depends on the two
// rows and D alone, not on the candidate's position, the tile or the grid.  The
// routine and the key packing live in mine_dev.h, which the cross-batch memory scan
// (xbm.hip) shares; the init / scan and final phases below are exported to it.
//
// Three launches:
//   mine_init_kernel    d_ap[i] = d(i, i); sel[i] = the empty key
//   mine_scan_kernel    a wave holds TA anchors and walks a strided share of the
//                       candidates: every candidate value it loads serves TA pairs.
//                       Its best (d, c) per anchor, packed as one 64-bit key that
//                       orders as (d, c) lexicographically, meets the other waves'
//                       in sel[i] by an unsigned 64-bit atomic minimum: a minimum
//                       does not depend on the order of arrival, so the result is
//                       the same bytes every run, and ties go to the lowest c
//   mine_final_kernel   key -> sel[i] (the given negative B + i when no candidate
//                       qualified) and d_sel[i] = d(i, sel[i]) by the same routine
#include "mine_dev.h"
#include "../../include/artsbir.h"

namespace artsbir {

// one wave per anchor
template <int METRIC>
__global__ void __launch_bounds__(256) mine_init_kernel(const float* __restrict__ a, const float* __restrict__ p, int B,
                                                        int D, float eps, unsigned long long* __restrict__ key,
                                                        float* __restrict__ d_ap) {
  const int lane = threadIdx.x & 63;
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= B) return;
  const float d = wave_dist1<METRIC>(a + (long long)i * D, p + (long long)i * D, D, eps, lane);
  if (lane == 0) { d_ap[i] = d; key[i] = MINE_EMPTY; }
}

// grid (anchor tiles, candidate shares / 4): wave (blockIdx.y, w) of tile blockIdx.x
// walks the candidates share, share + nshare, ...
template <int METRIC>
__global__ void __launch_bounds__(256) mine_scan_kernel(int mode, const float* __restrict__ a, const float* __restrict__ p,
                                                        const float* __restrict__ n, int B, int D, float eps,
                                                        const long long* __restrict__ cand_ids,
                                                        const float* __restrict__ d_ap,
                                                        unsigned long long* __restrict__ key) {
  const int lane = threadIdx.x & 63;
  const int i0 = blockIdx.x * MINE_TA;
  const int nshare = gridDim.y * 4;
  const int share = blockIdx.y * 4 + (threadIdx.x >> 6);
  const float* rows[MINE_TA];
  float aa[MINE_TA], dap[MINE_TA];
  long long aid[MINE_TA];
  unsigned long long best[MINE_TA];
#pragma unroll
  for (int t = 0; t < MINE_TA; ++t) {
    const int i = min(i0 + t, B - 1);  // a tile past the end repeats the last anchor; nothing is stored for it
    rows[t] = a + (long long)i * D;
    aa[t] = METRIC == 1 ? wave_sqnorm(rows[t], D, lane) : 0.f;
    dap[t] = d_ap[i];
    aid[t] = cand_ids ? cand_ids[i] : 0;
    best[t] = MINE_EMPTY;
  }
  for (int c = share; c < 2 * B; c += nshare) {
    float d[MINE_TA];
    wave_dist<METRIC, MINE_TA>(rows, aa, cand_row(p, n, B, D, c), D, eps, lane, d);
    const long long cid = cand_ids ? cand_ids[c] : 0;
    mine_update<MINE_TA>(mode, c, i0, d, dap, cand_ids != nullptr, cid, aid, best);
  }
  if (lane == 0) {
#pragma unroll
    for (int t = 0; t < MINE_TA; ++t)
      if (i0 + t < B && best[t] != MINE_EMPTY) atomicMin(key + i0 + t, best[t]);
  }
}

// one wave per anchor; a key's c >= 2B is a slot of the cross-batch memory mem (xbm.hip)
template <int METRIC>
__global__ void __launch_bounds__(256) mine_final_kernel(const float* __restrict__ a, const float* __restrict__ p,
                                                         const float* __restrict__ n, const float* __restrict__ mem,
                                                         int B, int D, float eps, long long* __restrict__ sel,
                                                         float* __restrict__ d_sel) {
  const int lane = threadIdx.x & 63;
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= B) return;
  const unsigned long long k = ((const unsigned long long*)sel)[i];
  const int c = k == MINE_EMPTY ? B + i : (int)(unsigned)k;
  const float d = wave_dist1<METRIC>(a + (long long)i * D, pool_row(p, n, mem, B, D, c), D, eps, lane);
  if (lane == 0) { sel[i] = c; d_sel[i] = d; }
}

// out[i] = C[sel[i]]; a selection outside [0, 2B) reads nothing and gives a row of NaN
__global__ void rows_gather2_kernel(const float* __restrict__ p, const float* __restrict__ n,
                                    const long long* __restrict__ sel, int B, int D, float* __restrict__ out) {
  const long long total = (long long)B * D;
  for (long long e = blockIdx.x * (long long)blockDim.x + threadIdx.x; e < total; e += (long long)gridDim.x * blockDim.x) {
    const int i = (int)(e / D);
    const int d = (int)(e - (long long)i * D);
    const long long c = sel[i];
    out[e] = (c < 0 || c >= 2LL * B) ? __uint_as_float(0x7fc00000u) : cand_row(p, n, B, D, (int)c)[d];
  }
}

// dC[c] = sum over the anchors i with sel[i] == c of dout[i], in ascending i: grid
// (2B candidates, D / 256 column blocks), a thread owns one element of dC.  The
// workgroup tests 256 anchors at a time (one ballot per wave) and every thread then
// walks the set bits from the lowest, so the sum has one order and no atomics;
// a row nobody selected is written as zeros.
__global__ void __launch_bounds__(256) rows_scatter2_kernel(const float* __restrict__ dout,
                                                            const long long* __restrict__ sel, int B, int D,
                                                            float* __restrict__ dp, float* __restrict__ dn) {
  __shared__ unsigned long long hit[4];
  const int c = blockIdx.x;
  const int d = blockIdx.y * 256 + threadIdx.x;
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  float acc = 0.f;
  for (int i0 = 0; i0 < B; i0 += 256) {
    const int i = i0 + threadIdx.x;
    const unsigned long long m = __ballot(i < B && sel[i] == (long long)c);
    if (lane == 0) hit[w] = m;
    __syncthreads();
    if (d < D) {
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        unsigned long long mm = hit[v];
        while (mm) {
          const int b = __ffsll((long long)mm) - 1;
          mm &= mm - 1;
          acc += dout[(long long)(i0 + v * 64 + b) * D + d];
        }
      }
    }
    __syncthreads();
  }
  if (d < D) {
    if (c < B) dp[(long long)c * D + d] = acc;
    else dn[(long long)(c - B) * D + d] = acc;
  }
}

bool mine_shape_ok(const char* name, int B, int D) {
  if (B < 1) { set_error("%s: B=%d must be >= 1", name, B); return false; }
  if (D < 1) { set_error("%s: D=%d must be >= 1", name, D); return false; }
  if (B > MINE_MAX_B) { set_error("%s: B=%d above 2^20", name, B); return false; }
  return true;
}

template <int METRIC>
static void mine_batch(int mode, const float* a, const float* p, const float* n, int B, int D, float eps,
                       const long long* cand_ids, long long* sel, float* d_ap, hipStream_t st) {
  unsigned long long* key = (unsigned long long*)sel;
  const unsigned rows4 = (unsigned)((B + 3) / 4);
  const int ntile = (B + MINE_TA - 1) / MINE_TA;
  // about 2048 waves over the device (256 CUs x 8), at most one candidate per wave of a tile
  int ny = (2048 / ntile + 3) / 4;
  const int ny_max = (2 * B + 3) / 4;
  if (ny > ny_max) ny = ny_max;
  if (ny < 1) ny = 1;
  hipLaunchKernelGGL(mine_init_kernel<METRIC>, dim3(rows4), dim3(256), 0, st, a, p, B, D, eps, key, d_ap);
  hipLaunchKernelGGL(mine_scan_kernel<METRIC>, dim3((unsigned)ntile, (unsigned)ny), dim3(256), 0, st, mode, a, p, n, B, D,
                     eps, cand_ids, d_ap, key);
}

void mine_launch_batch(int metric, int mode, const float* a, const float* p, const float* n, int B, int D, float eps,
                       const long long* cand_ids, long long* sel, float* d_ap, hipStream_t st) {
  if (metric == 0) mine_batch<0>(mode, a, p, n, B, D, eps, cand_ids, sel, d_ap, st);
  else mine_batch<1>(mode, a, p, n, B, D, eps, cand_ids, sel, d_ap, st);
}

void mine_launch_final(int metric, const float* a, const float* p, const float* n, const float* mem, int B, int D,
                       float eps, long long* sel, float* d_sel, hipStream_t st) {
  const unsigned rows4 = (unsigned)((B + 3) / 4);
  if (metric == 0)
    hipLaunchKernelGGL(mine_final_kernel<0>, dim3(rows4), dim3(256), 0, st, a, p, n, mem, B, D, eps, sel, d_sel);
  else
    hipLaunchKernelGGL(mine_final_kernel<1>, dim3(rows4), dim3(256), 0, st, a, p, n, mem, B, D, eps, sel, d_sel);
}

}  // namespace artsbir

using namespace artsbir;

extern "C" int artsbir_mine_negatives(int metric, int mode, const float* a, const float* p, const float* n, int B, int D,
                                      float eps, const long long* cand_ids, long long* sel, float* d_ap, float* d_sel,
                                      void* stream) {
  if (!mine_shape_ok("mine_negatives", B, D)) return -1;
  if (metric != 0 && metric != 1) { set_error("mine_negatives: metric=%d outside {0, 1}", metric); return -1; }
  if (mode != 0 && mode != 1) { set_error("mine_negatives: mode=%d outside {0, 1}", mode); return -1; }
  if (!a || !p || !n || !sel || !d_ap || !d_sel) { set_error("mine_negatives: NULL pointer"); return -1; }
  hipStream_t st = (hipStream_t)stream;
  mine_launch_batch(metric, mode, a, p, n, B, D, eps, cand_ids, sel, d_ap, st);
  mine_launch_final(metric, a, p, n, nullptr, B, D, eps, sel, d_sel, st);
  ARTSBIR_CHECK_LAUNCH("mine_negatives");
  return 0;
}

extern "C" int artsbir_rows_gather2(const float* p, const float* n, const long long* sel, int B, int D, float* out,
                                    void* stream) {
  if (!mine_shape_ok("rows_gather2", B, D)) return -1;
  if (!p || !n || !sel || !out) { set_error("rows_gather2: NULL pointer"); return -1; }
  long long g = ((long long)B * D + 255) / 256;
  if (g > 4096) g = 4096;
  hipLaunchKernelGGL(rows_gather2_kernel, dim3((unsigned)g), dim3(256), 0, (hipStream_t)stream, p, n, sel, B, D, out);
  ARTSBIR_CHECK_LAUNCH("rows_gather2");
  return 0;
}

extern "C" int artsbir_rows_scatter2(const float* dout, const long long* sel, int B, int D, float* dp, float* dn,
                                     void* stream) {
  if (!mine_shape_ok("rows_scatter2", B, D)) return -1;
  if (!dout || !sel || !dp || !dn) { set_error("rows_scatter2: NULL pointer"); return -1; }
  if ((D + 255) / 256 > 65535) { set_error("rows_scatter2: D=%d above 65535 * 256", D); return -1; }
  hipLaunchKernelGGL(rows_scatter2_kernel, dim3((unsigned)(2 * B), (unsigned)((D + 255) / 256)), dim3(256), 0,
                     (hipStream_t)stream, dout, sel, B, D, dp, dn);
  ARTSBIR_CHECK_LAUNCH("rows_scatter2");
  return 0;
}
