// The per-pair key of negative mining, shared by the in-batch scan (mining.hip) and
// the cross-batch memory scan (xbm.hip).
//
// d(i, c) is the loss's own key in the difference form, f32 from the f32 rows:
//   metric 0   || A[i] - C[c] + eps ||_2       (triplet_rows_kernel, loss_optim.hip)
//   metric 1   1 - cos with the clamps of cosine_fwd_kernel (heads.hip)
// One wave computes a pair: lane l sums the columns l, l + 64, ... in order
// (pair_term) and the 64 partial sums meet in warp_sum's butterfly (pair_finish),
// so the value depends on the two rows and D alone, not on where the rows live,
// the candidate's position, the tile or the grid.  Every scan builds its keys from
// these two routines and nothing else.
#pragma once
#include "common.h"

namespace artsbir {

#define MINE_TA 8            // anchors per wave of a scan
#define MINE_MAX_B (1 << 20)
#define MINE_MAX_M (1 << 24)  // slots of the cross-batch memory
#define MINE_EMPTY 0xFFFFFFFFFFFFFFFFull  // no real key: its distance bits would be a NaN's

// f32 -> u32 that orders as the floats do (negative keys occur: 1 - cos can round below 0)
__device__ __forceinline__ unsigned ord_f32(float d) {
  const unsigned u = __float_as_uint(d);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// (d, c) as one 64-bit key that orders lexicographically: the smaller d, then the lower c
__device__ __forceinline__ unsigned long long mine_key(float d, int c) {
  return ((unsigned long long)ord_f32(d) << 32) | (unsigned)c;
}

// one column of a pair into the lane's partial sum
template <int METRIC>
__device__ __forceinline__ float pair_term(float av, float cv, float eps, float acc) {
  if (METRIC == 0) {
    const float v = av - cv + eps;
    return __fmaf_rn(v, v, acc);
  }
  return __fmaf_rn(av, cv, acc);
}

// pair_term for two anchors against one candidate value: the packed f32 instructions
// round each half as the scalar ones do
typedef float f32x2 __attribute__((ext_vector_type(2)));
template <int METRIC>
__device__ __forceinline__ f32x2 pair_term2(f32x2 av, float cv, float eps, f32x2 acc) {
  const f32x2 c2 = {cv, cv}, e2 = {eps, eps};
  if (METRIC == 0) {
    const f32x2 v = av - c2 + e2;
    return __builtin_elementwise_fma(v, v, acc);
  }
  return __builtin_elementwise_fma(av, c2, acc);
}

// the sum over the lanes -> d; aa: wave_sqnorm of the anchor, nb: cand_norm of the
// candidate (metric 1 only)
template <int METRIC>
__device__ __forceinline__ float pair_value(float sum, float aa, float nb, float eps) {
  if (METRIC == 0) return sqrtf(sum);
  return 1.f - sum / (fmaxf(sqrtf(aa), eps) * nb);
}

// the lanes' partial sums -> d.  Every lane gets the result.
template <int METRIC>
__device__ __forceinline__ float pair_finish(float acc, float aa, float nb, float eps) {
  return pair_value<METRIC>(warp_sum(acc), aa, nb, eps);
}

// warp_sum of eight values at once: lane l gets the sum of v[(l >> 3) & 7], the bits
// warp_sum(v[t]) gives.  The butterfly adds lane l and lane l ^ o at every step, and an
// f32 sum does not depend on the order of its two operands, so after a step the two
// lanes of a pair hold the same value: one of them can carry it on for one value while
// the other carries another.  Lane l keeps the values whose index has bit 2 = bit 5 of
// l, then bit 1 = bit 4, then bit 0 = bit 3: 4 + 2 + 1 exchanges instead of 8 * 3, and
// the last three steps act on a single value.
__device__ __forceinline__ float warp_sum8(const float (&v)[8], int lane) {
  float r[4], q[2];
  const bool b5 = lane & 32, b4 = lane & 16, b3 = lane & 8;
#pragma unroll
  for (int k = 0; k < 4; ++k) r[k] = (b5 ? v[k + 4] : v[k]) + __shfl_xor(b5 ? v[k] : v[k + 4], 32, 64);
#pragma unroll
  for (int k = 0; k < 2; ++k) q[k] = (b4 ? r[k + 2] : r[k]) + __shfl_xor(b4 ? r[k] : r[k + 2], 16, 64);
  float u = (b3 ? q[1] : q[0]) + __shfl_xor(b3 ? q[0] : q[1], 8, 64);
#pragma unroll
  for (int o = 4; o > 0; o >>= 1) u += __shfl_xor(u, o, 64);
  return u;
}

// the candidate's clamped norm from its lanes' partial sums of squares (metric 1)
__device__ __forceinline__ float cand_norm(float bb, float eps) { return fmaxf(sqrtf(warp_sum(bb)), eps); }

// sum of squares of one row, one wave (the norm of the cosine key)
__device__ __forceinline__ float wave_sqnorm(const float* __restrict__ r, int D, int lane) {
  float s = 0.f;
  for (int d = lane; d < D; d += 64) s = __fmaf_rn(r[d], r[d], s);
  return warp_sum(s);
}

// d(anchor t, candidate) for TA anchor rows against one candidate row, one wave;
// aa[t]: wave_sqnorm of anchor t (metric 1 only).  Every lane gets every result.
template <int METRIC, int TA>
__device__ __forceinline__ void wave_dist(const float* const (&ar)[TA], const float (&aa)[TA],
                                          const float* __restrict__ cr, int D, float eps, int lane, float (&out)[TA]) {
  float acc[TA];
#pragma unroll
  for (int t = 0; t < TA; ++t) acc[t] = 0.f;
  float bb = 0.f;
  for (int d = lane; d < D; d += 64) {
    const float cv = cr[d];
    if (METRIC == 1) bb = __fmaf_rn(cv, cv, bb);
#pragma unroll
    for (int t = 0; t < TA; ++t) acc[t] = pair_term<METRIC>(ar[t][d], cv, eps, acc[t]);
  }
  const float nb = METRIC == 1 ? cand_norm(bb, eps) : 0.f;
#pragma unroll
  for (int t = 0; t < TA; ++t) out[t] = pair_finish<METRIC>(acc[t], aa[t], nb, eps);
}

// candidate c of C = [P; N]
__device__ __forceinline__ const float* cand_row(const float* __restrict__ p, const float* __restrict__ n, int B, int D,
                                                 int c) {
  return c < B ? p + (long long)c * D : n + (long long)(c - B) * D;
}

// candidate c of the pool: C, then the slots of the memory (c >= 2B)
__device__ __forceinline__ const float* pool_row(const float* __restrict__ p, const float* __restrict__ n,
                                                 const float* __restrict__ mem, int B, int D, int c) {
  return c < 2 * B ? cand_row(p, n, B, D, c) : mem + (long long)(c - 2 * B) * D;
}

template <int METRIC>
__device__ __forceinline__ float wave_dist1(const float* __restrict__ ar, const float* __restrict__ cr, int D, float eps,
                                            int lane) {
  const float* const rows[1] = {ar};
  float aa[1] = {0.f}, out[1];
  if (METRIC == 1) aa[0] = wave_sqnorm(ar, D, lane);
  wave_dist<METRIC, 1>(rows, aa, cr, D, eps, lane, out);
  return out[0];
}

// one candidate's keys into the running best of a wave's TA anchors (every lane alike)
template <int TA>
__device__ __forceinline__ void mine_update(int mode, int c, int i0, const float (&d)[TA], const float (&dap)[TA],
                                            bool use_ids, long long cid, const long long (&aid)[TA],
                                            unsigned long long (&best)[TA]) {
#pragma unroll
  for (int t = 0; t < TA; ++t) {
    bool ok = c != i0 + t && d[t] == d[t];  // never the anchor's own positive, never a NaN
    if (use_ids) ok = ok && cid != aid[t];
    if (mode == 1) ok = ok && d[t] > dap[t];
    const unsigned long long k = mine_key(d[t], c);
    if (ok && k < best[t]) best[t] = k;
  }
}

// ---- host side, mining.hip: the phases artsbir_mine_pool shares with artsbir_mine_negatives
bool mine_shape_ok(const char* name, int B, int D);
// d_ap[i] = d(i, i), the empty key into sel, and the scan over C = [P; N]
void mine_launch_batch(int metric, int mode, const float* a, const float* p, const float* n, int B, int D, float eps,
                       const long long* cand_ids, long long* sel, float* d_ap, hipStream_t st);
// key -> sel[i], d_sel[i] = d(i, sel[i]); mem: the memory's rows for sel >= 2B (NULL: none)
void mine_launch_final(int metric, const float* a, const float* p, const float* n, const float* mem, int B, int D,
                       float eps, long long* sel, float* d_sel, hipStream_t st);

}  // namespace artsbir
