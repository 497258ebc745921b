// InfoNCE (softmax contrastive) loss of one anchor against every gallery-side row of the
// step and of the cross-batch memory, forward and gradient in one call.
//
// Candidates use the index space of mining.hip / xbm.hip: c < B is p[c], B <= c < 2B is
// n[c - B], c = 2B + j is slot j of the ring for j < min(count, M) (count read on the
// device).  c = i is anchor i's positive; every other candidate is a negative unless ids
// are given and the candidate's id equals cand_ids[i].  The pool form (artsbir_info_nce_pool)
// runs the same kernels over one block cand [Nc][D] of gradient-carrying candidates in place
// of [p; n] (the ring starts at c = Nc) with anchor i's positive at c = pos0 + i: the rows of
// every rank, of which the local anchors' own are a slice.  With x^ = x / max(|x|, eps) and
// z(i, c) = scale * a^_i . c^_c, in the stable form:
//   L_i = log sum_{negatives} exp z(i, c)   (-inf with no negative)
//   u_i = L_i - z(i, i),  row_i = softplus(u_i),  q_i = sigmoid(u_i),  loss = mean row_i
//   w(i, c) = q_i exp(z(i, c) - L_i) (negative), -q_i (positive), 0 otherwise
//   da^_i = scale / B * sum_c w(i, c) c^_c,   dc^_c = scale / B * sum_i w(i, c) a^_i  (c < 2B)
//   dx = (dx^ - x^ (x^ . dx^)) / |x|  for |x| >= eps,  dx^ / eps below it
//
// The B x (2B + M) logits and weights never exist in memory.  All three big products run
// on the exact f32-input MFMA (v_mfma_f32_16x16x4_f32) over the RAW rows: the inverse
// norms (f64) scale the logit tile (z = scale * inva_i * invc_c * dot, in f64) and are folded into
// the weights ahead of the gradient products (W . C^ = (W diag(invc)) . C).
//
// A workgroup of four waves computes a 32-anchor x 64-candidate logit tile, K in chunks
// of 32 through LDS; wave w owns the candidates 16 w .. 16 w + 15 of the tile and two
// 16 x 16 tiles (anchors 0-15 and 16-31), each summed in four partial accumulators: eight
// independent MFMA chains, each added to an f64 sum and restarted every 64 columns.  A result
// register r of lane l is S[anchor 4 (l >> 4) + r][candidate l & 15]: the candidate on
// the lane, the anchors in the registers.  Both operands are read from LDS as float4 at
// k = 16 t + 4 (l >> 4) + j, and MFMA step j takes component j of both: a permuted k
// order, which a sum over k does not mind.
//
// Launches (no host synchronisation, no floating-point atomics: two runs give the
// same bytes):
//   nce_prep_kernel      inverse clamped norms of a, the batch candidates and the filled slots
//   nce_fwd_kernel       grid anchor tiles x candidate shares (nce_block): an online log-sum-exp per
//                        lane over the share's tiles, met across the lanes and the four
//                        waves in a fixed order -> one (max, sum) per (share, anchor);
//                        the tile that holds anchor i's positive stores z(i, i)
//   nce_lse_kernel       the shares' pairs in share order -> L, rows, q
//   nce_mean_kernel      loss = mean rows, one workgroup, fixed order
//   nce_da_kernel<ND>    the same grid: z recomputed, W diag(invc) through
//                        LDS once (the product sums over the lane index of the logit
//                        tile: one transpose), W . C accumulated in registers over the
//                        share (wave w owns 16 ND columns of the 32 anchors) -> a partial
//                        da^ tile per share
//   nce_dc_kernel        grid (tiles of the batch candidates, 256-column blocks): walks all
//                        anchors; the logit accumulators are the A operand of W^T . A as
//                        they stand (the product sums over their register index), so a
//                        dc^ tile has one owner and no partials
//   nce_finish_kernel    a wave per row of da and of dp, dn | dcand: the da^ partials in share order,
//                        scale / B and the backward of the normalisation
// An empty share and an all-masked row are (-inf, 0); the combine never forms inf - inf.
// A row past the filled part of the ring is never read: row indices are clamped to the
// last candidate and the pair is masked.
#include "mine_dev.h"
#include "../../include/artsbir.h"

#include <math.h>

namespace artsbir {

#define NCE_TA 32
#define NCE_TC 64
#define NCE_KC 32
#define NCE_FLUSH 2  // chunks an f32 MFMA chain runs before it is added to the f64 sum
#define NCE_LD (NCE_KC + 4)   // row pitch of the staged operands: 16-byte aligned rows
#define NCE_WLD (NCE_TC + 4)  // row pitch of the transposed weight tile
#define NCE_MAX_D 1024
#define NCE_DC_COLS 256       // columns of a dc^ tile: 16 accumulators of 16

// The candidates of a call.  c < split is row c of c0, split <= c < nb row c - split of c1,
// c = nb + j slot j of the ring; anchor i's positive is c = pos0 + i.
//   artsbir_info_nce        c0 = p, c1 = n, split = B, nb = 2B, pos0 = 0
//   artsbir_info_nce_pool   c0 = cand (c1 unused), split = nb = Nc, pos0 as given
struct NceGeo {
  int B, D, split, nb, pos0;
};

struct NcePool {
  const float* c0;
  const float* c1;
  const float* mem;
  int B, D, split, nb, pos0;
  int ctot;  // nb + filled slots
};

// row c of the blocks (mine_dev.h's cand_row / pool_row with the two bounds of their own)
__device__ __forceinline__ const float* nce_batch_row(const float* __restrict__ c0, const float* __restrict__ c1, int split,
                                                      int D, int c) {
  return c < split ? c0 + (long long)c * D : c1 + (long long)(c - split) * D;
}

__device__ __forceinline__ const float* nce_pool_row(const float* __restrict__ c0, const float* __restrict__ c1,
                                                     const float* __restrict__ mem, int split, int nb, int D, int c) {
  return c < nb ? nce_batch_row(c0, c1, split, D, c) : mem + (long long)(c - nb) * D;
}

// the row of candidate c; past the last candidate the last one again (masked by the caller)
__device__ __forceinline__ const float* nce_row(const NcePool& pl, int c) {
  c = min(c, pl.ctot - 1);
  return nce_pool_row(pl.c0, pl.c1, pl.mem, pl.split, pl.nb, pl.D, c);
}

__device__ __forceinline__ int nce_filled(const float* mem, const long long* __restrict__ state, int M) {
  if (!mem || M <= 0) return 0;
  const long long c = state[1];
  return c < 0 ? 0 : (c > M ? M : (int)c);
}

// the pool as a kernel sees it: the filled part of the ring is read here (state NULL: no ring)
__device__ __forceinline__ NcePool nce_open(const float* __restrict__ r0, const float* __restrict__ r1,
                                            const float* __restrict__ mem, const NceGeo& g,
                                            const long long* __restrict__ state, int M) {
  return NcePool{r0, r1, mem, g.B, g.D, g.split, g.nb, g.pos0, g.nb + (state ? nce_filled(mem, state, M) : 0)};
}

// four values of a row from column k; columns past D read as 0
__device__ __forceinline__ float4 nce_ld4(const float* __restrict__ row, int k, int D, bool vec) {
  if (vec) return k < D ? *reinterpret_cast<const float4*>(row + k) : make_float4(0.f, 0.f, 0.f, 0.f);
  float4 v;
  v.x = k < D ? row[k] : 0.f;
  v.y = k + 1 < D ? row[k + 1] : 0.f;
  v.z = k + 2 < D ? row[k + 2] : 0.f;
  v.w = k + 3 < D ? row[k + 3] : 0.f;
  return v;
}

// the logit: one expression for every sweep, so the second sweep recomputes the bits of the first
// In f64 from the f32 dot product: the inverse norms, the scale and every difference of two
// logits (z - max, z - L, L - z(i, i)) cost no rounding at the logits' magnitude, 1 / tau times
// the cosines'; only exp and log run in f32, on differences.
__device__ __forceinline__ double nce_z(double dot, double ia, double ic, float scale) {
  return dot * ia * ic * (double)scale;
}

// acc[h][r] = sum_k A[i0 + 16 h + 4 (l >> 4) + r][k] * C[c0 + 16 w + (l & 15)][k], raw rows.
// Called by all 256 threads; As, Cs are free to reuse after the next barrier.
__device__ __forceinline__ void nce_logits_tile(const float* __restrict__ a, int i0, const NcePool& pl, int c0, bool vec,
                                                float* As, float* Cs, double (&acc)[2][4]) {
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int sr = tid >> 3, sk = (tid & 7) * 4;  // staging: row sr (and sr + 32 of the candidates), columns sk .. sk + 3
  const int D = pl.D;
  const float* arow = a + (long long)min(i0 + sr, pl.B - 1) * D;
  const float* crow0 = nce_row(pl, c0 + sr);
  const float* crow1 = nce_row(pl, c0 + 32 + sr);
  const int l15 = lane & 15, g = lane >> 4;
  // four partial sums per tile (MFMA step j of every group of 16 columns feeds sum j):
  // eight independent MFMA chains a wave.  An f32 chain runs over NCE_FLUSH chunks only
  // (16 fused multiply-adds at most) and is then added to an f64 sum and restarted: the
  // f32 accumulation the MFMA defines rounds at the size of a 64-column partial sum, not of
  // the whole dot product, whose one f32 rounding alone is 1 / tau * 2^-24 of a logit
  f32x4 pa[2][4];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
#pragma unroll
    for (int j = 0; j < 4; ++j) pa[h][j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int r = 0; r < 4; ++r) acc[h][r] = 0.0;
  }
  int chunk = 0;
  float4 ra = nce_ld4(arow, sk, D, vec), rc0 = nce_ld4(crow0, sk, D, vec), rc1 = nce_ld4(crow1, sk, D, vec);
  for (int k0 = 0; k0 < D; k0 += NCE_KC) {
    __syncthreads();  // the previous chunk (or the caller's use of the buffers) is read
    *reinterpret_cast<float4*>(As + sr * NCE_LD + sk) = ra;
    *reinterpret_cast<float4*>(Cs + sr * NCE_LD + sk) = rc0;
    *reinterpret_cast<float4*>(Cs + (32 + sr) * NCE_LD + sk) = rc1;
    __syncthreads();
    if (k0 + NCE_KC < D) {  // the next chunk's loads ahead of this chunk's MFMAs
      ra = nce_ld4(arow, k0 + NCE_KC + sk, D, vec);
      rc0 = nce_ld4(crow0, k0 + NCE_KC + sk, D, vec);
      rc1 = nce_ld4(crow1, k0 + NCE_KC + sk, D, vec);
    }
#pragma unroll
    for (int t = 0; t < NCE_KC / 16; ++t) {
      const float4 bv = *reinterpret_cast<const float4*>(Cs + (16 * w + l15) * NCE_LD + 16 * t + 4 * g);
      const float4 a0 = *reinterpret_cast<const float4*>(As + l15 * NCE_LD + 16 * t + 4 * g);
      const float4 a1 = *reinterpret_cast<const float4*>(As + (16 + l15) * NCE_LD + 16 * t + 4 * g);
      pa[0][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0.x, bv.x, pa[0][0], 0, 0, 0);
      pa[1][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1.x, bv.x, pa[1][0], 0, 0, 0);
      pa[0][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0.y, bv.y, pa[0][1], 0, 0, 0);
      pa[1][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1.y, bv.y, pa[1][1], 0, 0, 0);
      pa[0][2] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0.z, bv.z, pa[0][2], 0, 0, 0);
      pa[1][2] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1.z, bv.z, pa[1][2], 0, 0, 0);
      pa[0][3] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0.w, bv.w, pa[0][3], 0, 0, 0);
      pa[1][3] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1.w, bv.w, pa[1][3], 0, 0, 0);
    }
    if (++chunk == NCE_FLUSH || k0 + NCE_KC >= D) {  // (the same in every lane)
      chunk = 0;
#pragma unroll
      for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
#pragma unroll
          for (int r = 0; r < 4; ++r) acc[h][r] += (double)pa[h][j][r];
          pa[h][j] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
    }
  }
}

// what a lane knows of its candidate column of a tile
struct NceCol {
  int c;        // pool index
  int rel;      // c - pos0: the anchor whose positive this candidate is, where that is one of the tile's
  bool valid;   // c < ctot
  double inv;   // inverse clamped norm
  long long id;
};

__device__ __forceinline__ NceCol nce_col(const NcePool& pl, int c, const double* __restrict__ invc,
                                          const double* __restrict__ invm, const long long* __restrict__ cand_ids,
                                          const long long* __restrict__ mem_ids) {
  NceCol col;
  col.c = c;
  col.rel = c - pl.pos0;
  col.valid = c < pl.ctot;
  const int cc = min(c, pl.ctot - 1);
  col.inv = cc < pl.nb ? invc[cc] : invm[cc - pl.nb];
  col.id = !cand_ids ? 0 : (cc < pl.nb ? cand_ids[cc] : mem_ids[cc - pl.nb]);
  return col;
}

// (m, s) of two disjoint candidate sets -> of their union.  m = -inf goes with s = 0 (or
// a NaN to pass on): its term is taken as it stands, so no inf - inf is formed.
__device__ __forceinline__ void nce_combine(double& m, float& s, double m2, float s2) {
  const double mm = fmax(m, m2);
  const float t1 = m == -INFINITY ? s : s * expf((float)(m - mm));
  const float t2 = m2 == -INFINITY ? s2 : s2 * expf((float)(m2 - mm));
  m = mm;
  s = t1 + t2;
}

__device__ __forceinline__ void nce_online(double& m, float& s, double z) {
  if (z > m) {
    s = (m == -INFINITY ? s : s * expf((float)(m - z))) + 1.f;
    m = z;
  } else {
    s += expf((float)(z - m));  // (a NaN z lands here and stays in s)
  }
}

// (anchor tile, candidate share) of a block of the 1-D grid of 8 * ceil(nta * ns / 8) blocks.
// Blocks b and b + 8 tend to share an XCD and its L2 (for speed only; nothing depends on
// it): block b takes pair (b % 8) * per + b / 8, so an XCD holds a run of consecutive
// pairs, and the anchor tiles of one share, which walk the same candidate tiles at about
// the same time, read them from HBM once and from that L2 otherwise.  false: no pair.
__device__ __forceinline__ bool nce_block(int nta, int ns, int& tile, int& share) {
  const int total = nta * ns, per = (total + 7) / 8;
  const int v = ((int)blockIdx.x % 8) * per + (int)blockIdx.x / 8;
  if (v >= total) return false;
  share = v / nta;
  tile = v % nta;
  return true;
}

// one wave per row: inverse clamped norms.  rows [0, B) a, [B, B + nb) the batch candidates,
// then the filled slots
__global__ void __launch_bounds__(256)
    nce_prep_kernel(const float* __restrict__ a, const float* __restrict__ r0, const float* __restrict__ r1, const float* __restrict__ mem, NceGeo geo, float eps, const long long* __restrict__ mem_state, int M,
                    double* __restrict__ inva, double* __restrict__ invc, double* __restrict__ invm) {
  const int lane = threadIdx.x & 63;
  const NcePool pl = nce_open(r0, r1, mem, geo, mem_state, M);
  const int B = pl.B, D = pl.D;
  const long long total = (long long)B + pl.ctot;
  for (long long r = blockIdx.x * 4LL + (threadIdx.x >> 6); r < total; r += 4LL * gridDim.x) {
    const float* row;
    double* out;
    if (r < B) { row = a + r * D; out = inva + r; }
    else {
      const int c = (int)(r - B);
      row = nce_row(pl, c);
      out = c < pl.nb ? invc + c : invm + (c - pl.nb);
    }
    double ss = 0.0;
    for (int d = lane; d < D; d += 64) ss = fma((double)row[d], (double)row[d], ss);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) ss += __shfl_xor(ss, o, 64);
    if (lane == 0) *out = 1.0 / fmax(sqrt(ss), (double)eps);
  }
}

__global__ void __launch_bounds__(256)
    nce_fwd_kernel(const float* __restrict__ a, const float* __restrict__ r0, const float* __restrict__ r1, const float* __restrict__ mem, NceGeo geo, float scale, const long long* __restrict__ cand_ids,
                   const long long* __restrict__ mem_ids, const long long* __restrict__ mem_state, int M, int vec,
                   const double* __restrict__ inva, const double* __restrict__ invc, const double* __restrict__ invm,
                   double* __restrict__ zpos, double* __restrict__ part, int nta, int ns) {
  int tile, share;
  if (!nce_block(nta, ns, tile, share)) return;  // (the same in the whole block, ahead of every barrier)
  __shared__ __attribute__((aligned(16))) float As[NCE_TA * NCE_LD];
  __shared__ __attribute__((aligned(16))) float Cs[NCE_TC * NCE_LD];
  __shared__ double red[4][NCE_TA][2];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, l15 = lane & 15, g = lane >> 4;
  const NcePool pl = nce_open(r0, r1, mem, geo, mem_state, M);
  const int B = pl.B;
  const int i0 = tile * NCE_TA;
  double ia[2][4], m[2][4];
  float s[2][4];
  long long aid[2][4];
#pragma unroll
  for (int h = 0; h < 2; ++h)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int i = min(i0 + 16 * h + 4 * g + r, B - 1);
      ia[h][r] = inva[i];
      aid[h][r] = cand_ids ? cand_ids[pl.pos0 + i] : 0;
      m[h][r] = -INFINITY;
      s[h][r] = 0.f;
    }
  const int nct = (pl.ctot + NCE_TC - 1) / NCE_TC;
  for (int ct = share; ct < nct; ct += ns) {
    double acc[2][4];
    nce_logits_tile(a, i0, pl, ct * NCE_TC, vec != 0, As, Cs, acc);
    const NceCol col = nce_col(pl, ct * NCE_TC + 16 * w + l15, invc, invm, cand_ids, mem_ids);
    if (col.valid) {
#pragma unroll
      for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int i = i0 + 16 * h + 4 * g + r;
          if (i < B) {
            const double z = nce_z(acc[h][r], ia[h][r], col.inv, scale);
            if (col.rel == i) zpos[i] = z;
            else if (!cand_ids || col.id != aid[h][r]) nce_online(m[h][r], s[h][r], z);
          }
        }
    }
  }
  // the 16 lanes of a row, then the four waves, in a fixed order
#pragma unroll
  for (int h = 0; h < 2; ++h)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
#pragma unroll
      for (int o = 1; o < 16; o <<= 1) {
        const double m2 = __shfl_xor(m[h][r], o, 64);
        const float s2 = __shfl_xor(s[h][r], o, 64);
        nce_combine(m[h][r], s[h][r], m2, s2);
      }
      if (l15 == 0) {
        red[w][16 * h + 4 * g + r][0] = m[h][r];
        red[w][16 * h + 4 * g + r][1] = s[h][r];
      }
    }
  __syncthreads();
  if (tid < NCE_TA && i0 + tid < B) {
    double mm = red[0][tid][0];
    float ss = (float)red[0][tid][1];
#pragma unroll
    for (int v = 1; v < 4; ++v) nce_combine(mm, ss, red[v][tid][0], (float)red[v][tid][1]);
    double* out = part + ((long long)share * B + i0 + tid) * 2;
    out[0] = mm;
    out[1] = ss;
  }
}

// a thread per anchor: the shares in order -> L, rows, q
__global__ void __launch_bounds__(256)
    nce_lse_kernel(const double* __restrict__ part, int nshare, const double* __restrict__ zpos, int B,
                   double* __restrict__ L, float* __restrict__ rows, float* __restrict__ q) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= B) return;
  double m = -INFINITY;
  float s = 0.f;
  for (int v = 0; v < nshare; ++v)
    nce_combine(m, s, part[((long long)v * B + i) * 2], (float)part[((long long)v * B + i) * 2 + 1]);
  const double l = (m == -INFINITY && s == 0.f) ? (double)-INFINITY : m + log((double)s);
  // in f64, one thread an anchor: an f32 rounding of u is up to 2^-25 |u|, and it is the
  // relative error of a small row, exp(u)
  const double u = l - zpos[i];
  const double e = exp(-fabs(u));
  rows[i] = (float)(fmax(u, 0.0) + log1p(e) + (u != u ? u : 0.0));  // (fmax drops a NaN; put it back)
  q[i] = (float)(u >= 0.0 ? 1.0 / (1.0 + e) : (u != u ? u : e / (1.0 + e)));
  L[i] = l;
}

// loss = mean rows: one workgroup, thread t sums rows t, t + 256, ... and a tree follows
__global__ void __launch_bounds__(256) nce_mean_kernel(const float* __restrict__ rows, int B, float* __restrict__ loss) {
  __shared__ float red[256];
  float s = 0.f;
  for (int i = threadIdx.x; i < B; i += 256) s += rows[i];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) *loss = red[0] / (float)B;
}

// w(i, c) of the stable form.  q = 0 goes with L = -inf (no negative): nothing to weigh.
__device__ __forceinline__ float nce_weight(double z, double l, float q, bool pos, bool neg) {
  if (pos) return -q;
  if (!neg || q == 0.f) return 0.f;
  return q * expf((float)(z - l));
}

// the partial da^ = W diag(invc) . C of a share; wave w owns the columns 16 ND w .. 16 ND (w + 1) - 1
template <int ND>
__global__ void __launch_bounds__(256)
    nce_da_kernel(const float* __restrict__ a, const float* __restrict__ r0, const float* __restrict__ r1, const float* __restrict__ mem, NceGeo geo, float scale, const long long* __restrict__ cand_ids,
                  const long long* __restrict__ mem_ids, const long long* __restrict__ mem_state, int M, int vec,
                  const double* __restrict__ inva, const double* __restrict__ invc, const double* __restrict__ invm,
                  const double* __restrict__ L, const float* __restrict__ q, float* __restrict__ part_da, int nta,
                  int ns) {
  int tile, share;
  if (!nce_block(nta, ns, tile, share)) return;  // (the same in the whole block, ahead of every barrier)
  __shared__ __attribute__((aligned(16))) float As[NCE_TA * NCE_LD];
  __shared__ __attribute__((aligned(16))) float Cs[NCE_TC * NCE_LD];
  __shared__ __attribute__((aligned(16))) float Wt[NCE_TA * NCE_WLD];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, l15 = lane & 15, g = lane >> 4;
  const NcePool pl = nce_open(r0, r1, mem, geo, mem_state, M);
  const int B = pl.B, D = pl.D;
  const int i0 = tile * NCE_TA;
  const int dbase = w * 16 * ND;
  double ia[2][4], li[2][4];
  float qi[2][4];
  long long aid[2][4];
#pragma unroll
  for (int h = 0; h < 2; ++h)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int i = min(i0 + 16 * h + 4 * g + r, B - 1);
      ia[h][r] = inva[i];
      li[h][r] = L[i];
      qi[h][r] = q[i];
      aid[h][r] = cand_ids ? cand_ids[pl.pos0 + i] : 0;
    }
  f32x4 dacc[2][ND];
#pragma unroll
  for (int h = 0; h < 2; ++h)
#pragma unroll
    for (int dt = 0; dt < ND; ++dt) dacc[h][dt] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int nct = (pl.ctot + NCE_TC - 1) / NCE_TC;
  for (int ct = share; ct < nct; ct += ns) {
    const int c0 = ct * NCE_TC;
    double acc[2][4];
    nce_logits_tile(a, i0, pl, c0, vec != 0, As, Cs, acc);
    const NceCol col = nce_col(pl, c0 + 16 * w + l15, invc, invm, cand_ids, mem_ids);
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = i0 + 16 * h + 4 * g + r;
        const bool live = col.valid && i < B;
        const bool pos = live && col.rel == i;
        const bool neg = live && !pos && (!cand_ids || col.id != aid[h][r]);
        const double z = nce_z(acc[h][r], ia[h][r], col.inv, scale);
        const float wv = live ? nce_weight(z, li[h][r], qi[h][r], pos, neg) : 0.f;
        Wt[(16 * h + 4 * g + r) * NCE_WLD + 16 * w + l15] = wv == 0.f ? 0.f : wv * (float)col.inv;
      }
    __syncthreads();  // (the next tile's first barrier keeps Wt until every wave has read it)
#pragma unroll
    for (int t = 0; t < NCE_TC / 16; ++t) {
      const float4 w0 = *reinterpret_cast<const float4*>(Wt + l15 * NCE_WLD + 16 * t + 4 * g);
      const float4 w1 = *reinterpret_cast<const float4*>(Wt + (16 + l15) * NCE_WLD + 16 * t + 4 * g);
      const float wa[4] = {w0.x, w0.y, w0.z, w0.w}, wb[4] = {w1.x, w1.y, w1.z, w1.w};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float* crow = nce_row(pl, c0 + 16 * t + 4 * g + j);
#pragma unroll
        for (int dt = 0; dt < ND; ++dt) {
          const int d = dbase + 16 * dt + l15;
          const float b = d < D ? crow[d] : 0.f;
          dacc[0][dt] = __builtin_amdgcn_mfma_f32_16x16x4f32(wa[j], b, dacc[0][dt], 0, 0, 0);
          dacc[1][dt] = __builtin_amdgcn_mfma_f32_16x16x4f32(wb[j], b, dacc[1][dt], 0, 0, 0);
        }
      }
    }
  }
  float* out = part_da + (long long)share * B * D;
#pragma unroll
  for (int h = 0; h < 2; ++h)
#pragma unroll
    for (int dt = 0; dt < ND; ++dt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = i0 + 16 * h + 4 * g + r, d = dbase + 16 * dt + l15;
        if (i < B && d < D) out[(long long)i * D + d] = dacc[h][dt][r];
      }
}

// dc^ (before scale / B) of the batch candidates c0 .. c0 + 63, columns d0 .. d0 + 255:
// wave w owns the candidates 16 w .. 16 w + 15, walks every anchor tile
__global__ void __launch_bounds__(256)
    nce_dc_kernel(const float* __restrict__ a, const float* __restrict__ r0, const float* __restrict__ r1, NceGeo geo, float scale, const long long* __restrict__ cand_ids, int vec,
                  const double* __restrict__ inva,
                  const double* __restrict__ invc, const double* __restrict__ L, const float* __restrict__ q,
                  float* __restrict__ dchat) {
  __shared__ __attribute__((aligned(16))) float As[NCE_TA * NCE_LD];
  __shared__ __attribute__((aligned(16))) float Cs[NCE_TC * NCE_LD];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, l15 = lane & 15, g = lane >> 4;
  const NcePool pl = nce_open(r0, r1, nullptr, geo, nullptr, 0);  // the batch candidates alone: no slot of the ring
  const int B = pl.B, D = pl.D, nb = pl.nb;
  const int c0 = blockIdx.x * NCE_TC, d0 = blockIdx.y * NCE_DC_COLS;
  NceCol col;
  col.c = c0 + 16 * w + l15;
  col.rel = col.c - pl.pos0;
  col.valid = col.c < nb;
  col.inv = invc[min(col.c, nb - 1)];
  col.id = cand_ids ? cand_ids[min(col.c, nb - 1)] : 0;
  constexpr int NT = NCE_DC_COLS / 16;
  f32x4 dacc[NT];
#pragma unroll
  for (int dt = 0; dt < NT; ++dt) dacc[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int i0 = 0; i0 < B; i0 += NCE_TA) {
    double acc[2][4];
    nce_logits_tile(a, i0, pl, c0, vec != 0, As, Cs, acc);
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = i0 + 16 * h + 4 * g + r, ic = min(i, B - 1);
        const bool live = col.valid && i < B;
        const bool pos = live && col.rel == i;
        const bool neg = live && !pos && (!cand_ids || col.id != cand_ids[pl.pos0 + ic]);
        const double iav = inva[ic];
        const double z = nce_z(acc[h][r], iav, col.inv, scale);
        const float wv = live ? nce_weight(z, L[ic], q[ic], pos, neg) : 0.f;
        // W[i][c] sits where the A operand of W^T . A wants it: row c on the lane, k = the anchor
        const float wk = wv == 0.f ? 0.f : wv * (float)iav;
        const float* arow = a + (long long)ic * D;
#pragma unroll
        for (int dt = 0; dt < NT; ++dt) {
          if (d0 + 16 * dt < D) {  // (the same in every lane)
            const int d = d0 + 16 * dt + l15;
            const float b = d < D ? arow[d] : 0.f;
            dacc[dt] = __builtin_amdgcn_mfma_f32_16x16x4f32(wk, b, dacc[dt], 0, 0, 0);
          }
        }
      }
  }
#pragma unroll
  for (int dt = 0; dt < NT; ++dt)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int c = c0 + 16 * w + 4 * g + r, d = d0 + 16 * dt + l15;
      if (c < nb && d < D) dchat[(long long)c * D + d] = dacc[dt][r];
    }
}

// a wave per row of da and of the batch candidates' gradient (d0 [split][D], then d1): dx^ =
// scale / B * (the partials in share order | the dc^ row), then the backward of
// x^ = x / max(|x|, eps)
__global__ void __launch_bounds__(256)
    nce_finish_kernel(const float* __restrict__ a, const float* __restrict__ r0, const float* __restrict__ r1, NceGeo geo, float scale, float eps,
                      const float* __restrict__ part_da, int nshare, const float* __restrict__ dchat,
                      float* __restrict__ da, float* __restrict__ d0, float* __restrict__ d1) {
  const int lane = threadIdx.x & 63;
  const long long r = blockIdx.x * 4LL + (threadIdx.x >> 6);
  const NcePool pl = nce_open(r0, r1, nullptr, geo, nullptr, 0);
  const int B = pl.B, D = pl.D;
  if (r >= (long long)B + pl.nb) return;
  const float* x;
  float* out;
  if (r < B) { x = a + r * D; out = da + r * D; }
  else {
    const int c = (int)(r - B);
    x = nce_row(pl, c);
    out = c < pl.split ? d0 + (long long)c * D : d1 + (long long)(c - pl.split) * D;
  }
  const float nrm = sqrtf(wave_sqnorm(x, D, lane));
  const float den = fmaxf(nrm, eps);  // divisions, not an inverse: at D = 1 x^ is +-1 and dx 0, exactly
  const float sb = scale / (float)B;
  constexpr int NV = NCE_MAX_D / 64;
  float v[NV], xh[NV];
  float dot = 0.f;
#pragma unroll
  for (int k = 0; k < NV; ++k) {
    const int d = lane + 64 * k;
    v[k] = 0.f;
    xh[k] = 0.f;
    if (d < D) {
      float s = 0.f;
      if (r < B) {
        for (int u = 0; u < nshare; ++u) s += part_da[((long long)u * B + r) * D + d];
      } else {
        s = dchat[(r - B) * D + d];
      }
      v[k] = sb * s;
      xh[k] = x[d] / den;
      dot = __fmaf_rn(xh[k], v[k], dot);
    }
  }
  dot = warp_sum(dot);
  const bool proj = nrm >= eps;
#pragma unroll
  for (int k = 0; k < NV; ++k) {
    const int d = lane + 64 * k;
    if (d < D) out[d] = (proj ? v[k] - xh[k] * dot : v[k]) / den;
  }
}

// the launch geometry, from the shapes alone (the workspace is sized by it): candidate
// shares of the forward sweep and of the da^ sweep
struct NcePlan {
  int nta, ns_fwd, ns_da;
};

static NcePlan nce_plan(int B, int D) {
  NcePlan pn;
  pn.nta = (B + NCE_TA - 1) / NCE_TA;
  int ns = 2048 / pn.nta;  // about eight workgroups a CU
  pn.ns_fwd = ns < 1 ? 1 : (ns > 256 ? 256 : ns);
  // da^ partials: [share][B][D] f32 within 32 MiB, about four workgroups a CU
  long long nb = (32LL << 20) / ((long long)B * D * 4);
  const int want = 1024 / pn.nta;
  if (nb > want) nb = want;
  pn.ns_da = nb < 1 ? 1 : (int)nb;
  return pn;
}

// f64 first (offsets in doubles): inva [B], invc [nb], invm [M], zpos [B], L [B],
// part [ns_fwd][B][2] = (max, sum); then f32 (offsets in floats from the f64 part's end):
// dchat [nb][D], part_da [ns_da][B][D]; bytes: the whole.  nb: the batch candidates (2B | Nc)
struct NceWs {
  long long inva, invc, invm, zpos, L, part, nd, dchat, part_da, bytes;
};

static NceWs nce_ws(int B, int nb, int D, int M, bool with_grad) {
  const NcePlan pn = nce_plan(B, D);
  NceWs o;
  long long at = 0;
  o.inva = at; at += B;
  o.invc = at; at += nb;
  o.invm = at; at += M;
  o.zpos = at; at += B;
  o.L = at; at += B;
  o.part = at; at += 2LL * pn.ns_fwd * B;
  o.nd = at;
  at = 0;
  o.dchat = at; at += with_grad ? (long long)nb * D : 0;
  o.part_da = at; at += with_grad ? (long long)pn.ns_da * B * D : 0;
  o.bytes = 8 * o.nd + 4 * at;
  return o;
}

static bool nce_shape_ok(const char* name, int B, int D, int M) {
  if (!mine_shape_ok(name, B, D)) return false;
  if (D > NCE_MAX_D) { set_error("%s: D=%d above %d", name, D, NCE_MAX_D); return false; }
  if (M < 0) { set_error("%s: M=%d must be >= 0", name, M); return false; }
  if (M > MINE_MAX_M) { set_error("%s: M=%d above 2^24", name, M); return false; }
  return true;
}

// the pool form's own: B <= Nc, and Nc + M far enough below 2^31 that a tile's last
// column index (a multiple of the tile past the last candidate) still is an int
#define NCE_MAX_POOL (2147483647LL - 4 * NCE_TC)
static bool nce_pool_shape_ok(const char* name, int B, int Nc, int D, int M) {
  if (!nce_shape_ok(name, B, D, M)) return false;
  if (Nc < B) { set_error("%s: Nc=%d below B=%d", name, Nc, B); return false; }
  if ((long long)Nc + M > NCE_MAX_POOL) {
    set_error("%s: Nc=%d + M=%d above 2^31 - %d", name, Nc, M, 4 * NCE_TC + 1);
    return false;
  }
  return true;
}

// what both entry points do once their own arguments are checked: the ring's pointers, the
// workspace, then the launches.  pl: all but ctot; d0, d1: the candidates' gradient as
// nce_finish_kernel takes it (all of da, d0, d1 NULL: forward alone)
static int nce_run(const char* name, const float* a, NcePool pl, float scale, float eps, const long long* cand_ids,
                   const long long* mem_ids, const long long* mem_state, int M, float* loss, float* rows, float* q,
                   float* da, float* d0, float* d1, void* ws, long long ws_bytes, void* stream) {
  const int B = pl.B, D = pl.D;
  const bool ring = pl.mem != nullptr && M > 0;
  if (ring && !mem_state) { set_error("%s: mem given with mem_state NULL", name); return -1; }
  if (ring && cand_ids && !mem_ids) { set_error("%s: mem and cand_ids given with mem_ids NULL", name); return -1; }
  const bool grad = da != nullptr;
  const NceWs o = nce_ws(B, pl.nb, D, M, grad);
  if (!ws || ws_bytes < o.bytes) {
    set_error("%s: workspace of %lld bytes, %lld needed", name, ws ? ws_bytes : 0LL, o.bytes);
    return -1;
  }
  if (((uintptr_t)ws & 7) != 0) { set_error("%s: workspace not 8-byte aligned", name); return -1; }
  hipStream_t st = (hipStream_t)stream;
  if (!ring) { pl.mem = nullptr; M = 0; }
  const NceGeo geo{pl.B, pl.D, pl.split, pl.nb, pl.pos0};
  double* dw = (double*)ws;
  double *inva = dw + o.inva, *invc = dw + o.invc, *invm = dw + o.invm, *zpos = dw + o.zpos, *L = dw + o.L;
  double* part = dw + o.part;
  float* f = (float*)(dw + o.nd);
  float *dchat = f + o.dchat, *part_da = f + o.part_da;
  // 16-byte loads of the rows: every row start must be aligned
  const uintptr_t al = (uintptr_t)a | (uintptr_t)pl.c0 | (uintptr_t)pl.c1 | (uintptr_t)pl.mem;
  const int vec = (D % 4 == 0 && (al & 15) == 0) ? 1 : 0;
  const NcePlan pn = nce_plan(B, D);
  const int nct = (int)(((long long)pl.nb + M + NCE_TC - 1) / NCE_TC);  // tiles of the whole pool: the grid is sized from M
  const int ns_fwd = pn.ns_fwd < nct ? pn.ns_fwd : nct;
  const int ns_da = pn.ns_da < nct ? pn.ns_da : nct;

  long long gp = ((long long)B + pl.nb + M + 3) / 4;
  if (gp > 4096) gp = 4096;
  hipLaunchKernelGGL(nce_prep_kernel, dim3((unsigned)gp), dim3(256), 0, st, a, pl.c0, pl.c1, pl.mem, geo, eps, mem_state, M, inva,
                     invc, invm);
  hipLaunchKernelGGL(nce_fwd_kernel, dim3((unsigned)(8 * ((pn.nta * ns_fwd + 7) / 8))), dim3(256), 0, st, a, pl.c0, pl.c1,
                     pl.mem, geo, scale,
                     cand_ids, mem_ids, mem_state, M, vec, inva, invc, invm, zpos, part, pn.nta, ns_fwd);
  hipLaunchKernelGGL(nce_lse_kernel, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, st, part, ns_fwd, zpos, B, L, rows,
                     q);
  hipLaunchKernelGGL(nce_mean_kernel, dim3(1), dim3(256), 0, st, rows, B, loss);
  if (grad) {
    const dim3 gda((unsigned)(8 * ((pn.nta * ns_da + 7) / 8)));
#define NCE_DA(ND)                                                                                                   \
  hipLaunchKernelGGL(nce_da_kernel<ND>, gda, dim3(256), 0, st, a, pl.c0, pl.c1, pl.mem, geo, scale, cand_ids, mem_ids, mem_state, M, vec, inva, \
                     invc, invm, L, q, part_da, pn.nta, ns_da)
    if (D <= 256) NCE_DA(4);
    else if (D <= 512) NCE_DA(8);
    else NCE_DA(16);
#undef NCE_DA
    const dim3 gdc((unsigned)((pl.nb + NCE_TC - 1) / NCE_TC), (unsigned)((D + NCE_DC_COLS - 1) / NCE_DC_COLS));
    hipLaunchKernelGGL(nce_dc_kernel, gdc, dim3(256), 0, st, a, pl.c0, pl.c1, geo, scale, cand_ids, vec, inva, invc, L, q,
                       dchat);
    hipLaunchKernelGGL(nce_finish_kernel, dim3((unsigned)(((long long)B + pl.nb + 3) / 4)), dim3(256), 0, st, a, pl.c0,
                       pl.c1, geo, scale, eps, part_da, ns_da, dchat, da, d0, d1);
  }
  ARTSBIR_CHECK_LAUNCH(name);
  return 0;
}

static bool nce_scale_ok(const char* name, float scale) {
  if (scale > 0.f && std::isfinite(scale)) return true;
  set_error("%s: scale=%g must be finite and > 0", name, (double)scale);
  return false;
}

}  // namespace artsbir

using namespace artsbir;

extern "C" long long artsbir_info_nce_workspace(int B, int D, int M, int with_grad) {
  if (!nce_shape_ok("info_nce_workspace", B, D, M)) return -1;
  return nce_ws(B, 2 * B, D, M, with_grad != 0).bytes;
}

extern "C" int artsbir_info_nce(const float* a, const float* p, const float* n, int B, int D, float scale, float eps,
                                const long long* cand_ids, const float* mem, const long long* mem_ids,
                                const long long* mem_state, int M, float* loss, float* rows, float* q, float* da,
                                float* dp, float* dn, void* ws, long long ws_bytes, void* stream) {
  if (!nce_shape_ok("info_nce", B, D, M)) return -1;
  if (!nce_scale_ok("info_nce", scale)) return -1;
  if (!a || !p || !n || !loss || !rows || !q) { set_error("info_nce: NULL pointer"); return -1; }
  const int ngrad = (da != nullptr) + (dp != nullptr) + (dn != nullptr);
  if (ngrad != 0 && ngrad != 3) { set_error("info_nce: da, dp, dn must be given together or not at all"); return -1; }
  const NcePool pl{p, n, mem, B, D, B, 2 * B, 0, 0};
  return nce_run("info_nce", a, pl, scale, eps, cand_ids, mem_ids, mem_state, M, loss, rows, q, da, dp, dn, ws, ws_bytes,
                 stream);
}

extern "C" long long artsbir_info_nce_pool_workspace(int B, int Nc, int D, int M, int with_grad) {
  if (!nce_pool_shape_ok("info_nce_pool_workspace", B, Nc, D, M)) return -1;
  return nce_ws(B, Nc, D, M, with_grad != 0).bytes;
}

extern "C" int artsbir_info_nce_pool(const float* a, const float* cand, int B, int Nc, int pos0, int D, float scale,
                                     float eps, const long long* cand_ids, const float* mem, const long long* mem_ids,
                                     const long long* mem_state, int M, float* loss, float* rows, float* q, float* da,
                                     float* dcand, void* ws, long long ws_bytes, void* stream) {
  if (!nce_pool_shape_ok("info_nce_pool", B, Nc, D, M)) return -1;
  if (pos0 < 0) { set_error("info_nce_pool: pos0=%d must be >= 0", pos0); return -1; }
  if ((long long)pos0 + B > Nc) { set_error("info_nce_pool: pos0=%d + B=%d above Nc=%d", pos0, B, Nc); return -1; }
  if (!nce_scale_ok("info_nce_pool", scale)) return -1;
  if (!a || !cand || !loss || !rows || !q) { set_error("info_nce_pool: NULL pointer"); return -1; }
  if ((da != nullptr) != (dcand != nullptr)) {
    set_error("info_nce_pool: da and dcand must be given together or not at all");
    return -1;
  }
  const NcePool pl{cand, cand, mem, B, D, Nc, Nc, pos0, 0};
  return nce_run("info_nce_pool", a, pl, scale, eps, cand_ids, mem_ids, mem_state, M, loss, rows, q, da, dcand, dcand, ws,
                 ws_bytes, stream);
}
