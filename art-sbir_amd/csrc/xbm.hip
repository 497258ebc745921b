// Cross-batch memory for negative mining (Wang et al., "Cross-Batch Memory for
// Embedding Learning", CVPR 2020): a ring of the last M gallery-side embeddings on the
// device, mined together with the step's own 2*B candidates.
//
//   mem f32 [M][D], mem_ids int64 [M], mem_state int64 [2] = {head, count}
//
// The candidate index space continues the in-batch one: c < 2B is C = [P; N]
// (mining.hip), c = 2B + j is slot j, a candidate only when j < min(count, M); count is
// read by the kernels, never by the host.  The keys are those of mine_dev.h, so a pair
// gives the same bits whether its candidate row lives in the batch or in the ring.
//
// artsbir_mine_pool = the phases of artsbir_mine_negatives with one more scan between
// the in-batch scan and the final kernel, feeding the same 64-bit atomic minimum:
//   pool_scan_kernel<METRIC, NC, FULL>   D <= 64 * NC: a wave keeps its MINE_TA anchors
//       in registers (lane l owns the columns l, l + 64, ... of each: NC values per
//       anchor), walks whole rows of the ring with coalesced 256-B loads, the next
//       row's loads issued ahead of the current row's arithmetic, and every value it
//       loads serves the MINE_TA anchors with no further memory traffic, two anchors
//       a packed f32 instruction (pair_term2).  The eight sums of a row meet in one
//       transposed butterfly (warp_sum8: the bits of warp_sum), after which lane l
//       holds the key of anchor l / 8 and keeps that anchor's best: one square root
//       and one 64-bit compare per row, not eight.  The four waves of a workgroup
//       hold four anchor tiles and walk the same rows, so three of the four reads of
//       a row hit the L1.  FULL: D == 64 * NC, no column test.
//   pool_scan_ptr_kernel<METRIC>         any wider D: the pointer form of the in-batch scan
// artsbir_xbm_enqueue: the ring rule (row r of R -> slot (head + r) mod M, the last M
// rows only, so no two writers meet in a slot) and, as a launch of its own behind the
// copy, the state update.
#include "mine_dev.h"
#include "../../include/artsbir.h"

namespace artsbir {

#define XBM_MAX_R (1 << 24)

// slots that hold a row: min(count, M), whatever the state's words hold
__device__ __forceinline__ int xbm_filled(const long long* __restrict__ state, int M) {
  const long long c = state[1];
  return c < 0 ? 0 : (c > M ? M : (int)c);
}

// waves per SIMD of a register-resident variant, the most its registers allow with no
// scratch: 8 * NC vector registers hold the anchors (64 of 106-111 at NC = 8, 128 of
// 188-194 at NC = 16)
constexpr int pool_waves(int nc) { return nc > 8 ? 2 : 4; }

// grid (anchor tiles / 4, row shares): wave w of workgroup (x, y) holds tile 4 x + w and
// walks the rows y, y + gridDim.y, ... of the filled part of the ring
template <int METRIC, int NC, bool FULL>
__global__ void __launch_bounds__(256, pool_waves(NC))
    pool_scan_kernel(int mode, const float* __restrict__ a, int B, int D, float eps,
                     const long long* __restrict__ cand_ids, const float* __restrict__ mem,
                     const long long* __restrict__ mem_ids, const long long* __restrict__ mem_state, int M,
                     const float* __restrict__ d_ap, unsigned long long* __restrict__ key) {
  const int lane = threadIdx.x & 63;
  const int i0 = (blockIdx.x * 4 + (threadIdx.x >> 6)) * MINE_TA;
  if (i0 >= B) return;  // (no workgroup barrier below)
  const int filled = xbm_filled(mem_state, M);
  const int step = gridDim.y;
  static_assert(MINE_TA == 8, "warp_sum8 leaves the key of anchor l / 8 in lane l");
  const int mine = min(i0 + (lane >> 3), B - 1);  // the anchor whose keys this lane follows
  f32x2 av[MINE_TA / 2][NC];  // anchors 2 u and 2 u + 1 side by side: one packed operation serves both
  float aa = 0.f;
#pragma unroll
  for (int t = 0; t < MINE_TA; ++t) {
    const int i = min(i0 + t, B - 1);  // a tile past the end repeats the last anchor; nothing is stored for it
    const float* row = a + (long long)i * D;
#pragma unroll
    for (int k = 0; k < NC; ++k) av[t / 2][k][t % 2] = (FULL || lane + 64 * k < D) ? row[lane + 64 * k] : 0.f;
    if (METRIC == 1) {
      const float s = wave_sqnorm(row, D, lane);
      aa = (lane >> 3) == t ? s : aa;
    }
  }
  const float dap = d_ap[mine];
  const long long aid = cand_ids ? cand_ids[mine] : 0;
  unsigned long long best = MINE_EMPTY;
  float cur[NC] = {}, nxt[NC] = {};
  int j = blockIdx.y;
  if (j < filled) {
    const float* row = mem + (long long)j * D;
#pragma unroll
    for (int k = 0; k < NC; ++k) cur[k] = (FULL || lane + 64 * k < D) ? row[lane + 64 * k] : 0.f;
  }
  for (; j < filled; j += step) {
    if (j + step < filled) {  // the next row's loads, ahead of this row's arithmetic
      const float* row = mem + (long long)(j + step) * D;
#pragma unroll
      for (int k = 0; k < NC; ++k) nxt[k] = (FULL || lane + 64 * k < D) ? row[lane + 64 * k] : 0.f;
    }
    f32x2 acc2[MINE_TA / 2];
#pragma unroll
    for (int u = 0; u < MINE_TA / 2; ++u) acc2[u] = f32x2{0.f, 0.f};
    float bb = 0.f;
#pragma unroll
    for (int k = 0; k < NC; ++k) {
      if (FULL || 64 * k < D) {  // (the same in every lane)
        const bool in = FULL || lane + 64 * k < D;
        const float cv = cur[k];
        if (METRIC == 1 && in) bb = __fmaf_rn(cv, cv, bb);
#pragma unroll
        for (int u = 0; u < MINE_TA / 2; ++u) {
          const f32x2 s = pair_term2<METRIC>(av[u][k], cv, eps, acc2[u]);
          acc2[u] = in ? s : acc2[u];
        }
      }
    }
    const float nb = METRIC == 1 ? cand_norm(bb, eps) : 0.f;
    float acc[MINE_TA];
#pragma unroll
    for (int t = 0; t < MINE_TA; ++t) acc[t] = acc2[t / 2][t % 2];
    const float d = pair_value<METRIC>(warp_sum8(acc, lane), aa, nb, eps);
    bool ok = d == d;  // never a NaN (and a slot is never the anchor's own positive)
    if (cand_ids) ok = ok && mem_ids[j] != aid;
    if (mode == 1) ok = ok && d > dap;
    const unsigned long long k = mine_key(d, 2 * B + j);
    if (ok && k < best) best = k;
#pragma unroll
    for (int k = 0; k < NC; ++k) cur[k] = nxt[k];
  }
  if ((lane & 7) == 0 && i0 + (lane >> 3) < B && best != MINE_EMPTY) atomicMin(key + i0 + (lane >> 3), best);
}

// the pointer form: grid (anchor tiles, row shares / 4), as mine_scan_kernel
template <int METRIC>
__global__ void __launch_bounds__(256)
    pool_scan_ptr_kernel(int mode, const float* __restrict__ a, int B, int D, float eps,
                         const long long* __restrict__ cand_ids, const float* __restrict__ mem,
                         const long long* __restrict__ mem_ids, const long long* __restrict__ mem_state, int M,
                         const float* __restrict__ d_ap, unsigned long long* __restrict__ key) {
  const int lane = threadIdx.x & 63;
  const int i0 = blockIdx.x * MINE_TA;
  const int nshare = gridDim.y * 4;
  const int share = blockIdx.y * 4 + (threadIdx.x >> 6);
  const int filled = xbm_filled(mem_state, M);
  const float* rows[MINE_TA];
  float aa[MINE_TA], dap[MINE_TA];
  long long aid[MINE_TA];
  unsigned long long best[MINE_TA];
#pragma unroll
  for (int t = 0; t < MINE_TA; ++t) {
    const int i = min(i0 + t, B - 1);
    rows[t] = a + (long long)i * D;
    aa[t] = METRIC == 1 ? wave_sqnorm(rows[t], D, lane) : 0.f;
    dap[t] = d_ap[i];
    aid[t] = cand_ids ? cand_ids[i] : 0;
    best[t] = MINE_EMPTY;
  }
  for (int j = share; j < filled; j += nshare) {
    float d[MINE_TA];
    wave_dist<METRIC, MINE_TA>(rows, aa, mem + (long long)j * D, D, eps, lane, d);
    mine_update<MINE_TA>(mode, 2 * B + j, i0, d, dap, cand_ids != nullptr, mem_ids[j], aid, best);
  }
  if (lane == 0) {
#pragma unroll
    for (int t = 0; t < MINE_TA; ++t)
      if (i0 + t < B && best[t] != MINE_EMPTY) atomicMin(key + i0 + t, best[t]);
  }
}

// out[i] = C[sel[i]] or mem[sel[i] - 2B]; a selection outside [0, 2B + M) reads nothing
// and gives a row of NaN
__global__ void rows_gather3_kernel(const float* __restrict__ p, const float* __restrict__ n,
                                    const float* __restrict__ mem, const long long* __restrict__ sel, int B, int D,
                                    int M, float* __restrict__ out) {
  const long long total = (long long)B * D;
  for (long long e = blockIdx.x * (long long)blockDim.x + threadIdx.x; e < total; e += (long long)gridDim.x * blockDim.x) {
    const int i = (int)(e / D);
    const int d = (int)(e - (long long)i * D);
    const long long c = sel[i];
    out[e] = (c < 0 || c >= 2LL * B + M) ? __uint_as_float(0x7fc00000u) : pool_row(p, n, mem, B, D, (int)c)[d];
  }
}

// head in [0, M), whatever the state's word holds
__device__ __forceinline__ int xbm_head(const long long* __restrict__ state, int M) {
  const long long h = state[0] % M;
  return (int)(h < 0 ? h + M : h);
}

// rows r0 .. R - 1 (the last min(R, M)) into their slots; an element per thread
__global__ void xbm_copy_kernel(const float* __restrict__ rows, const long long* __restrict__ ids, int r0, int R, int D,
                                float* __restrict__ mem, long long* __restrict__ mem_ids,
                                const long long* __restrict__ mem_state, int M) {
  const int head = xbm_head(mem_state, M);
  const long long total = (long long)(R - r0) * D;
  for (long long e = blockIdx.x * (long long)blockDim.x + threadIdx.x; e < total; e += (long long)gridDim.x * blockDim.x) {
    const int q = (int)(e / D);
    const int d = (int)(e - (long long)q * D);
    const int r = r0 + q;
    const int slot = (int)(((long long)head + r) % M);
    mem[(long long)slot * D + d] = rows[(long long)r * D + d];
    if (d == 0) mem_ids[slot] = ids ? ids[r] : -1;
  }
}

__global__ void xbm_state_kernel(long long* __restrict__ mem_state, int R, int M) {
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    const int head = xbm_head(mem_state, M);
    const int filled = xbm_filled(mem_state, M);
    mem_state[0] = ((long long)head + R) % M;
    mem_state[1] = (long long)filled + R > M ? M : filled + R;
  }
}

template <int METRIC>
static void pool_scan_launch(int mode, const float* a, int B, int D, float eps, const long long* cand_ids,
                             const float* mem, const long long* mem_ids, const long long* mem_state, int M,
                             const float* d_ap, unsigned long long* key, hipStream_t st) {
  const int ntile = (B + MINE_TA - 1) / MINE_TA;
  if (D > 1024) {
    int ny = (2048 / ntile + 3) / 4;  // about 2048 waves over the device, at most one row per wave of a tile
    const int ny_max = (M + 3) / 4;
    if (ny > ny_max) ny = ny_max;
    if (ny < 1) ny = 1;
    if (ny > 65535) ny = 65535;
    hipLaunchKernelGGL(pool_scan_ptr_kernel<METRIC>, dim3((unsigned)ntile, (unsigned)ny), dim3(256), 0, st, mode, a, B, D,
                       eps, cand_ids, mem, mem_ids, mem_state, M, d_ap, key);
    return;
  }
  // the workgroups one pass of the device holds: 256 CUs x the waves per SIMD of the variant
  const int nbx = (ntile + 3) / 4;
  int ny = 256 * pool_waves(D <= 512 ? 8 : 16) / nbx;
  if (ny > M) ny = M;  // at most one workgroup per row
  if (ny < 1) ny = 1;
  if (ny > 65535) ny = 65535;
  const dim3 grid((unsigned)nbx, (unsigned)ny);
#define XBM_SCAN(NC, FULL)                                                                                         \
  hipLaunchKernelGGL((pool_scan_kernel<METRIC, NC, FULL>), grid, dim3(256), 0, st, mode, a, B, D, eps, cand_ids, mem, \
                     mem_ids, mem_state, M, d_ap, key)
  if (D == 512) XBM_SCAN(8, true);
  else if (D < 512) XBM_SCAN(8, false);
  else if (D == 1024) XBM_SCAN(16, true);
  else XBM_SCAN(16, false);
#undef XBM_SCAN
}

}  // namespace artsbir

using namespace artsbir;

// M and the index space 2B + M of a memory; B is known to be in range
static bool xbm_size_ok(const char* name, int B, int M, int m_min) {
  if (M < m_min) { set_error("%s: M=%d must be >= %d", name, M, m_min); return false; }
  if (2LL * B + M >= (1LL << 31)) { set_error("%s: 2B+M=%lld does not fit 31 bits", name, 2LL * B + M); return false; }
  if (M > MINE_MAX_M) { set_error("%s: M=%d above 2^24", name, M); return false; }
  return true;
}

extern "C" int artsbir_mine_pool(int metric, int mode, const float* a, const float* p, const float* n, int B, int D,
                                 float eps, const long long* cand_ids, const float* mem, const long long* mem_ids,
                                 const long long* mem_state, int M, long long* sel, float* d_ap, float* d_sel,
                                 void* stream) {
  if (!mine_shape_ok("mine_pool", B, D)) return -1;
  if (!xbm_size_ok("mine_pool", B, M, 0)) return -1;
  if (metric != 0 && metric != 1) { set_error("mine_pool: metric=%d outside {0, 1}", metric); return -1; }
  if (mode != 0 && mode != 1) { set_error("mine_pool: mode=%d outside {0, 1}", mode); return -1; }
  if (!a || !p || !n || !sel || !d_ap || !d_sel) { set_error("mine_pool: NULL pointer"); return -1; }
  const bool ring = mem != nullptr && M > 0;
  if (ring && !mem_state) { set_error("mine_pool: mem given with mem_state NULL"); return -1; }
  if (ring && !mem_ids) { set_error("mine_pool: mem given with mem_ids NULL"); return -1; }
  hipStream_t st = (hipStream_t)stream;
  mine_launch_batch(metric, mode, a, p, n, B, D, eps, cand_ids, sel, d_ap, st);
  if (ring) {
    unsigned long long* key = (unsigned long long*)sel;
    if (metric == 0) pool_scan_launch<0>(mode, a, B, D, eps, cand_ids, mem, mem_ids, mem_state, M, d_ap, key, st);
    else pool_scan_launch<1>(mode, a, B, D, eps, cand_ids, mem, mem_ids, mem_state, M, d_ap, key, st);
  }
  mine_launch_final(metric, a, p, n, ring ? mem : nullptr, B, D, eps, sel, d_sel, st);
  ARTSBIR_CHECK_LAUNCH("mine_pool");
  return 0;
}

extern "C" int artsbir_xbm_enqueue(const float* rows, const long long* ids, int R, int D, float* mem,
                                   long long* mem_ids, long long* mem_state, int M, void* stream) {
  if (R < 1) { set_error("xbm_enqueue: R=%d must be >= 1", R); return -1; }
  if (R > XBM_MAX_R) { set_error("xbm_enqueue: R=%d above 2^24", R); return -1; }
  if (D < 1) { set_error("xbm_enqueue: D=%d must be >= 1", D); return -1; }
  if (!xbm_size_ok("xbm_enqueue", 0, M, 1)) return -1;
  if (!rows || !mem || !mem_ids || !mem_state) { set_error("xbm_enqueue: NULL pointer"); return -1; }
  hipStream_t st = (hipStream_t)stream;
  const int r0 = R > M ? R - M : 0;  // when R > M only the last M rows stay
  long long g = ((long long)(R - r0) * D + 255) / 256;
  if (g > 4096) g = 4096;
  hipLaunchKernelGGL(xbm_copy_kernel, dim3((unsigned)g), dim3(256), 0, st, rows, ids, r0, R, D, mem, mem_ids, mem_state, M);
  hipLaunchKernelGGL(xbm_state_kernel, dim3(1), dim3(64), 0, st, mem_state, R, M);
  ARTSBIR_CHECK_LAUNCH("xbm_enqueue");
  return 0;
}

extern "C" int artsbir_rows_gather3(const float* p, const float* n, const float* mem, const long long* sel, int B, int D,
                                    int M, float* out, void* stream) {
  if (!mine_shape_ok("rows_gather3", B, D)) return -1;
  if (!xbm_size_ok("rows_gather3", B, M, 0)) return -1;
  if (!p || !n || !sel || !out) { set_error("rows_gather3: NULL pointer"); return -1; }
  if (M > 0 && !mem) { set_error("rows_gather3: M=%d with mem NULL", M); return -1; }
  long long g = ((long long)B * D + 255) / 256;
  if (g > 4096) g = 4096;
  hipLaunchKernelGGL(rows_gather3_kernel, dim3((unsigned)g), dim3(256), 0, (hipStream_t)stream, p, n, mem, sel, B, D, M,
                     out);
  ARTSBIR_CHECK_LAUNCH("rows_gather3");
  return 0;
}
