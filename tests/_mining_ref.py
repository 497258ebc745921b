"""float64 restatement of in-batch negative mining (test infrastructure, numpy only):
the semantics of artsbir_mine_negatives / losses.mine_negatives, the bars of
tests/_tail.py re-exported for the mining tests, and the "decided" rule that says
for which anchors an f32 kernel must reproduce the f64 selection exactly.

Candidates are C = [P; N] (2B rows).  d(i, c) is computed in `dtype` from the f32
inputs (float64: the reference; float32: the yardstick of _tail.check_f32):
  metric 0   || A[i] - C[c] + eps ||_2, eps = float32(1e-6)
  metric 1   1 - a.c / (max(|a|, eps) max(|c|, eps)), eps = float32(1e-8)
c is valid for anchor i when c != i and, with cand_ids, cand_ids[c] != cand_ids[i].
mode 0: the valid c of smallest d; mode 1: the valid c of smallest d among d(i, c) >
d(i, i) (strict).  Ties -> lowest c; a NaN distance is never selected; no candidate ->
B + i."""
import numpy as np

from _tail import U32, check_exact, check_f32, f64  # noqa: F401  (the bars, unchanged)

EPS = {0: np.float32(1e-6), 1: np.float32(1e-8)}
MODES = {"hardest": 0, "semihard": 1}
METRICS = {"euclidean": 0, "cosine": 1}


def distances(a, p, n, metric, eps=None, dtype=np.float64):
    """[B, 2B] distances in `dtype` from the f32 inputs, one anchor at a time"""
    eps = dtype(EPS[metric] if eps is None else np.float32(eps))
    a, c = np.asarray(a, np.float32).astype(dtype), np.concatenate([p, n]).astype(np.float32).astype(dtype)
    out = np.empty((a.shape[0], c.shape[0]), dtype)
    cc = np.maximum(np.sqrt((c * c).sum(1, dtype=dtype)), eps) if metric == 1 else None
    with np.errstate(invalid="ignore"):
        for i in range(a.shape[0]):
            if metric == 0:
                t = a[i][None, :] - c + eps
                out[i] = np.sqrt((t * t).sum(1, dtype=dtype))
            else:
                na = np.maximum(np.sqrt((a[i] * a[i]).sum(dtype=dtype)), eps)
                out[i] = dtype(1) - (c @ a[i]) / (na * cc)
    return out


def valid_mask(B, cand_ids=None):
    v = np.ones((B, 2 * B), bool)
    v[np.arange(B), np.arange(B)] = False
    if cand_ids is not None:
        ids = np.asarray(cand_ids)
        v &= ids[None, :] != ids[:B, None]
    return v


def select(dist, valid, mode):
    """sel [B] from a [B, 2B] distance matrix and validity mask"""
    B = dist.shape[0]
    sel = np.empty(B, np.int64)
    for i in range(B):
        with np.errstate(invalid="ignore"):
            ok = valid[i] & ~np.isnan(dist[i])
            if mode == 1:
                ok &= dist[i] > dist[i, i]
        if not ok.any():
            sel[i] = B + i
            continue
        sel[i] = np.argmin(np.where(ok, dist[i], np.inf))  # argmin: the first (lowest c) of equal minima
        if not ok[sel[i]]:  # every qualifying distance is +inf: the lowest qualifying c
            sel[i] = np.flatnonzero(ok)[0]
    return sel


def mine(a, p, n, mode, metric, eps=None, cand_ids=None, dtype=np.float64):
    """(sel, d_ap, d_sel, dist) in `dtype`"""
    dist = distances(a, p, n, metric, eps, dtype)
    B = dist.shape[0]
    sel = select(dist, valid_mask(B, cand_ids), mode)
    return sel, dist[np.arange(B), np.arange(B)], dist[np.arange(B), sel], dist


def tol(dist64, D, metric):
    """the derived worst case of an f32 sum of D terms in any order, as it moves the key:
    (D + 8) 2^-24 d for the euclidean key, 3 (D + 8) 2^-24 for the cosine key"""
    if metric == 0:
        return (D + 8) * U32 * np.abs(dist64)
    return np.full(dist64.shape, 3 * (D + 8) * U32)


def decided(dist64, valid, mode, D, metric):
    """bool [B]: anchors whose f64 selection an f32 kernel must reproduce: (a) the two
    smallest valid distances differ by more than 2 t_i; in mode 1 also (b) no valid
    candidate lies within 2 t_i of d(i, i), and (c) the two smallest valid distances
    above d(i, i) differ by more than 2 t_i.  t_i: the largest tol of row i."""
    B = dist64.shape[0]
    out = np.zeros(B, bool)
    t_all = tol(dist64, D, metric)
    for i in range(B):
        row = dist64[i]
        if np.isnan(row).any():
            continue
        t2 = 2 * float(t_all[i].max())
        v = np.sort(row[valid[i]])
        ok = v.size < 2 or v[1] - v[0] > t2
        if mode == 1:
            ok = ok and not (np.abs(row[valid[i]] - row[i]) <= t2).any()
            above = v[v > row[i]]
            ok = ok and (above.size < 2 or above[1] - above[0] > t2)
        out[i] = ok
    return out


def scatter(dout, sel, dtype=np.float64):
    """(dP, dN): dC[c] = sum of dout[i] over sel[i] == c, in ascending i, in `dtype`"""
    dout = np.asarray(dout, np.float32).astype(dtype)
    B, D = dout.shape
    dc = np.zeros((2 * B, D), dtype)
    np.add.at(dc, np.asarray(sel), dout)  # unbuffered: repeated indices add in order of i
    return dc[:B], dc[B:]


def brute_force(a, p, n, mode, metric, cand_ids=None):
    """the rule once more as plain loops over python floats (the hand case of the host test)"""
    import math
    a, c = np.asarray(a, np.float32), np.concatenate([p, n]).astype(np.float32)
    B, D = a.shape
    eps = float(EPS[metric])

    def d(i, k):
        x, y = [float(v) for v in a[i]], [float(v) for v in c[k]]
        if metric == 0:
            return math.sqrt(sum((u - w + eps) ** 2 for u, w in zip(x, y)))
        nx = max(math.sqrt(sum(u * u for u in x)), eps)
        ny = max(math.sqrt(sum(w * w for w in y)), eps)
        return 1.0 - sum(u * w for u, w in zip(x, y)) / (nx * ny)

    sel = []
    for i in range(B):
        best, arg = None, B + i
        for k in range(2 * B):
            if k == i or (cand_ids is not None and cand_ids[k] == cand_ids[i]):
                continue
            dk = d(i, k)
            if math.isnan(dk) or (mode == 1 and not dk > d(i, i)):
                continue
            if best is None or dk < best:
                best, arg = dk, k
        sel.append(arg)
    return np.array(sel, np.int64)
