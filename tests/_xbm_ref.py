"""float64 restatement of mining over the batch and a cross-batch memory (test
infrastructure, numpy only): the semantics of artsbir_mine_pool / artsbir_xbm_enqueue /
artsbir_rows_gather3, on top of tests/_mining_ref.py, which is imported and unchanged.

Candidates: c in [0, 2B) is C = [P; N]; c = 2B + j is slot j of mem [M, D], a
candidate only when j < min(count, M).  d(i, c) is _mining_ref.distances over
[N; mem] in the place of N.  c is valid for anchor i when it is a candidate, c != i
and, with ids, the id of c differs from anchor i's (ids of the batch: cand_ids [2B],
of the slots: mem_ids [M]; a slot without id holds -1).  Selection: _mining_ref.select
(ties to the lowest c, NaN never, no candidate -> B + i)."""
import numpy as np

import _mining_ref as mref


def distances(a, p, n, mem, metric, eps=None, dtype=np.float64):
    """[B, 2B + M] distances in `dtype` from the f32 inputs"""
    mem = np.asarray(mem, np.float32).reshape(-1, np.asarray(a).shape[1])
    return mref.distances(a, p, np.concatenate([np.asarray(n, np.float32), mem]), metric, eps, dtype)


def valid_mask(B, M, count, cand_ids=None, mem_ids=None):
    """bool [B, 2B + M]: the batch part as _mining_ref.valid_mask, then the filled slots"""
    v = np.ones((B, 2 * B + M), bool)
    v[:, :2 * B] = mref.valid_mask(B, cand_ids)
    v[:, 2 * B + min(max(int(count), 0), M):] = False
    if cand_ids is not None and M:
        v[:, 2 * B:] &= np.asarray(mem_ids)[None, :] != np.asarray(cand_ids)[:B, None]
    return v


def mine(a, p, n, mem, count, mode, metric, eps=None, cand_ids=None, mem_ids=None, dtype=np.float64):
    """(sel, d_ap, d_sel, dist, valid) in `dtype`"""
    dist = distances(a, p, n, mem, metric, eps, dtype)
    B = dist.shape[0]
    valid = valid_mask(B, dist.shape[1] - 2 * B, count, cand_ids, mem_ids)
    sel = mref.select(dist, valid, mode)
    rows = np.arange(B)
    return sel, dist[rows, rows], dist[rows, sel], dist, valid


def gather(p, n, mem, sel):
    return np.concatenate([p, n, np.asarray(mem, np.float32).reshape(-1, p.shape[1])])[sel]


def scatter(dout, sel, dtype=np.float64):
    """(dP, dN): the scatter of _mining_ref restricted to sel < 2B (a ring row is a
    constant), in ascending i"""
    dout = np.asarray(dout, np.float32).astype(dtype)
    B, D = dout.shape
    dc = np.zeros((2 * B, D), dtype)
    for i in range(B):
        if sel[i] < 2 * B:
            dc[sel[i]] += dout[i]
    return dc[:B], dc[B:]


class Ring:
    """the ring rule as a plain loop: row r of an enqueue goes to slot (head + r) mod M,
    a later row over an earlier one; then head = (head + R) mod M, count = min(count + R, M)"""

    def __init__(self, M, D, mem=None, ids=None):
        self.M = M
        self.mem = np.zeros((M, D), np.float32) if mem is None else np.array(mem, np.float32)
        self.ids = np.full(M, -1, np.int64) if ids is None else np.array(ids, np.int64)
        self.head = self.count = 0

    def enqueue(self, rows, ids=None):
        rows = np.asarray(rows, np.float32)
        for r in range(rows.shape[0]):
            slot = (self.head + r) % self.M
            self.mem[slot] = rows[r]
            self.ids[slot] = -1 if ids is None else ids[r]
        self.head = (self.head + rows.shape[0]) % self.M
        self.count = min(self.count + rows.shape[0], self.M)

    def reset(self):
        self.head = self.count = 0

    def state(self):
        return np.array([self.head, self.count], np.int64)


def brute_force(a, p, n, mem, count, mode, metric, cand_ids=None, mem_ids=None):
    """the rule once more as plain loops over python floats (the hand case of the host test)"""
    import math
    a = np.asarray(a, np.float32)
    B, D = a.shape
    c_all = np.concatenate([p, n, np.asarray(mem, np.float32).reshape(-1, D)]).astype(np.float32)
    M = c_all.shape[0] - 2 * B
    eps = float(mref.EPS[metric])

    def d(i, k):
        x, y = [float(v) for v in a[i]], [float(v) for v in c_all[k]]
        if metric == 0:
            return math.sqrt(sum((u - w + eps) ** 2 for u, w in zip(x, y)))
        nx = max(math.sqrt(sum(u * u for u in x)), eps)
        ny = max(math.sqrt(sum(w * w for w in y)), eps)
        return 1.0 - sum(u * w for u, w in zip(x, y)) / (nx * ny)

    sel = []
    for i in range(B):
        best, arg = None, B + i
        for k in range(2 * B + min(count, M)):
            if k == i:
                continue
            if cand_ids is not None:
                kid = cand_ids[k] if k < 2 * B else mem_ids[k - 2 * B]
                if kid == cand_ids[i]:
                    continue
            dk = d(i, k)
            if math.isnan(dk) or (mode == 1 and not dk > d(i, i)):
                continue
            if best is None or dk < best:
                best, arg = dk, k
        sel.append(arg)
    return np.array(sel, np.int64)
