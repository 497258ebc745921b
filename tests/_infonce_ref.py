"""Restatement of the InfoNCE loss of artsbir_info_nce (test infrastructure, numpy only),
in float64 or float32, in the stable form the kernel uses:

  x^ = x / max(|x|, eps),  z(i, c) = scale * a^_i . c^_c  over the pool [p; n; filled slots]
  L_i = log sum over the negatives of exp z(i, c)   (-inf with none)
  u_i = L_i - z(i, i),  row_i = softplus(u_i),  q_i = sigmoid(u_i),  loss = mean row_i
  w(i, c) = q_i exp(z(i, c) - L_i) (negative), -q_i (c = i), 0 otherwise
  da^ = scale / B * W C^,  dc^ = scale / B * W^T A^ (c < 2B),
  dx = (dx^ - x^ (x^ . dx^)) / |x| for |x| >= eps, dx^ / eps below it

c = i is the positive; every other candidate is a negative unless ids are given and its id
(cand_ids[c] in the batch, mem_ids[j] for slot j) equals cand_ids[i].  With dtype=float32
the same formulas run in f32 with BLAS matmuls: the error an f32 implementation makes."""
import numpy as np


def negatives_mask(B, M, count, cand_ids=None, mem_ids=None):
    """bool [B, 2B + M]: True where candidate c is a negative of anchor i"""
    filled = min(max(int(count), 0), M)
    neg = np.ones((B, 2 * B + M), bool)
    neg[np.arange(B), np.arange(B)] = False
    neg[:, 2 * B + filled:] = False
    if cand_ids is not None:
        cand_ids = np.asarray(cand_ids)
        ids = np.concatenate([cand_ids, np.asarray(mem_ids)[:M] if M else np.zeros(0, cand_ids.dtype)])
        neg &= ids[None, :] != cand_ids[:B, None]
    return neg


def _normalise(x, eps):
    nrm = np.sqrt((x * x).sum(1))
    return x / np.maximum(nrm, x.dtype.type(eps))[:, None], nrm


def _normalise_bwd(x, xh, nrm, dxh, eps):
    big = (nrm >= eps)[:, None]
    with np.errstate(divide="ignore", invalid="ignore"):
        proj = (dxh - xh * (xh * dxh).sum(1)[:, None]) / nrm[:, None]
    return np.where(big, proj, dxh / x.dtype.type(eps))


def info_nce(a, p, n, temperature=0.07, cand_ids=None, mem=None, mem_ids=None, count=0, eps=1e-8,
             dtype=np.float64):
    """dict(loss, rows, q, L, da, dp, dn) in `dtype` from the f32 inputs"""
    a, p, n = (np.asarray(t, np.float32).astype(dtype) for t in (a, p, n))
    B, D = a.shape
    M = 0 if mem is None else np.asarray(mem).shape[0]
    filled = min(max(int(count), 0), M)
    pool = np.concatenate([p, n] + ([np.asarray(mem, np.float32)[:filled].astype(dtype)] if filled else []))
    neg = negatives_mask(B, M, count, cand_ids, mem_ids)[:, :2 * B + filled]
    scale = dtype(1.0) / dtype(temperature)
    ah, an = _normalise(a, eps)
    ch, cn = _normalise(pool, eps)
    z = (ah @ ch.T) * scale
    rows_i = np.arange(B)
    zpos = z[rows_i, rows_i]
    zn = np.where(neg, z, -np.inf)
    m = zn.max(1)
    has = neg.any(1)
    msafe = np.where(has, m, 0).astype(dtype)
    with np.errstate(divide="ignore"):
        s = np.where(neg, np.exp(zn - msafe[:, None]), 0).sum(1, dtype=dtype)
        L = np.where(has, msafe + np.log(s), -np.inf).astype(dtype)
    u = L - zpos
    e = np.exp(-np.abs(u))
    rows = (np.maximum(u, 0) + np.log1p(e)).astype(dtype)
    q = np.where(u >= 0, 1 / (1 + e), e / (1 + e)).astype(dtype)
    rows = np.where(has, rows, 0).astype(dtype)
    q = np.where(has, q, 0).astype(dtype)
    Lsafe = np.where(has, L, 0)
    w = np.where(neg, q[:, None] * np.exp(np.where(neg, z, 0) - Lsafe[:, None]), 0).astype(dtype)
    w[rows_i, rows_i] = -q
    sb = scale / dtype(B)
    dah = (w @ ch) * sb
    dch = (w[:, :2 * B].T @ ah) * sb
    da = _normalise_bwd(a, ah, an, dah, eps)
    dc = _normalise_bwd(pool[:2 * B], ch[:2 * B], cn[:2 * B], dch, eps)
    return dict(loss=rows.mean(dtype=dtype), rows=rows, q=q, L=L, da=da.astype(dtype), dp=dc[:B].astype(dtype),
                dn=dc[B:].astype(dtype))
