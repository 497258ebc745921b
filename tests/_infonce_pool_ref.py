"""Restatement of artsbir_info_nce_pool (test infrastructure, numpy only), in float64 or
float32: tests/_infonce_ref.py's stable form with the batch-side candidates one block
cand [Nc, D] in place of [p; n] and anchor i's positive at c = pos0 + i.

  pool = [cand; filled slots],  z(i, c) = scale * a^_i . pool^_c
  negative: c != pos0 + i and (no ids, or id(c) != cand_ids[pos0 + i]),
            id(c) = cand_ids[c] for c < Nc, mem_ids[c - Nc] for a slot
  L, u, rows, q, w as in _infonce_ref (w(i, pos0 + i) = -q_i), loss = mean rows over the B anchors
  da^ = scale / B * W pool^,  dcand^ = scale / B * W[:, :Nc]^T a^,  then the normalisation's backward

With cand = [p; n] and pos0 = 0 this is _infonce_ref.info_nce.  global_loss_textbook is the
loss a gathered data-parallel step trains, by torch float64 autograd: cross_entropy of all
W B anchors against all W 2B rows and the ring."""
import numpy as np

from _infonce_ref import _normalise, _normalise_bwd


def negatives_mask(B, Nc, pos0, M, count, cand_ids=None, mem_ids=None):
    """bool [B, Nc + M]: True where candidate c is a negative of anchor i"""
    filled = min(max(int(count), 0), M)
    neg = np.ones((B, Nc + M), bool)
    neg[np.arange(B), pos0 + np.arange(B)] = False
    neg[:, Nc + filled:] = False
    if cand_ids is not None:
        cand_ids = np.asarray(cand_ids)
        ids = np.concatenate([cand_ids, np.asarray(mem_ids)[:M] if M else np.zeros(0, cand_ids.dtype)])
        neg &= ids[None, :] != cand_ids[pos0:pos0 + B, None]
    return neg


def info_nce_pool(a, cand, pos0, temperature=0.07, cand_ids=None, mem=None, mem_ids=None, count=0, eps=1e-8,
                  dtype=np.float64):
    """dict(loss, rows, q, L, da, dcand) in `dtype` from the f32 inputs"""
    a, cand = (np.asarray(t, np.float32).astype(dtype) for t in (a, cand))
    (B, D), Nc = a.shape, cand.shape[0]
    assert 0 <= pos0 and pos0 + B <= Nc
    M = 0 if mem is None else np.asarray(mem).shape[0]
    filled = min(max(int(count), 0), M)
    pool = np.concatenate([cand] + ([np.asarray(mem, np.float32)[:filled].astype(dtype)] if filled else []))
    neg = negatives_mask(B, Nc, pos0, M, count, cand_ids, mem_ids)[:, :Nc + filled]
    scale = dtype(1.0) / dtype(temperature)
    ah, an = _normalise(a, eps)
    ch, cn = _normalise(pool, eps)
    z = (ah @ ch.T) * scale
    ri, ci = np.arange(B), pos0 + np.arange(B)
    zpos = z[ri, ci]
    zn = np.where(neg, z, -np.inf)
    has = neg.any(1)
    msafe = np.where(has, zn.max(1), 0).astype(dtype)
    with np.errstate(divide="ignore"):
        s = np.where(neg, np.exp(zn - msafe[:, None]), 0).sum(1, dtype=dtype)
        L = np.where(has, msafe + np.log(s), -np.inf).astype(dtype)
    u = L - zpos
    e = np.exp(-np.abs(u))
    rows = np.where(has, np.maximum(u, 0) + np.log1p(e), 0).astype(dtype)
    q = np.where(has, np.where(u >= 0, 1 / (1 + e), e / (1 + e)), 0).astype(dtype)
    Lsafe = np.where(has, L, 0)
    w = np.where(neg, q[:, None] * np.exp(np.where(neg, z, 0) - Lsafe[:, None]), 0).astype(dtype)
    w[ri, ci] = -q
    sb = scale / dtype(B)
    da = _normalise_bwd(a, ah, an, (w @ ch) * sb, eps)
    dcand = _normalise_bwd(cand, ch[:Nc], cn[:Nc], (w[:, :Nc].T @ ah) * sb, eps)
    return dict(loss=rows.mean(dtype=dtype), rows=rows, q=q, L=L, da=da.astype(dtype), dcand=dcand.astype(dtype))


def global_loss_textbook(a_all, g_all, per_rank, temperature=0.07, ids_all=None, mem=None, mem_ids=None, count=0,
                         eps=1e-8, weights=None):
    """The loss over the global batch by torch float64 autograd.  a_all [W B, D]: every
    rank's anchors, rank-major; g_all [W 2B, D]: every rank's [p; n], rank-major
    (per_rank = B); anchor r B + i's positive is row r 2B + i.  cross_entropy (clamped
    normalisation, masked_fill(-inf)) over all rows and the filled slots, masked as
    negatives_mask does.  weights None: the mean over all W B anchors; weights [W]: the sum
    over the ranks of weights[r] * (mean over rank r's anchors).
    Returns (loss, per-rank mean losses [W], d a_all, d g_all)."""
    import torch
    B = per_rank
    W = a_all.shape[0] // B
    M = 0 if mem is None else mem.shape[0]
    filled = min(max(int(count), 0), M)
    ta = torch.from_numpy(np.asarray(a_all, np.float32).astype(np.float64)).requires_grad_(True)
    tg = torch.from_numpy(np.asarray(g_all, np.float32).astype(np.float64)).requires_grad_(True)
    pool = torch.cat([tg, torch.from_numpy(np.asarray(mem, np.float32)[:filled].astype(np.float64))]) if filled else tg
    norm = lambda x: x / x.norm(dim=1, keepdim=True).clamp_min(eps)  # noqa: E731
    z = norm(ta) @ norm(pool).T / temperature
    target = np.concatenate([r * 2 * B + np.arange(B) for r in range(W)])
    keep = np.concatenate([negatives_mask(B, W * 2 * B, r * 2 * B, M, count, ids_all, mem_ids)[:, :W * 2 * B + filled]
                           for r in range(W)])
    keep[np.arange(W * B), target] = True
    per_anchor = torch.nn.functional.cross_entropy(z.masked_fill(~torch.from_numpy(keep), float("-inf")),
                                                   torch.from_numpy(target), reduction="none")
    per = per_anchor.reshape(W, B).mean(1)
    loss = per.mean() if weights is None else (per * torch.as_tensor(weights, dtype=torch.float64)).sum()
    loss.backward()
    return loss.item(), per.detach().numpy(), ta.grad.numpy(), tg.grad.numpy()
