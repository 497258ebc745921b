"""Losses and distances of the training step on libartsbir_hip.

  TripletMarginLoss            nn.TripletMarginLoss(margin=utils.MARGIN) (train.py:169): p=2,
                               eps=1e-6 added to the difference (torch.pairwise_distance),
                               swap=False, mean of clamp_min(margin + d(a,p) - d(a,n), 0)
  TripletMarginWithDistanceLoss  nn.TripletMarginWithDistanceLoss (train.py:175, utils.py:56,69)
                               for the two distance functions of the reference:
                               utils.euclidean_distance and utils.cosine_distance
  CrossEntropyLoss             nn.CrossEntropyLoss() (utils.py:57,70), mean, ignore_index=-100
  cosine_distance              1 - CosineSimilarity(dim=1, eps=1e-8)  (utils.py:31-40)
  mine_negatives / MinedNegatives  in-batch hard / semi-hard negative mining (an addition:
                               the reference trains on the negative the dataset drew)
  CrossBatchMemory             a ring of past gallery-side embeddings on the device that the
                               mining above can search as well (an addition)
  info_nce / InfoNCELoss       the softmax contrastive loss over all 2B gallery-side rows of
                               the step and that ring (an addition); gather=True: over the rows
                               of every rank, their gradients sent home in the backward
All run on the GPU kernels with explicit backward kernels.
"""
from __future__ import annotations

import torch
from torch import nn

import _hip
from _hip import call, ptr


def _s():
    return _hip.stream()


def _cuda(*ts):
    for t in ts:
        if not t.is_cuda:
            raise RuntimeError("libartsbir_hip losses need CUDA tensors")


class _TripletFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, p, n, margin, eps):
        _cuda(a, p, n)
        a, p, n = (t.contiguous().float() for t in (a, p, n))
        B, D = a.shape
        dist = torch.empty(2 * B, dtype=torch.float32, device=a.device)
        loss = torch.empty((), dtype=torch.float32, device=a.device)
        call("artsbir_triplet_fwd", ptr(a), ptr(p), ptr(n), B, D, margin, eps, ptr(dist), ptr(loss), _s())
        ctx.save_for_backward(a, p, n, dist)
        ctx.margin, ctx.eps = margin, eps
        return loss

    @staticmethod
    def backward(ctx, gout):
        a, p, n, dist = ctx.saved_tensors
        B, D = a.shape
        gout = gout.contiguous().float()
        da, dp, dn = (torch.empty_like(a) for _ in range(3))
        call("artsbir_triplet_bwd", ptr(a), ptr(p), ptr(n), B, D, ctx.margin, ctx.eps, ptr(dist), ptr(gout),
             ptr(da), ptr(dp), ptr(dn), _s())
        return da, dp, dn, None, None


class TripletMarginLoss(nn.Module):
    """Drop-in for nn.TripletMarginLoss(margin) with p=2, eps=1e-6, swap=False, mean."""

    def __init__(self, margin: float = 1.0, p: float = 2.0, eps: float = 1e-6, swap: bool = False,
                 reduction: str = "mean"):
        super().__init__()
        if p != 2.0 or swap or reduction != "mean":
            raise NotImplementedError("only p=2, swap=False, reduction='mean' (the reference's configuration)")
        self.margin, self.p, self.eps, self.swap, self.reduction = margin, p, eps, swap, reduction

    def forward(self, anchor, positive, negative):
        return _TripletFn.apply(anchor, positive, negative, float(self.margin), float(self.eps))


# ------------------------------------------------------------ distances
class _PairwiseL2Fn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x1, x2, eps):
        _cuda(x1, x2)
        a = x1.contiguous().float().reshape(-1, x1.shape[-1])
        b = x2.contiguous().float().reshape(-1, x2.shape[-1])
        n = max(a.shape[0], b.shape[0])
        out = torch.empty(n, dtype=torch.float32, device=a.device)
        call("artsbir_pairwise_l2", ptr(a), a.shape[0], ptr(b), b.shape[0], a.shape[1], eps, ptr(out), _s())
        ctx.save_for_backward(a, b, out)
        ctx.eps, ctx.shapes = eps, (x1.shape, x2.shape)
        return out

    @staticmethod
    def backward(ctx, g):
        a, b, out = ctx.saved_tensors
        g = g.contiguous().float()
        d1 = torch.zeros_like(a) if ctx.needs_input_grad[0] else None
        d2 = torch.zeros_like(b) if ctx.needs_input_grad[1] else None
        call("artsbir_pairwise_l2_bwd", ptr(a), a.shape[0], ptr(b), b.shape[0], a.shape[1], ctx.eps, ptr(out), ptr(g),
             ptr(d1), ptr(d2), _s())
        return (d1.view(ctx.shapes[0]) if d1 is not None else None,
                d2.view(ctx.shapes[1]) if d2 is not None else None, None)


def pairwise_l2_autograd(x1, x2, eps=1e-6):
    return _PairwiseL2Fn.apply(x1, x2, float(eps))


class _CosineFn(torch.autograd.Function):
    """cos = (x1/max|x1|,eps) . (x2/max|x2|,eps); returns 1 - cos (the reference's CosineLoss)."""

    @staticmethod
    def forward(ctx, x1, x2, eps):
        _cuda(x1, x2)
        a = x1.contiguous().float()
        b = x2.contiguous().float()
        n = max(a.shape[0], b.shape[0])
        cosv = torch.empty(n, dtype=torch.float32, device=a.device)
        norms = torch.empty(2 * n, dtype=torch.float32, device=a.device)
        call("artsbir_cosine_fwd", ptr(a), a.shape[0], ptr(b), b.shape[0], a.shape[1], eps, ptr(cosv), ptr(norms),
             _s())
        ctx.save_for_backward(a, b, cosv, norms)
        return 1.0 - cosv

    @staticmethod
    def backward(ctx, g):
        a, b, cosv, norms = ctx.saved_tensors
        gcos = (-g).contiguous().float()
        d1 = torch.zeros_like(a) if ctx.needs_input_grad[0] else None
        d2 = torch.zeros_like(b) if ctx.needs_input_grad[1] else None
        call("artsbir_cosine_bwd", ptr(a), a.shape[0], ptr(b), b.shape[0], a.shape[1], ptr(cosv), ptr(norms),
             ptr(gcos), ptr(d1), ptr(d2), _s())
        return d1, d2, None


def cosine_distance(x1, x2, eps=1e-8):
    return _CosineFn.apply(x1, x2, float(eps))


class _HingeFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, dp, dn, margin):
        dp, dn = dp.contiguous().float(), dn.contiguous().float()
        loss = torch.empty((), dtype=torch.float32, device=dp.device)
        call("artsbir_hinge_fwd", ptr(dp), ptr(dn), dp.numel(), margin, ptr(loss), _s())
        ctx.save_for_backward(dp, dn)
        ctx.margin = margin
        return loss

    @staticmethod
    def backward(ctx, g):
        dp, dn = ctx.saved_tensors
        gdp, gdn = torch.empty_like(dp), torch.empty_like(dn)
        call("artsbir_hinge_bwd", ptr(dp), ptr(dn), dp.numel(), ctx.margin, ptr(g.contiguous().float()), ptr(gdp),
             ptr(gdn), _s())
        return gdp, gdn, None


class TripletMarginWithDistanceLoss(nn.Module):
    """mean(clamp_min(margin + d(a,p) - d(a,n), 0)), swap=False, for d in
    {utils.euclidean_distance (fused triplet kernel), utils.cosine_distance}."""

    def __init__(self, distance_function=None, margin: float = 1.0, swap: bool = False, reduction: str = "mean"):
        super().__init__()
        if swap or reduction != "mean":
            raise NotImplementedError("only swap=False, reduction='mean' (the reference's configuration)")
        self.distance_function = distance_function
        self.margin, self.swap, self.reduction = margin, swap, reduction

    def forward(self, anchor, positive, negative):
        f = self.distance_function
        if f is None or getattr(f, "p", None) == 2.0:  # euclidean (PairwiseDistance) -> fused kernel
            return _TripletFn.apply(anchor, positive, negative, float(self.margin), float(getattr(f, "eps", 1e-6)))
        dp = f(anchor, positive)
        dn = f(anchor, negative)
        return _HingeFn.apply(dp, dn, float(self.margin))


# ------------------------------------------------------------ cross entropy
class _CEFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, labels, ignore_index):
        _cuda(logits, labels)
        x = logits.contiguous().float()
        lab = labels.contiguous().to(torch.int64)
        B, C = x.shape
        prob = torch.empty_like(x)
        loss2 = torch.empty(2, dtype=torch.float32, device=x.device)
        call("artsbir_cross_entropy_fwd", ptr(x), ptr(lab), B, C, ignore_index, ptr(prob), ptr(loss2), _s())
        ctx.save_for_backward(prob, lab, loss2)
        ctx.ignore_index = ignore_index
        return loss2[0].clone()

    @staticmethod
    def backward(ctx, g):
        prob, lab, loss2 = ctx.saved_tensors
        B, C = prob.shape
        d = torch.empty_like(prob)
        call("artsbir_cross_entropy_bwd", ptr(prob), ptr(lab), B, C, ctx.ignore_index, ptr(g.contiguous().float()),
             ptr(loss2), ptr(d), _s())
        return d, None, None


class CrossEntropyLoss(nn.Module):
    """nn.CrossEntropyLoss(ignore_index, reduction='mean') on artsbir_cross_entropy_fwd/_bwd.

    One deviation: when every label equals ignore_index, nn.CrossEntropyLoss returns NaN
    (0 / 0) with zero gradients; this returns 0 with zero gradients."""

    def __init__(self, ignore_index: int = -100, reduction: str = "mean"):
        super().__init__()
        if reduction != "mean":
            raise NotImplementedError("only reduction='mean' (the reference's configuration)")
        self.ignore_index, self.reduction = ignore_index, reduction

    def forward(self, logits, labels):
        return _CEFn.apply(logits, labels, int(self.ignore_index))


# ------------------------------------------------------------ in-batch negative mining
_MODES = {"hardest": 0, "semihard": 1}
_METRICS = {"euclidean": 0, "cosine": 1}
_MINE_EPS = {"euclidean": 1e-6, "cosine": 1e-8}  # the eps of TripletMarginLoss / cosine_distance


def _mine_codes(mode, metric, eps):
    if mode not in _MODES:
        raise ValueError(f"mode must be one of {sorted(_MODES)}, not {mode!r}")
    if metric not in _METRICS:
        raise ValueError(f"metric must be one of {sorted(_METRICS)}, not {metric!r}")
    return _MODES[mode], _METRICS[metric], float(_MINE_EPS[metric] if eps is None else eps)


def _gather_ranks(rows, ids):
    """(rows, ids) of every rank, rank-major, identical on all ranks: all_gather_into_tensor
    under an initialised process group of more than one rank, the arguments otherwise.
    ids may be None, on every rank alike."""
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1):
        return rows, ids
    world = dist.get_world_size()
    rows = rows.contiguous()
    all_rows = rows.new_empty((world * rows.shape[0],) + tuple(rows.shape[1:]))
    dist.all_gather_into_tensor(all_rows, rows)
    if ids is None:
        return all_rows, None
    ids = ids.contiguous()
    all_ids = ids.new_empty(world * ids.shape[0])
    dist.all_gather_into_tensor(all_ids, ids)
    return all_rows, all_ids


class CrossBatchMemory:
    """A ring of the last `size` gallery-side embeddings on the device (Wang et al.,
    "Cross-Batch Memory for Embedding Learning", CVPR 2020) for select_negatives /
    mine_negatives / MinedNegatives(memory=...): mem f32 [size, dim], mem_ids int64 [size]
    (the photo of every row; -1: none) and mem_state int64 [2] = (head, count).  Plain
    tensors: no checkpoint holds them.  The state lives on the device and only kernels
    read and write it (artsbir_xbm_enqueue, artsbir_mine_pool); rows in the ring are
    constants: no gradient reaches them.  dim None: the width (and, with device None, the
    device) of the first rows it meets, allocated then."""

    def __init__(self, size, dim, device=None):
        size = int(size)
        if size < 1 or (dim is not None and int(dim) < 1):
            raise ValueError(f"CrossBatchMemory needs size >= 1 and dim >= 1, not {size} x {dim}")
        self.size, self.dim, self.mem, self.mem_ids, self.mem_state = size, None, None, None, None
        if dim is not None:
            self._allocate(int(dim), torch.device("cuda" if device is None else device))
        self._device = device

    def _allocate(self, dim, device):
        self.dim = dim
        self.mem = torch.zeros(self.size, dim, dtype=torch.float32, device=device)
        self.mem_ids = torch.full((self.size,), -1, dtype=torch.int64, device=device)
        self.mem_state = torch.zeros(2, dtype=torch.int64, device=device)

    def _ready(self, rows):
        """allocated, and of the width and on the device of rows [*, dim]"""
        if self.mem is None:
            self._allocate(rows.shape[1], rows.device if self._device is None else torch.device(self._device))
        if rows.dim() != 2 or self.dim != rows.shape[1] or self.mem.device != rows.device:
            raise ValueError(f"the memory holds rows of width {self.dim} on {self.mem.device}, not "
                             f"{tuple(rows.shape)} on {rows.device}")

    @torch.no_grad()
    def enqueue(self, rows, ids=None, gathered=False):
        """rows [R, dim] (ids int64 [R] or None) into the ring, row r at slot (head + r) mod
        size; with more than one rank every rank's rows first, rank-major.  gathered=True:
        rows and ids are every rank's already, rank-major and the same on all ranks (the
        gather of a step that has done it), and are not gathered again"""
        _cuda(rows)
        rows = rows.detach().contiguous().float()
        self._ready(rows)
        if ids is not None:
            _cuda(ids)
            ids = ids.detach().contiguous().to(torch.int64)
            if ids.shape != (rows.shape[0],):
                raise ValueError(f"ids must have shape [{rows.shape[0]}], not {tuple(ids.shape)}")
        if not gathered:
            rows, ids = _gather_ranks(rows, ids)
        call("artsbir_xbm_enqueue", ptr(rows), ptr(ids), rows.shape[0], self.dim, ptr(self.mem), ptr(self.mem_ids),
             ptr(self.mem_state), self.size, _s())

    def reset(self):
        """forget every row: head = count = 0, on the device"""
        if self.mem_state is not None:
            self.mem_state.zero_()

    def filled(self) -> int:
        """slots that hold a row.  For debugging only: it synchronises with the device."""
        return 0 if self.mem_state is None else min(int(self.mem_state[1].item()), self.size)


@torch.no_grad()
def select_negatives(a, p, n, mode="hardest", metric="euclidean", eps=None, cand_ids=None, memory=None):
    """The selection alone: (sel int64 [B], d_ap [B], d_sel [B]) over the candidates
    C = [p; n] (artsbir_mine_negatives) and, with a CrossBatchMemory, its filled slots as
    the candidates 2B + j (artsbir_mine_pool).  It has no gradient."""
    mode_c, metric_c, eps = _mine_codes(mode, metric, eps)
    _cuda(a, p, n)
    a, p, n = (t.detach().contiguous().float() for t in (a, p, n))
    if not (a.dim() == 2 and a.shape == p.shape == n.shape):
        raise ValueError(f"a, p, n must share one [B, D] shape: {tuple(a.shape)} {tuple(p.shape)} {tuple(n.shape)}")
    B, D = a.shape
    if cand_ids is not None:
        _cuda(cand_ids)
        cand_ids = cand_ids.detach().contiguous().to(torch.int64)
        if cand_ids.shape != (2 * B,):
            raise ValueError(f"cand_ids must have shape [{2 * B}], not {tuple(cand_ids.shape)}")
    sel = torch.empty(B, dtype=torch.int64, device=a.device)
    d_ap, d_sel = (torch.empty(B, dtype=torch.float32, device=a.device) for _ in range(2))
    if memory is None:
        call("artsbir_mine_negatives", metric_c, mode_c, ptr(a), ptr(p), ptr(n), B, D, eps, ptr(cand_ids), ptr(sel),
             ptr(d_ap), ptr(d_sel), _s())
    else:
        memory._ready(a)
        call("artsbir_mine_pool", metric_c, mode_c, ptr(a), ptr(p), ptr(n), B, D, eps, ptr(cand_ids),
             ptr(memory.mem), ptr(memory.mem_ids), ptr(memory.mem_state), memory.size, ptr(sel), ptr(d_ap),
             ptr(d_sel), _s())
    return sel, d_ap, d_sel


class _MineFn(torch.autograd.Function):
    """N' = C[sel] with C = [p; n]; backward dC[c] = sum of dN'[i] over sel[i] == c in
    ascending i (no atomics: two runs give the same bytes), dp = dC[:B], dn = dC[B:].
    With a memory sel[i] >= 2B takes N'[i] from the ring: a constant, so it adds to no
    row of dC."""

    @staticmethod
    def forward(ctx, a, p, n, mode, metric, eps, cand_ids, memory):
        sel, _, _ = select_negatives(a, p, n, mode, metric, eps, cand_ids, memory)
        p, n = (t.contiguous().float() for t in (p, n))
        B, D = p.shape
        out = torch.empty_like(p)
        if memory is None:
            call("artsbir_rows_gather2", ptr(p), ptr(n), ptr(sel), B, D, ptr(out), _s())
        else:
            call("artsbir_rows_gather3", ptr(p), ptr(n), ptr(memory.mem), ptr(sel), B, D, memory.size, ptr(out),
                 _s())
        ctx.save_for_backward(sel)
        ctx.mark_non_differentiable(sel)
        return out, sel

    @staticmethod
    def backward(ctx, g, _gsel):
        sel, = ctx.saved_tensors
        g = g.contiguous().float()
        B, D = g.shape
        dp, dn = torch.empty_like(g), torch.empty_like(g)
        call("artsbir_rows_scatter2", ptr(g), ptr(sel), B, D, ptr(dp), ptr(dn), _s())
        return None, dp, dn, None, None, None, None, None


def mine_negatives(a, p, n, mode="hardest", metric="euclidean", eps=None, cand_ids=None, memory=None):
    """In-batch negative mining: for every anchor a[i] the hardest ('hardest') or the
    semi-hardest ('semihard': the closest one farther than the positive, strictly)
    of the 2B gallery-side rows C = [p; n], by the loss's own distance (metric
    'euclidean': ||a - c + eps||, eps 1e-6; 'cosine': 1 - cos, eps 1e-8).  Candidate
    c is valid for anchor i when c != i and, with cand_ids (int64 [2B], the photo of
    every candidate), cand_ids[c] != cand_ids[i]; ties go to the lowest c; with no
    candidate left the given negative n[i] stays (sel[i] = B + i).
    With memory (a CrossBatchMemory) its filled slots are candidates too: c = 2B + j
    is slot j, valid unless memory.mem_ids[j] == cand_ids[i]; a batch row wins a tie
    against a ring row and a lower slot against a higher one.
    Returns (n_mined [B, D], sel int64 [B]).  The selection has no gradient; the
    gradient of n_mined flows to the selected rows of p and n, and to nothing where
    the selection is a ring slot."""
    return _MineFn.apply(a, p, n, mode, metric, eps, cand_ids, memory)


class MinedNegatives(nn.Module):
    """loss_fn with its negatives mined in the batch:
    forward(a, p, n, *rest, cand_ids=None) = loss_fn(a, p, mine_negatives(a, p, n)[0], *rest)
    for TripletMarginLoss, TripletMarginWithDistanceLoss and the two
    TripletMarginLoss_with_classification composites of utils.  metric must be the
    wrapped loss's distance.  Device counters (no host synchronisation) follow the
    anchors seen with gradients enabled, those whose selection is not the given
    negative and those whose selection is a slot of the memory; mined_fraction() and
    memory_fraction() read them and reset their own.
    memory (a CrossBatchMemory, default None): with gradients enabled the negatives are
    mined over the batch and the ring, and cat(p, n).detach() with cand_ids is enqueued
    after the selection, so a step never meets its own rows in the ring; under
    torch.no_grad() the ring is neither read nor written."""

    def __init__(self, loss_fn, mode="hardest", metric="euclidean", memory=None):
        super().__init__()
        _mine_codes(mode, metric, None)
        self.loss_fn, self.mode, self.metric, self.memory = loss_fn, mode, metric, memory
        self._counts = None  # int64 [4] on the device: anchors seen, mined | seen, from the memory
        self._given = None   # arange(B, 2B) of the last batch size

    margin = property(lambda self: self.loss_fn.margin)
    classification_weight = property(lambda self: self.loss_fn.classification_weight)
    classification_weight2 = property(lambda self: self.loss_fn.classification_weight2)

    def forward(self, anchor, positive, negative, *rest, cand_ids=None):
        memory = self.memory if torch.is_grad_enabled() else None
        mined, sel = mine_negatives(anchor, positive, negative, self.mode, self.metric, None, cand_ids, memory)
        if torch.is_grad_enabled():
            B = sel.shape[0]
            if self._counts is None or self._counts.device != sel.device:
                self._counts = torch.zeros(4, dtype=torch.int64, device=sel.device)
            if self._given is None or self._given.shape[0] != B or self._given.device != sel.device:
                self._given = torch.arange(B, 2 * B, dtype=torch.int64, device=sel.device)
            self._counts[0] += B
            self._counts[1] += (sel != self._given).sum()
            if memory is not None:
                self._counts[2] += B
                self._counts[3] += (sel >= 2 * B).sum()
                memory.enqueue(torch.cat((positive, negative)).detach(), cand_ids)
        return self.loss_fn(anchor, positive, mined, *rest)

    def _fraction(self, k) -> float:
        if self._counts is None:
            return 0.0
        seen, hit = (int(v) for v in self._counts[k:k + 2].tolist())
        self._counts[k:k + 2].zero_()
        return hit / seen if seen else 0.0

    def mined_fraction(self) -> float:
        """mined / seen anchors since the last call (0.0 when none was seen); resets both"""
        return self._fraction(0)

    def memory_fraction(self) -> float:
        """anchors whose selection is a slot of the memory / anchors seen with the memory
        since the last call (0.0 when none was seen); resets both"""
        return self._fraction(2)


# ------------------------------------------------------------ InfoNCE over the batch and the memory
def _info_nce_raw(a, p, n, temperature, cand_ids, memory, eps, with_grad):
    """one artsbir_info_nce call: (loss [], rows [B], q [B], (da, dp, dn) or None)"""
    _cuda(a, p, n)
    a, p, n = (t.detach().contiguous().float() for t in (a, p, n))
    if not (a.dim() == 2 and a.shape == p.shape == n.shape):
        raise ValueError(f"a, p, n must share one [B, D] shape: {tuple(a.shape)} {tuple(p.shape)} {tuple(n.shape)}")
    temperature = float(temperature)
    if not temperature > 0:
        raise ValueError(f"temperature must be > 0, not {temperature}")
    B, D = a.shape
    if cand_ids is not None:
        _cuda(cand_ids)
        cand_ids = cand_ids.detach().contiguous().to(torch.int64)
        if cand_ids.shape != (2 * B,):
            raise ValueError(f"cand_ids must have shape [{2 * B}], not {tuple(cand_ids.shape)}")
    mem = mem_ids = mem_state = None
    M = 0
    if memory is not None:
        memory._ready(a)
        mem, mem_ids, mem_state, M = memory.mem, memory.mem_ids, memory.mem_state, memory.size
    nbytes = _hip.lib().artsbir_info_nce_workspace(B, D, M, int(with_grad))
    if nbytes < 0:
        raise _hip.HipError(_hip.lib().artsbir_last_error().decode(errors="replace"))
    ws = torch.empty(max(int(nbytes), 4), dtype=torch.uint8, device=a.device)
    loss = torch.empty((), dtype=torch.float32, device=a.device)
    rows, q = (torch.empty(B, dtype=torch.float32, device=a.device) for _ in range(2))
    grads = tuple(torch.empty_like(a) for _ in range(3)) if with_grad else (None, None, None)
    call("artsbir_info_nce", ptr(a), ptr(p), ptr(n), B, D, 1.0 / temperature, float(eps), ptr(cand_ids), ptr(mem),
         ptr(mem_ids), ptr(mem_state), M, ptr(loss), ptr(rows), ptr(q), ptr(grads[0]), ptr(grads[1]), ptr(grads[2]),
         ptr(ws), int(nbytes), _s())
    return loss, rows, q, (grads if with_grad else None)


class _InfoNCEFn(torch.autograd.Function):
    """The forward asks artsbir_info_nce for the gradients too when any input needs one:
    they are taken from the ring as the forward saw it (an enqueue right after the forward
    changes the ring), and the backward only scales them."""

    @staticmethod
    def forward(ctx, a, p, n, temperature, cand_ids, memory, eps):
        with_grad = any(ctx.needs_input_grad[:3])
        loss, rows, q, grads = _info_nce_raw(a, p, n, temperature, cand_ids, memory, eps, with_grad)
        if with_grad:
            ctx.save_for_backward(*grads)
        ctx.mark_non_differentiable(q)
        return loss, q

    @staticmethod
    def backward(ctx, gout, _gq):
        da, dp, dn = ctx.saved_tensors
        need = ctx.needs_input_grad
        return (gout * da if need[0] else None, gout * dp if need[1] else None, gout * dn if need[2] else None,
                None, None, None, None)


def _info_nce_pool_raw(a, cand, pos0, temperature, cand_ids, memory, eps, with_grad):
    """one artsbir_info_nce_pool call: anchors a [B, D] against the candidates cand [Nc, D]
    (ids cand_ids [Nc] or None) and the memory's filled slots, anchor i's positive at
    cand[pos0 + i] -> (loss [], rows [B], q [B], (da [B, D], dcand [Nc, D]) or None)"""
    _cuda(a, cand)
    a, cand = (t.detach().contiguous().float() for t in (a, cand))
    if not (a.dim() == 2 and cand.dim() == 2 and a.shape[1] == cand.shape[1]):
        raise ValueError(f"a [B, D] and cand [Nc, D] must share D: {tuple(a.shape)} {tuple(cand.shape)}")
    temperature = float(temperature)
    if not temperature > 0:
        raise ValueError(f"temperature must be > 0, not {temperature}")
    (B, D), Nc = a.shape, cand.shape[0]
    if cand_ids is not None:
        _cuda(cand_ids)
        cand_ids = cand_ids.detach().contiguous().to(torch.int64)
        if cand_ids.shape != (Nc,):
            raise ValueError(f"cand_ids must have shape [{Nc}], not {tuple(cand_ids.shape)}")
    mem = mem_ids = mem_state = None
    M = 0
    if memory is not None:
        memory._ready(a)
        mem, mem_ids, mem_state, M = memory.mem, memory.mem_ids, memory.mem_state, memory.size
    nbytes = _hip.lib().artsbir_info_nce_pool_workspace(B, Nc, D, M, int(with_grad))
    if nbytes < 0:
        raise _hip.HipError(_hip.lib().artsbir_last_error().decode(errors="replace"))
    ws = torch.empty(max(int(nbytes), 4), dtype=torch.uint8, device=a.device)
    loss = torch.empty((), dtype=torch.float32, device=a.device)
    rows, q = (torch.empty(B, dtype=torch.float32, device=a.device) for _ in range(2))
    grads = (torch.empty_like(a), torch.empty_like(cand)) if with_grad else (None, None)
    call("artsbir_info_nce_pool", ptr(a), ptr(cand), B, Nc, int(pos0), D, 1.0 / temperature, float(eps), ptr(cand_ids),
         ptr(mem), ptr(mem_ids), ptr(mem_state), M, ptr(loss), ptr(rows), ptr(q), ptr(grads[0]), ptr(grads[1]), ptr(ws),
         int(nbytes), _s())
    return loss, rows, q, (grads if with_grad else None)


def _reduce_rows(rows):
    """the sum of rows [world * R, D] over the ranks; this rank keeps its own R rows:
    reduce_scatter_tensor where the backend has it, all_reduce and a slice on gloo (chosen
    as ddp._avg_op chooses)"""
    import torch.distributed as dist
    world, rank = dist.get_world_size(), dist.get_rank()
    R = rows.shape[0] // world
    rows = rows.contiguous()
    if dist.get_backend() == "nccl":
        own = rows.new_empty((R,) + tuple(rows.shape[1:]))
        dist.reduce_scatter_tensor(own, rows, op=dist.ReduceOp.SUM)
        return own
    dist.all_reduce(rows, op=dist.ReduceOp.SUM)
    return rows[rank * R:(rank + 1) * R]


def _gathering() -> bool:
    """gather=True takes effect: gradients enabled and a process group of more than one rank"""
    import torch.distributed as dist
    return (torch.is_grad_enabled() and dist.is_available() and dist.is_initialized()
            and dist.get_world_size() > 1)


class _InfoNCEGatherFn(torch.autograd.Function):
    """The loss of this rank's anchors against G = every rank's [p; n], rank-major (this
    rank's own rows start at pos0 = rank * 2B), and the ring.  The forward takes da and
    dG from the kernel (the ring changes right after it); the backward scales them by
    gout, which is rank-local, sums gout * dG over the ranks and keeps this rank's rows:
    the gradient of sum_s loss_s with respect to its own p and n."""

    @staticmethod
    def forward(ctx, a, p, n, G, ids_G, pos0, temperature, memory, eps, kernel, reduce_rows):
        with_grad = any(ctx.needs_input_grad[:3])
        loss, rows, q, grads = kernel(a.detach(), G, pos0, temperature, ids_G, memory, eps, with_grad)
        if with_grad:
            ctx.save_for_backward(*grads)
        ctx.reduce_rows = reduce_rows
        ctx.mark_non_differentiable(q)
        return loss, q

    @staticmethod
    def backward(ctx, gout, _gq):
        da, dG = ctx.saved_tensors
        B = da.shape[0]
        own = ctx.reduce_rows(gout * dG)  # a collective: every rank runs this backward
        need = ctx.needs_input_grad
        return (gout * da if need[0] else None, own[:B] if need[1] else None, own[B:] if need[2] else None,
                None, None, None, None, None, None, None, None)


def _info_nce(a, p, n, temperature, cand_ids, memory, eps, gather, kernel, all_gather, reduce_rows):
    """(loss, q, gathered): gathered = (G, ids_G) of the step when the gather took effect,
    None when the local call ran"""
    if not (gather and _gathering()):
        if kernel is None:
            loss, q = _InfoNCEFn.apply(a, p, n, temperature, cand_ids, memory, eps)
        else:  # a stand-in for the kernel: the local call in the pool form
            loss, q = _InfoNCEGatherFn.apply(a, p, n, torch.cat((p, n)).detach(), cand_ids, 0, temperature, memory,
                                             eps, kernel, lambda rows: rows)
        return loss, q, None
    import torch.distributed as dist
    if not (a.dim() == 2 and a.shape == p.shape == n.shape):
        raise ValueError(f"a, p, n must share one [B, D] shape: {tuple(a.shape)} {tuple(p.shape)} {tuple(n.shape)}")
    if cand_ids is not None:
        cand_ids = cand_ids.detach().contiguous().to(torch.int64)
        if cand_ids.shape != (2 * a.shape[0],):
            raise ValueError(f"cand_ids must have shape [{2 * a.shape[0]}], not {tuple(cand_ids.shape)}")
    G, ids_G = (all_gather or _gather_ranks)(torch.cat((p, n)).detach().float(), cand_ids)
    loss, q = _InfoNCEGatherFn.apply(a, p, n, G, ids_G, dist.get_rank() * 2 * a.shape[0], temperature, memory, eps,
                                     kernel or _info_nce_pool_raw, reduce_rows or _reduce_rows)
    return loss, q, (G, ids_G)


def info_nce(a, p, n, temperature=0.07, cand_ids=None, memory=None, eps=1e-8, gather=False, *, kernel=None,
             all_gather=None, reduce_rows=None):
    """InfoNCE (softmax contrastive) loss of every anchor a[i] against its positive p[i] and
    every other gallery-side row of the step, C = [p; n], and of a CrossBatchMemory's filled
    slots: mean over i of -log softmax_i(positive) of the logits cos(a[i], c) / temperature.
    Candidate c != i is a negative unless cand_ids (int64 [2B], the photo of every row of C)
    is given and the candidate's photo (cand_ids[c], memory.mem_ids[j]) is cand_ids[i].
    Exact f32 on the f32-input MFMA; the logit matrix never exists in memory; two runs give
    the same bytes.  Gradients flow to a, p and n; ring rows are constants.

    gather=True, with gradients enabled under an initialised process group of more than one
    rank (otherwise the call above runs unchanged: no group, one rank, torch.no_grad()): the
    candidates are the rows of EVERY rank, G = all_gather(cat(p, n).detach()) rank-major with
    cand_ids gathered alike, in one artsbir_info_nce_pool call (Nc = 2B world, the positives
    at rank 2B + i); every rank passes the same B.  The value is the mean over this rank's
    anchors.  The backward returns gout da, and sums gout dG over the ranks and keeps the
    rows of this rank's own p and n (reduce_scatter_tensor; all_reduce and a slice on gloo):
    rank r back-propagates d(sum_s loss_s) / d(its own rows), so the parameter gradient that
    ddp averages over the ranks is that of the mean loss over all world B anchors.  That sum
    is a collective in the backward (gout is rank-local): every rank must run the backward of
    every gathered loss, as for any data-parallel step.  It is issued from the host before
    the encoder's backward starts, so it precedes the reducer's bucket all-reduces on every
    rank alike.  The ranks must also agree on whether any of a, p, n requires a gradient:
    a rank whose inputs need none takes no gradients in the forward and never enters that
    collective, and the others would wait for it.
    kernel / all_gather / reduce_rows (keyword only) stand in for the kernel call
    (_info_nce_pool_raw's signature) and the two collectives (_gather_ranks, _reduce_rows),
    as knn.knn_sharded's local_search / merge do: tests run the protocol without a GPU.
    A kernel stand-in replaces the local call too (where the gather does not take effect
    it is called in the pool form, cand = [p; n] and pos0 = 0, in place of
    artsbir_info_nce), so a test that passes one never reaches the device."""
    return _info_nce(a, p, n, temperature, cand_ids, memory, eps, gather, kernel, all_gather, reduce_rows)[0]


class InfoNCELoss(nn.Module):
    """forward(a, p, n, cand_ids=None) = info_nce(a, p, n, temperature, cand_ids, memory,
    gather=gather).
    memory (a CrossBatchMemory, default None): with gradients enabled the ring's filled slots
    are negatives too, and cat(p, n).detach() with cand_ids is enqueued after the loss has
    read the ring, so a step never meets its own rows; under torch.no_grad() the ring is
    neither read nor written.  A device counter (no host synchronisation) follows the
    probability of the positive, 1 - q, over the anchors seen with gradients enabled;
    positive_probability() reads and resets it.
    gather=True (see info_nce; it takes effect with gradients enabled under more than one
    rank): every rank's rows are candidates, their gradients go home in the backward, which
    every rank must run; the gathered rows are what the ring receives, so a gathered step
    does one all-gather, not two.  kernel / all_gather / reduce_rows: info_nce's stand-ins."""

    margin = None  # there is no margin: the triplet losses' attribute, for the training record

    def __init__(self, temperature: float = 0.07, memory=None, gather=False, *, kernel=None, all_gather=None,
                 reduce_rows=None):
        super().__init__()
        if not float(temperature) > 0:
            raise ValueError(f"temperature must be > 0, not {temperature}")
        self.temperature, self.memory, self.gather = float(temperature), memory, bool(gather)
        self._hooks = (kernel, all_gather, reduce_rows)
        self._sums = None  # f64 [2] on the device: anchors seen, sum of 1 - q

    def forward(self, anchor, positive, negative, cand_ids=None):
        grad = torch.is_grad_enabled()
        memory = self.memory if grad else None
        loss, q, gathered = _info_nce(anchor, positive, negative, self.temperature, cand_ids, memory, 1e-8,
                                      self.gather, *self._hooks)
        if grad:
            if self._sums is None or self._sums.device != q.device:
                self._sums = torch.zeros(2, dtype=torch.float64, device=q.device)
            self._sums[0] += q.shape[0]
            self._sums[1] += (1.0 - q.double()).sum()
            if memory is not None and gathered is not None:
                memory.enqueue(*gathered, gathered=True)
            elif memory is not None:
                memory.enqueue(torch.cat((positive, negative)).detach(), cand_ids)
        return loss

    def positive_probability(self) -> float:
        """mean probability of the positive over the anchors seen with gradients enabled
        since the last call (0.0 when none was seen); resets"""
        if self._sums is None:
            return 0.0
        seen, total = self._sums.tolist()
        self._sums.zero_()
        return total / seen if seen else 0.0
