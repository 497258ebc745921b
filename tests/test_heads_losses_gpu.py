"""Classification heads, distances and losses (csrc/heads.hip, csrc/loss_optim.hip,
artsbir_pairwise_l2 of csrc/retrieval.hip) called on their own, against float64
restatements, with the torch CPU f32 op the reference calls as the yardstick:
nn.PairwiseDistance, nn.CosineSimilarity(dim=1), F.cross_entropy, F.linear and
clamp_min(...).mean().  Shapes leave the four waves of a workgroup partly empty,
put class counts below, at and across 64 and batch sizes across the 256-thread
hinge block; one-row (broadcast) operands take the atomic path of the backward
kernels.  The bars are tests/_tail.py's; a broadcast gradient is held to the
worst-case bound of an f32 sum in arbitrary order (check_atomic_sum)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from _tail import check_atomic_sum, check_f32, f64

pytestmark = pytest.mark.gpu

EPS_L2 = float(np.float32(1e-6))  # the kernels take f32 eps
EPS_COS = float(np.float32(1e-8))


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _dirty_allocator(dev, *shapes):
    """fill and free blocks of the given shapes, so that an uninitialised
    allocation of the same size that follows does not happen to hold zeros"""
    junk = [torch.full(s, 777.0, device=dev) for s in shapes for _ in range(8)]
    torch.cuda.synchronize()
    del junk


# ------------------------------------------------------------------ distances
DIST_SHAPES = [(5, 5, 1), (7, 7, 63), (4, 4, 64), (9, 9, 65), (1, 300, 512), (300, 1, 512), (1, 1, 33), (1000, 1000, 8)]


def _l2_ref(x1, x2, g, eps):
    """-> dist [n], per-row gradient terms t [n][D] (d1 = sum/identity of t, d2 of -t)"""
    diff = x1 - x2 + x1.dtype.type(eps)
    dist = np.sqrt((diff * diff).sum(1))
    t = g[:, None] * diff / dist[:, None]
    return dist, t


def _cos_ref(x1, x2, g, eps):
    """distance 1 - cos and the per-row gradient terms of both operands for an
    upstream gradient g of the distance"""
    eps = x1.dtype.type(eps)
    na = np.maximum(np.sqrt((x1 * x1).sum(1)), eps)[:, None]
    nb = np.maximum(np.sqrt((x2 * x2).sum(1)), eps)[:, None]
    n = max(len(x1), len(x2))
    c = ((x1 * x2).sum(1)[:, None] / (na * nb)) * np.ones((n, 1), x1.dtype)
    gc = -g[:, None]
    ta = gc * (x2 / (na * nb) - c * x1 / (na * na))
    tb = gc * (x1 / (na * nb) - c * x2 / (nb * nb))
    return 1 - c[:, 0], ta, tb


def _reduce(t, n_op):
    return t.sum(0, keepdims=True) if n_op == 1 and t.shape[0] > 1 else t


def _dist_inputs(n1, n2, D):
    rng = np.random.default_rng(n1 * 1009 + n2 * 31 + D)
    x1 = rng.normal(0, 1, (n1, D)).astype(np.float32)
    x2 = rng.normal(0, 1, (n2, D)).astype(np.float32)
    g = rng.normal(0, 1, max(n1, n2)).astype(np.float32)
    return x1, x2, g


def _torch_cpu(fn, x1, x2, g):
    a, b = (torch.from_numpy(x).clone().requires_grad_(True) for x in (x1, x2))
    out = fn(a, b)
    out.backward(torch.from_numpy(g))
    return out.detach(), a.grad, b.grad


def _check_grad(label, hip, t64, n_op, cpu32):
    """one operand's gradient: elementwise f32 bar, or the atomic-sum bound when
    the operand is one row broadcast over n > 1 rows"""
    if n_op == 1 and t64.shape[0] > 1:
        check_atomic_sum(label, hip, t64.sum(0), t64)
    else:
        check_f32(label, hip, _reduce(t64, n_op), cpu32)


def _twice(fn, x1, x2, g, dev):
    """two forward calls on fresh inputs, one backward through both: -> out, (d1, d2) x 2"""
    _dirty_allocator(dev, x1.shape, x2.shape)
    leaves = [[_t(x, dev).requires_grad_(True) for x in (x1, x2)] for _ in range(2)]
    outs = [fn(a, b) for a, b in leaves]
    gd = _t(g, dev)
    loss = sum((o * gd).sum() for o in outs)
    _dirty_allocator(dev, x1.shape, x2.shape)  # again: the forward took blocks of these sizes
    loss.backward()
    torch.cuda.synchronize()
    return outs[0].detach(), [(a.grad, b.grad) for a, b in leaves]


@pytest.mark.parametrize("n1,n2,D", DIST_SHAPES)
def test_pairwise_l2_autograd(n1, n2, D, dev):
    import losses
    x1, x2, g = _dist_inputs(n1, n2, D)
    out, grads = _twice(lambda a, b: losses.pairwise_l2_autograd(a, b, 1e-6), x1, x2, g, dev)
    d64, t64 = _l2_ref(x1.astype(np.float64), x2.astype(np.float64), g.astype(np.float64), EPS_L2)
    c_out, c1, c2 = _torch_cpu(torch.nn.PairwiseDistance(p=2.0, eps=1e-6), x1, x2, g)
    tag = f"pairwise_l2 n1={n1} n2={n2} D={D}"
    check_f32(f"{tag} dist", out, d64, c_out)
    for k, (d1, d2) in enumerate(grads):
        assert d1.shape == x1.shape and d2.shape == x2.shape
        _check_grad(f"{tag} d1 (call {k + 1})", d1, t64, n1, c1)
        _check_grad(f"{tag} d2 (call {k + 1})", d2, -t64, n2, c2)
    # the second call's broadcast gradient equals the first's to the same bound (a
    # buffer that was not zeroed before the atomics shows here)
    if n1 == 1 and n2 > 1:
        check_atomic_sum(f"{tag} d1 call 2 vs call 1", grads[1][0], f64(grads[0][0]).reshape(-1), t64)
    if n2 == 1 and n1 > 1:
        check_atomic_sum(f"{tag} d2 call 2 vs call 1", grads[1][1], f64(grads[0][1]).reshape(-1), t64)


@pytest.mark.parametrize("n1,n2,D", DIST_SHAPES)
def test_cosine_distance(n1, n2, D, dev):
    import losses
    x1, x2, g = _dist_inputs(n1, n2, D)
    out, grads = _twice(lambda a, b: losses.cosine_distance(a, b, 1e-8), x1, x2, g, dev)
    d64, ta, tb = _cos_ref(x1.astype(np.float64), x2.astype(np.float64), g.astype(np.float64), EPS_COS)
    c_out, c1, c2 = _torch_cpu(lambda a, b: 1 - torch.nn.CosineSimilarity(dim=1, eps=1e-8)(a, b), x1, x2, g)
    tag = f"cosine n1={n1} n2={n2} D={D}"
    check_f32(f"{tag} 1-cos", out, d64, c_out)
    for k, (d1, d2) in enumerate(grads):
        assert d1.shape == x1.shape and d2.shape == x2.shape
        _check_grad(f"{tag} d1 (call {k + 1})", d1, ta, n1, c1)
        _check_grad(f"{tag} d2 (call {k + 1})", d2, tb, n2, c2)
    if n1 == 1 and n2 > 1:
        check_atomic_sum(f"{tag} d1 call 2 vs call 1", grads[1][0], f64(grads[0][0]).reshape(-1), ta)
    if n2 == 1 and n1 > 1:
        check_atomic_sum(f"{tag} d2 call 2 vs call 1", grads[1][1], f64(grads[0][1]).reshape(-1), tb)


def test_pairwise_l2_direct_call(dev):
    """raw entry points, x1 one row: d1 accumulates by atomics into what the caller
    left there (the wrapper zero-fills), d2 is overwritten; NULL gradients are skipped"""
    import _hip
    n, D = 7, 65
    x1, x2, g = _dist_inputs(1, n, D)
    a, b, gd = _t(x1, dev), _t(x2, dev), _t(g, dev)
    dist = torch.empty(n, device=dev)
    _hip.call("artsbir_pairwise_l2", a.data_ptr(), 1, b.data_ptr(), n, D, EPS_L2, dist.data_ptr(), _hip.stream())
    pre = np.random.default_rng(5).normal(0, 1, (1, D)).astype(np.float32)
    d1, d2 = _t(pre, dev), torch.full((n, D), 777.0, device=dev)
    _hip.call("artsbir_pairwise_l2_bwd", a.data_ptr(), 1, b.data_ptr(), n, D, EPS_L2, dist.data_ptr(), gd.data_ptr(),
              d1.data_ptr(), d2.data_ptr(), _hip.stream())
    d2_only = torch.full((n, D), 777.0, device=dev)
    _hip.call("artsbir_pairwise_l2_bwd", a.data_ptr(), 1, b.data_ptr(), n, D, EPS_L2, dist.data_ptr(), gd.data_ptr(),
              None, d2_only.data_ptr(), _hip.stream())
    torch.cuda.synchronize()
    d64, t64 = _l2_ref(x1.astype(np.float64), x2.astype(np.float64), g.astype(np.float64), EPS_L2)
    d32, t32 = _l2_ref(x1, x2, g, EPS_L2)
    check_f32("pairwise_l2 direct dist", dist, d64, d32)
    terms = np.concatenate([pre.astype(np.float64), t64])  # the pre-filled value is one more term of the sum
    check_atomic_sum("pairwise_l2_bwd direct d1 += (n1 == 1)", d1, terms.sum(0), terms)
    check_f32("pairwise_l2_bwd direct d2", d2, -t64, -t32)
    assert torch.equal(d2, d2_only)


def test_cosine_bwd_accumulates_into_one_row_operand(dev):
    """artsbir_cosine_bwd with n1 == 1 adds to a pre-filled d1"""
    import _hip
    n, D = 9, 65
    x1, x2, g = _dist_inputs(1, n, D)
    a, b = _t(x1, dev), _t(x2, dev)
    cosv, norms = torch.empty(n, device=dev), torch.empty(2 * n, device=dev)
    _hip.call("artsbir_cosine_fwd", a.data_ptr(), 1, b.data_ptr(), n, D, EPS_COS, cosv.data_ptr(), norms.data_ptr(),
              _hip.stream())
    pre = np.random.default_rng(6).normal(0, 1, (1, D)).astype(np.float32)
    d1, d2 = _t(pre, dev), torch.full((n, D), 777.0, device=dev)
    gcos = _t(-g, dev)  # the kernel takes the gradient of cos; g is the gradient of 1 - cos
    _hip.call("artsbir_cosine_bwd", a.data_ptr(), 1, b.data_ptr(), n, D, cosv.data_ptr(), norms.data_ptr(),
              gcos.data_ptr(), d1.data_ptr(), d2.data_ptr(), _hip.stream())
    torch.cuda.synchronize()
    c64, ta, tb = _cos_ref(x1.astype(np.float64), x2.astype(np.float64), g.astype(np.float64), EPS_COS)
    c32, _, tb32 = _cos_ref(x1, x2, g, EPS_COS)
    check_f32("cosine_fwd direct cos", cosv, 1 - c64, 1 - c32)
    terms = np.concatenate([pre.astype(np.float64), ta])
    check_atomic_sum("cosine_bwd direct d1 += (n1 == 1)", d1, terms.sum(0), terms)
    check_f32("cosine_bwd direct d2", d2, tb, tb32)
    assert not np.allclose(f64(d1), pre, atol=1e-3)  # and something was added


def test_cosine_zero_row(dev):
    """an exactly zero x1 row (what torch 2.10 gives on the CPU): cos = 0,
    d1 = g x2 / (eps |x2|), d2 = 0"""
    import losses
    rng = np.random.default_rng(11)
    x1 = rng.normal(0, 1, (4, 33)).astype(np.float32)
    x2 = rng.normal(0, 1, (4, 33)).astype(np.float32)
    x1[2] = 0.0
    g = rng.normal(0, 1, 4).astype(np.float32)
    a, b = _t(x1, dev).requires_grad_(True), _t(x2, dev).requires_grad_(True)
    out = losses.cosine_distance(a, b, 1e-8)
    out.backward(_t(g, dev))
    c_out, c1, c2 = _torch_cpu(lambda a, b: 1 - torch.nn.CosineSimilarity(dim=1, eps=1e-8)(a, b), x1, x2, g)
    d64, ta, tb = _cos_ref(x1.astype(np.float64), x2.astype(np.float64), g.astype(np.float64), EPS_COS)
    assert out[2].item() == 1.0  # cos == 0 exactly
    nb = np.sqrt((x2[2].astype(np.float64) ** 2).sum())
    np.testing.assert_allclose(ta[2], -g[2] * x2[2].astype(np.float64) / (EPS_COS * nb), rtol=1e-12)
    check_f32("cosine zero row 1-cos", out, d64, c_out)
    check_f32("cosine zero row d1[zero row]", a.grad[2], ta[2], c1[2])
    keep = [0, 1, 3]
    check_f32("cosine zero row d1[other rows]", a.grad[keep], ta[keep], c1[keep])
    check_f32("cosine zero row d2", b.grad, tb, c2)
    assert (b.grad[2] == 0).all()


def test_pairwise_l2_zero_distance_row(dev):
    """x1 - x2 + eps == 0 exactly (x2 = 0, x1 = -eps): distance 0 and a zero gradient, as torch"""
    import losses
    rng = np.random.default_rng(12)
    x1 = rng.normal(0, 1, (4, 8)).astype(np.float32)
    x2 = rng.normal(0, 1, (4, 8)).astype(np.float32)
    x1[1], x2[1] = -np.float32(1e-6), 0.0
    g = rng.normal(0, 1, 4).astype(np.float32)
    a, b = _t(x1, dev).requires_grad_(True), _t(x2, dev).requires_grad_(True)
    out = losses.pairwise_l2_autograd(a, b, 1e-6)
    out.backward(_t(g, dev))
    c_out, c1, c2 = _torch_cpu(torch.nn.PairwiseDistance(p=2.0, eps=1e-6), x1, x2, g)
    assert c_out[1].item() == 0.0 and (c1[1] == 0).all() and (c2[1] == 0).all()  # the reference's values
    assert out[1].item() == 0.0 and (a.grad[1] == 0).all() and (b.grad[1] == 0).all()
    keep = [0, 2, 3]
    d64, t64 = _l2_ref(x1[keep].astype(np.float64), x2[keep].astype(np.float64), g[keep].astype(np.float64), EPS_L2)
    check_f32("pairwise_l2 zero-distance: other rows dist", out[keep], d64, c_out[keep])
    check_f32("pairwise_l2 zero-distance: other rows d1", a.grad[keep], t64, c1[keep])


# --------------------------------------------------------------- hinge, triplet
BATCHES = [1, 3, 255, 256, 257, 1000]
MARGIN = 0.25
GOUT = 1.7  # upstream gradient of the loss, not 1


@pytest.mark.parametrize("B", BATCHES)
def test_hinge(B, dev):
    """mean(clamp_min(margin + dp - dn, 0)) over precomputed distances; row 0 is an
    exact tie (0.25 + 1.0 - 1.25 == 0: clamp_min's backward passes the gradient),
    row 1 strictly negative (exact zeros)"""
    import losses
    rng = np.random.default_rng(B)
    dp = rng.uniform(0, 2, B).astype(np.float32)
    dn = rng.uniform(0, 2, B).astype(np.float32)
    dp[0], dn[0] = 1.0, 1.25
    if B > 1:
        dp[1], dn[1] = 0.5, 2.0
    a, b = _t(dp, dev).requires_grad_(True), _t(dn, dev).requires_grad_(True)
    loss = losses._HingeFn.apply(a, b, MARGIN)
    (loss * GOUT).backward()
    ca, cb = (torch.from_numpy(x).clone().requires_grad_(True) for x in (dp, dn))
    closs = torch.clamp_min(MARGIN + ca - cb, 0).mean()
    (closs * GOUT).backward()
    h = MARGIN + dp.astype(np.float64) - dn.astype(np.float64)
    g64 = np.where(h >= 0, GOUT / B, 0.0)
    check_f32(f"hinge B={B} loss", loss.reshape(1), np.maximum(h, 0).mean().reshape(1), closs.detach().reshape(1))
    check_f32(f"hinge B={B} d(dp)", a.grad, g64, ca.grad)
    check_f32(f"hinge B={B} d(dn)", b.grad, -g64, cb.grad)
    assert ca.grad[0].item() > 0 and cb.grad[0].item() < 0  # torch passes the tie
    assert a.grad[0].item() > 0 and b.grad[0].item() < 0
    if B > 1:
        assert a.grad[1].item() == 0.0 and b.grad[1].item() == 0.0


def _triplet_inputs(B, D):
    rng = np.random.default_rng(B * 13 + D)
    a = rng.normal(0, 1, (B, D)).astype(np.float32)
    p = rng.normal(0, 1, (B, D)).astype(np.float32)
    n = rng.normal(0, 1, (B, D)).astype(np.float32)
    eps = np.float32(1e-6)
    # row 0, an exact tie: a = 0 and p = n = eps off coordinate 0, so a - p + eps == 0
    # there; coordinate 0 leaves t_p = fl(1 + eps) and t_n = fl(1.25 + eps) = 0.25 + t_p
    # (one binade), the distances are sqrt(t^2) = t exactly and 0.25 + t_p - t_n == 0
    a[0] = 0.0
    p[0] = eps
    n[0] = eps
    p[0, 0], n[0, 0] = -1.0, -1.25
    if B > 1:  # row 1, strictly negative: the positive next to the anchor, the negative far away
        p[1] = a[1] + np.float32(0.01)
        n[1] = a[1] + np.float32(5.0)
    return a, p, n


@pytest.mark.parametrize("B", BATCHES)
def test_triplet(B, dev):
    import losses
    D = 33
    a, p, n = _triplet_inputs(B, D)
    tp, tn = np.float32(1.0) + np.float32(1e-6), np.float32(1.25) + np.float32(1e-6)
    assert np.float32(MARGIN) + tp - tn == 0  # the tie is exact in f32
    leaves = [_t(x, dev).requires_grad_(True) for x in (a, p, n)]
    loss = losses.TripletMarginLoss(margin=MARGIN)(*leaves)
    (loss * GOUT).backward()
    cl = [torch.from_numpy(x).clone().requires_grad_(True) for x in (a, p, n)]
    closs = torch.nn.TripletMarginLoss(margin=MARGIN)(*cl)
    (closs * GOUT).backward()
    a64, p64, n64 = (x.astype(np.float64) for x in (a, p, n))
    dpos, dneg = a64 - p64 + EPS_L2, a64 - n64 + EPS_L2
    dap, dan = np.sqrt((dpos ** 2).sum(1)), np.sqrt((dneg ** 2).sum(1))
    h = MARGIN + dap - dan
    h[0] = 0.0  # exact in f32 (above); float64 sees the rounding of 1 + eps
    on = (h >= 0)[:, None] * (GOUT / B)
    up, un = dpos / dap[:, None], dneg / dan[:, None]
    check_f32(f"triplet B={B} loss", loss.reshape(1), np.maximum(h, 0).mean().reshape(1), closs.detach().reshape(1))
    check_f32(f"triplet B={B} da", leaves[0].grad, on * (up - un), cl[0].grad)
    check_f32(f"triplet B={B} dp", leaves[1].grad, -on * up, cl[1].grad)
    check_f32(f"triplet B={B} dn", leaves[2].grad, on * un, cl[2].grad)
    assert cl[1].grad[0, 0].item() < 0 and cl[2].grad[0, 0].item() > 0  # torch passes the tie
    assert leaves[1].grad[0, 0].item() < 0 and leaves[2].grad[0, 0].item() > 0
    if B > 1:
        for t in leaves:
            assert (t.grad[1] == 0).all()


# --------------------------------------------------------------- cross entropy
CE_CASES = [(1, 5), (3, 64), (5, 65), (16, 125), (9, 1000)]


def _ce_inputs(B, C, ignore_index):
    rng = np.random.default_rng(B * 1000 + C + (ignore_index % 97))
    x = rng.normal(0, 1, (B, C)).astype(np.float32)
    x[0] += 80.0  # exp() of the raw logits overflows f32: pins the max subtraction
    if B > 4:
        x[4] += 80.0
    lab = rng.integers(0, C, B).astype(np.int64)
    if B > 1:
        lab[1] = ignore_index
    if B > 8:
        lab[8] = ignore_index
    return x, lab


def _ce_ref(x, lab, ignore_index, g):
    m = x.max(1, keepdims=True)
    lse = m + np.log(np.exp(x - m).sum(1, keepdims=True))
    prob = np.exp(x - lse)
    on = lab != ignore_index
    cnt = int(on.sum())
    safe = np.where(on, lab, 0)
    rows = (lse[:, 0] - x[np.arange(len(x)), safe]) * on
    onehot = np.zeros_like(x)
    onehot[np.arange(len(x)), safe] = 1
    d = (g / max(cnt, 1)) * (prob - onehot) * on[:, None]
    return rows.sum() / max(cnt, 1), cnt, prob, d


def _ce_direct(x, lab, ignore_index, g, dev):
    import _hip
    B, C = x.shape
    dx, dl = _t(x, dev), _t(lab, dev)
    prob = torch.full((B * C + C,), 777.0, device=dev)
    loss2 = torch.full((3,), 777.0, device=dev)
    _hip.call("artsbir_cross_entropy_fwd", dx.data_ptr(), dl.data_ptr(), B, C, ignore_index, prob.data_ptr(),
              loss2.data_ptr(), _hip.stream())
    d = torch.full((B * C + C,), 777.0, device=dev)
    gout = torch.tensor([g], dtype=torch.float32, device=dev)
    _hip.call("artsbir_cross_entropy_bwd", prob.data_ptr(), dl.data_ptr(), B, C, ignore_index, gout.data_ptr(),
              loss2.data_ptr(), d.data_ptr(), _hip.stream())
    torch.cuda.synchronize()
    assert (prob[B * C:] == 777.0).all() and (d[B * C:] == 777.0).all() and loss2[2].item() == 777.0
    return loss2[:2].cpu(), prob[:B * C].view(B, C), d[:B * C].view(B, C)


@pytest.mark.parametrize("ignore_index", [-100, 7])
@pytest.mark.parametrize("B,C", CE_CASES)
def test_cross_entropy(B, C, ignore_index, dev):
    g = 0.37
    x, lab = _ce_inputs(B, C, ignore_index)
    loss2, prob, d = _ce_direct(x, lab, ignore_index, g, dev)
    l64, cnt, p64, d64 = _ce_ref(x.astype(np.float64), lab, ignore_index, g)
    cx = torch.from_numpy(x).clone().requires_grad_(True)
    closs = F.cross_entropy(cx, torch.from_numpy(lab), ignore_index=ignore_index)
    (closs * g).backward()
    cprob = torch.softmax(torch.from_numpy(x), 1)
    tag = f"cross_entropy B={B} C={C} ignore={ignore_index}"
    assert cnt >= 1 and loss2[1].item() == float(cnt)
    check_f32(f"{tag} loss", loss2[:1], np.array([l64]), closs.detach().reshape(1))
    check_f32(f"{tag} prob", prob, p64, cprob)
    check_f32(f"{tag} sum_c prob", prob.double().sum(1), np.ones(B), cprob.sum(1))
    check_f32(f"{tag} dlogits", d, d64, cx.grad)
    assert (d[_t(lab == ignore_index, dev)] == 0).all()


@pytest.mark.parametrize("ignore_index", [-100, 7])
def test_cross_entropy_all_rows_ignored(ignore_index, dev):
    """torch returns NaN here (0 / 0) with zero gradients; the kernel returns 0 with
    zero gradients (documented at artsbir_cross_entropy_fwd and losses.CrossEntropyLoss)"""
    import losses
    x, _ = _ce_inputs(5, 65, ignore_index)
    lab = np.full(5, ignore_index, np.int64)
    loss2, prob, d = _ce_direct(x, lab, ignore_index, 0.37, dev)
    assert loss2[0].item() == 0.0 and loss2[1].item() == 0.0
    assert (d == 0).all()
    lx = _t(x, dev).requires_grad_(True)
    loss = losses.CrossEntropyLoss(ignore_index=ignore_index)(lx, _t(lab, dev))
    loss.backward()
    assert loss.item() == 0.0 and (lx.grad == 0).all()


# ---------------------------------------------------------------------- linear
LIN_CASES = [(1, 1, 1), (3, 65, 7), (16, 1024, 125), (4, 2048, 250)]


def _lin_inputs(B, D, C):
    rng = np.random.default_rng(B * 7 + D * 3 + C)
    x = rng.normal(0, 1, (B, D)).astype(np.float32)
    w = (rng.normal(0, 1, (C, D)) / np.sqrt(D)).astype(np.float32)
    b = rng.normal(0, 0.5, C).astype(np.float32)
    dy = rng.normal(0, 1, (B, C)).astype(np.float32)
    return x, w, b, dy


def _lin_cpu(x, w, b, dy):
    cx, cw = (torch.from_numpy(t).clone().requires_grad_(True) for t in (x, w))
    cb = torch.from_numpy(b).clone().requires_grad_(True) if b is not None else None
    y = F.linear(cx, cw, cb)
    y.backward(torch.from_numpy(dy))
    return y.detach(), cx.grad, cw.grad, (cb.grad if cb is not None else None)


@pytest.mark.parametrize("B,D,C", LIN_CASES)
def test_linear_direct_call_accumulates(B, D, C, dev):
    """artsbir_linear_fwd / _bwd on raw pointers: dW and db come back as old + gradient,
    dx is overwritten; bias, db and dx may be NULL"""
    import _hip
    x, w, b, dy = _lin_inputs(B, D, C)
    rng = np.random.default_rng(99)
    w_old = rng.normal(0, 1, (C, D)).astype(np.float32)
    b_old = rng.normal(0, 1, C).astype(np.float32)
    dx_, dw_, db_, ddy = _t(x, dev), _t(w, dev), _t(b, dev), _t(dy, dev)
    y, y_nb = torch.full((B * C + 1,), 777.0, device=dev), torch.empty(B, C, device=dev)
    _hip.call("artsbir_linear_fwd", dx_.data_ptr(), dw_.data_ptr(), db_.data_ptr(), B, D, C, y.data_ptr(), _hip.stream())
    _hip.call("artsbir_linear_fwd", dx_.data_ptr(), dw_.data_ptr(), None, B, D, C, y_nb.data_ptr(), _hip.stream())
    gx, gw, gb = torch.full((B * D + 1,), 777.0, device=dev), _t(w_old, dev), _t(b_old, dev)
    _hip.call("artsbir_linear_bwd", ddy.data_ptr(), dx_.data_ptr(), dw_.data_ptr(), B, D, C, gx.data_ptr(), gw.data_ptr(),
              gb.data_ptr(), _hip.stream())
    gw_only = _t(w_old, dev)  # bias = None: db NULL, and no input gradient: dx NULL
    _hip.call("artsbir_linear_bwd", ddy.data_ptr(), dx_.data_ptr(), dw_.data_ptr(), B, D, C, None, gw_only.data_ptr(), None,
              _hip.stream())
    torch.cuda.synchronize()
    assert y[B * C].item() == 777.0 and gx[B * D].item() == 777.0
    x64, w64, b64, dy64 = (t.astype(np.float64) for t in (x, w, b, dy))
    cy, cdx, cdw, cdb = _lin_cpu(x, w, b, dy)
    cy_nb = _lin_cpu(x, w, None, dy)[0]
    tag = f"linear B={B} D={D} C={C}"
    check_f32(f"{tag} y", y[:B * C].view(B, C), x64 @ w64.T + b64, cy)
    check_f32(f"{tag} y (no bias)", y_nb, x64 @ w64.T, cy_nb)
    check_f32(f"{tag} dx", gx[:B * D].view(B, D), dy64 @ w64, cdx)
    check_f32(f"{tag} dW (old + grad)", gw, w_old.astype(np.float64) + dy64.T @ x64, torch.from_numpy(w_old) + cdw)
    check_f32(f"{tag} db (old + grad)", gb, b_old.astype(np.float64) + dy64.sum(0), torch.from_numpy(b_old) + cdb)
    assert torch.equal(gw_only, gw)


@pytest.mark.parametrize("B,D,C", LIN_CASES)
@pytest.mark.parametrize("bias", [True, False], ids=["bias", "nobias"])
def test_linear_autograd_does_not_double_count(B, D, C, bias, dev):
    """through heads.linear: the wrapper hands the accumulating kernel zero-filled
    buffers, so a second forward/backward gives the same gradients as the first"""
    import heads
    x, w, b, dy = _lin_inputs(B, D, C)
    if not bias:
        b = None
    cy, cdx, cdw, cdb = _lin_cpu(x, w, b, dy)
    x64, w64, dy64 = (t.astype(np.float64) for t in (x, w, dy))
    tag = f"heads.linear B={B} D={D} C={C} {'bias' if bias else 'nobias'}"
    for k in range(2):
        _dirty_allocator(dev, (C, D), (C,))
        lx, lw = _t(x, dev).requires_grad_(True), _t(w, dev).requires_grad_(True)
        lb = _t(b, dev).requires_grad_(True) if bias else None
        y = heads.linear(lx, lw, lb)
        y.backward(_t(dy, dev))
        check_f32(f"{tag} y (pass {k + 1})", y, x64 @ w64.T + (b.astype(np.float64) if bias else 0.0), cy)
        check_f32(f"{tag} dx (pass {k + 1})", lx.grad, dy64 @ w64, cdx)
        check_f32(f"{tag} dW (pass {k + 1})", lw.grad, dy64.T @ x64, cdw)
        if bias:
            check_f32(f"{tag} db (pass {k + 1})", lb.grad, dy64.sum(0), cdb)
    # the weight alone: no input gradient is asked for (dx NULL)
    lw = _t(w, dev).requires_grad_(True)
    heads.linear(_t(x, dev), lw, None).backward(_t(dy, dev))
    check_f32(f"{tag} dW (x without grad)", lw.grad, dy64.T @ x64, cdw)


def test_cross_entropy_on_linear_head(dev):
    """losses.CrossEntropyLoss(ignore_index=7) on heads.linear logits, gout != 1"""
    import heads
    import losses
    B, D, C = 5, 65, 65
    x, w, b, _ = _lin_inputs(B, D, C)
    lab = np.array([3, 7, 64, 0, 7], np.int64)

    def run(x, w, b, lab, lin, ce):
        leaves = [t.clone().requires_grad_(True) for t in (x, w, b)]
        loss = ce(lin(*leaves), lab)
        (loss * 0.37).backward()
        return loss.detach(), [t.grad for t in leaves]
    cl, cg = run(*(torch.from_numpy(t) for t in (x, w, b, lab)), F.linear,
                 lambda z, t: F.cross_entropy(z, t, ignore_index=7))
    hl, hg = run(*(_t(t, dev) for t in (x, w, b, lab)), heads.linear, losses.CrossEntropyLoss(ignore_index=7))
    x64, w64, b64 = (t.astype(np.float64) for t in (x, w, b))
    l64, cnt, _, dz = _ce_ref(x64 @ w64.T + b64, lab, 7, 0.37)
    assert cnt == 3
    check_f32("linear+cross_entropy loss", hl.reshape(1), np.array([l64]), cl.reshape(1))
    check_f32("linear+cross_entropy dx", hg[0], dz @ w64, cg[0])
    check_f32("linear+cross_entropy dW", hg[1], dz.T @ x64, cg[1])
    check_f32("linear+cross_entropy db", hg[2], dz.sum(0), cg[2])
