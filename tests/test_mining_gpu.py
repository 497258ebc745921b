"""In-batch negative mining on the GPU (csrc/mining.hip, losses.mine_negatives,
losses.MinedNegatives, train.py --negatives) against the float64 restatement of
tests/_mining_ref.py.

Selection: an anchor is *decided* when the f64 reference has gaps wider than the
derived worst case of an f32 sum of D terms (_mining_ref.tol / decided); decided
anchors must match exactly, the others are skipped, and the skipped share over all
cases stays <= 2 %.  Distances and gradients: the f32 bar of tests/_tail.py."""
import functools

import numpy as np
import pytest
import torch

import _mining_ref as mref
from _mining_ref import check_exact, check_f32

pytestmark = pytest.mark.gpu

BATCHES = (1, 2, 5, 37, 130, 384)
WIDTHS = (1, 3, 63, 64, 65, 512)
MODES = ("hardest", "semihard")
METRICS = ("euclidean", "cosine")
# D = 1 for the euclidean metric only: its cosine keys are all 0 or 2
SHAPES = [(B, D, m) for B in BATCHES for D in WIDTHS for m in (0, 1) if not (D == 1 and m == 1)]


def _dirty_allocator(dev, *shapes):
    """fill and free blocks of the given shapes, so that an uninitialised allocation of
    the same size that follows does not happen to hold zeros"""
    junk = [torch.full(s, 777.0, device=dev) for s in shapes for _ in range(8)]
    torch.cuda.synchronize()
    del junk


def _t(x, dev):
    return torch.from_numpy(np.array(x)).to(dev)  # a copy: the cached inputs are read-only


@functools.lru_cache(maxsize=None)
def _inputs(B, D, metric):
    """(a, p, n, ids) and the f64 / f32 distance matrices, computed once per shape"""
    rng = np.random.default_rng(B * 1009 + D * 31 + metric)
    a = rng.standard_normal((B, D)).astype(np.float32)
    p = (a + 0.7 * rng.standard_normal((B, D))).astype(np.float32)
    n = rng.standard_normal((B, D)).astype(np.float32)
    ids = np.arange(2 * B, dtype=np.int64)
    for _ in range(3):  # three planted collisions: candidate c carries anchor i's photo
        i, c = int(rng.integers(0, B)), int(rng.integers(0, 2 * B))
        ids[c] = ids[i]
    d64 = mref.distances(a, p, n, metric)
    d32 = mref.distances(a, p, n, metric, dtype=np.float32)
    for x in (a, p, n, ids, d64, d32):
        x.setflags(write=False)
    return a, p, n, ids, d64, d32


def _select(dev, a, p, n, mode, metric, ids=None):
    import losses
    sel, d_ap, d_sel = losses.select_negatives(_t(a, dev), _t(p, dev), _t(n, dev), MODES[mode], METRICS[metric],
                                               cand_ids=None if ids is None else _t(ids, dev))
    torch.cuda.synchronize()
    return sel.cpu().numpy(), d_ap.cpu().numpy(), d_sel.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _selection_case(B, D, metric):
    """runs the four (mode, ids) selections of one shape against f64; returns
    (anchors skipped as undecided, anchors)"""
    dev = torch.device("cuda:0")
    a, p, n, ids, d64, d32 = _inputs(B, D, metric)
    rows = np.arange(B)
    skipped = total = 0
    for mode in (0, 1):
        for use_ids in (False, True):
            cid = ids if use_ids else None
            tag = f"mine B={B} D={D} {METRICS[metric]} {MODES[mode]}{' ids' if use_ids else ''}"
            sel, d_ap, d_sel = _select(dev, a, p, n, mode, metric, cid)
            valid = mref.valid_mask(B, cid)
            want = mref.select(d64, valid, mode)
            dec = mref.decided(d64, valid, mode, D, metric)
            skipped += int((~dec).sum())
            total += B
            print(f"SELECT {tag:<52s} decided={int(dec.sum())}/{B} mismatches={int((sel[dec] != want[dec]).sum())}")
            assert sel.dtype == np.int64 and ((sel >= 0) & (sel < 2 * B)).all(), tag
            assert (sel[dec] == want[dec]).all(), (tag, np.flatnonzero(dec & (sel != want)))
            # whatever it selected is a valid candidate (or the fallback B + i)
            assert (valid[rows, sel] | (sel == B + rows)).all(), tag
            check_f32(f"{tag} d_ap", d_ap, d64[rows, rows], d32[rows, rows], quiet=True)
            check_f32(f"{tag} d_sel", d_sel, d64[rows, sel], d32[rows, sel], quiet=True)
    return skipped, total


@pytest.mark.parametrize("B,D,metric", SHAPES)
def test_selection_matches_f64_where_decided(B, D, metric, dev):
    _selection_case(B, D, metric)


def test_selection_skips_at_most_two_percent(dev):
    counts = [_selection_case(*s) for s in SHAPES]  # cached when the cases above ran in this process
    skipped, total = (sum(c[k] for c in counts) for k in (0, 1))
    print(f"SELECT skipped {skipped} of {total} anchors ({100.0 * skipped / total:.3f} %)")
    assert skipped <= 0.02 * total, (skipped, total)


# ------------------------------------------------------------ ties and boundaries
def _base(metric, B=37, D=64, seed=7):
    rng = np.random.default_rng(seed + metric)
    a = rng.standard_normal((B, D)).astype(np.float32)
    p = (a + 0.7 * rng.standard_normal((B, D))).astype(np.float32)
    n = rng.standard_normal((B, D)).astype(np.float32)
    delta = rng.standard_normal(D).astype(np.float32)
    return a, p, n, delta


@pytest.mark.parametrize("metric", (0, 1))
def test_bit_identical_candidates_tie_to_the_lowest(metric, dev):
    B, i, c1, c2 = 37, 5, 9, 37 + 20
    a, p, n, delta = _base(metric)
    p[c1] = n[c2 - B] = a[i] + np.float32(1e-3) * delta
    for mode in (0, 1):
        sel, d_ap, d_sel = _select(dev, a, p, n, mode, metric)
        if mode == 0:
            assert sel[i] == c1
            ids = np.arange(2 * B, dtype=np.int64)
            ids[c1] = ids[i]
            assert _select(dev, a, p, n, mode, metric, ids)[0][i] == c2
            # the same rows give the same bits wherever the candidate sits
            n2 = n.copy()
            n2[B - 1] = p[c1]
            sel2, _, d_sel2 = _select(dev, a, p, n2, mode, metric)
            assert sel2[i] == c1 and d_sel2[i].tobytes() == d_sel[i].tobytes()
            ids[c2] = ids[i]
            sel3, _, d_sel3 = _select(dev, a, p, n2, mode, metric, ids)
            assert sel3[i] == 2 * B - 1 and d_sel3[i].tobytes() == d_sel[i].tobytes()
        else:  # both lie far inside the positive's distance: semi-hard takes neither
            assert sel[i] not in (c1, c2) and d_sel[i] > d_ap[i]


@pytest.mark.parametrize("metric", (0, 1))
def test_copy_of_the_positive_is_hardest_but_never_semihard(metric, dev):
    B, i, c = 37, 5, 37 + 3
    a, p, n, _ = _base(metric)
    n[c - B] = p[i]
    sel, d_ap, d_sel = _select(dev, a, p, n, 0, metric)
    assert sel[i] == c and d_sel[i].tobytes() == d_ap[i].tobytes()
    sel, d_ap, d_sel = _select(dev, a, p, n, 1, metric)
    assert sel[i] != c and d_sel[i] > d_ap[i]  # strict >
    want = mref.mine(a, p, n, 1, metric)[0]
    assert sel[i] == want[i]


@pytest.mark.parametrize("metric", (0, 1))
@pytest.mark.parametrize("mode", (0, 1))
def test_smallest_batches_and_fallback(mode, metric, dev):
    rng = np.random.default_rng(11)
    a, p, n = (rng.standard_normal((1, 64)).astype(np.float32) for _ in range(3))
    assert _select(dev, a, p, n, mode, metric)[0].tolist() == [1]
    a, p, n = (rng.standard_normal((2, 64)).astype(np.float32) for _ in range(3))
    ids = np.full(4, 7, np.int64)  # every candidate shares the anchor's id
    sel, d_ap, d_sel = _select(dev, a, p, n, mode, metric, ids)
    assert sel.tolist() == [2, 3]
    d64 = mref.distances(a, p, n, metric)
    d32 = mref.distances(a, p, n, metric, dtype=np.float32)
    check_f32("fallback d_sel", d_sel, d64[[0, 1], [2, 3]], d32[[0, 1], [2, 3]])


@pytest.mark.parametrize("metric", (0, 1))
@pytest.mark.parametrize("mode", (0, 1))
def test_nan_rows_are_never_selected(mode, metric, dev):
    B, i, c = 37, 5, 37 + 20
    a, p, n, delta = _base(metric)
    n[c - B] = a[i] + np.float32(1e-3) * delta  # the nearest candidate of anchor i by far ...
    n[c - B, 17] = np.nan                        # ... but for a NaN
    a[30, 0] = np.nan                            # and an anchor none of whose distances compares
    sel, _, _ = _select(dev, a, p, n, mode, metric)
    assert c not in np.delete(sel, c - B).tolist()  # (anchor c - B could only meet it as its fallback)
    assert sel[30] == B + 30
    want = mref.mine(a, p, n, mode, metric)[0]
    assert sel[i] == want[i]


# ------------------------------------------------------------ gather and scatter
def _gather_scatter(dev, a, p, n, mode, metric, ids, tag):
    """n_mined = C[sel] exactly; dP, dN against f64 given the GPU's own sel; rows nobody
    selected exactly zero; two runs the same bytes"""
    import losses
    B, D = a.shape
    g = np.random.default_rng(B * 7 + D).standard_normal((B, D)).astype(np.float32)
    runs = []
    for _ in range(2):
        _dirty_allocator(dev, (B, D))
        lp, ln = _t(p, dev).requires_grad_(True), _t(n, dev).requires_grad_(True)
        la = _t(a, dev).requires_grad_(True)
        mined, sel = losses.mine_negatives(la, lp, ln, MODES[mode], METRICS[metric],
                                           cand_ids=None if ids is None else _t(ids, dev))
        assert not sel.requires_grad and mined.requires_grad
        _dirty_allocator(dev, (B, D))
        mined.backward(_t(g, dev))
        torch.cuda.synchronize()
        assert la.grad is None  # the selection has no gradient
        runs.append([t.detach().cpu().numpy() for t in (mined, sel, lp.grad, ln.grad)])
    mined, sel, dP, dN = runs[0]
    check_exact(f"{tag} n_mined", mined, np.concatenate([p, n])[sel])
    dP64, dN64 = mref.scatter(g, sel)
    dP32, dN32 = mref.scatter(g, sel, np.float32)
    check_f32(f"{tag} dP", dP, dP64, dP32, quiet=True)
    check_f32(f"{tag} dN", dN, dN64, dN32, quiet=True)
    unselected = np.setdiff1d(np.arange(2 * B), sel)
    assert (np.concatenate([dP, dN])[unselected] == 0).all(), tag
    for x, y in zip(runs[0], runs[1]):
        assert x.tobytes() == y.tobytes(), tag
    return sel


@pytest.mark.parametrize("B,D,metric", [s for s in SHAPES if s[2] == 0])
def test_gather_and_scatter(B, D, metric, dev):
    a, p, n, ids, _, _ = _inputs(B, D, metric)
    mode = (B + D) % 2
    _gather_scatter(dev, a, p, n, mode, metric, ids if D % 2 else None, f"mine B={B} D={D} {MODES[mode]}")


def test_scatter_when_every_anchor_selects_one_candidate(dev):
    B, D, c = 130, 65, 130 + 7
    rng = np.random.default_rng(3)
    base = rng.standard_normal(D).astype(np.float32)
    a = (base + 1e-3 * rng.standard_normal((B, D))).astype(np.float32)
    p = (a + 0.7 * rng.standard_normal((B, D))).astype(np.float32)
    n = (4.0 * rng.standard_normal((B, D))).astype(np.float32)
    n[c - B] = base
    sel = _gather_scatter(dev, a, p, n, 0, 0, None, "mine B=130 D=65 one candidate")
    assert (sel == c).all()


def test_real_size_case(dev):
    """B = 384, D = 512 (configuration C2), hardest with ids: selection and gather / scatter"""
    B, D, metric = 384, 512, 0
    a, p, n, ids, d64, d32 = _inputs(B, D, metric)
    sel, d_ap, d_sel = _select(dev, a, p, n, 0, metric, ids)
    valid = mref.valid_mask(B, ids)
    dec = mref.decided(d64, valid, 0, D, metric)
    want = mref.select(d64, valid, 0)
    assert (sel[dec] == want[dec]).all()
    rows = np.arange(B)
    check_f32("C2 d_ap", d_ap, d64[rows, rows], d32[rows, rows])
    check_f32("C2 d_sel", d_sel, d64[rows, sel], d32[rows, sel])
    got = _gather_scatter(dev, a, p, n, 0, metric, ids, "C2 hardest ids")
    assert (got == sel).all()


# ------------------------------------------------------------ composition
def _triplet_grads(a, p, m, margin, metric, dtype):
    """(per-row hinge argument, dP, dM) of mean(max(0, margin + d(a,p) - d(a,m))) in `dtype`"""
    a, p, m = (np.asarray(x, np.float32).astype(dtype) for x in (a, p, m))
    B = a.shape[0]
    eps = dtype(mref.EPS[metric])
    if metric == 0:
        up, um = a - p + eps, a - m + eps
        dap, dam = np.sqrt((up * up).sum(1)), np.sqrt((um * um).sum(1))
        gp, gm = -up / dap[:, None], um / dam[:, None]   # d d_ap / dp and -d d_am / dm
    else:
        def cos_grad(x, y):  # d (1 - cos(x, y)) / dy
            nx = np.maximum(np.sqrt((x * x).sum(1)), eps)[:, None]
            ny = np.maximum(np.sqrt((y * y).sum(1)), eps)[:, None]
            cos = (x * y).sum(1)[:, None] / (nx * ny)
            return 1 - cos[:, 0], -(x / (nx * ny) - cos * y / (ny * ny))
        dap, gp = cos_grad(a, p)
        dam, gm = cos_grad(a, m)
        gm = -gm
    h = dtype(margin) + dap - dam
    act = (h >= 0).astype(dtype)[:, None] / dtype(B)
    return h, gp * act, gm * act


@pytest.mark.parametrize("kind", ("euclidean", "cosine", "with_classification"))
def test_composition_with_the_losses(kind, dev):
    import losses
    import utils
    B, D, margin = 37, 64, 0.2
    metric = 1 if kind == "cosine" else 0
    rng = np.random.default_rng(21 + metric)
    a = rng.standard_normal((B, D)).astype(np.float32)
    # positives about as far as the hardest negative, so that the hinge is active in a mixed set of rows
    p = (a + (1.1 if metric == 0 else 1.7) * rng.standard_normal((B, D))).astype(np.float32)
    n = rng.standard_normal((B, D)).astype(np.float32)
    rest = []
    if kind == "euclidean":
        inner = losses.TripletMarginLoss(margin)
    elif kind == "cosine":
        inner = losses.TripletMarginWithDistanceLoss(distance_function=utils.cosine_distance, margin=margin)
    else:
        inner = utils.TripletMarginLoss_with_classification(margin=margin)
        rest = [_t(rng.standard_normal((B, 10)).astype(np.float32), dev) for _ in range(2)]
        rest.append(_t(rng.integers(0, 10, B).astype(np.int64), dev))
    mined_loss = losses.MinedNegatives(inner, "hardest", METRICS[metric])
    assert mined_loss.margin == margin

    la, lp, ln = (_t(x, dev).requires_grad_(True) for x in (a, p, n))
    loss = mined_loss(la, lp, ln, *rest)
    loss.backward()
    sel = _select(dev, a, p, n, 0, metric)[0]
    m = np.concatenate([p, n])[sel]
    ra, rp, rm = (_t(x, dev).requires_grad_(True) for x in (a, p, m))
    ref = inner(ra, rp, rm, *rest)
    ref.backward()
    torch.cuda.synchronize()
    assert loss.detach().cpu().numpy().tobytes() == ref.detach().cpu().numpy().tobytes()
    check_exact(f"{kind} dA", la.grad, ra.grad.cpu().numpy())

    h64, gp64, gm64 = _triplet_grads(a, p, m, margin, metric, np.float64)
    _, gp32, gm32 = _triplet_grads(a, p, m, margin, metric, np.float32)
    assert 0 < (h64 >= 0).sum() < B and np.abs(h64).min() > 1e-4  # a mixed set, no row on the hinge's edge
    s64, s32 = mref.scatter(gm64, sel), mref.scatter(gm32.astype(np.float32), sel, np.float32)
    check_f32(f"{kind} dP", lp.grad, gp64 + s64[0], gp32 + s32[0])
    check_f32(f"{kind} dN", ln.grad, s64[1], s32[1])
    frac = mined_loss.mined_fraction()
    assert frac == float((sel != B + np.arange(B)).mean()) and mined_loss.mined_fraction() == 0.0


@pytest.mark.parametrize("metric", (0, 1))
def test_hardest_hinge_is_never_below_the_given_negatives(metric, dev):
    B, D = 130, 65
    a, p, n, _, _, _ = _inputs(B, D, metric)
    _, d_ap, d_sel = _select(dev, a, p, n, 0, metric)
    # the given negative's distance by the same routine: with one id everywhere nothing qualifies
    sel_g, _, d_given = _select(dev, a, p, n, 0, metric, np.zeros(2 * B, np.int64))
    assert (sel_g == B + np.arange(B)).all()
    hinge = lambda d: np.maximum(np.float32(0.2) + d_ap - d, 0)  # noqa: E731
    assert (d_sel <= d_given).all() and (hinge(d_sel) >= hinge(d_given)).all()


def test_counters_follow_training_anchors_only(dev):
    import losses
    a, p, n, _, _, _ = _inputs(37, 64, 0)
    fn = losses.MinedNegatives(losses.TripletMarginLoss(0.2), "semihard")
    ta, tp, tn = (_t(x, dev) for x in (a, p, n))
    with torch.no_grad():
        fn(ta, tp, tn)
    assert fn.mined_fraction() == 0.0
    sel = _select(dev, a, p, n, 1, 0)[0]
    fn(ta, tp, tn)
    fn(ta, tp, tn)
    assert fn.mined_fraction() == float((sel != 37 + np.arange(37)).mean())


# ------------------------------------------------------------ CLI
TINY = ["--layers", "1,1,1,1", "--width", "16", "--resolution", "64", "--output_dim", "32", "-b", "4",
        "--synthetic_n", "40", "-e", "1"]


def test_train_cli_with_and_without_mining(tmp_path, dev, monkeypatch):
    import train
    monkeypatch.chdir(tmp_path)
    training, _ = train.main(TINY + ["--negatives", "hardest", "--no_save"])
    assert len(training["train_losses"]) == 1 and np.isfinite(training["train_losses"][0])
    assert len(training["mined_fraction"]) == 1 and 0.0 <= training["mined_fraction"][0] <= 1.0
    given, _ = train.main(TINY + ["--negatives", "given", "--no_save"])
    assert set(given) == {"train_losses", "test_losses", "itrain_losses", "itest_losses", "iteration_loss_frequency",
                          "iteration_test_size", "training_time"}
    assert set(training) == set(given) | {"mined_fraction"}
