"""The cross-batch memory on the GPU (csrc/xbm.hip, losses.CrossBatchMemory, the
memory= argument of losses.select_negatives / mine_negatives / MinedNegatives,
train.py --memory_size) against the float64 restatement of tests/_xbm_ref.py.

Selection: as tests/test_mining_gpu.py, an anchor is *decided* when the f64 reference
has gaps wider than the derived worst case of an f32 sum of D terms (_mining_ref.tol /
decided, over the pool's validity mask); decided anchors must match exactly, the others
are skipped, and the skipped share over all cases stays <= 2 % (the f64 reference alone
leaves out 58 of the 13 840 anchor decisions of the grid below, 0.42 %).  Distances and
gradients: the f32 bar of tests/_tail.py.  The ring, the gather and everything said to
be "the same bytes" is compared byte for byte."""
import functools

import numpy as np
import pytest
import torch

import _mining_ref as mref
import _xbm_ref as xref
from _mining_ref import check_exact, check_f32
from test_mining_gpu import METRICS, MODES, TINY, _dirty_allocator, _t, _triplet_grads

pytestmark = pytest.mark.gpu

BATCHES = (1, 5, 37, 130)
WIDTHS = (3, 64, 65, 512)
SIZES = (0, 1, 7, 300, 4096)
# one width per scan variant of xbm.hip: registers 8 columns a lane (D <= 512; 512 with no
# column test), 16 columns (D <= 1024; 1024 with no column test), the pointer form beyond
VARIANT_WIDTHS = (64, 512, 700, 1024, 1100)
SENT = -768.0


def _b(x):
    return x.detach().cpu().numpy().tobytes()


def _memory(dev, mem, mem_ids=None, count=None, head=0):
    """a CrossBatchMemory holding the given rows, ids and state"""
    import losses
    mem = np.asarray(mem, np.float32)
    M, D = mem.shape
    memory = losses.CrossBatchMemory(M, D, dev)
    memory.mem.copy_(_t(mem, dev))
    if mem_ids is not None:
        memory.mem_ids.copy_(_t(np.asarray(mem_ids, np.int64), dev))
    memory.mem_state.copy_(_t(np.array([head, M if count is None else count], np.int64), dev))
    return memory


def _select(dev, a, p, n, mode, metric, ids=None, memory=None):
    import losses
    sel, d_ap, d_sel = losses.select_negatives(_t(a, dev), _t(p, dev), _t(n, dev), MODES[mode], METRICS[metric],
                                               cand_ids=None if ids is None else _t(ids, dev), memory=memory)
    torch.cuda.synchronize()
    return sel.cpu().numpy(), d_ap.cpu().numpy(), d_sel.cpu().numpy()


def _pool_raw(dev, a, p, n, mode, metric, ids, mem, mem_ids, state, M):
    """artsbir_mine_pool itself (the module cannot express M = 0 or a NULL memory)"""
    import _hip
    B, D = a.shape
    ta, tp, tn = (_t(x, dev) for x in (a, p, n))
    tid = None if ids is None else _t(ids, dev)
    sel = torch.empty(B, dtype=torch.int64, device=dev)
    d_ap, d_sel = (torch.empty(B, dtype=torch.float32, device=dev) for _ in range(2))
    _hip.call("artsbir_mine_pool", metric, mode, _hip.ptr(ta), _hip.ptr(tp), _hip.ptr(tn), B, D,
              float(mref.EPS[metric]), _hip.ptr(tid), _hip.ptr(mem), _hip.ptr(mem_ids), _hip.ptr(state), M,
              _hip.ptr(sel), _hip.ptr(d_ap), _hip.ptr(d_sel), _hip.stream())
    torch.cuda.synchronize()
    return sel.cpu().numpy(), d_ap.cpu().numpy(), d_sel.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _inputs(B, D, metric, M):
    """(a, p, n, mem, ids [2B + M]) and the f64 / f32 distance matrices, computed once per shape"""
    rng = np.random.default_rng(B * 1009 + D * 31 + metric + 7919 * M)
    a = rng.standard_normal((B, D)).astype(np.float32)
    p = (a + 0.7 * rng.standard_normal((B, D))).astype(np.float32)
    n = rng.standard_normal((B, D)).astype(np.float32)
    mem = rng.standard_normal((M, D)).astype(np.float32)
    ids = np.arange(2 * B + M, dtype=np.int64)
    for _ in range(3):  # three planted collisions: candidate c carries anchor i's photo
        i, c = int(rng.integers(0, B)), int(rng.integers(0, 2 * B + M))
        ids[c] = ids[i]
    d64 = xref.distances(a, p, n, mem, metric)
    d32 = xref.distances(a, p, n, mem, metric, dtype=np.float32)
    for x in (a, p, n, mem, ids, d64, d32):
        x.setflags(write=False)
    return a, p, n, mem, ids, d64, d32


# ------------------------------------------------------------ 1. an empty memory is today's mining
@pytest.mark.parametrize("metric", (0, 1))
@pytest.mark.parametrize("D", WIDTHS)
@pytest.mark.parametrize("B", BATCHES)
def test_empty_memory_is_the_in_batch_mining(B, D, metric, dev):
    a, p, n, _, ids, _, _ = _inputs(B, D, metric, 0)
    # a ring of rows that would win every anchor (its own bits, or nearly), but count = 0
    rows = np.concatenate([a, a + np.float32(1e-3)])[:7] if B >= 4 else np.repeat(a, 7, 0)[:7]
    full = _memory(dev, rows, np.full(rows.shape[0], -1), count=0, head=3)
    state0 = torch.zeros(2, dtype=torch.int64, device=dev)
    for mode in (0, 1):
        for cid in (None, ids):
            want = _select(dev, a, p, n, mode, metric, cid)
            tag = f"B={B} D={D} {METRICS[metric]} {MODES[mode]}{' ids' if cid is not None else ''}"
            got = {
                "memory=None": _select(dev, a, p, n, mode, metric, cid, memory=None),
                "count=0": _select(dev, a, p, n, mode, metric, cid, memory=full),
                "M=0": _pool_raw(dev, a, p, n, mode, metric, cid, full.mem, full.mem_ids, state0, 0),
                "mem=NULL": _pool_raw(dev, a, p, n, mode, metric, cid, None, None, None, 7),
            }
            for form, out in got.items():
                for x, y, name in zip(out, want, ("sel", "d_ap", "d_sel")):
                    assert x.dtype == y.dtype and x.tobytes() == y.tobytes(), (tag, form, name)


# ------------------------------------------------------------ 2. selection against float64 where decided
def _check_selection(dev, tag, a, p, n, mem, ids, d64, d32, mode, metric, count=None, memory=None):
    """one selection against f64; returns (anchors skipped as undecided, anchors, sel)"""
    B, D = a.shape
    M = mem.shape[0]
    count = M if count is None else count
    cid, mid = (None, None) if ids is None else (ids[:2 * B], ids[2 * B:])
    if M == 0:
        sel, d_ap, d_sel = _pool_raw(dev, a, p, n, mode, metric, cid, None, None, None, 0)
    else:
        memory = memory if memory is not None else _memory(dev, mem, mid, count)
        sel, d_ap, d_sel = _select(dev, a, p, n, mode, metric, cid, memory)
    rows = np.arange(B)
    valid = xref.valid_mask(B, M, count, cid, mid)
    want = mref.select(d64, valid, mode)
    dec = mref.decided(d64, valid, mode, D, metric)
    print(f"SELECT {tag:<60s} decided={int(dec.sum())}/{B} mismatches={int((sel[dec] != want[dec]).sum())} "
          f"from the memory={int((sel >= 2 * B).sum())}")
    assert sel.dtype == np.int64 and ((sel >= 0) & (sel < 2 * B + M)).all(), tag
    assert (sel[dec] == want[dec]).all(), (tag, np.flatnonzero(dec & (sel != want)))
    # whatever it selected is a valid candidate (or the fallback B + i)
    assert (valid[rows, sel] | (sel == B + rows)).all(), tag
    # d_ap and d_sel of a call as one array: check_f32 is relative to the largest reference
    # value it is given, and the error of a key does not shrink with the key (1 - cos carries
    # a few ulp of 1 however small it is: _mining_ref.tol), so a lone d_ap of a one-anchor
    # batch has no scale of its own; with its d_sel it has the scale of the keys of the call
    check_f32(f"{tag} d_ap|d_sel", np.concatenate([d_ap, d_sel]), np.concatenate([d64[rows, rows], d64[rows, sel]]),
              np.concatenate([d32[rows, rows], d32[rows, sel]]), quiet=True)
    return int((~dec).sum()), B, sel


@functools.lru_cache(maxsize=None)
def _selection_case(B, D, metric, M):
    dev = torch.device("cuda:0")
    a, p, n, mem, ids, d64, d32 = _inputs(B, D, metric, M)
    memory = _memory(dev, mem, ids[2 * B:]) if M else None
    skipped = total = 0
    for mode in (0, 1):
        tag = f"pool B={B} D={D} M={M} {METRICS[metric]} {MODES[mode]} ids"
        s, t, _ = _check_selection(dev, tag, a, p, n, mem, ids, d64, d32, mode, metric, memory=memory)
        skipped, total = skipped + s, total + t
    return skipped, total


GRID = [(B, D, metric, M) for B in BATCHES for D in WIDTHS for metric in (0, 1) for M in SIZES]


@pytest.mark.parametrize("B,D,metric,M", GRID)
def test_selection_matches_f64_where_decided(B, D, metric, M, dev):
    _selection_case(B, D, metric, M)


def test_selection_skips_at_most_two_percent(dev):
    counts = [_selection_case(*s) for s in GRID]  # cached when the cases above ran in this process
    skipped, total = (sum(c[k] for c in counts) for k in (0, 1))
    print(f"SELECT skipped {skipped} of {total} anchors ({100.0 * skipped / total:.3f} %)")
    assert total == 13840 and skipped <= 0.02 * total, (skipped, total)


# ------------------------------------------------------------ 3. a partially filled ring
@pytest.mark.parametrize("fill", ("anchors", "nan"))
@pytest.mark.parametrize("metric", (0, 1))
def test_unfilled_slots_are_never_selected(metric, fill, dev):
    B, D, M = 37, 64, 40
    a, p, n, _, _, _, _ = _inputs(B, D, metric, 0)
    rng = np.random.default_rng(5 + metric)
    for count in (1, M - 1):
        mem = rng.standard_normal((M, D)).astype(np.float32)
        # beyond count: bit copies of the anchors (distance about eps: they would win) or NaN
        mem[count:] = np.resize(a, (M, D))[count:] if fill == "anchors" else np.nan
        d64 = xref.distances(a, p, n, mem[:count], metric)
        d32 = xref.distances(a, p, n, mem[:count], metric, dtype=np.float32)
        memory = _memory(dev, mem, None, count)
        for mode in (0, 1):
            tag = f"partial {fill} count={count} {METRICS[metric]} {MODES[mode]}"
            sel, d_ap, d_sel = _select(dev, a, p, n, mode, metric, None, memory)
            assert (sel < 2 * B + count).all(), tag
            valid = xref.valid_mask(B, count, count)
            dec = mref.decided(d64, valid, mode, D, metric)
            assert (sel[dec] == mref.select(d64, valid, mode)[dec]).all(), tag
            rows = np.arange(B)
            check_f32(f"{tag} d_sel", d_sel, d64[rows, sel], d32[rows, sel], quiet=True)


# ------------------------------------------------------------ 4. key bits, 5. ties
def _planted(metric, D, B=13, M=12, seed=7):
    """a batch and a full ring; delta: a direction to plant near rows along"""
    rng = np.random.default_rng(seed + metric + D)
    a = rng.standard_normal((B, D)).astype(np.float32)
    p = (a + 0.7 * rng.standard_normal((B, D))).astype(np.float32)
    n = rng.standard_normal((B, D)).astype(np.float32)
    mem = rng.standard_normal((M, D)).astype(np.float32)
    delta = rng.standard_normal(D).astype(np.float32)
    return a, p, n, mem, delta


@pytest.mark.parametrize("D", VARIANT_WIDTHS)
@pytest.mark.parametrize("metric", (0, 1))
def test_key_bits_are_those_of_the_in_batch_routine(metric, D, dev):
    """d_sel of a ring selection and of a batch selection, bit for bit the key
    select_negatives computes when that row is the anchor's given negative and one id
    everywhere forces the fallback"""
    B, M = 13, 12
    a, p, n, mem, delta = _planted(metric, D)
    mem[5] = a[2] + np.float32(1e-3) * delta   # anchor 2 selects slot 5
    mem[11] = a[12] + np.float32(1e-3) * delta  # anchor 12 (the ragged tile) selects slot 11
    n[4] = a[9] + np.float32(1e-3) * delta     # anchor 9 selects the batch row B + 4
    memory = _memory(dev, mem)
    sel, d_ap, d_sel = _select(dev, a, p, n, 0, metric, None, memory)
    assert sel[2] == 2 * B + 5 and sel[12] == 2 * B + 11 and sel[9] == B + 4
    assert ((sel >= 2 * B).sum() >= 2) and ((sel < 2 * B).sum() >= 1)
    rows = xref.gather(p, n, mem, sel)
    sel_g, d_ap_g, d_given = _select(dev, a, p, rows, 0, metric, np.zeros(2 * B, np.int64))
    assert (sel_g == B + np.arange(B)).all()
    assert d_sel.tobytes() == d_given.tobytes() and d_ap.tobytes() == d_ap_g.tobytes()


@pytest.mark.parametrize("D", VARIANT_WIDTHS)
@pytest.mark.parametrize("metric", (0, 1))
def test_ties_between_the_batch_and_the_ring(metric, D, dev):
    B, M, i = 13, 12, 5
    a, p, n, mem, delta = _planted(metric, D)
    near = a[i] + np.float32(1e-3) * delta
    # a ring row bit-identical to a batch candidate: the batch index wins, in P and in N
    for c in (9, B + 3):
        p2, n2, mem2 = p.copy(), n.copy(), mem.copy()
        (p2 if c < B else n2)[c % B] = near
        mem2[4] = mem2[8] = near
        memory = _memory(dev, mem2, np.arange(100, 100 + M))
        sel, d_ap, d_sel = _select(dev, a, p2, n2, 0, metric, None, memory)
        assert sel[i] == c, (c, sel[i])
        # with the batch row's id excluded: the lower of the two identical slots, and the same bits
        ids = np.arange(2 * B, dtype=np.int64)
        ids[c] = ids[i]
        sel2, _, d_sel2 = _select(dev, a, p2, n2, 0, metric, ids, memory)
        assert sel2[i] == 2 * B + 4 and d_sel2[i].tobytes() == d_sel[i].tobytes()
        # a ring row carrying the anchor's id is never selected: slot 4 out, slot 8 next; both out, neither
        memory.mem_ids[4] = int(ids[i])
        sel3, _, d_sel3 = _select(dev, a, p2, n2, 0, metric, ids, memory)
        assert sel3[i] == 2 * B + 8 and d_sel3[i].tobytes() == d_sel[i].tobytes()
        memory.mem_ids[8] = int(ids[i])
        sel4 = _select(dev, a, p2, n2, 0, metric, ids, memory)[0]
        assert sel4[i] not in (c, 2 * B + 4, 2 * B + 8)
        assert (sel4 == xref.mine(a, p2, n2, mem2, M, 0, metric, cand_ids=ids,
                                  mem_ids=memory.mem_ids.cpu().numpy())[0])[i]
        # without ids the slots' ids play no part
        assert _select(dev, a, p2, n2, 0, metric, None, memory)[0][i] == c
    # two identical ring rows and no batch copy: the lower slot
    mem2 = mem.copy()
    mem2[10] = mem2[3] = near
    sel = _select(dev, a, p, n, 0, metric, None, _memory(dev, mem2))[0]
    assert sel[i] == 2 * B + 3
    # both lie far inside the positive's distance: semi-hard takes neither
    sel, d_ap, d_sel = _select(dev, a, p, n, 1, metric, None, _memory(dev, mem2))
    assert sel[i] not in (2 * B + 3, 2 * B + 10) and d_sel[i] > d_ap[i]


@pytest.mark.parametrize("D", VARIANT_WIDTHS)
@pytest.mark.parametrize("metric", (0, 1))
def test_ring_copy_of_the_positive_is_hardest_but_never_semihard(metric, D, dev):
    """the scan's own key of the ring row equals d_ap bit for bit: were it one ulp above,
    the strict d > d_ap of semihard would select it"""
    B, M, i, j = 13, 12, 5, 7
    a, p, n, mem, _ = _planted(metric, D)
    p[i] = a[i] + np.float32(0.05) * (p[i] - a[i])  # a close positive: its copy is the hardest by far
    mem[j] = p[i]
    memory = _memory(dev, mem)
    sel, d_ap, d_sel = _select(dev, a, p, n, 0, metric, None, memory)
    assert sel[i] == 2 * B + j and d_sel[i].tobytes() == d_ap[i].tobytes()
    sel, d_ap, d_sel = _select(dev, a, p, n, 1, metric, None, memory)
    assert sel[i] != 2 * B + j and d_sel[i] > d_ap[i]  # strict >
    assert sel[i] == xref.mine(a, p, n, mem, M, 1, metric)[0][i]


@pytest.mark.parametrize("metric", (0, 1))
@pytest.mark.parametrize("mode", (0, 1))
def test_nan_ring_rows_are_never_selected(mode, metric, dev):
    B, M, D, i = 13, 12, 64, 5
    a, p, n, mem, delta = _planted(metric, D)
    mem[6] = a[i] + np.float32(1e-3) * delta  # the nearest candidate of anchor i by far ...
    mem[6, 17] = np.nan                        # ... but for a NaN
    mem[9] = np.nan
    sel = _select(dev, a, p, n, mode, metric, None, _memory(dev, mem))[0]
    assert 2 * B + 6 not in sel.tolist() and 2 * B + 9 not in sel.tolist()
    assert sel[i] == xref.mine(a, p, n, mem, M, mode, metric)[0][i]


# ------------------------------------------------------------ 6. the ring
def _guarded_memory(dev, M, D):
    """a CrossBatchMemory whose rows and ids are the head of larger blocks of sentinels"""
    import losses
    _dirty_allocator(dev, (M + 4, D), (M + 4,))
    memory = losses.CrossBatchMemory(M, D, dev)
    big = torch.full((M + 4, D), SENT, device=dev)
    big_ids = torch.full((M + 4,), -768, dtype=torch.int64, device=dev)
    big[:M], big_ids[:M] = memory.mem, memory.mem_ids
    memory.mem, memory.mem_ids = big[:M], big_ids[:M]
    return memory, big, big_ids


@pytest.mark.parametrize("M,D,B", [(64, 65, 5), (30, 3, 5), (7, 64, 5), (300, 512, 37), (1, 3, 1)])
def test_ring_follows_the_rule_byte_for_byte(M, D, B, dev):
    """R = 1, 2B < M, 2B not dividing M, 2B dividing M (M = 30) and 2B > M, with and without ids"""
    memory, big, big_ids = _guarded_memory(dev, M, D)
    ring = xref.Ring(M, D)
    rng = np.random.default_rng(M + D)
    assert _b(memory.mem_state) == ring.state().tobytes() and memory.filled() == 0
    calls = [1, 2 * B, 2 * B, 1, 2 * B, 2 * B, 2 * B, 3, 2 * B] + [2 * B] * (M // (2 * B) + 1 if M <= 64 else 2)
    for k, R in enumerate(calls):
        rows = rng.standard_normal((R, D)).astype(np.float32)
        ids = None if k % 3 == 2 else rng.integers(0, 1 << 40, R).astype(np.int64)
        memory.enqueue(_t(rows, dev), None if ids is None else _t(ids, dev))
        ring.enqueue(rows, ids)
        torch.cuda.synchronize()
        tag = (M, D, k, R)
        assert _b(memory.mem) == ring.mem.tobytes(), tag
        assert _b(memory.mem_ids) == ring.ids.tobytes(), tag
        assert _b(memory.mem_state) == ring.state().tobytes(), tag
        assert memory.filled() == ring.count, tag
        assert bool((big[M:] == SENT).all()) and bool((big_ids[M:] == -768).all()), tag
    assert ring.count == M and (2 * B < M) == (M in (64, 30, 300))
    memory.reset()
    ring.reset()
    assert _b(memory.mem_state) == ring.state().tobytes() == np.zeros(2, np.int64).tobytes() and memory.filled() == 0
    rows = rng.standard_normal((2, D)).astype(np.float32)
    memory.enqueue(_t(rows, dev))
    ring.enqueue(rows)
    assert _b(memory.mem) == ring.mem.tobytes() and _b(memory.mem_state) == ring.state().tobytes()
    assert _b(memory.mem_ids) == ring.ids.tobytes()


def test_a_step_mines_the_ring_as_it_was_before_its_own_rows(dev):
    """the enqueue follows the selection: a step never meets its own rows in the ring"""
    import losses
    B, D = 5, 64
    a, p, n, _, _, _, _ = _inputs(B, D, 0, 0)
    fn = losses.MinedNegatives(losses.TripletMarginLoss(0.2), "hardest", memory=losses.CrossBatchMemory(16, D, dev))
    ids = np.arange(2 * B, dtype=np.int64)
    ta, tp, tn = (_t(x, dev) for x in (a, p, n))
    fn(ta, tp, tn, cand_ids=_t(ids, dev))
    ring = xref.Ring(16, D)
    ring.enqueue(np.concatenate([p, n]), ids)
    assert _b(fn.memory.mem) == ring.mem.tobytes() and _b(fn.memory.mem_ids) == ring.ids.tobytes()
    assert _b(fn.memory.mem_state) == ring.state().tobytes()
    assert fn.memory_fraction() == 0.0  # the ring was empty when the step selected
    # the same batch again: its rows are in the ring now; the copy of an anchor's own positive
    # carries the anchor's id, every other copy loses its tie against the batch row
    fn(ta, tp, tn, cand_ids=_t(ids, dev))
    assert fn.memory_fraction() == 0.0 and fn.memory.filled() == 16
    ring.enqueue(np.concatenate([p, n]), ids)
    assert _b(fn.memory.mem) == ring.mem.tobytes() and _b(fn.memory.mem_ids) == ring.ids.tobytes()


# ------------------------------------------------------------ 7. gather and scatter
def test_rows_gather3_is_exact_and_nan_outside_the_range(dev):
    import _hip
    B, D, M = 5, 65, 7
    a, p, n, mem, delta = _planted(0, D, B, M)
    sel = np.array([0, 2 * B - 1, 2 * B, 2 * B + M - 1, B], np.int64)
    tp, tn, tm = (_t(x, dev) for x in (p, n, mem))

    def gather(sel):
        _dirty_allocator(dev, (B, D))
        out = torch.empty(B, D, device=dev)
        _hip.call("artsbir_rows_gather3", _hip.ptr(tp), _hip.ptr(tn), _hip.ptr(tm), _hip.ptr(_t(sel, dev)), B, D, M,
                  _hip.ptr(out), _hip.stream())
        torch.cuda.synchronize()
        return out.cpu().numpy()

    assert gather(sel).tobytes() == xref.gather(p, n, mem, sel).tobytes()
    bad = sel.copy()
    bad[1], bad[3] = -1, 2 * B + M
    out = gather(bad)
    assert np.isnan(out[[1, 3]]).all()
    assert out[[0, 2, 4]].tobytes() == xref.gather(p, n, mem, sel)[[0, 2, 4]].tobytes()


def _gather_scatter(dev, a, p, n, mem, mode, metric, tag):
    """n_mined exact; dP, dN against the restricted f64 scatter given the GPU's own sel;
    rows nobody selected exactly zero; two runs the same bytes"""
    import losses
    B, D = a.shape
    g = np.random.default_rng(B * 7 + D).standard_normal((B, D)).astype(np.float32)
    memory = _memory(dev, mem)
    runs = []
    for _ in range(2):
        _dirty_allocator(dev, (B, D))
        la, lp, ln = (_t(x, dev).requires_grad_(True) for x in (a, p, n))
        mined, sel = losses.mine_negatives(la, lp, ln, MODES[mode], METRICS[metric], memory=memory)
        assert not sel.requires_grad and mined.requires_grad
        _dirty_allocator(dev, (B, D))
        mined.backward(_t(g, dev))
        torch.cuda.synchronize()
        assert la.grad is None  # the selection has no gradient
        runs.append([t.detach().cpu().numpy() for t in (mined, sel, lp.grad, ln.grad)])
    mined, sel, dP, dN = runs[0]
    check_exact(f"{tag} n_mined", mined, xref.gather(p, n, mem, sel))
    dP64, dN64 = xref.scatter(g, sel)
    dP32, dN32 = xref.scatter(g, sel, np.float32)
    check_f32(f"{tag} dP", dP, dP64, dP32, quiet=True)
    check_f32(f"{tag} dN", dN, dN64, dN32, quiet=True)
    unselected = np.setdiff1d(np.arange(2 * B), sel)
    assert (np.concatenate([dP, dN])[unselected] == 0).all(), tag
    for x, y in zip(runs[0], runs[1]):
        assert x.tobytes() == y.tobytes(), tag
    return sel


@pytest.mark.parametrize("B,D,M", [(5, 3, 7), (37, 65, 40), (130, 512, 300)])
def test_gather_and_scatter_with_a_memory(B, D, M, dev):
    a, p, n, mem, _, _, _ = _inputs(B, D, 0, M)
    mem = mem.copy()
    rng = np.random.default_rng(B)
    # a third of the anchors meet a near copy of themselves in the ring, some slots serve two anchors
    for i in range(0, B, 3):
        mem[i % M] = a[i] + np.float32(1e-3) * rng.standard_normal(D).astype(np.float32)
    sel = _gather_scatter(dev, a, p, n, mem, (B + D) % 2, 0, f"pool B={B} D={D} M={M}")
    assert (sel >= 2 * B).any() and (sel < 2 * B).any()


def test_scatter_when_every_anchor_selects_a_ring_slot(dev):
    B, D = 37, 65
    a, p, n, _, _, _, _ = _inputs(B, D, 0, 0)
    mem = (a + np.float32(1e-4)).astype(np.float32)
    sel = _gather_scatter(dev, a, p, n, mem, 0, 0, "pool B=37 D=65 every anchor from the ring")
    assert (sel == 2 * B + np.arange(B)).all()  # so dP = dN = 0: checked as the unselected rows


# ------------------------------------------------------------ 8. composition
@pytest.mark.parametrize("kind", ("euclidean", "cosine", "with_classification"))
def test_composition_with_the_losses(kind, dev):
    import losses
    import utils
    B, D, M, margin = 37, 64, 100, 0.2
    metric = 1 if kind == "cosine" else 0
    rng = np.random.default_rng(21 + metric)

    def batch():
        a = rng.standard_normal((B, D)).astype(np.float32)
        p = (a + (1.1 if metric == 0 else 1.7) * rng.standard_normal((B, D))).astype(np.float32)
        return a, p, rng.standard_normal((B, D)).astype(np.float32)

    rest = []
    if kind == "euclidean":
        inner = losses.TripletMarginLoss(margin)
    elif kind == "cosine":
        inner = losses.TripletMarginWithDistanceLoss(distance_function=utils.cosine_distance, margin=margin)
    else:
        inner = utils.TripletMarginLoss_with_classification(margin=margin)
        rest = [_t(rng.standard_normal((B, 10)).astype(np.float32), dev) for _ in range(2)]
        rest.append(_t(rng.integers(0, 10, B).astype(np.int64), dev))
    memory = losses.CrossBatchMemory(M, D, dev)
    with_memory = losses.MinedNegatives(inner, "hardest", METRICS[metric], memory=memory)
    in_batch = losses.MinedNegatives(inner, "hardest", METRICS[metric])
    ids1 = np.arange(2 * B, dtype=np.int64)

    # step 1, on an empty ring: the loss bytes and dA of the wrapper without memory
    a1, p1, n1 = batch()
    grads = []
    for fn in (with_memory, in_batch):
        la, lp, ln = (_t(x, dev).requires_grad_(True) for x in (a1, p1, n1))
        loss = fn(la, lp, ln, *rest, cand_ids=_t(ids1, dev))
        loss.backward()
        grads.append((loss, la.grad, lp.grad, ln.grad))
    torch.cuda.synchronize()
    for x, y in zip(*grads):
        assert _b(x) == _b(y)
    assert with_memory.memory_fraction() == 0.0 and with_memory.mined_fraction() == in_batch.mined_fraction()
    ring = xref.Ring(M, D)
    ring.enqueue(np.concatenate([p1, n1]), ids1)
    assert _b(memory.mem) == ring.mem.tobytes() and _b(memory.mem_state) == ring.state().tobytes()

    # step 2: eight planted anchors lie next to a row of step 1, now in the ring
    a2, p2, n2 = batch()
    planted = np.arange(0, B, 5)
    for k, i in enumerate(planted):
        a2[i] = ring.mem[3 * k + 1] + np.float32(1e-2) * rng.standard_normal(D).astype(np.float32)
    ids2 = np.arange(1000, 1000 + 2 * B, dtype=np.int64)
    before = _memory(dev, ring.mem, ring.ids, ring.count, ring.head)
    sel = _select(dev, a2, p2, n2, 0, metric, ids2, before)[0]
    assert (sel[planted] == 2 * B + 3 * np.arange(planted.size) + 1).all()
    m = xref.gather(p2, n2, ring.mem, sel)
    la, lp, ln = (_t(x, dev).requires_grad_(True) for x in (a2, p2, n2))
    loss = with_memory(la, lp, ln, *rest, cand_ids=_t(ids2, dev))
    loss.backward()
    ra, rp, rm = (_t(x, dev).requires_grad_(True) for x in (a2, p2, m))
    ref = inner(ra, rp, rm, *rest)
    ref.backward()
    torch.cuda.synchronize()
    assert _b(loss) == _b(ref)
    check_exact(f"{kind} dA", la.grad, ra.grad.cpu().numpy())
    h64, gp64, gm64 = _triplet_grads(a2, p2, m, margin, metric, np.float64)
    _, gp32, gm32 = _triplet_grads(a2, p2, m, margin, metric, np.float32)
    assert 0 < (h64 >= 0).sum() and np.abs(h64).min() > 1e-4  # active rows, none on the hinge's edge
    s64, s32 = xref.scatter(gm64, sel), xref.scatter(gm32.astype(np.float32), sel, np.float32)
    check_f32(f"{kind} dP", lp.grad, gp64 + s64[0], gp32 + s32[0])
    check_f32(f"{kind} dN", ln.grad, s64[1], s32[1])
    assert with_memory.memory_fraction() == float((sel >= 2 * B).mean()) >= planted.size / B
    assert with_memory.memory_fraction() == 0.0
    ring.enqueue(np.concatenate([p2, n2]), ids2)
    assert _b(memory.mem) == ring.mem.tobytes() and _b(memory.mem_ids) == ring.ids.tobytes()
    assert _b(memory.mem_state) == ring.state().tobytes()

    # under no_grad the ring is neither read nor written: the in-batch outputs
    with torch.no_grad():
        got = with_memory(_t(a2, dev), _t(p2, dev), _t(n2, dev), *rest, cand_ids=_t(ids2, dev))
        want = in_batch(_t(a2, dev), _t(p2, dev), _t(n2, dev), *rest, cand_ids=_t(ids2, dev))
    torch.cuda.synchronize()
    assert _b(got) == _b(want)
    assert _b(memory.mem) == ring.mem.tobytes() and _b(memory.mem_ids) == ring.ids.tobytes()
    assert _b(memory.mem_state) == ring.state().tobytes()
    assert with_memory.memory_fraction() == 0.0


# ------------------------------------------------------------ 9. kernel boundaries
@pytest.mark.parametrize("M", (3, 300))
@pytest.mark.parametrize("D", (511, 512, 513, 1023, 1024, 1025))
def test_kernel_boundaries(D, M, dev):
    """one width below and above each register-resident variant (512 | 513 changes the
    columns per lane, 1024 | 1025 goes to the pointer form), B = 13 not a multiple of the 8
    anchors of a wave, M = 3 smaller than the scanning workgroups of any variant"""
    B = 13
    for metric in (0, 1):
        a, p, n, mem, ids, d64, d32 = _inputs(B, D, metric, M)
        for mode in (0, 1):
            tag = f"edge B={B} D={D} M={M} {METRICS[metric]} {MODES[mode]} ids"
            sel = _check_selection(dev, tag, a, p, n, mem, ids, d64, d32, mode, metric)[2]
            if mode == 0 and metric == 0 and M == 300:
                assert (sel >= 2 * B).any()  # 300 random rows against 26: the ring does win anchors


def test_real_size_case(dev):
    """B = 384, D = 512 (configuration C2), M = 4096, hardest with ids"""
    B, D, M, metric = 384, 512, 4096, 0
    a, p, n, mem, ids, d64, d32 = _inputs(B, D, metric, M)
    sel = _check_selection(dev, "C2 hardest ids M=4096", a, p, n, mem, ids, d64, d32, 0, metric)[2]
    assert (sel >= 2 * B).sum() > B // 2  # 4096 of the 4864 candidates are rows of the ring


# ------------------------------------------------------------ 10. CLI
def test_train_cli_with_and_without_the_memory(tmp_path, dev, monkeypatch):
    import train
    monkeypatch.chdir(tmp_path)
    training, _ = train.main(TINY + ["--negatives", "hardest", "--memory_size", "16", "--no_save"])
    assert len(training["train_losses"]) == 1 and np.isfinite(training["train_losses"][0])
    assert len(training["memory_fraction"]) == 1 and 0.0 <= training["memory_fraction"][0] <= 1.0
    assert len(training["mined_fraction"]) == 1 and 0.0 <= training["mined_fraction"][0] <= 1.0
    mined, _ = train.main(TINY + ["--negatives", "hardest", "--no_save"])
    assert set(mined) == {"train_losses", "test_losses", "itrain_losses", "itest_losses", "iteration_loss_frequency",
                          "iteration_test_size", "training_time", "mined_fraction"}
    assert set(training) == set(mined) | {"memory_fraction"}
    with pytest.raises(SystemExit, match="--memory_size needs"):
        train.main(TINY + ["--memory_size", "16", "--no_save"])
