"""artsbir_info_nce / losses.info_nce / losses.InfoNCELoss / train.py --negatives all on the
GPU against the float64 restatement tests/_infonce_ref.py.

rows, q, da, dp, dn take tests/_tail.check_f32: e_hip <= max(8 e_f32, 8 * 2^-24) with e_f32
the error of the f32 restatement of the same stable formulas.  The scalar loss is held to
  |loss - mean64(kernel rows)| <= B * 2^-24 * mean|rows|       (any f32 summation order of
                                                                B terms, derived)
  |loss - ref64| <= (bar measured for rows) * max|rows_ref| + the first bound.
The grid is every (B, D) pair of BS x DS with M walking its list along both
axes (a Latin square: every M meets every B and every D, not the full B x D x M product),
plus two corners the square misses; each case with and without ids and with sigma 3 and 0.7.
profiles/infonce_parity.txt is the PARITY table of this file as measured on an MI355X."""
import json

import numpy as np
import pytest
import torch

import _infonce_ref as nref
import _xbm_ref as xref
from _tail import SENT, U32, check_f32, f64, tail_intact

pytestmark = pytest.mark.gpu
TAIL = 64
NAMES = ("loss", "rows", "q", "da", "dp", "dn")


def _dirty_allocator(dev, *shapes):
    """fill and free blocks of the given shapes, so that an uninitialised allocation of the
    same size that follows does not happen to hold zeros"""
    junk = [torch.full(s, 777.0, device=dev) for s in shapes for _ in range(8)]
    torch.cuda.synchronize()
    del junk


def make(B, D, M, sigma, seed, ids=False, count=None, hard=3):
    """a, n, mem ~ N(0, 1), p = a + sigma * noise, a few ring rows planted next to anchors
    (hard negatives), and with ids three planted collisions, one of them in the ring"""
    rng = np.random.default_rng(seed)
    a = rng.standard_normal((B, D)).astype(np.float32)
    n = rng.standard_normal((B, D)).astype(np.float32)
    p = (a + sigma * rng.standard_normal((B, D))).astype(np.float32)
    mem = rng.standard_normal((M, D)).astype(np.float32)
    count = M if count is None else count
    filled = min(count, M)
    for k in range(min(hard, filled)):
        j = int(rng.integers(filled))
        mem[j] = a[k % B] + 0.1 * rng.standard_normal(D).astype(np.float32)
    case = dict(a=a, p=p, n=n, mem=mem, count=count, cand_ids=None, mem_ids=None)
    if ids:
        cand = np.arange(100, 100 + 2 * B, dtype=np.int64)  # all distinct ...
        mids = np.arange(10_000, 10_000 + M, dtype=np.int64)
        cand[B + (B - 1)] = cand[0]            # ... but n[B-1] is anchor 0's photo,
        if B > 1:
            cand[1] = cand[B - 1]              # p[1] is anchor B-1's (and so anchor 1's id changes),
        if filled:
            mids[filled // 2] = cand[B // 2]   # and a filled slot is anchor B/2's
        elif B > 2:
            cand[B + 1] = cand[2]
        case.update(cand_ids=cand, mem_ids=mids)
    return case


def ref_pair(case, tau):
    kw = dict(temperature=tau, cand_ids=case["cand_ids"], mem=case["mem"], mem_ids=case["mem_ids"], count=case["count"])
    return (nref.info_nce(case["a"], case["p"], case["n"], dtype=np.float64, **kw),
            nref.info_nce(case["a"], case["p"], case["n"], dtype=np.float32, **kw))


def _dev(x, dev, dtype):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(dev).to(dtype)


def run_raw(case, tau, dev, grad=True, ring="given", head=0, eps=1e-8, shift=0):
    """one artsbir_info_nce call into sentinel-tailed buffers -> dict of flat tensors (with
    their tails) and the sizes of the live parts.  ring: 'given' | 'null' (mem NULL, M as
    given) | 'm0' (M = 0 with the pointers given); shift: the rows of a, p, n and mem start that
    many floats into their allocations (1: no 16-byte alignment)"""
    import _hip

    def rows(x):
        t = _dev(x, dev, torch.float32)
        if not shift:
            return t
        buf = torch.empty(t.numel() + shift, dtype=torch.float32, device=dev)
        buf[shift:] = t.reshape(-1)
        view = buf[shift:].reshape(t.shape)
        assert view.data_ptr() % 16 == (4 * shift) % 16 and view.is_contiguous()
        return view

    a, p, n = (rows(case[k]) for k in ("a", "p", "n"))
    B, D = a.shape
    M = case["mem"].shape[0]
    ids = _dev(case["cand_ids"], dev, torch.int64)
    mem = mem_ids = state = None
    if M:
        mem = rows(case["mem"])
        mem_ids = _dev(case["mem_ids"] if case["mem_ids"] is not None else np.full(M, -1, np.int64), dev, torch.int64)
        state = torch.tensor([head, case["count"]], dtype=torch.int64, device=dev)
    Mc = M
    if ring == "null":
        mem = None
    elif ring == "m0":
        Mc = 0
    nbytes = _hip.lib().artsbir_info_nce_workspace(B, D, Mc, int(grad))
    assert nbytes > 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    sizes = dict(loss=1, rows=B, q=B, da=B * D, dp=B * D, dn=B * D)
    out = {k: torch.full((sizes[k] + TAIL,), SENT, dtype=torch.float32, device=dev) for k in NAMES}
    g = [out[k] if grad else None for k in ("da", "dp", "dn")]
    _hip.call("artsbir_info_nce", _hip.ptr(a), _hip.ptr(p), _hip.ptr(n), B, D, 1.0 / tau, eps, _hip.ptr(ids),
              _hip.ptr(mem), _hip.ptr(mem_ids), _hip.ptr(state), Mc, _hip.ptr(out["loss"]), _hip.ptr(out["rows"]),
              _hip.ptr(out["q"]), _hip.ptr(g[0]), _hip.ptr(g[1]), _hip.ptr(g[2]), _hip.ptr(ws), nbytes, _hip.stream())
    torch.cuda.synchronize()
    for k in NAMES:
        if grad or k in ("loss", "rows", "q"):
            assert tail_intact(out[k], sizes[k]), k
        else:
            assert bool((out[k] == SENT).all()), k  # no gradient asked: nothing written
    return out, sizes


def live(out, sizes, k, shape=None):
    v = out[k][:sizes[k]]
    return v.reshape(shape) if shape else v


def check_all(tag, out, sizes, r64, r32, B, D, skip_rows=None):
    """the five outputs to the f32 bar, then the two bounds of the scalar loss"""
    e_rows = check_f32(f"{tag} rows", live(out, sizes, "rows"), r64["rows"], r32["rows"])
    check_f32(f"{tag} q", live(out, sizes, "q"), r64["q"], r32["q"])
    for k in ("da", "dp", "dn"):
        hip, want, f32 = f64(live(out, sizes, k, (B, D))), r64[k], f64(r32[k])
        if skip_rows and k in skip_rows:
            keep = np.ones(B, bool)
            keep[skip_rows[k]] = False
            hip, want, f32 = hip[keep], want[keep], f32[keep]
        check_f32(f"{tag} {k}", hip, want, f32)
    rows_hip = f64(live(out, sizes, "rows"))
    loss = float(out["loss"][0])
    first = B * U32 * float(np.abs(rows_hip).mean())
    d1 = abs(loss - float(rows_hip.mean()))
    bar_rows = max(8 * e_rows[1], 8 * U32)
    second = bar_rows * float(np.abs(r64["rows"]).max()) + first
    d2 = abs(loss - float(r64["loss"]))
    print(f"PARITY {tag + ' loss':<58s} f32  |loss-mean64(rows)|={d1:.3e} bound={first:.3e}  "
          f"|loss-ref64|={d2:.3e} bound={second:.3e}  loss={loss:.6g}")
    assert d1 <= first, (tag, d1, first)
    assert d2 <= second, (tag, d2, second)


BS, DS, MS = (1, 2, 5, 37, 130), (1, 3, 64, 65, 512, 1024), (0, 1, 7, 300, 4096)
# every (B, D) pair; M walks its list along both axes, so every M meets every B and every D
GRID = [(B, D, MS[(ib + idd) % len(MS)]) for ib, B in enumerate(BS) for idd, D in enumerate(DS)]
GRID += [c for c in [(1, 1024, 4096), (37, 65, 300)] if c not in GRID]


@pytest.mark.parametrize("sigma", [3.0, 0.7])
@pytest.mark.parametrize("ids", [False, True])
@pytest.mark.parametrize("B,D,M", GRID)
def test_parity_grid(B, D, M, ids, sigma, dev):
    case = make(B, D, M, sigma, seed=B * 7919 + D * 31 + M, ids=ids)
    r64, r32 = ref_pair(case, 0.07)
    out, sizes = run_raw(case, 0.07, dev)
    check_all(f"B{B} D{D} M{M} ids{int(ids)} s{sigma}", out, sizes, r64, r32, B, D)


@pytest.mark.parametrize("B,D,M", [(130, 1024, 4096), (37, 512, 300)])
def test_parity_low_temperature(B, D, M, dev):
    case = make(B, D, M, 3.0, seed=11 + B, ids=True)
    r64, r32 = ref_pair(case, 0.02)
    out, sizes = run_raw(case, 0.02, dev)
    check_all(f"B{B} D{D} M{M} tau0.02", out, sizes, r64, r32, B, D)


def test_every_candidate_is_the_anchors_photo(dev):
    case = make(37, 64, 300, 3.0, seed=3)
    case.update(cand_ids=np.full(74, 5, np.int64), mem_ids=np.full(300, 5, np.int64))
    out, sizes = run_raw(case, 0.07, dev)
    for k in NAMES:
        assert bool((live(out, sizes, k) == 0).all()), k


def test_one_anchor_alone_without_a_negative(dev):
    """p[c] carries anchor c's id, so an anchor whose every candidate is masked shares its
    id with every other anchor: among several anchors none can lack a negative alone.  The
    case is the batch of one anchor whose n[0] and whose ring are its own photo."""
    case = make(1, 64, 7, 3.0, seed=4)
    case.update(cand_ids=np.array([3, 3], np.int64), mem_ids=np.full(7, 3, np.int64))
    out, sizes = run_raw(case, 0.07, dev)
    for k in NAMES:
        assert bool((live(out, sizes, k) == 0).all()), k
    # one slot of another photo: that slot is the only negative
    case["mem_ids"][5] = 4
    r64, r32 = ref_pair(case, 0.07)
    assert r64["rows"][0] > 0
    out, sizes = run_raw(case, 0.07, dev)
    check_all("B1 M7: one slot the only negative", out, sizes, r64, r32, 1, 64)


def test_single_anchor_single_negative(dev):
    case = make(1, 64, 0, 3.0, seed=5)
    r64, r32 = ref_pair(case, 0.07)
    out, sizes = run_raw(case, 0.07, dev)
    check_all("B1 M0: n[0] the only negative", out, sizes, r64, r32, 1, 64)


def test_zero_row_in_p(dev):
    B, D = 37, 64
    case = make(B, D, 300, 3.0, seed=6)
    case["p"][4] = 0
    r64, r32 = ref_pair(case, 0.07)
    out, sizes = run_raw(case, 0.07, dev)
    check_all("zero row in p", out, sizes, r64, r32, B, D, skip_rows={"dp": [4]})
    assert bool(torch.isfinite(live(out, sizes, "dp")).all())


def test_identical_rows_at_low_temperature_are_finite(dev):
    B, D = 37, 64
    row = np.random.default_rng(7).standard_normal(D).astype(np.float32)
    case = dict(a=np.tile(row, (B, 1)), p=np.tile(row, (B, 1)), n=np.tile(row, (B, 1)), mem=np.tile(row, (300, 1)),
                count=300, cand_ids=None, mem_ids=None)
    out, sizes = run_raw(case, 0.01, dev)
    for k in NAMES:
        assert bool(torch.isfinite(live(out, sizes, k)).all()), k
    r64, r32 = ref_pair(case, 0.01)
    check_f32("identical rows tau0.01 rows", live(out, sizes, "rows"), r64["rows"], r32["rows"])


def test_unfilled_slots_hold_nan(dev):
    B, D, M, count = 37, 64, 4096, 4001
    case = make(B, D, M, 3.0, seed=8, ids=True, count=count)
    case["mem"][count:] = np.nan
    r64, r32 = ref_pair(case, 0.07)
    out, sizes = run_raw(case, 0.07, dev)
    check_all("count 4001 of 4096, NaN beyond", out, sizes, r64, r32, B, D)


def test_wrapped_ring_uses_every_slot(dev):
    B, D, M = 37, 64, 300
    case = make(B, D, M, 3.0, seed=9, ids=True, count=M + 500)  # count > M: the state's word, as it stands
    r64, r32 = ref_pair(case, 0.07)
    out, sizes = run_raw(case, 0.07, dev, head=123)
    check_all("head 123, count > M", out, sizes, r64, r32, B, D)
    part = dict(case, count=M - 1)
    assert abs(ref_pair(part, 0.07)[0]["loss"] - r64["loss"]) > 0  # the last slot carries weight


def test_no_ring_in_four_spellings_gives_the_same_bytes(dev):
    import losses
    B, D = 37, 64
    base = make(B, D, 0, 3.0, seed=10, ids=True)
    ring = make(B, D, 300, 3.0, seed=10, ids=True, count=0)
    ring.update(a=base["a"], p=base["p"], n=base["n"], cand_ids=base["cand_ids"])
    want, sizes = run_raw(base, 0.07, dev)
    for spelling, kw in (("count 0", dict()), ("mem NULL", dict(ring="null")), ("M 0", dict(ring="m0"))):
        got, _ = run_raw(ring, 0.07, dev, **kw)
        for k in NAMES:
            assert torch.equal(live(want, sizes, k).view(torch.int32), live(got, sizes, k).view(torch.int32)), (spelling, k)
    # and memory=None of the Python surface
    leaves = [torch.from_numpy(base[k]).to(dev).requires_grad_(True) for k in ("a", "p", "n")]
    loss = losses.info_nce(*leaves, cand_ids=torch.from_numpy(base["cand_ids"]).to(dev))
    loss.backward()
    assert torch.equal(loss.detach().reshape(1), live(want, sizes, "loss"))
    for leaf, k in zip(leaves, ("da", "dp", "dn")):
        assert torch.equal(leaf.grad, live(want, sizes, k, (B, D))), k


@pytest.mark.parametrize("B,D,M", [(37, 64, 300), (130, 1024, 4096), (5, 65, 7)])
def test_two_runs_give_the_same_bytes(B, D, M, dev):
    case = make(B, D, M, 3.0, seed=12, ids=True)
    first, sizes = run_raw(case, 0.07, dev)
    first = {k: v.clone() for k, v in first.items()}
    _dirty_allocator(dev, (B * D + TAIL,), (B + TAIL,), (1 + TAIL,))
    import _hip
    nbytes = _hip.lib().artsbir_info_nce_workspace(B, D, M, 1)
    junk = [torch.full((nbytes,), 0xAB, dtype=torch.uint8, device=dev) for _ in range(4)]  # the workspace's block too
    torch.cuda.synchronize()
    del junk
    second, _ = run_raw(case, 0.07, dev)
    for k in NAMES:
        assert torch.equal(first[k].view(torch.int32), second[k].view(torch.int32)), k


@pytest.mark.parametrize("B,D,M", [(37, 64, 300), (5, 1024, 7)])
def test_unaligned_rows_give_the_same_bytes(B, D, M, dev):
    """D % 4 == 0 takes 16-byte loads only when every base pointer allows them; rows that
    start one float into their allocation take the scalar loads and give the same bytes"""
    case = make(B, D, M, 3.0, seed=14, ids=True)
    want, sizes = run_raw(case, 0.07, dev)
    got, _ = run_raw(case, 0.07, dev, shift=1)
    for k in NAMES:
        assert torch.equal(live(want, sizes, k).view(torch.int32), live(got, sizes, k).view(torch.int32)), k
    r64, r32 = ref_pair(case, 0.07)
    check_all(f"B{B} D{D} M{M} rows one float off alignment", got, sizes, r64, r32, B, D)


def test_forward_only_writes_no_gradient(dev):
    case = make(37, 64, 300, 3.0, seed=13)
    full, sizes = run_raw(case, 0.07, dev)
    fwd, _ = run_raw(case, 0.07, dev, grad=False)
    for k in ("loss", "rows", "q"):
        assert torch.equal(live(full, sizes, k), live(fwd, sizes, k)), k


# ------------------------------------------------------------------ module
def _module_case(dev, B=37, D=64, seed=20):
    case = make(B, D, 0, 3.0, seed=seed, ids=True)
    t = {k: torch.from_numpy(case[k]).to(dev) for k in ("a", "p", "n")}
    return case, t, torch.from_numpy(case["cand_ids"]).to(dev)


def test_module_backward_scales_the_saved_gradients(dev):
    import losses
    B, D = 37, 64
    case, t, ids = _module_case(dev)
    want, sizes = run_raw(case, 0.07, dev)
    leaves = [t[k].clone().requires_grad_(True) for k in ("a", "p", "n")]
    loss_fn = losses.InfoNCELoss()
    assert loss_fn.margin is None and loss_fn.temperature == 0.07
    (2.5 * loss_fn(*leaves, cand_ids=ids)).backward()
    for leaf, k in zip(leaves, ("da", "dp", "dn")):
        assert torch.equal(leaf.grad, 2.5 * live(want, sizes, k, (B, D))), k


def test_module_ring_rules(dev):
    import losses
    B, D, M = 37, 64, 100
    case1, t1, ids1 = _module_case(dev, seed=21)
    case2, t2, ids2 = _module_case(dev, seed=22)
    memory = losses.CrossBatchMemory(M, D, device=dev)
    loss_fn = losses.InfoNCELoss(0.07, memory=memory)
    # under no_grad the ring is neither read nor written
    before = [x.clone() for x in (memory.mem, memory.mem_ids, memory.mem_state)]
    with torch.no_grad():
        l0 = loss_fn(t1["a"], t1["p"], t1["n"], cand_ids=ids1)
    for x, y in zip(before, (memory.mem, memory.mem_ids, memory.mem_state)):
        assert torch.equal(x, y)
    assert loss_fn.positive_probability() == 0.0  # nothing seen with gradients enabled
    # step 1 with gradients: the empty ring adds nothing, then [p; n] is enqueued
    leaves = [t1[k].clone().requires_grad_(True) for k in ("a", "p", "n")]
    l1 = loss_fn(*leaves, cand_ids=ids1)
    assert torch.equal(l1.detach(), l0)
    ring = xref.Ring(M, D)
    ring.enqueue(np.concatenate([case1["p"], case1["n"]]), ids=case1["cand_ids"])
    assert torch.equal(memory.mem.cpu(), torch.from_numpy(ring.mem))
    assert memory.mem_ids.cpu().tolist() == ring.ids.tolist() and memory.mem_state.cpu().tolist() == ring.state().tolist()
    q1 = nref.info_nce(case1["a"], case1["p"], case1["n"], cand_ids=case1["cand_ids"])["q"]
    q1_32 = nref.info_nce(case1["a"], case1["p"], case1["n"], cand_ids=case1["cand_ids"], dtype=np.float32)["q"]
    # step 2 sees step 1's rows and not its own
    leaves2 = [t2[k].clone().requires_grad_(True) for k in ("a", "p", "n")]
    l2 = loss_fn(*leaves2, cand_ids=ids2)
    kw = dict(cand_ids=case2["cand_ids"], mem=ring.mem, mem_ids=ring.ids, count=ring.count)
    r64 = nref.info_nce(case2["a"], case2["p"], case2["n"], **kw)
    r32 = nref.info_nce(case2["a"], case2["p"], case2["n"], dtype=np.float32, **kw)
    raw, sizes = run_raw(dict(case2, mem=ring.mem.copy(), mem_ids=ring.ids.copy(), count=ring.count), 0.07, dev)
    assert torch.equal(l2.detach().reshape(1), live(raw, sizes, "loss"))  # (the raw call's parity: the tests above)
    check_f32("module step 2 rows (raw call on the ring's copy)", live(raw, sizes, "rows"), r64["rows"], r32["rows"])
    ring.enqueue(np.concatenate([case2["p"], case2["n"]]), ids=case2["cand_ids"])
    own = nref.info_nce(case2["a"], case2["p"], case2["n"], cand_ids=case2["cand_ids"], mem=ring.mem, mem_ids=ring.ids,
                        count=ring.count)
    assert abs(own["loss"] - r64["loss"]) > 1e-3 * abs(r64["loss"])  # its own rows in the ring would show
    assert torch.equal(memory.mem.cpu(), torch.from_numpy(ring.mem)) and memory.mem_state.cpu().tolist() == [48, 100]
    l2.backward()
    for leaf, k in zip(leaves2, ("da", "dp", "dn")):  # the gradients of the ring the forward saw, not of the ring now
        assert torch.equal(leaf.grad, live(raw, sizes, k, (B, D))), k
    # the probability of the positive over the two steps seen with gradients, then reset
    want = float(np.concatenate([1 - q1, 1 - r64["q"]]).mean())
    got = loss_fn.positive_probability()
    # a mean of values each within the f32 bar of q is within that bar
    qs, qs32 = np.concatenate([q1, r64["q"]]), np.concatenate([q1_32, r32["q"]]).astype(np.float64)
    bar = max(8 * float(np.abs(qs32 - qs).max()) / float(qs.max()), 8 * U32) * float(qs.max())
    assert abs(got - want) <= bar, (got, want, bar)
    assert loss_fn.positive_probability() == 0.0


def test_cpu_tensors_are_refused(dev):
    import losses
    a = torch.zeros(4, 8)
    with pytest.raises(RuntimeError, match="CUDA tensors"):
        losses.info_nce(a, a, a)
    with pytest.raises(RuntimeError, match="CUDA tensors"):
        losses.InfoNCELoss()(a, a, a)


# ------------------------------------------------------------------ end to end
TINY = ["--layers", "1,1,1,1", "--width", "16", "--resolution", "64", "--output_dim", "32", "-b", "4",
        "--synthetic_n", "40", "-e", "1"]


def test_train_cli_negatives_all(tmp_path, dev, monkeypatch):
    import train
    monkeypatch.chdir(tmp_path)
    training, inf = train.main(TINY + ["--negatives", "all", "--loss_type", "cosine", "--memory_size", "16",
                                       "--inference"])
    assert len(training["train_losses"]) == 1 and np.isfinite(training["train_losses"][0])
    assert len(training["positive_probability"]) == 1 and 0.0 <= training["positive_probability"][0] <= 1.0
    for key in ("mean_reciprocal_rank", "topk_acc", "map@10", "image_features"):
        assert key in inf, key
    res = list((tmp_path / "results").iterdir())
    params = json.loads((res[0] / "training_params.json").read_text())
    assert params["negatives"] == "all" and params["temperature"] == 0.07 and params["memory_size"] == 16
    assert params["loss_margin"] is None and params["loss_fn"] == "InfoNCELoss"


def test_encoder_step_under_info_nce(dev):
    import losses
    import models
    m = models.ModifiedResNet((1, 1, 1, 1), 32, heads=8, input_resolution=64, width=16).to(dev)
    m.train()
    outs = [m(torch.randn(4, 3, 64, 64, device=dev)) for _ in range(3)]
    loss = losses.InfoNCELoss(0.07, memory=losses.CrossBatchMemory(16, None))(*outs)
    loss.backward()
    assert torch.isfinite(loss) and m.conv1.weight.grad.abs().sum() > 0
