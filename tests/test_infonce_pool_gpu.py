"""artsbir_info_nce_pool on the GPU: the byte contract against artsbir_info_nce (cand = [p; n]
in one allocation, Nc = 2B, pos0 = 0 gives the same bytes), and parity against the float64
restatement tests/_infonce_pool_ref.py where Nc != 2B and pos0 != 0.

Every call goes into sentinel-tailed buffers with dcand prefilled with NaN (an unwritten row
shows), and is launched twice: the stored bytes must be equal.  rows, q, da, dcand take
tests/_tail.check_f32 (e_hip <= max(8 e_f32, 8 * 2^-24)) and the scalar loss the two derived
bounds of tests/test_infonce_gpu.py; no other tolerance.  The shapes are the smallest at which
the pool indexing can go wrong: tiles are 32 anchors x 64 candidates, the da^ variants sit at
D <= 256 / 512 / 1024, a dc^ block covers 256 columns.
profiles/infonce_pool_parity.txt is the PARITY table of this file as measured on an MI355X."""
import numpy as np
import pytest
import torch

import _infonce_pool_ref as pref
import test_infonce_gpu as tig
from _tail import SENT, U32, check_f32, f64, tail_intact

pytestmark = pytest.mark.gpu
TAIL = 64
NAMES = ("loss", "rows", "q", "da", "dcand")


def run_pool(case, tau, dev, grad=True, head=0, eps=1e-8, shift=0):
    """artsbir_info_nce_pool twice into fresh sentinel-tailed buffers (dcand's live part NaN);
    the two runs' bytes are compared here.  case: a [B, D], cand [Nc, D], pos0, cand_ids,
    mem [M, D], mem_ids, count.  shift: the rows of a, cand and mem start that many floats
    into their allocations.  -> dict of flat tensors and the sizes of their live parts"""
    import _hip

    def rows(x):
        t = tig._dev(x, dev, torch.float32)
        if not shift:
            return t
        buf = torch.empty(t.numel() + shift, dtype=torch.float32, device=dev)
        buf[shift:] = t.reshape(-1)
        return buf[shift:].reshape(t.shape)

    a, cand = rows(case["a"]), rows(case["cand"])
    (B, D), Nc, M = a.shape, cand.shape[0], case["mem"].shape[0]
    ids = tig._dev(case["cand_ids"], dev, torch.int64)
    mem = mem_ids = state = None
    if M:
        mem = rows(case["mem"])
        mem_ids = tig._dev(case["mem_ids"] if case["mem_ids"] is not None else np.full(M, -1, np.int64), dev, torch.int64)
        state = torch.tensor([head, case["count"]], dtype=torch.int64, device=dev)
    nbytes = _hip.lib().artsbir_info_nce_pool_workspace(B, Nc, D, M, int(grad))
    assert nbytes > 0
    sizes = dict(loss=1, rows=B, q=B, da=B * D, dcand=Nc * D)
    runs = []
    for _ in range(2):
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        out = {k: torch.full((sizes[k] + TAIL,), SENT, dtype=torch.float32, device=dev) for k in NAMES}
        if grad:
            out["dcand"][:sizes["dcand"]] = float("nan")
        g = [out[k] if grad else None for k in ("da", "dcand")]
        _hip.call("artsbir_info_nce_pool", _hip.ptr(a), _hip.ptr(cand), B, Nc, int(case["pos0"]), D, 1.0 / tau, eps,
                  _hip.ptr(ids), _hip.ptr(mem), _hip.ptr(mem_ids), _hip.ptr(state), M, _hip.ptr(out["loss"]),
                  _hip.ptr(out["rows"]), _hip.ptr(out["q"]), _hip.ptr(g[0]), _hip.ptr(g[1]), _hip.ptr(ws), nbytes,
                  _hip.stream())
        torch.cuda.synchronize()
        for k in NAMES:
            if grad or k in ("loss", "rows", "q"):
                assert tail_intact(out[k], sizes[k]), k
            else:
                assert bool((out[k] == SENT).all()), k
        runs.append(out)
    for k in NAMES:
        assert torch.equal(runs[0][k].view(torch.int32), runs[1][k].view(torch.int32)), ("two runs differ", k)
    return runs[0], sizes


def live(out, sizes, k, shape=None):
    v = out[k][:sizes[k]]
    return v.reshape(shape) if shape else v


def ref_pair(case, tau):
    kw = dict(temperature=tau, cand_ids=case["cand_ids"], mem=case["mem"], mem_ids=case["mem_ids"], count=case["count"])
    return tuple(pref.info_nce_pool(case["a"], case["cand"], case["pos0"], dtype=dt, **kw) for dt in (np.float64, np.float32))


def check_pool(tag, out, sizes, r64, r32, B, Nc, D):
    """rows, q, da, dcand to the f32 bar, then the two bounds of the scalar loss (test_infonce_gpu.check_all's)"""
    e_rows = check_f32(f"{tag} rows", live(out, sizes, "rows"), r64["rows"], r32["rows"])
    check_f32(f"{tag} q", live(out, sizes, "q"), r64["q"], r32["q"])
    check_f32(f"{tag} da", live(out, sizes, "da", (B, D)), r64["da"], r32["da"])
    check_f32(f"{tag} dcand", live(out, sizes, "dcand", (Nc, D)), r64["dcand"], r32["dcand"])
    rows_hip = f64(live(out, sizes, "rows"))
    loss = float(out["loss"][0])
    first = B * U32 * float(np.abs(rows_hip).mean())
    d1 = abs(loss - float(rows_hip.mean()))
    second = max(8 * e_rows[1], 8 * U32) * float(np.abs(r64["rows"]).max()) + first
    d2 = abs(loss - float(r64["loss"]))
    print(f"PARITY {tag + ' loss':<58s} f32  |loss-mean64(rows)|={d1:.3e} bound={first:.3e}  "
          f"|loss-ref64|={d2:.3e} bound={second:.3e}  loss={loss:.6g}")
    assert d1 <= first, (tag, d1, first)
    assert d2 <= second, (tag, d2, second)


# ------------------------------------------------------------ the byte contract
@pytest.mark.parametrize("shift", [0, 1])
@pytest.mark.parametrize("ids", [False, True])
@pytest.mark.parametrize("B,D,M,count", [(1, 4, 0, 0), (33, 65, 0, 0), (33, 65, 100, 37), (100, 512, 300, 300),
                                         (64, 1024, 0, 0)])
def test_bytes_of_the_batch_call(B, D, M, count, ids, shift, dev):
    case = tig.make(B, D, M, 3.0, seed=B + D + M, ids=ids, count=count)
    want, wsz = tig.run_raw(case, 0.07, dev, shift=shift)
    pool = dict(case, cand=np.concatenate([case["p"], case["n"]]), pos0=0)
    got, gsz = run_pool(pool, 0.07, dev, shift=shift)
    bits = lambda t: t.contiguous().view(torch.int32)  # noqa: E731
    for k in ("loss", "rows", "q", "da"):
        assert torch.equal(bits(tig.live(want, wsz, k)), bits(live(got, gsz, k))), k
    dcand = live(got, gsz, "dcand")
    assert torch.equal(bits(tig.live(want, wsz, "dp")), bits(dcand[:B * D])), "dp"
    assert torch.equal(bits(tig.live(want, wsz, "dn")), bits(dcand[B * D:])), "dn"
    assert bool(torch.isfinite(dcand).all())
    # forward alone: the same loss, rows and q, no gradient written
    fwd, fsz = run_pool(pool, 0.07, dev, grad=False, shift=shift)
    for k in ("loss", "rows", "q"):
        assert torch.equal(bits(live(fwd, fsz, k)), bits(live(got, gsz, k))), k


# ------------------------------------------------------------ parity where Nc != 2B, pos0 != 0
def make_pool(B, Nc, pos0, D, M, sigma, seed, ids=False, count=None):
    """test_infonce_gpu.make's a, p and ring (a few slots planted next to anchors); cand ~ N(0, 1)
    with p at [pos0, pos0 + B).  ids: all distinct, but a row outside the anchors' own
    2B-block (another rank's) carries anchor 0's photo, one carries anchor B-1's, and a
    filled slot carries anchor B/2's"""
    base = tig.make(B, D, M, sigma, seed, count=count)
    rng = np.random.default_rng(seed + 17)
    cand = rng.standard_normal((Nc, D)).astype(np.float32)
    cand[pos0:pos0 + B] = base["p"]
    case = dict(a=base["a"], cand=cand, pos0=pos0, mem=base["mem"], count=base["count"], cand_ids=None, mem_ids=None)
    if ids:
        cid = np.arange(100, 100 + Nc, dtype=np.int64)
        mids = np.arange(10_000, 10_000 + M, dtype=np.int64)
        other = [c for c in range(Nc) if not pos0 <= c < pos0 + B]
        if other:
            cid[other[-1]] = cid[pos0]               # the last row outside the slice: anchor 0's photo
            cid[other[0]] = cid[pos0 + B - 1]        # the first one: anchor B-1's
        filled = min(case["count"], M)
        if filled:
            mids[filled // 2] = cid[pos0 + B // 2]
        case.update(cand_ids=cid, mem_ids=mids)
    return case


SHAPES = [(33, 198, 0), (33, 198, 66), (33, 198, 132),  # W = 3: four candidate tiles, the last holds 6; at 66 the
          # positives 66..98 straddle two tiles
          (1, 4, 2),
          (40, 100, 60),      # pos0 + B = Nc, an unaligned offset
          (64, 1024, 448)]    # more candidate tiles than forward shares: the shares wrap


@pytest.mark.parametrize("sigma", [3.0, 0.7])
@pytest.mark.parametrize("ids", [False, True])
@pytest.mark.parametrize("M,count", [(0, 0), (100, 37)])
@pytest.mark.parametrize("D", [3, 65, 512, 1024])
@pytest.mark.parametrize("B,Nc,pos0", SHAPES)
def test_parity_pool(B, Nc, pos0, D, M, count, ids, sigma, dev):
    case = make_pool(B, Nc, pos0, D, M, sigma, seed=B * 7919 + Nc * 131 + pos0 * 7 + D + M, ids=ids, count=count)
    r64, r32 = ref_pair(case, 0.07)
    if ids and Nc > B:  # the planted collisions carry weight: without ids the loss differs
        assert r64["loss"] != pref.info_nce_pool(case["a"], case["cand"], pos0, 0.07, None, case["mem"], None, count)["loss"]
    out, sizes = run_pool(case, 0.07, dev)
    check_pool(f"B{B} Nc{Nc} pos{pos0} D{D} M{M} ids{int(ids)} s{sigma}", out, sizes, r64, r32, B, Nc, D)


@pytest.mark.parametrize("B,Nc,pos0", [(1, 4, 2), (33, 198, 66)])
def test_every_candidate_masked(B, Nc, pos0, dev):
    """an anchor whose every candidate carries its photo: row 0, q 0 and zero gradient rows.
    p[i]'s id is anchor i's, so among several anchors this happens to all at once"""
    case = make_pool(B, Nc, pos0, 65, 100, 3.0, seed=5, count=37)
    case.update(cand_ids=np.full(Nc, 5, np.int64), mem_ids=np.full(100, 5, np.int64))
    out, sizes = run_pool(case, 0.07, dev)
    for k in NAMES:
        assert bool((live(out, sizes, k) == 0).all()), k
    # one slot of another photo: the only negative of every anchor; every dcand row but the positives' is exact zeros
    case["mem_ids"][5] = 4
    r64, r32 = ref_pair(case, 0.07)
    assert (r64["rows"] > 0).all()
    out, sizes = run_pool(case, 0.07, dev)
    check_pool(f"B{B} Nc{Nc} pos{pos0}: one slot the only negative", out, sizes, r64, r32, B, Nc, 65)
    dcand = live(out, sizes, "dcand", (Nc, 65))
    outside = torch.ones(Nc, dtype=torch.bool, device=dcand.device)
    outside[pos0:pos0 + B] = False
    assert bool((dcand[outside] == 0).all()) and bool((dcand[~outside] != 0).any())


def test_unfilled_slots_hold_nan_and_a_wrapped_ring(dev):
    B, Nc, pos0, D, M = 33, 198, 66, 64, 300
    case = make_pool(B, Nc, pos0, D, M, 3.0, seed=8, ids=True, count=211)
    case["mem"][211:] = np.nan
    r64, r32 = ref_pair(case, 0.07)
    out, sizes = run_pool(case, 0.07, dev)
    check_pool("count 211 of 300, NaN beyond", out, sizes, r64, r32, B, Nc, D)
    case = make_pool(B, Nc, pos0, D, M, 3.0, seed=9, ids=True, count=M + 500)
    r64, r32 = ref_pair(case, 0.07)
    out, sizes = run_pool(case, 0.07, dev, head=123)
    check_pool("head 123, count > M", out, sizes, r64, r32, B, Nc, D)


def test_python_surface_at_world_one(dev):
    """no process group: gather=True is the batch call, byte for byte, gradients included"""
    import losses
    case = tig.make(37, 65, 0, 3.0, seed=12, ids=True)
    ids = torch.from_numpy(case["cand_ids"]).to(dev)
    got = []
    for gather in (False, True):
        leaves = [torch.from_numpy(case[k]).to(dev).requires_grad_(True) for k in ("a", "p", "n")]
        loss = losses.info_nce(*leaves, cand_ids=ids, gather=gather)
        loss.backward()
        got.append([loss.detach()] + [t.grad for t in leaves])
    for x, y in zip(*got):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))
    # the pool call of the Python layer, against the batch call
    loss, rows, q, (da, dcand) = losses._info_nce_pool_raw(got[0][1].new_tensor(case["a"]),
                                                          torch.from_numpy(np.concatenate([case["p"], case["n"]])).to(dev),
                                                          0, 0.07, ids, None, 1e-8, True)
    assert torch.equal(loss.view(torch.int32), got[0][0].view(torch.int32))
    assert torch.equal(da, got[0][1]) and torch.equal(dcand[:37], got[0][2]) and torch.equal(dcand[37:], got[0][3])
