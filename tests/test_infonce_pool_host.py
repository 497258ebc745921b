"""The pool form of the InfoNCE loss (artsbir_info_nce_pool, losses.info_nce(gather=True),
train.py --gather_negatives) without a GPU: the float64 restatement tests/_infonce_pool_ref.py
against tests/_infonce_ref.py and against the textbook loss over the global batch by torch
float64 autograd, the entry points' refusals ahead of any launch, the workspace rule and the
training entry's switches."""
import ctypes
import os
import re

import numpy as np
import pytest

import _infonce_pool_ref as pref
import _infonce_ref as nref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rel(got, want):
    scale = np.abs(want).max()
    return np.abs(got - want).max() / (scale if scale else 1.0)


@pytest.mark.parametrize("ids", [False, True])
@pytest.mark.parametrize("B,D,M", [(5, 3, 7), (37, 65, 300)])
def test_pool_restatement_is_the_batch_restatement_at_p_n(B, D, M, ids):
    rng = np.random.default_rng(B + D)
    a, n = (rng.standard_normal((B, D)).astype(np.float32) for _ in range(2))
    p = (a + 3.0 * rng.standard_normal((B, D))).astype(np.float32)
    mem = rng.standard_normal((M, D)).astype(np.float32)
    cand = rng.integers(0, B, 2 * B).astype(np.int64) if ids else None
    mids = rng.integers(0, B, M).astype(np.int64) if ids else None
    for count in (M, M // 2, 0):
        want = nref.info_nce(a, p, n, 0.07, cand, mem, mids, count)
        got = pref.info_nce_pool(a, np.concatenate([p, n]), 0, 0.07, cand, mem, mids, count)
        assert abs(got["loss"] - want["loss"]) <= 1e-14 * abs(want["loss"])
        for k in ("rows", "q", "da"):
            assert _rel(got[k], want[k]) <= 1e-14, k
        assert _rel(got["dcand"], np.concatenate([want["dp"], want["dn"]])) <= 1e-14


@pytest.mark.parametrize("ids", [False, True])
@pytest.mark.parametrize("B,D,M", [(5, 3, 7), (37, 65, 300)])
@pytest.mark.parametrize("W", [2, 3])
def test_ranks_of_pool_calls_sum_to_the_global_loss(W, B, D, M, ids):
    """what the gathered protocol computes, with the ranks simulated: rank r's call has
    pos0 = r 2B in the gather G; the mean of the ranks' losses, da_r / W and the sum over the
    ranks of dG_s's slice of rank r, / W, are the loss over all W B anchors and its gradient
    (ddp's average of the parameter gradients is the / W)"""
    rng = np.random.default_rng(1000 * W + B + D + ids)
    a = rng.standard_normal((W * B, D)).astype(np.float32)
    G = rng.standard_normal((W * 2 * B, D)).astype(np.float32)
    for r in range(W):  # positives near their anchors
        G[r * 2 * B:r * 2 * B + B] = a[r * B:(r + 1) * B] + 3.0 * rng.standard_normal((B, D)).astype(np.float32)
    mem = rng.standard_normal((M, D)).astype(np.float32)
    count = M // 2
    ids_G = rng.integers(0, W * B, W * 2 * B).astype(np.int64) if ids else None  # many collisions, across ranks too
    mids = rng.integers(0, W * B, M).astype(np.int64) if ids else None
    loss, per, da, dG = pref.global_loss_textbook(a, G, B, 0.07, ids_G, mem, mids, count)
    calls = [pref.info_nce_pool(a[r * B:(r + 1) * B], G, r * 2 * B, 0.07, ids_G, mem, mids, count) for r in range(W)]
    assert abs(np.mean([c["loss"] for c in calls]) - loss) <= 1e-12 * abs(loss)
    dG_sum = sum(c["dcand"] for c in calls) / W
    for r, c in enumerate(calls):
        assert abs(c["loss"] - per[r]) <= 1e-12 * abs(per[r])
        assert np.abs(c["da"] / W - da[r * B:(r + 1) * B]).max() <= 1e-12 * np.abs(da).max(), r
        sl = slice(r * 2 * B, (r + 1) * 2 * B)
        assert np.abs(dG_sum[sl] - dG[sl]).max() <= 1e-12 * np.abs(dG).max(), r
        assert np.allclose(c["q"], -np.expm1(-c["rows"]), rtol=1e-12, atol=0)


def test_a_row_no_anchor_weighs_gets_exact_zeros():
    rng = np.random.default_rng(2)
    a = rng.standard_normal((3, 4)).astype(np.float32)
    cand = rng.standard_normal((8, 4)).astype(np.float32)
    ids = np.array([0, 1, 2, 3, 4, 7, 7, 7], np.int64)
    ids[2:5] = 7  # the anchors (pos0 = 2) all carry photo 7: rows 5, 6, 7 are masked for every anchor
    for dtype in (np.float64, np.float32):
        got = pref.info_nce_pool(a, cand, 2, 0.07, ids, dtype=dtype)
        assert not got["dcand"][5:].any() and got["dcand"][:5].any() and (got["rows"] > 0).all()


def test_entry_points_declared_exported_and_bound():
    import _hip
    header = open(os.path.join(ROOT, "include", "artsbir.h")).read()
    lib = _hip.lib()
    assert re.search(r"\blong long\s+artsbir_info_nce_pool_workspace\s*\(", header)
    assert re.search(r"\bint\s+artsbir_info_nce_pool\s*\(", header)
    assert hasattr(lib, "artsbir_info_nce_pool") and hasattr(lib, "artsbir_info_nce_pool_workspace")
    assert len(_hip.SIGNATURES["artsbir_info_nce_pool"]) == 21
    assert len(_hip.SIGNATURES["artsbir_info_nce_pool_workspace"]) == 5
    assert len(_hip.SIGNATURES["artsbir_info_nce"]) == 21  # the batch form keeps its signature


def test_refusals_without_touching_the_gpu():
    """every argument check sits ahead of the first launch: NULL pointers are never read
    and the non-NULL stand-ins are never dereferenced"""
    import _hip
    lib = _hip.lib()
    buf = ctypes.c_void_p(64)

    def nce(B=4, Nc=24, pos0=8, D=8, scale=1 / 0.07, a=buf, cand=buf, ids=None, mem=buf, mem_ids=buf, state=buf, M=16,
            loss=buf, rows=buf, q=buf, da=buf, dcand=buf, ws=buf, ws_bytes=1 << 40):
        rc = lib.artsbir_info_nce_pool(a, cand, B, Nc, pos0, D, scale, 1e-8, ids, mem, mem_ids, state, M, loss, rows, q,
                                       da, dcand, ws, ws_bytes, None)
        assert rc != 0
        return lib.artsbir_last_error()

    assert b"info_nce_pool: pos0=-1 must be >= 0" in nce(pos0=-1)
    assert b"info_nce_pool: pos0=21 + B=4 above Nc=24" in nce(pos0=21)
    assert b"info_nce_pool: pos0=2147483647 + B=4 above Nc=24" in nce(pos0=2 ** 31 - 1)
    assert b"info_nce_pool: Nc=3 below B=4" in nce(Nc=3, pos0=0)
    assert b"info_nce_pool: Nc=-5 below B=4" in nce(Nc=-5, pos0=0)
    assert b"info_nce_pool: D=1025 above 1024" in nce(D=1025)
    assert b"info_nce_pool: D=0 must be >= 1" in nce(D=0)
    assert b"info_nce_pool: B=0 must be >= 1" in nce(B=0)
    assert b"info_nce_pool: B=1048577 above 2^20" in nce(B=(1 << 20) + 1, Nc=1 << 22)
    assert b"info_nce_pool: M=-1 must be >= 0" in nce(M=-1)
    assert b"info_nce_pool: M=16777217 above 2^24" in nce(M=(1 << 24) + 1)
    assert b"info_nce_pool: Nc=2147483448 + M=16 above 2^31 - 257" in nce(Nc=2147483448)
    for bad in (0.0, -2.0, float("inf"), float("nan")):
        assert b"info_nce_pool: scale=" in nce(scale=bad) and b"must be finite and > 0" in nce(scale=bad)
    for some in (dict(da=None), dict(dcand=None)):
        assert b"info_nce_pool: da and dcand must be given together or not at all" in nce(**some)
    for arg in ("a", "cand", "loss", "rows", "q"):
        assert b"info_nce_pool: NULL pointer" in nce(**{arg: None})
    assert b"info_nce_pool: mem given with mem_state NULL" in nce(state=None)
    assert b"info_nce_pool: mem and cand_ids given with mem_ids NULL" in nce(ids=buf, mem_ids=None)
    need = lib.artsbir_info_nce_pool_workspace(4, 24, 8, 16, 1)
    assert need > 0
    assert b"info_nce_pool: workspace of %d bytes, %d needed" % (need - 1, need) in nce(ws_bytes=need - 1)
    assert b"info_nce_pool: workspace of 0 bytes" in nce(ws=None)
    assert b"info_nce_pool: workspace not 8-byte aligned" in nce(ws=ctypes.c_void_p(68))
    # forward alone asks for less, and is refused below that
    fwd = lib.artsbir_info_nce_pool_workspace(4, 24, 8, 16, 0)
    assert 0 < fwd < need
    assert b"info_nce_pool: workspace of %d bytes, %d needed" % (fwd - 1, fwd) in nce(da=None, dcand=None, ws_bytes=fwd - 1)
    # everything NULL with a bad shape: the shape is refused first
    assert b"info_nce_pool: B=0" in nce(B=0, a=None, cand=None, loss=None, rows=None, q=None, ws=None)
    for args, msg in (((0, 8, 8, 0, 1), b"info_nce_pool_workspace: B=0"), ((4, 8, 0, 0, 1), b"info_nce_pool_workspace: D=0"),
                      ((4, 8, 1025, 0, 0), b"info_nce_pool_workspace: D=1025 above 1024"),
                      ((4, 3, 8, 0, 0), b"info_nce_pool_workspace: Nc=3 below B=4"),
                      (((1 << 20) + 1, 1 << 22, 8, 0, 0), b"above 2^20"), ((4, 8, 8, -1, 0), b"M=-1"),
                      ((4, 8, 8, (1 << 24) + 1, 0), b"above 2^24"),
                      ((4, 2 ** 31 - 1, 8, 0, 0), b"above 2^31 - 257")):
        assert lib.artsbir_info_nce_pool_workspace(*args) < 0 and msg in lib.artsbir_last_error(), args
    with pytest.raises(_hip.HipError, match="info_nce_pool"):
        _hip.call("artsbir_info_nce_pool", None, None, 4, 8, 0, 2000, 1.0, 1e-8, None, None, None, None, 0, None, None,
                  None, None, None, None, 0, None)


def test_workspace_rule():
    """at Nc = 2B the batch form's own workspace (one geometry: the byte contract), and never
    less than the layout's fixed part: the inverse norms of a, cand and the slots, z(i, i) and
    L, one share's (max, sum) pairs in f64; with gradients dchat [Nc, D] and one share's
    partial da^ [B, D] in f32.  A candidate row more costs its inverse norm and its dchat row."""
    import _hip
    pool, batch = _hip.lib().artsbir_info_nce_pool_workspace, _hip.lib().artsbir_info_nce_workspace
    for B, D in ((384, 1024), (384, 512), (37, 65), (1, 1)):
        for M in (0, 300, 1 << 20):
            for grad in (0, 1):
                assert pool(B, 2 * B, D, M, grad) == batch(B, D, M, grad), (B, D, M, grad)
                for Nc in (B, 2 * B, 6 * B + 1, 16 * B):
                    need = 8 * (B + Nc + M + B + B + 2 * B) + grad * 4 * (Nc * D + B * D)
                    assert pool(B, Nc, D, M, grad) >= need, (B, Nc, D, M, grad)
                    assert pool(B, Nc + 1, D, M, grad) - pool(B, Nc, D, M, grad) == 8 + grad * 4 * D
    # the headline multi-GPU shape: 8 ranks x 384 triplets
    assert pool(384, 6144, 1024, 0, 1) < 96 << 20


def test_python_surface_without_a_process_group_runs_the_batch_call():
    """gather=True with no process group is the existing call: here it gets as far as that
    call's own refusal of CPU tensors"""
    import torch

    import losses
    a = torch.zeros(4, 8, requires_grad=True)
    with pytest.raises(RuntimeError, match="CUDA tensors"):
        losses.info_nce(a, a, a, gather=True)
    with pytest.raises(RuntimeError, match="CUDA tensors"):
        losses.InfoNCELoss(gather=True)(a, a, a)
    with pytest.raises(RuntimeError, match="CUDA tensors"):
        losses._info_nce_pool_raw(a, torch.zeros(8, 8), 0, 0.07, None, None, 1e-8, True)
    fn = losses.InfoNCELoss(0.05, gather=True)
    assert fn.gather is True and fn.temperature == 0.05 and losses.InfoNCELoss().gather is False


def test_train_switches():
    import losses
    import train
    with pytest.raises(SystemExit, match="--gather_negatives needs --negatives all"):
        train.parse_args(["--gather_negatives"])
    with pytest.raises(SystemExit, match="--gather_negatives needs --negatives all"):
        train.parse_args(["--gather_negatives", "--negatives", "hardest"])
    args = train.parse_args(["--gather_negatives", "--negatives", "all", "--loss_type", "cosine"])
    assert args.gather_negatives is True and args.negatives == "all"
    assert train.parse_args(["--negatives", "all", "--loss_type", "cosine"]).gather_negatives is False
    assert train.parse_args([]).gather_negatives is False
    fn = train.make_loss('cosine', False, "SyntheticTripletDataset", 0.2, 'all', memory_size=48, gather_negatives=True)
    assert isinstance(fn, losses.InfoNCELoss) and fn.gather is True and fn.memory.size == 48
    assert train.make_loss('cosine', False, "SyntheticTripletDataset", 0.2, 'all').gather is False
    with pytest.raises(SystemExit, match="--gather_negatives needs --negatives all"):
        train.make_loss('cosine', False, "SyntheticTripletDataset", 0.2, 'semihard', gather_negatives=True)
    with pytest.raises(SystemExit, match="--gather_negatives needs --negatives all"):
        train.make_loss('euclidean', False, "SyntheticTripletDataset", 0.2, gather_negatives=True)
