"""The InfoNCE loss without a GPU: the float64 restatement the GPU tests lean on
(tests/_infonce_ref.py) against the textbook definition by torch float64 autograd, the
entry points' refusals ahead of any launch, the workspace rule, and the training entry's
--negatives all / --temperature switches."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import _infonce_ref as nref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _inputs(B, D, M, ids, seed):
    rng = np.random.default_rng(seed)
    a = rng.standard_normal((B, D)).astype(np.float32)
    n = rng.standard_normal((B, D)).astype(np.float32)
    p = (a + 3.0 * rng.standard_normal((B, D))).astype(np.float32)
    mem = rng.standard_normal((M, D)).astype(np.float32)
    cand = mids = None
    if ids:
        cand = rng.integers(0, B, 2 * B).astype(np.int64)  # many collisions
        mids = rng.integers(0, B, M).astype(np.int64)
    return a, p, n, mem, cand, mids


def _textbook(a, p, n, mem, count, cand, mids, tau, eps=1e-8):
    """clamped normalisation, masked_fill(-inf), cross_entropy with target i; torch f64 autograd"""
    B = a.shape[0]
    ta, tp, tn = (torch.from_numpy(x.astype(np.float64)).requires_grad_(True) for x in (a, p, n))
    pool = torch.cat([tp, tn, torch.from_numpy(mem[:count].astype(np.float64))])
    norm = lambda x: x / x.norm(dim=1, keepdim=True).clamp_min(eps)  # noqa: E731
    z = norm(ta) @ norm(pool).T / tau
    neg = torch.from_numpy(nref.negatives_mask(B, mem.shape[0], count, cand, mids)[:, :2 * B + count])
    keep = neg.clone()
    keep[torch.arange(B), torch.arange(B)] = True
    loss = torch.nn.functional.cross_entropy(z.masked_fill(~keep, float("-inf")), torch.arange(B))
    loss.backward()
    return loss.item(), ta.grad.numpy(), tp.grad.numpy(), tn.grad.numpy()


@pytest.mark.parametrize("ids", [False, True])
@pytest.mark.parametrize("B,D,M", [(5, 3, 7), (37, 65, 300)])
def test_f64_restatement_against_the_textbook_definition(B, D, M, ids):
    a, p, n, mem, cand, mids = _inputs(B, D, M, ids, seed=B + D)
    for count in (M, M // 2):
        got = nref.info_nce(a, p, n, 0.07, cand, mem, mids, count)
        loss, da, dp, dn = _textbook(a, p, n, mem, count, cand, mids, 0.07)
        assert abs(got["loss"] - loss) <= 1e-12 * abs(loss)
        for name, want in (("da", da), ("dp", dp), ("dn", dn)):
            assert np.abs(got[name] - want).max() <= 1e-12 * np.abs(want).max(), name
        # the probability of the positive is 1 - q
        assert np.allclose(got["q"], -np.expm1(-got["rows"]), rtol=1e-12, atol=0)


def test_an_anchor_without_a_negative():
    """p[c] carries anchor c's id, so an anchor loses every candidate only when all anchors
    share its id: row 0, q 0 and zero gradients, for all of them (and the single anchor)"""
    a, p, n, mem, _, _ = _inputs(4, 6, 5, False, seed=1)
    for dtype in (np.float64, np.float32):
        got = nref.info_nce(a, p, n, 0.07, np.full(8, 9), mem, np.full(5, 9), 5, dtype=dtype)
        assert got["loss"] == 0 and (got["rows"] == 0).all() and (got["q"] == 0).all()
        assert not got["da"].any() and not got["dp"].any() and not got["dn"].any()
        assert (got["L"] == -np.inf).all()
        one = nref.info_nce(a[:1], p[:1], n[:1], 0.07, np.array([9, 9]), dtype=dtype)
        assert one["rows"][0] == 0 and one["q"][0] == 0 and not one["da"].any() and not one["dn"].any()
    # without ids the single anchor's only negative is its own n[0]
    assert nref.info_nce(a[:1], p[:1], n[:1])["rows"][0] > 0


def test_entry_points_declared_exported_and_bound():
    import _hip
    header = open(os.path.join(ROOT, "include", "artsbir.h")).read()
    lib = _hip.lib()
    assert re.search(r"\blong long\s+artsbir_info_nce_workspace\s*\(", header)
    assert re.search(r"\bint\s+artsbir_info_nce\s*\(", header)
    assert hasattr(lib, "artsbir_info_nce") and hasattr(lib, "artsbir_info_nce_workspace")
    assert len(_hip.SIGNATURES["artsbir_info_nce"]) == 21 and len(_hip.SIGNATURES["artsbir_info_nce_workspace"]) == 4


def test_refusals_without_touching_the_gpu():
    """every argument check sits ahead of the first launch: NULL pointers are never read
    and the non-NULL stand-ins are never dereferenced"""
    import _hip
    lib = _hip.lib()
    buf = ctypes.c_void_p(64)

    def nce(B=4, D=8, scale=1 / 0.07, a=buf, p=buf, n=buf, ids=None, mem=buf, mem_ids=buf, state=buf, M=16, loss=buf,
            rows=buf, q=buf, da=buf, dp=buf, dn=buf, ws=buf, ws_bytes=1 << 40):
        rc = lib.artsbir_info_nce(a, p, n, B, D, scale, 1e-8, ids, mem, mem_ids, state, M, loss, rows, q, da, dp, dn, ws,
                                  ws_bytes, None)
        assert rc != 0
        return lib.artsbir_last_error()

    assert b"info_nce: B=0 must be >= 1" in nce(B=0)
    assert b"info_nce: D=0 must be >= 1" in nce(D=0)
    assert b"info_nce: D=1025 above 1024" in nce(D=1025)
    assert b"info_nce: B=1048577 above 2^20" in nce(B=(1 << 20) + 1)
    assert b"info_nce: M=-1 must be >= 0" in nce(M=-1)
    assert b"info_nce: M=16777217 above 2^24" in nce(M=(1 << 24) + 1)
    for bad in (0.0, -2.0, float("inf"), float("nan")):
        assert b"must be finite and > 0" in nce(scale=bad)
    for some in (dict(da=None), dict(dp=None, dn=None), dict(da=None, dp=None)):
        assert b"info_nce: da, dp, dn must be given together or not at all" in nce(**some)
    assert b"info_nce: mem given with mem_state NULL" in nce(state=None)
    assert b"info_nce: mem and cand_ids given with mem_ids NULL" in nce(ids=buf, mem_ids=None)
    for arg in ("a", "p", "n", "loss", "rows", "q"):
        assert b"info_nce: NULL pointer" in nce(**{arg: None})
    need = lib.artsbir_info_nce_workspace(4, 8, 16, 1)
    assert need > 0
    assert b"info_nce: workspace of %d bytes, %d needed" % (need - 1, need) in nce(ws_bytes=need - 1)
    assert b"info_nce: workspace of 0 bytes" in nce(ws=None)
    assert b"info_nce: workspace not 8-byte aligned" in nce(ws=ctypes.c_void_p(68))
    # everything NULL with a bad shape: the shape is refused first
    assert b"info_nce: B=0" in nce(B=0, a=None, p=None, n=None, loss=None, rows=None, q=None, ws=None)
    for args, msg in (((0, 8, 0, 1), b"info_nce_workspace: B=0"), ((4, 0, 0, 1), b"info_nce_workspace: D=0"),
                      ((4, 1025, 0, 0), b"info_nce_workspace: D=1025 above 1024"),
                      (((1 << 20) + 1, 8, 0, 0), b"above 2^20"), ((4, 8, -1, 0), b"M=-1"),
                      ((4, 8, (1 << 24) + 1, 0), b"above 2^24")):
        assert lib.artsbir_info_nce_workspace(*args) < 0 and msg in lib.artsbir_last_error(), args
    with pytest.raises(_hip.HipError, match="info_nce"):
        _hip.call("artsbir_info_nce", None, None, None, 4, 2000, 1.0, 1e-8, None, None, None, None, 0, None, None, None,
                  None, None, None, None, 0, None)


def test_workspace_rule():
    """the workspace grows with M by the inverse norms alone, at most 8 bytes per slot, and
    its M-free part stays under 64 MiB at the largest training shape; forward only needs
    no more than forward and gradient"""
    import _hip
    ws = _hip.lib().artsbir_info_nce_workspace
    for B, D in ((384, 1024), (384, 512), (37, 65), (1, 1)):
        base = ws(B, D, 0, 1)
        assert 0 < ws(B, D, 0, 0) <= base
        for M in (4096, 1 << 20):
            for grad in (0, 1):
                assert 0 <= ws(B, D, M, grad) - ws(B, D, 0, grad) <= 8 * M, (B, D, M)
    assert ws(384, 1024, 0, 1) < 64 << 20
    for M in (4096, 1 << 20, 1 << 24):
        assert ws(384, 1024, M, 1) - 8 * M < 64 << 20


def test_python_surface_refuses_cpu_tensors_and_bad_arguments():
    import losses
    a = torch.zeros(4, 8)
    with pytest.raises(RuntimeError, match="CUDA tensors"):
        losses.info_nce(a, a, a)
    with pytest.raises(RuntimeError, match="CUDA tensors"):
        losses.InfoNCELoss(memory=losses.CrossBatchMemory(16, None))(a, a, a)
    with pytest.raises(ValueError, match="temperature must be > 0"):
        losses.InfoNCELoss(0.0)
    fn = losses.InfoNCELoss()  # touches no GPU
    assert fn.margin is None and fn.temperature == 0.07 and fn.memory is None and fn.positive_probability() == 0.0


def test_make_loss_all():
    import losses
    import train
    fn = train.make_loss('cosine', False, "SyntheticTripletDataset", 0.2, 'all', memory_size=48)
    assert isinstance(fn, losses.InfoNCELoss) and isinstance(fn.memory, losses.CrossBatchMemory)
    assert fn.memory.size == 48 and fn.memory.mem is None and fn.temperature == 0.07 and fn.margin is None
    fn = train.make_loss('cosine', False, "SyntheticTripletDataset", 0.2, 'all', temperature=0.02)
    assert isinstance(fn, losses.InfoNCELoss) and fn.memory is None and fn.temperature == 0.02
    with pytest.raises(SystemExit, match="--negatives all needs --loss_type cosine"):
        train.make_loss('euclidean', False, "SyntheticTripletDataset", 0.2, 'all')
    with pytest.raises(SystemExit, match="without classification heads"):
        train.make_loss('cosine', True, "SketchyV2", 0.2, 'all')
    with pytest.raises(SystemExit, match="--temperature needs --negatives all"):
        train.make_loss('cosine', False, "SyntheticTripletDataset", 0.2, 'hardest', temperature=0.1)
    with pytest.raises(SystemExit, match="must be > 0"):
        train.make_loss('cosine', False, "SyntheticTripletDataset", 0.2, 'all', temperature=0.0)
    # the existing memory-size cases stand
    with pytest.raises(SystemExit, match="--memory_size needs --negatives hardest or semihard"):
        train.make_loss('cosine', False, "SyntheticTripletDataset", 0.2, 'given', memory_size=48)
    with pytest.raises(SystemExit, match="must be >= 0"):
        train.make_loss('cosine', False, "SyntheticTripletDataset", 0.2, 'all', memory_size=-1)


def test_parse_args_negatives_all_and_temperature():
    import train
    args = train.parse_args(["--negatives", "all", "--loss_type", "cosine"])
    assert args.negatives == "all" and args.temperature == 0.07 and args.memory_size == 0
    args = train.parse_args(["--negatives", "all", "--loss_type", "cosine", "--temperature", "0.02", "--memory_size", "64"])
    assert args.temperature == 0.02 and args.memory_size == 64
    assert train.parse_args([]).temperature is None
    with pytest.raises(SystemExit, match="--temperature needs --negatives all"):
        train.parse_args(["--temperature", "0.1"])
    with pytest.raises(SystemExit, match="--temperature needs --negatives all"):
        train.parse_args(["--negatives", "hardest", "--temperature", "0.1"])
    with pytest.raises(SystemExit, match="--negatives all needs --loss_type cosine"):
        train.parse_args(["--negatives", "all"])
    with pytest.raises(SystemExit, match="without classification heads"):
        train.parse_args(["--negatives", "all", "--loss_type", "cosine", "--model_type",
                          "ModifiedResNet_with_classification"])
    with pytest.raises(SystemExit, match="must be > 0"):
        train.parse_args(["--negatives", "all", "--loss_type", "cosine", "--temperature", "-1"])
