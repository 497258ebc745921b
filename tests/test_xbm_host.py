"""The cross-batch memory without a GPU: the three entry points exist and refuse bad
arguments ahead of any launch, the training entry has the --memory_size switch, and the
float64 restatement the GPU tests lean on (tests/_xbm_ref.py) agrees with a hand case
and a brute-force loop."""
import ctypes
import os
import re

import numpy as np
import pytest

import _mining_ref as mref
import _xbm_ref as xref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {"artsbir_mine_pool": 17, "artsbir_xbm_enqueue": 9, "artsbir_rows_gather3": 9}


def test_entry_points_declared_exported_and_bound():
    import _hip
    header = open(os.path.join(ROOT, "include", "artsbir.h")).read()
    lib = _hip.lib()
    for name, nargs in ENTRIES.items():
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert hasattr(lib, name), name
        assert len(_hip.SIGNATURES[name]) == nargs, name
    assert "train.py:59-70" in header[header.index("Cross-batch memory"):header.index("artsbir_mine_pool(")]


def test_entry_points_reject_bad_arguments_without_touching_the_gpu():
    """every argument check sits ahead of the launch, so NULL pointers are never read
    and the non-NULL stand-ins are never dereferenced"""
    import _hip
    lib = _hip.lib()
    buf = ctypes.c_void_p(64)  # a non-NULL pointer that is never read

    def refused(name, *args):
        assert getattr(lib, name)(*args) != 0, (name, args)
        return lib.artsbir_last_error()

    def pool(metric=0, mode=0, a=buf, p=buf, n=buf, B=4, D=8, ids=None, mem=buf, mem_ids=buf, state=buf, M=16,
             sel=buf, d_ap=buf, d_sel=buf):
        return refused("artsbir_mine_pool", metric, mode, a, p, n, B, D, 1e-6, ids, mem, mem_ids, state, M, sel, d_ap,
                       d_sel, None)

    big = (1 << 20) + 1
    assert b"mine_pool: B=0 must be >= 1" in pool(B=0)
    assert b"mine_pool: B=-3 must be >= 1" in pool(B=-3)
    assert b"mine_pool: D=0 must be >= 1" in pool(D=0)
    assert b"mine_pool: B=1048577 above 2^20" in pool(B=big)
    assert b"mine_pool: M=-1 must be >= 0" in pool(M=-1)
    assert b"mine_pool: M=16777217 above 2^24" in pool(M=(1 << 24) + 1)
    assert b"mine_pool: 2B+M=2147483655 does not fit 31 bits" in pool(M=(1 << 31) - 1)
    assert b"mine_pool: 2B+M=2147483648 does not fit 31 bits" in pool(B=1 << 20, M=(1 << 31) - (1 << 21))
    for bad in (-1, 2):
        assert b"mine_pool: metric=%d outside {0, 1}" % bad in pool(metric=bad)
        assert b"mine_pool: mode=%d outside {0, 1}" % bad in pool(mode=bad)
    for arg in ("a", "p", "n", "sel", "d_ap", "d_sel"):
        assert b"mine_pool: NULL pointer" in pool(**{arg: None})
    assert b"mine_pool: mem given with mem_state NULL" in pool(state=None)
    assert b"mine_pool: mem given with mem_ids NULL" in pool(mem_ids=None)
    # all of them NULL with a bad shape: the shape is refused first, nothing is read
    assert b"mine_pool: B=0" in pool(B=0, a=None, p=None, n=None, sel=None, d_ap=None, d_sel=None, mem=None)

    def enqueue(rows=buf, ids=None, R=4, D=8, mem=buf, mem_ids=buf, state=buf, M=16):
        return refused("artsbir_xbm_enqueue", rows, ids, R, D, mem, mem_ids, state, M, None)

    assert b"xbm_enqueue: R=0 must be >= 1" in enqueue(R=0)
    assert b"xbm_enqueue: R=-2 must be >= 1" in enqueue(R=-2)
    assert b"xbm_enqueue: R=16777217 above 2^24" in enqueue(R=(1 << 24) + 1)
    assert b"xbm_enqueue: D=0 must be >= 1" in enqueue(D=0)
    assert b"xbm_enqueue: M=0 must be >= 1" in enqueue(M=0)
    assert b"xbm_enqueue: M=16777217 above 2^24" in enqueue(M=(1 << 24) + 1)
    for arg in ("rows", "mem", "mem_ids", "state"):
        assert b"xbm_enqueue: NULL pointer" in enqueue(**{arg: None})
    assert b"xbm_enqueue: R=0" in enqueue(R=0, rows=None, mem=None, mem_ids=None, state=None)

    def gather(p=buf, n=buf, mem=buf, sel=buf, B=4, D=8, M=16, out=buf):
        return refused("artsbir_rows_gather3", p, n, mem, sel, B, D, M, out, None)

    assert b"rows_gather3: B=0 must be >= 1" in gather(B=0)
    assert b"rows_gather3: D=-1 must be >= 1" in gather(D=-1)
    assert b"rows_gather3: B=1048577 above 2^20" in gather(B=big)
    assert b"rows_gather3: M=-1 must be >= 0" in gather(M=-1)
    assert b"rows_gather3: M=16777217 above 2^24" in gather(M=(1 << 24) + 1)
    assert b"rows_gather3: 2B+M=2147483655 does not fit 31 bits" in gather(M=(1 << 31) - 1)
    for arg in ("p", "n", "sel", "out"):
        assert b"rows_gather3: NULL pointer" in gather(**{arg: None})
    assert b"rows_gather3: M=16 with mem NULL" in gather(mem=None)
    with pytest.raises(_hip.HipError, match="mine_pool"):
        _hip.call("artsbir_mine_pool", 0, 3, None, None, None, 4, 8, 1e-6, None, None, None, None, 0, None, None, None,
                  None)


def test_python_surface_refuses_cpu_tensors_and_bad_sizes():
    import losses
    import torch
    a, p, n = (torch.zeros(4, 8) for _ in range(3))
    memory = losses.CrossBatchMemory(16, None)
    assert memory.filled() == 0
    memory.reset()  # nothing allocated yet: nothing to do
    with pytest.raises(RuntimeError, match="CUDA tensors"):
        losses.mine_negatives(a, p, n, memory=memory)
    with pytest.raises(RuntimeError, match="CUDA tensors"):
        memory.enqueue(a)
    with pytest.raises(ValueError, match="size >= 1"):
        losses.CrossBatchMemory(0, 8)
    with pytest.raises(ValueError, match="dim >= 1"):
        losses.CrossBatchMemory(4, 0)
    fn = losses.MinedNegatives(losses.TripletMarginLoss(0.2), "hardest", memory=memory)
    assert fn.memory is memory and fn.memory_fraction() == 0.0 and fn.mined_fraction() == 0.0


def test_gather_ranks_is_the_identity_without_a_process_group():
    import losses
    import torch
    rows, ids = torch.arange(6.0).reshape(3, 2), torch.arange(3)
    out = losses._gather_ranks(rows, ids)
    assert out[0] is rows and out[1] is ids
    assert losses._gather_ranks(rows, None)[1] is None


def test_parse_args_memory_size():
    import train
    assert train.parse_args([]).memory_size == 0
    assert train.parse_args(["--negatives", "hardest"]).memory_size == 0
    for v in ("hardest", "semihard"):
        assert train.parse_args(["--negatives", v, "--memory_size", "4096"]).memory_size == 4096
    with pytest.raises(SystemExit, match="--memory_size needs --negatives hardest or semihard"):
        train.parse_args(["--memory_size", "16"])
    with pytest.raises(SystemExit, match="--memory_size needs --negatives hardest or semihard"):
        train.parse_args(["--negatives", "given", "--memory_size", "16"])
    with pytest.raises(SystemExit, match="must be >= 0"):
        train.parse_args(["--negatives", "hardest", "--memory_size", "-1"])


@pytest.mark.parametrize("loss_type,with_cls,dataset,inner", [
    ("euclidean", False, "SyntheticTripletDataset", "TripletMarginLoss"),
    ("cosine", True, "KaggleV2", "TripletMarginLoss_with_classification2"),
])
def test_make_loss_gives_the_wrapper_a_memory_only_when_asked(loss_type, with_cls, dataset, inner):
    import losses
    import train
    for mode in ("hardest", "semihard"):
        assert train.make_loss(loss_type, with_cls, dataset, 0.3, mode).memory is None
        assert train.make_loss(loss_type, with_cls, dataset, 0.3, mode, memory_size=0).memory is None
        mined = train.make_loss(loss_type, with_cls, dataset, 0.3, mode, memory_size=48)
        assert isinstance(mined, losses.MinedNegatives) and type(mined.loss_fn).__name__ == inner
        assert isinstance(mined.memory, losses.CrossBatchMemory) and mined.memory.size == 48
        assert mined.memory.mem is None  # allocated at the first step, at the embeddings' width
        assert (mined.mode, mined.metric, mined.margin) == (mode, loss_type, 0.3)
    assert type(train.make_loss(loss_type, with_cls, dataset, 0.3, "given", memory_size=0)).__name__ == inner
    with pytest.raises(SystemExit, match="--memory_size needs"):
        train.make_loss(loss_type, with_cls, dataset, 0.3, "given", memory_size=48)
    with pytest.raises(SystemExit, match="--memory_size needs"):
        train.make_loss(loss_type, with_cls, dataset, 0.3, memory_size=48)


def test_ring_restatement_on_a_hand_case():
    # M = 5 slots, D = 1; rows are numbered so that a slot shows which row it holds
    ring = xref.Ring(5, 1)
    assert ring.state().tolist() == [0, 0]
    ring.enqueue(np.array([[1], [2], [3]], np.float32), ids=[10, 20, 30])  # R = 3 does not divide M
    assert ring.mem[:, 0].tolist() == [1, 2, 3, 0, 0] and ring.ids.tolist() == [10, 20, 30, -1, -1]
    assert ring.state().tolist() == [3, 3]
    ring.enqueue(np.array([[4], [5], [6]], np.float32))  # wraps: slots 3, 4, 0; no ids -> -1
    assert ring.mem[:, 0].tolist() == [6, 2, 3, 4, 5] and ring.ids.tolist() == [-1, 20, 30, -1, -1]
    assert ring.state().tolist() == [1, 5]
    # R = 7 > M from head 1: rows 0 and 1 (slots 1, 2) are overwritten by rows 5 and 6; the last 5 stay
    ring.enqueue(np.arange(7, 14, dtype=np.float32)[:, None], ids=np.arange(7, 14))
    assert ring.mem[:, 0].tolist() == [11, 12, 13, 9, 10] and ring.ids.tolist() == [11, 12, 13, 9, 10]
    assert ring.state().tolist() == [(1 + 7) % 5, 5]
    ring.enqueue(np.array([[14]], np.float32))  # R = 1
    assert ring.mem[:, 0].tolist() == [11, 12, 13, 14, 10] and ring.state().tolist() == [4, 5]
    ring.reset()
    assert ring.state().tolist() == [0, 0] and ring.mem[:, 0].tolist() == [11, 12, 13, 14, 10]  # rows stay, unseen


def test_pool_restatement_agrees_with_brute_force_on_a_hand_case():
    # the 5 anchors of tests/test_mining_host.py, D = 3; candidates 0..4 = P, 5..9 = N, 10..13 = the memory
    a = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 1, 1]], np.float32)
    p = np.array([[0.5, 0, 0], [1, 0.5, 0], [0, 1, 0.25], [0, 0, 2], [1, 1, 0]], np.float32)
    n = np.array([[3, 0, 0], [1, 0.25, 0], [1, 0.25, 0], [0, 0.5, 1], [2, 2, 2]], np.float32)
    mem = np.array([[0, 0.125, 0], [1, 0.25, 0], [0, 0, 1.0625], [0, 0.125, 0]], np.float32)
    ids = np.array([0, 1, 2, 3, 4, 5, 1, 7, 8, 9])
    mem_ids = np.array([50, 1, -1, 0])  # slot 1 is anchor 1's photo, slot 3 anchor 0's
    # worked by hand, euclidean, all four slots filled: anchor 0 is 0.125 from slots 0 and 3
    # (c = 10, 13): the tie goes to c = 10; anchor 1's nearest, N[1] = N[2] = slot 1 =
    # (1, .25, 0), ties at c = 6, 7, 11: the batch row c = 6 wins; anchor 3 takes slot 2
    sel, d_ap, d_sel, dist, valid = xref.mine(a, p, n, mem, 4, 0, 0)
    assert dist.shape == (5, 14) and valid.all(1).sum() == 0 and valid.sum() == 5 * 13
    assert sel.tolist()[:2] == [10, 6] and sel[3] == 12
    assert d_sel[0] == pytest.approx(0.125, abs=1e-5) and d_sel[3] == pytest.approx(0.0625, abs=1e-5)
    # with ids: anchor 0 loses slot 3 only (c = 10 stays), anchor 1 loses c = 6 and slot 1: c = 7
    with_ids = xref.mine(a, p, n, mem, 4, 0, 0, cand_ids=ids, mem_ids=mem_ids)[0]
    assert with_ids.tolist()[:2] == [10, 7]
    # one slot filled: only c = 10 joins the batch
    assert xref.mine(a, p, n, mem, 1, 0, 0)[0].tolist()[:2] == [10, 6]
    assert xref.mine(a, p, n, mem, 1, 0, 0)[0][3] == mref.mine(a, p, n, 0, 0)[0][3]
    # an empty memory (count 0, or no rows at all) is the in-batch selection
    for metric in (0, 1):
        for mode in (0, 1):
            want = mref.mine(a, p, n, mode, metric, cand_ids=ids)[0].tolist()
            assert xref.mine(a, p, n, mem, 0, mode, metric, cand_ids=ids, mem_ids=mem_ids)[0].tolist() == want
            assert xref.mine(a, p, n, np.zeros((0, 3)), 0, mode, metric, cand_ids=ids,
                             mem_ids=np.zeros(0, np.int64))[0].tolist() == want
    # semi-hard: strictly farther than the positive, so anchor 0 (d_ap = 0.5) takes neither slot 0 nor 3
    semi = xref.mine(a, p, n, mem, 4, 1, 0)[0]
    assert semi[0] not in (10, 13) and dist[0, semi[0]] > d_ap[0]
    for metric in (0, 1):
        for mode in (0, 1):
            for count in (0, 1, 3, 4):
                for cid, mid in ((None, None), (ids, mem_ids)):
                    got = xref.mine(a, p, n, mem, count, mode, metric, cand_ids=cid, mem_ids=mid)[0]
                    want = xref.brute_force(a, p, n, mem, count, mode, metric, cid, mid)
                    assert got.tolist() == want.tolist(), (metric, mode, count, cid is not None)
    # NaN slots are never selected
    mem2 = mem.copy()
    mem2[0, 1] = np.nan
    got = xref.mine(a, p, n, mem2, 4, 0, 0)[0]
    assert got[0] == 13 and got.tolist() == xref.brute_force(a, p, n, mem2, 4, 0, 0).tolist()
    # gather and the restricted scatter: ring selections add to no row
    sel = np.array([10, 6, 6, 12, 9])
    out = xref.gather(p, n, mem, sel)
    assert out[0].tolist() == mem[0].tolist() and out[1].tolist() == n[1].tolist() and out[3].tolist() == mem[2].tolist()
    dP, dN = xref.scatter(np.ones((5, 3), np.float32), sel)
    assert dP.sum() == 0 and dN[1].tolist() == [2, 2, 2] and dN[4].tolist() == [1, 1, 1] and dN.sum() == 9
    dP, dN = xref.scatter(np.ones((5, 3), np.float32), np.array([10, 11, 12, 13, 10]))
    assert dP.sum() == 0 and dN.sum() == 0
