"""In-batch negative mining without a GPU: the three entry points exist and refuse bad
arguments ahead of any launch, the training entry has the --negatives switch, the
synthetic dataset can carry the photo identities, and the float64 restatement the
GPU tests lean on (tests/_mining_ref.py) agrees with a brute-force loop."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import _mining_ref as mref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("artsbir_mine_negatives", "artsbir_rows_gather2", "artsbir_rows_scatter2")


def test_entry_points_declared_exported_and_bound():
    import _hip
    header = open(os.path.join(ROOT, "include", "artsbir.h")).read()
    lib = _hip.lib()
    for name in ENTRIES:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert hasattr(lib, name), name
        assert name in _hip.SIGNATURES, name
    assert len(_hip.SIGNATURES["artsbir_mine_negatives"]) == 13
    assert len(_hip.SIGNATURES["artsbir_rows_gather2"]) == 7
    assert len(_hip.SIGNATURES["artsbir_rows_scatter2"]) == 7


def test_entry_points_reject_bad_arguments_without_touching_the_gpu():
    """every argument check sits ahead of the launch, so NULL pointers are never read
    and the non-NULL stand-ins are never dereferenced"""
    import _hip
    lib = _hip.lib()
    buf = ctypes.c_void_p(64)  # a non-NULL pointer that is never read

    def refused(name, *args):
        assert getattr(lib, name)(*args) != 0, (name, args)
        return lib.artsbir_last_error()

    def mine(metric=0, mode=0, a=buf, p=buf, n=buf, B=4, D=8, ids=None, sel=buf, d_ap=buf, d_sel=buf):
        return refused("artsbir_mine_negatives", metric, mode, a, p, n, B, D, 1e-6, ids, sel, d_ap, d_sel, None)

    big = (1 << 20) + 1
    assert b"mine_negatives: B=0 must be >= 1" in mine(B=0)
    assert b"mine_negatives: B=-3 must be >= 1" in mine(B=-3)
    assert b"mine_negatives: D=0 must be >= 1" in mine(D=0)
    assert b"mine_negatives: B=1048577 above 2^20" in mine(B=big)
    for bad in (-1, 2):
        assert b"mine_negatives: metric=%d outside {0, 1}" % bad in mine(metric=bad)
        assert b"mine_negatives: mode=%d outside {0, 1}" % bad in mine(mode=bad)
    for arg in ("a", "p", "n", "sel", "d_ap", "d_sel"):
        assert b"mine_negatives: NULL pointer" in mine(**{arg: None})
    # all of them NULL with a bad shape: the shape is refused first, nothing is read
    assert b"mine_negatives: B=0" in mine(B=0, a=None, p=None, n=None, sel=None, d_ap=None, d_sel=None)

    def gather(p=buf, n=buf, sel=buf, B=4, D=8, out=buf):
        return refused("artsbir_rows_gather2", p, n, sel, B, D, out, None)

    def scatter(dout=buf, sel=buf, B=4, D=8, dp=buf, dn=buf):
        return refused("artsbir_rows_scatter2", dout, sel, B, D, dp, dn, None)

    for fn, tag in ((gather, b"rows_gather2"), (scatter, b"rows_scatter2")):
        assert tag + b": B=0 must be >= 1" in fn(B=0)
        assert tag + b": D=0 must be >= 1" in fn(D=0)
        assert tag + b": D=-1 must be >= 1" in fn(D=-1)
        assert tag + b": B=1048577 above 2^20" in fn(B=big)
    for arg in ("p", "n", "sel", "out"):
        assert b"rows_gather2: NULL pointer" in gather(**{arg: None})
    for arg in ("dout", "sel", "dp", "dn"):
        assert b"rows_scatter2: NULL pointer" in scatter(**{arg: None})
    with pytest.raises(_hip.HipError, match="mine_negatives"):
        _hip.call("artsbir_mine_negatives", 0, 3, None, None, None, 4, 8, 1e-6, None, None, None, None, None)


def test_python_surface_refuses_cpu_tensors_and_bad_names():
    import losses
    a, p, n = (torch.zeros(4, 8) for _ in range(3))
    with pytest.raises(RuntimeError, match="CUDA tensors"):
        losses.mine_negatives(a, p, n)
    with pytest.raises(ValueError, match="mode"):
        losses.mine_negatives(a, p, n, mode="easiest")
    with pytest.raises(ValueError, match="metric"):
        losses.MinedNegatives(losses.TripletMarginLoss(0.2), "hardest", "manhattan")


def test_parse_args_negatives():
    import train
    assert train.parse_args([]).negatives == "given"
    for v in ("given", "hardest", "semihard"):
        assert train.parse_args(["--negatives", v]).negatives == v
    with pytest.raises(SystemExit):
        train.parse_args(["--negatives", "random"])


@pytest.mark.parametrize("loss_type,with_cls,dataset,inner", [
    ("euclidean", False, "SyntheticTripletDataset", "TripletMarginLoss"),
    ("cosine", False, "SyntheticTripletDataset", "TripletMarginWithDistanceLoss"),
    ("euclidean", True, "SketchyV2", "TripletMarginLoss_with_classification"),
    ("cosine", True, "KaggleV2", "TripletMarginLoss_with_classification2"),
])
def test_make_loss_wraps_only_when_mining(loss_type, with_cls, dataset, inner):
    import losses
    import train
    plain = train.make_loss(loss_type, with_cls, dataset, 0.3)
    assert type(plain).__name__ == inner
    assert type(train.make_loss(loss_type, with_cls, dataset, 0.3, "given")).__name__ == inner
    for mode in ("hardest", "semihard"):
        mined = train.make_loss(loss_type, with_cls, dataset, 0.3, mode)
        assert isinstance(mined, losses.MinedNegatives)
        assert type(mined.loss_fn).__name__ == inner
        assert (mined.mode, mined.metric) == (mode, loss_type)
        assert mined.margin == plain.margin == 0.3
        if with_cls:
            assert mined.classification_weight == plain.classification_weight
            assert mined.classification_weight2 == plain.classification_weight2
        assert mined.mined_fraction() == 0.0  # nothing seen yet


def test_dataset_ids_leave_the_draws_and_images_alone():
    import data_preparation
    kw = dict(n=40, resolution=8, seed=42)
    plain, _ = data_preparation.get_datasets("Synthetic", **kw)
    items = [plain[i] for i in range(12)]            # the draws continue the stream seeded at construction
    with_ids, _ = data_preparation.get_datasets("Synthetic", ids=True, **kw)
    hits = 0
    for i, ref in enumerate(items):
        item = with_ids[i]
        assert len(ref) == 3 and len(item) == 5
        for x, y in zip(ref, item[:3]):
            assert torch.equal(x, y)
        pos_id, neg_id = item[3], item[4]
        assert pos_id.dtype == neg_id.dtype == torch.int64 and pos_id.shape == neg_id.shape == ()
        assert int(pos_id) == data_preparation.photo_number(with_ids.photo_paths[i])
        same_image = torch.equal(item[1], item[2])   # the draw hit the positive's photo
        assert (int(pos_id) == int(neg_id)) == same_image
        hits += same_image
    # a draw that does hit the positive: the negative's id is then the positive's
    ds = data_preparation.SyntheticTripletDataset(n=2, resolution=8, split_ratio=0.5, ids=True)
    assert len(ds.photo_paths) == 1
    item = ds[0]
    assert int(item[3]) == int(item[4]) and torch.equal(item[1], item[2])
    # and the collated batch carries them as int64 [B]
    batch = torch.utils.data.default_collate([with_ids[0], with_ids[1]])
    assert batch[3].dtype == torch.int64 and batch[3].shape == (2,) and batch[4].shape == (2,)


def test_reference_agrees_with_brute_force_on_a_hand_case():
    # 5 anchors, D = 3; candidates 0..4 = P, 5..9 = N
    a = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 1, 1]], np.float32)
    p = np.array([[0.5, 0, 0], [1, 0.5, 0], [0, 1, 0.25], [0, 0, 2], [1, 1, 0]], np.float32)
    n = np.array([[3, 0, 0], [1, 0.25, 0], [1, 0.25, 0], [0, 0.5, 1], [2, 2, 2]], np.float32)
    ids = np.array([0, 1, 2, 3, 4, 5, 1, 7, 8, 9])  # candidate 6 is anchor 1's photo again
    # worked by hand, euclidean: anchor 0 (its own P[0] is out) is 1.031 from P[2] = (0, 1, .25)
    # and from N[1] = N[2] = (1, .25, 0), i.e. c = 2, 6, 7: the tie goes to c = 2
    sel, d_ap, d_sel, dist = mref.mine(a, p, n, 0, 0)
    assert sel[0] == 2 and sel[1] == 6 and sel[3] == 8
    assert d_ap == pytest.approx([0.5, 0.5, 0.25, 1.0, 1.0], abs=1e-5)
    # with ids anchor 1 may not take c = 6 any more: the bit-identical c = 7 is next
    assert mref.mine(a, p, n, 0, 0, cand_ids=ids)[0][1] == 7
    # semi-hard: strictly farther than the positive
    semi = mref.mine(a, p, n, 1, 0)[0]
    assert dist[1, semi[1]] > d_ap[1] and semi[1] != 6  # d(1, 6) = 0.25 < d_ap = 0.5
    for metric in (0, 1):
        for mode in (0, 1):
            for cid in (None, ids):
                got = mref.mine(a, p, n, mode, metric, cand_ids=cid)[0]
                want = mref.brute_force(a, p, n, mode, metric, cid)
                assert got.tolist() == want.tolist(), (metric, mode, cid is not None)
    # NaN candidates are never selected, and a NaN anchor falls back to B + i
    n2 = n.copy()
    n2[1, 0] = np.nan
    a2 = a.copy()
    a2[4, 2] = np.nan
    got = mref.mine(a2, p, n2, 0, 0)[0]
    assert 6 not in got.tolist() and got[4] == 9
    assert got.tolist() == mref.brute_force(a2, p, n2, 0, 0).tolist()
    # the f32 restatement selects the same on this case, and the scatter adds in order
    assert mref.mine(a, p, n, 0, 0, dtype=np.float32)[0].tolist() == sel.tolist()
    dP, dN = mref.scatter(np.ones((5, 3), np.float32), np.array([7, 7, 0, 9, 7]))
    assert dN[2].tolist() == [3, 3, 3] and dP[0].tolist() == [1, 1, 1] and dN[4].tolist() == [1, 1, 1]
    assert dP[1:].sum() == 0 and dN[[0, 1, 3]].sum() == 0
    # decided: the tie of anchor 0 is not, an anchor with clear gaps is
    dec = mref.decided(dist, mref.valid_mask(5), 0, 3, 0)
    assert dec.tolist() == [False, False, True, True, False]  # anchors 1 and 4 tie too
