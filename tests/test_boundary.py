"""The drop-in boundary without a GPU: the C-ABI library loads and exports every
entry point include/artsbir.h declares, rejects bad shapes with a status and a
message, and the Python mirror of models.py has the reference's constructor
signatures, parameter names and counts (models.py:191-379 of the reference)."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "artsbir.h")


def _declared():
    src = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    src = re.sub(r"//[^\n]*", "", src)
    return sorted(set(re.findall(r"\b(artsbir_[a-z0-9_]+)\s*\(", src)))


def test_library_exports_every_declared_symbol():
    import _hip
    lib = _hip.lib()
    names = _declared()
    assert len(names) >= 40
    missing = [n for n in names if not hasattr(lib, n)]
    assert not missing, missing
    # and the ctypes signature table covers exactly the header
    assert sorted(_hip.SIGNATURES) == names
    assert lib.artsbir_version() >= 1


def test_no_cpu_fallback_when_library_missing(monkeypatch):
    import _hip
    monkeypatch.setattr(_hip, "_lib", None)
    monkeypatch.setattr(_hip, "LIB_PATH", os.path.join(ROOT, "does-not-exist.so"))
    with pytest.raises(RuntimeError, match="no fallback"):
        _hip.lib()


def test_capi_rejects_bad_shapes_without_touching_the_gpu():
    import _hip
    lib = _hip.lib()
    d = _hip.ConvDesc(_hip.DT_BF16, 2, 8, 8, 3, 64, 3, 3, 1, 1)
    rc = lib.artsbir_conv2d_fwd(ctypes.byref(d), None, None, None, 0, 0, 0, None, None, None, 0, None, None)
    assert rc != 0 and b"multiple of 8" in lib.artsbir_last_error()
    rc = lib.artsbir_gemm_nt(_hip.DT_BF16, 16, 16, 12, None, 12, None, None, 16, 0, 0, None, None, None)
    assert rc != 0 and b"K=12" in lib.artsbir_last_error()
    with pytest.raises(_hip.HipError, match="gemm_nt"):
        _hip.call("artsbir_gemm_nt", _hip.DT_BF16, 16, 16, 12, None, 12, None, None, 16, 0, 0, None, None, None)


def test_tail_entry_points_reject_bad_arguments_without_touching_the_gpu():
    """attention pool, tokens, distances and Adam: every argument check sits ahead of
    the launch, so NULL pointers are never read"""
    import _hip
    lib = _hip.lib()

    def refused(name, *args):
        assert getattr(lib, name)(*args) != 0, name
        return lib.artsbir_last_error()

    for dt in (_hip.DT_F32, _hip.DT_BF16):
        for T, msg in ((0, b"tokens=0 outside [1,128]"), (129, b"tokens=129 outside [1,128]")):
            assert msg in refused("artsbir_attnpool_fwd", dt, None, None, 2, 128, 2, T, None, None, None)
            assert msg in refused("artsbir_attnpool_bwd", dt, None, None, None, None, 2, 128, 2, T, None, None, None)
        msg = b"head_dim must be 64 (C=100 heads=2)"  # C != 64 * heads
        assert msg in refused("artsbir_attnpool_fwd", dt, None, None, 2, 100, 2, 5, None, None, None)
        assert msg in refused("artsbir_attnpool_bwd", dt, None, None, None, None, 2, 100, 2, 5, None, None, None)
        assert b"tokens_fwd: C % 8" in refused("artsbir_tokens_fwd", dt, None, None, 2, 4, 12, None, None)
        assert b"tokens_bwd: C % 8" in refused("artsbir_tokens_bwd", dt, None, 2, 4, 12, None, None)
        assert b"tokens_bwd_ex: C % 8" in refused("artsbir_tokens_bwd_ex", dt, None, None, 2, 4, 12, None, None)
    assert b"cosine: shapes 3 vs 5" in refused("artsbir_cosine_fwd", None, 3, None, 5, 8, 1e-8, None, None, None)
    assert b"pairwise_l2: shapes 3 vs 5" in refused("artsbir_pairwise_l2", None, 3, None, 5, 8, 1e-6, None, None)
    assert b"step must be >= 1" in refused("artsbir_adam_step", None, None, 1, 4096, 1e-3, 0.9, 0.999, 1e-8, 0.0, 0, None)
    with pytest.raises(_hip.HipError, match="attnpool"):
        _hip.call("artsbir_attnpool_fwd", _hip.DT_F32, None, None, 2, 128, 2, 129, None, None, None)


def _bnb_desc(**kw):
    """a BatchNorm-backward descriptor of NULL pointers with a valid geometry, then kw"""
    import _hip
    d = _hip.BnBwdDesc()
    d.dtype, d.kind, d.pool, d.ntarget = _hip.DT_F32, 0, 0, 1
    d.B, d.H, d.W, d.C, d.nseg = 2, 4, 4, 64, 1
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def test_bn_and_layout_entry_points_reject_bad_arguments_without_touching_the_gpu():
    """the BatchNorm, element-wise and layout entry points of csrc/elementwise.hip:
    every argument check sits ahead of the launch, so NULL pointers are never read"""
    import _hip
    lib = _hip.lib()

    def refused(name, *args):
        assert getattr(lib, name)(*args) != 0, (name, args)
        return lib.artsbir_last_error()

    C64 = 2 * _hip.NSLOT * 64
    bnb = [
        (dict(C=12), b"bn_bwd: C=12 unsupported"),            # not a multiple of 8
        (dict(C=24), b"bn_bwd: C=24 unsupported"),            # C/8 = 3 does not divide 256
        (dict(C=2056), b"bn_bwd: C=2056 unsupported"),        # C > 2048
        (dict(C=0), b"bn_bwd: C=0 unsupported"),
        (dict(ntarget=0), b"bn_bwd: ntarget must be 1 or 2"),
        (dict(ntarget=3), b"bn_bwd: ntarget must be 1 or 2"),
        (dict(kind=4), b"bn_bwd: kind must be 0 .. 3"),
        (dict(kind=-1), b"bn_bwd: kind must be 0 .. 3"),
        (dict(kind=0, pool=2), b"bn_bwd: pool only with kind 1"),
        (dict(kind=1, pool=3), b"bn_bwd: pool must be <= 2"),
        (dict(kind=1, pool=2, H=5), b"bn_bwd: odd H/W with pool"),
        (dict(kind=1, pool=2, W=7), b"bn_bwd: odd H/W with pool"),
        (dict(B=0), b"bn_bwd: empty geometry 0x4x4"),
        (dict(nseg=3, pstride=4 * 64 - 1, cstride=3 * 64, sstride=C64), b"bn_bwd: segment strides below one parameter block"),
        (dict(nseg=3, pstride=4 * 64, cstride=3 * 64 - 1, sstride=C64), b"bn_bwd: segment strides below one parameter block"),
        (dict(nseg=3, pstride=4 * 64, cstride=3 * 64, sstride=C64 - 1), b"bn_bwd: segment strides below one parameter block"),
        (dict(B=1 << 15, H=1 << 8, W=1 << 8), b"bn_bwd: too many pixels"),
        # units * nseg is the int the launch geometry is sized from: 2^29 pixels in 4 segments
        (dict(B=1 << 13, H=1 << 8, W=1 << 8, nseg=4, pstride=4 * 64, cstride=3 * 64, sstride=C64), b"bn_bwd: too many pixels"),
    ]
    for kw, msg in bnb:
        for entry in ("artsbir_bn_bwd_reduce", "artsbir_bn_bwd_apply"):
            assert msg in refused(entry, ctypes.byref(_bnb_desc(**kw)), None), (kw, lib.artsbir_last_error())
    assert b"unknown dtype 7" in refused("artsbir_bn_bwd_apply", ctypes.byref(_bnb_desc(dtype=7)), None)
    # at pool 2 the reduce writes no g (one store per quad would drop three pixels): only the apply takes gout
    assert b"bn_bwd_reduce: gout with pool 2" in refused(
        "artsbir_bn_bwd_reduce", ctypes.byref(_bnb_desc(kind=1, pool=2, gout=ctypes.c_void_p(64))), None)

    buf = ctypes.c_void_p(64)  # a non-NULL pointer that is never read
    for dt in (_hip.DT_F32, _hip.DT_BF16):
        assert b"bn_stats_det: bad arguments" in refused("artsbir_bn_stats_det", dt, None, 1, 4, 8, buf, 512, None)
        assert b"bn_stats_det: bad arguments" in refused("artsbir_bn_stats_det", dt, buf, 1, 4, 8, None, 512, None)
        assert b"bn_stats_det: bad arguments" in refused("artsbir_bn_stats_det", dt, buf, 0, 4, 8, buf, 512, None)
        assert b"bn_stats_det: bad arguments" in refused("artsbir_bn_stats_det", dt, buf, 1, 0, 8, buf, 512, None)
        assert b"bn_stats_det: bad arguments" in refused("artsbir_bn_stats_det", dt, buf, 1, 4, 0, buf, 512, None)
        assert b"bn_stats_det: seg_stride < NSLOT*2*C" in refused("artsbir_bn_stats_det", dt, buf, 2, 4, 8, buf, 511, None)
        assert b"act_pool: C % 8" in refused("artsbir_act_pool", dt, None, None, 1, 0, 2, 4, 4, 12, 1, None, None)
        assert b"act_pool: C % 8" in refused("artsbir_act_pool", dt, None, None, 1, 0, 2, 4, 4, 0, 1, None, None)
        assert b"act_pool: 3 segments do not split 4 images" in refused(
            "artsbir_act_pool", dt, None, None, 1, 0, 4, 4, 4, 8, 3, None, None)
        assert b"act_pool: 0 segments do not split 4 images" in refused(
            "artsbir_act_pool_colsum", dt, None, None, 1, 0, 4, 4, 4, 8, 0, None, None, None)
        assert b"act_pool: H,W not divisible by pool" in refused(
            "artsbir_act_pool", dt, None, None, 1, 2, 2, 5, 4, 8, 1, None, None)
        assert b"act_pool: H,W not divisible by pool" in refused(
            "artsbir_act_pool_colsum", dt, None, None, 1, 2, 2, 4, 7, 8, 1, None, None, None)
        assert b"block_out: C % 8" in refused("artsbir_block_out", dt, None, buf, None, None, buf, 4, 12, 1, None, None)
        assert b"block_out: C % 8" in refused("artsbir_block_out", dt, None, buf, None, None, buf, 4, 0, 1, None, None)
        assert b"block_out: 3 segments do not split 4 rows" in refused(
            "artsbir_block_out", dt, None, buf, None, None, buf, 4, 8, 3, None, None)
        assert b"block_out: need downsample or identity input" in refused(
            "artsbir_block_out", dt, None, buf, None, None, None, 4, 8, 1, None, None)
        assert b"block_out: missing BN parameter block" in refused(
            "artsbir_block_out_mask", dt, None, buf, buf, None, None, 4, 8, 1, None, None, None)
        assert b"block_out: missing BN parameter block" in refused(
            "artsbir_block_out_colsum", dt, None, None, None, None, buf, 4, 8, 1, None, None, None, None)
        assert b"colsum: C and ld must be multiples of 8" in refused("artsbir_colsum", dt, None, 4, 12, 8, None, None)
        assert b"colsum: C and ld must be multiples of 8" in refused("artsbir_colsum", dt, None, 4, 16, 12, None, None)
        assert b"pack_input: Cin=9 > 8" in refused("artsbir_pack_input", dt, None, 1, 9, 4, 4, None, None)
        assert b"pack_weight: ci_pad < Ci" in refused("artsbir_pack_weight", dt, None, 8, 16, 1, 1, 8, 0, 0, None, None)
        assert b"pack_weights: n=0 nblocks=1" in refused("artsbir_pack_weights", dt, buf, 0, 1, None)
        assert b"pack_weights: n=1 nblocks=0" in refused("artsbir_pack_weights", dt, buf, 1, 0, None)
        assert b"pack_weights: n=1 nblocks=1" in refused("artsbir_pack_weights", dt, None, 1, 1, None)
    assert b"cast: bad dtypes" in refused("artsbir_cast", 2, None, _hip.DT_F32, None, 8, None)
    assert b"cast: bad dtypes" in refused("artsbir_cast", _hip.DT_BF16, None, -1, None, 8, None)
    assert b"bn_fold: bad shape" in refused("artsbir_bn_fold", None, 4, 0, None, None, None, None, 1e-5, None, None, None)
    assert b"bn_fold: bad shape" in refused("artsbir_bn_fold", None, 0, 4, None, None, None, None, 1e-5, None, None, None)
    assert b"bn_finalize: train mode needs stats" in refused(
        "artsbir_bn_finalize", None, 8, 4.0, None, None, None, None, None, 0.1, 1e-5, 1, None, None, None, None, None)
    assert b"bn_finalize: eval mode needs running stats" in refused(
        "artsbir_bn_finalize", buf, 8, 4.0, None, None, None, buf, None, 0.1, 1e-5, 0, None, None, None, None, None)
    assert b"bn_bwd_finalize_seg: nseg=0" in refused(
        "artsbir_bn_bwd_finalize_seg", None, 0, 512, 8, 4.0, None, None, 8, None, None, None, None)
    with pytest.raises(_hip.HipError, match="bn_bwd_reduce"):
        _hip.call("artsbir_bn_bwd_reduce", ctypes.byref(_bnb_desc(C=12)), None)


@pytest.mark.parametrize("output_dim,count", [(1024, 38_316_896), (512, 37_267_808)])
def test_modified_resnet_signature_keys_and_counts(output_dim, count):
    import models
    from oracle import encoder as oenc
    m = models.ModifiedResNet((3, 4, 6, 3), output_dim, heads=32, input_resolution=224, width=64)
    ref = oenc.ModifiedResNet((3, 4, 6, 3), output_dim, heads=32, input_resolution=224, width=64)
    assert sum(p.numel() for p in m.parameters()) == count
    sd, rsd = m.state_dict(), ref.state_dict()
    assert list(sd) == list(rsd)
    for k in sd:
        assert sd[k].shape == rsd[k].shape, k
    # a checkpoint written from the reference layout loads strictly
    m.load_state_dict(rsd, strict=True)


def test_classification_head_keys():
    import models
    m = models.ModifiedResNet_with_classification((3, 4, 6, 3), 1024, heads=32, input_resolution=224, width=64,
                                                  num_classes=125)
    keys = list(m.state_dict())
    assert "classifier.weight" in keys and "classifier.bias" in keys  # models.py:370
    assert m.state_dict()["classifier.weight"].shape == (125, 1024)
    assert "classifier2.weight" not in keys


def test_encoder_refuses_cpu_input():
    import models
    m = models.ModifiedResNet((1, 1, 1, 1), 32, heads=8, input_resolution=64, width=16)
    with pytest.raises(RuntimeError, match="GPU"):
        with torch.no_grad():
            m(torch.zeros(1, 3, 64, 64))


def test_grad_order_covers_every_parameter_once():
    import models
    m = models.ModifiedResNet((2, 1, 1, 1), 64, heads=8, input_resolution=64, width=16)
    order = [id(p) for p in m.grad_order()]
    assert len(order) == len(set(order))
    assert sorted(order) == sorted(id(p) for p in m.parameters())
