"""256-pixel tiles that start in one BN segment and end in the next.

pg_supported, sconv_ok and pp256's predicate take a segment of seg_m pixels whenever
seg_m % 64 == 0 and seg_m >= 256, so with seg_m % 256 in {64, 128, 192} a tile holds
the last waves of one segment and the first of the next.  Only then do the second LDS
accumulator (red[1], stats_rseg), the second segment's constants (pg_prm_fill), the
per-wave segment of the epilogues (wseg) and stats_flush's second pass (nsg) run; a
ragged last batch reaches them in training.  Three segments of whole images, seg_m =
320, 384, 448 (5, 6, 7 images of 8x8) and 576 (one 24x24 image) for the 3x3 kernels;
320, 448 and 576 also leave a pixel tail (M % 256 != 0).  The segments' inputs and BN
parameter blocks differ (_convref), so a sum credited to the wrong segment or read with
the wrong segment's constants moves far (test_conv_tiles_inputs.py holds the inputs to
that).  Reference, bars and the way every case runs: _convref.py."""
import pytest
import torch

import _convref as cr
import _hip
import _kernels
from test_tune_table_gpu import FOLD_PREFIX as TUNE_FOLD_PREFIX

pytestmark = pytest.mark.gpu

# images per segment, H, W  -> seg_m
SEGS_1X1 = [(5, 8, 8), (6, 8, 8), (7, 8, 8)]
SEGS_3X3 = SEGS_1X1 + [(1, 24, 24)]
G = 3

# forward: C, Cout, R, stride, pad (the channel shapes the launchers take)
FWD_SHAPES = [(64, 64, 1, 1, 0), (64, 128, 1, 1, 0), (256, 64, 1, 1, 0), (32, 32, 3, 1, 1), (64, 64, 3, 1, 1),
              (8, 32, 3, 2, 1)]
FWD_CFGS = ["0", "1", "2", "3", "4", "5", "10", "15", "19", "20", "22", "24", "25"]


def takes_fwd(cfg, C, Co, R, stride):
    """the launchers' predicates (pgemm.hip, pstream_k.hip, pgemm_glb.hip, conv3x3.hip, pp256.hip)"""
    multi = C % 64 != 0
    if cfg == "20":
        return R == 3 and ((stride == 1 and C in (32, 64) and Co in (32, 64)) or (stride == 2 and C == 8 and Co == 32))
    if C == 8:
        return False  # the stride-2 stem shape is here for sconv alone
    if cfg in ("5", "19"):
        return not multi
    if cfg in ("15", "25"):
        return not multi and Co > 32
    if cfg == "22":
        return C % 32 == 0
    return True


def _fwd_cases():
    out = []
    for C, Co, R, stride, pad in FWD_SHAPES:
        for per, H, W in (SEGS_3X3 if R == 3 else SEGS_1X1):
            if stride == 2:
                # seg_m counts output pixels: 8x8 inputs give 4x4 outputs, 20 / 24 / 28 images per segment;
                # 576: 36 images
                per, H, W = (4 * per, H, W) if (H, W) == (8, 8) else (36, 8, 8)
            for cfg in FWD_CFGS:
                if takes_fwd(cfg, C, Co, R, stride):
                    out.append(((G * per, G, H, W, C, Co, R, stride, pad), cfg))
    return out


FWD_CASES = _fwd_cases()

# fused BN-backward data gradient: the epilogues (kind, targets, res_mode)
ACT = (1, 1, 0)
EPILOGUES = [ACT] + [(kind, nt, rm) for kind in (0, 3) for rm in (1, 2) for nt in (1, 2)]
BNB_CFGS = ["0", "1", "2", "3", "4", "10", "11", "12", "13", "14", "16", "18", "20", "22"]
# Ci (BN / dX channels), Co (dY channels), R, pad
BNB_SHAPES = [(64, 64, 1, 0), (32, 32, 3, 1), (64, 64, 3, 1)]


def takes_bnb(cfg, epi, Ci, Co, R):
    """pg_launch_bnb, pstream_plain_launch, pg_pf_launch, pstream_bnb_launch, pg_glb_launch,
    pg_glb2_launch, sconv_ok and pp256_launch, as the launchers spell them out"""
    kind, nt, rm = epi
    multi = Co % 64 != 0  # the GEMM's reduction channels
    act = epi == ACT
    res = kind in (0, 3) and rm in (1, 2)
    if cfg == "20":
        return R == 3 and Ci in (32, 64) and Co in (32, 64)
    if cfg == "10":
        return True
    if cfg in ("0", "1", "2", "3", "4"):
        return act or (res and not multi)
    if multi:
        return cfg == "22" and act
    if cfg in ("11", "12", "13"):
        return act or (kind == 3 and rm != 0)
    if cfg == "14":
        return Ci >= 64 and (act or res)
    if cfg == "18":
        return kind == 3 and nt == 1 and rm != 0
    return act or res  # 16, 22


def _bnb_cases():
    out = []
    for Ci, Co, R, pad in BNB_SHAPES:
        for per, H, W in (SEGS_3X3 if R == 3 else SEGS_1X1):
            for epi in (EPILOGUES if R == 1 else [ACT]):
                for cfg in BNB_CFGS:
                    if takes_bnb(cfg, epi, Ci, Co, R):
                        out.append(((G * per, G, H, W, Ci, Co, R, pad) + epi, cfg))
    return out


BNB_CASES = _bnb_cases()
PROBLEMS = sorted({("fwd", k) for k, _ in FWD_CASES} | {("bnb", k) for k, _ in BNB_CASES})


@pytest.mark.parametrize("key,cfg", FWD_CASES, ids=lambda v: v if isinstance(v, str) else cr.ident(v))
def test_straddle_forward_stats(key, cfg, dev):
    cr.run_fwd(cr.Fwd(key), cfg, dev, f"straddle fwd {cr.ident(key)}")


@pytest.mark.parametrize("key,cfg", BNB_CASES, ids=lambda v: v if isinstance(v, str) else cr.ident(v))
def test_straddle_dgrad_bn_reduce(key, cfg, dev):
    cr.run_bnb(cr.Bnb(key), cfg, dev, f"straddle bnb {cr.ident(key)}")


FOLD_PREFIX = dict(TUNE_FOLD_PREFIX, **{"17": "pstream_kernel<32,"})


@pytest.mark.parametrize("fused", [False, True], ids=["plain", "bnb"])
@pytest.mark.parametrize("cfg", ["2", "10", "14", "16", "17", "19", "22"])
def test_straddle_fold_whole_batch_refused(cfg, fused, dev):
    """The per-segment-weight fold (artsbir_conv1x1_dgrad_fold, three segments of 320 pixels).  A tile
    that straddled two segments would need two weight sets, so pg_fold_ok refuses every tiled and
    streaming candidate for the whole batch (seg_m % 256 != 0) and the entry point launches each
    segment on its own (fold_dgrad), where no tile straddles — on the same two-operand kernels, so a
    `fold>` name IS reported and cannot tell the two routes apart (test_fold_gpu.py asserts that name
    for its 196-pixel case).  What tells them apart is the result: the segments' weights differ by
    factors 1, 2, 3 and their biases by whole units, so a tile of a whole-batch launch that read
    one segment's weights for another's pixels is far outside the bar.  The name is held to the forced
    candidate's fold form or the concatenated-operand fallback, never another candidate's kernel."""
    G_, per, H, W, Co, Ci = 3, 5, 8, 8, 256, 64
    B, M = G_ * per, G_ * per * H * W
    seg_m = M // G_
    seg = torch.arange(M) // seg_m
    g = torch.Generator().manual_seed(23)
    gr = cr.bf(torch.randn(M, Co, generator=g))
    x = cr.bf(torch.relu(torch.randn(M, Ci, generator=g)) + 0.5 * seg.view(-1, 1))
    w = cr.bf(torch.randn(G_, Ci, Co + Ci, generator=g) / (Co + Ci) ** 0.5 * (1 + torch.arange(G_)).view(-1, 1, 1))
    bias = torch.randn(G_, Ci, generator=g) + torch.arange(G_).view(-1, 1)
    ref = torch.einsum("pk,pik->pi", torch.cat([gr, x], 1), w[seg]) + bias.double()[seg]
    gd, xd, wd, bd = gr.to(dev, cr.BF), x.to(dev, cr.BF), w.to(dev, cr.BF), bias.to(dev)
    d = _hip.conv_desc(cr.BF, B, H, W, Ci, Co, 1, 1, 1, 0)
    desc, slots, p = None, None, None
    if fused:  # kind 1 on top: the mask of relu(bn2(y2)), sum g', sum g' xhat_2 (Bnb's y, parameters and mask)
        p = cr.Bnb((B, G_, H, W, Ci, 64, 1, 0, 1, 1, 0))
        ref = torch.where(p.keep, ref, torch.zeros_like(ref))
        yd, prm = p.ys[0].to(dev, cr.BF), p.params[0].to(dev)
        slots = [torch.zeros(G_, _hip.NSLOT, 2, Ci, device=dev) for _ in range(2)]
        desc = _hip.BnBwdDesc()
        desc.dtype, desc.kind, desc.pool, desc.ntarget = _hip.DT_BF16, 1, 0, 1
        desc.mask_bn = prm.data_ptr()
        desc.y[0], desc.mean[0], desc.istd[0] = yd.data_ptr(), prm.data_ptr(), prm[0, 1].data_ptr()
        desc.B, desc.H, desc.W, desc.C = B, H, W, Ci

    def launch(o, i):
        if fused:
            desc.slots[0] = slots[i].data_ptr()
        _hip.call("artsbir_conv1x1_dgrad_fold", d, gd.data_ptr(), xd.data_ptr(), wd.data_ptr(), bd.data_ptr(),
                  o.data_ptr(), desc, G_, 4 * Ci, _hip.stream())

    with cr.forced(cfg):
        dx = cr._twice(launch, (M, Ci), dev)
    name = _kernels.last_kernel()
    assert "fold" not in name or (name.startswith(FOLD_PREFIX[cfg]) and name.endswith("fold>")), (cfg, name)
    r = cr.Report(f"straddle fold 3x320 cfg {cfg} {'bnb' if fused else 'plain'} {name}")
    r.out("dx", dx.double().cpu(), ref)
    if fused:
        # the fold kernels sum the f32 result; the concatenated-operand fallback stores g and sums the
        # stored values in a pass of its own (_convref.run_bnb)
        gs = ref if "fold" in name else dx.double().cpu()
        s = slots[0].double().sum(1).cpu().numpy()
        r.sums("sum g", s[:, 0], gs, G_)
        r.sums("sum g xhat", s[:, 1], gs * p.xhat[0], G_)
    r.done()


