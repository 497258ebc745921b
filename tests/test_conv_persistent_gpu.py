"""Persistent workgroups that run more than one tile.

pstream_kernel (candidates 10, 14, 15, 24, 25, the fold forms 10 / 14 / 17 and the fold with its
weight-gradient operands) launches min(tiles, 256) workgroups, sconv_kernel (candidate 20) 256 x its
occupancy (<= 4).  Only past that many tiles does a workgroup own two: the stage ring runs across the
tile boundary, the flushing wave zeroes the LDS accumulators before the next stage barrier,
stats_flush counts to NWC (ti + 1) - 1, pg_epilogue_fwd carries WaveStats across tiles and flushes on
a segment or channel-block change, pstream_wg_loader accumulates g^T x / x^T x across tiles, the
G % 8 == 0 slot remap applies and the last round is ragged.  Tile t covers pixel tile t / ntc and
channel block t % ntc.  The smallest shapes past 256 tiles:

  B1  1x1 64 -> 64, 64-channel blocks, ntc = 1: 1029 images of 8x8 (257.25 -> 258 tiles) and 2060
      (515 tiles, two or three per workgroup, no tail)
  B2  1x1 64 -> 320, 128-channel blocks with a partial last one, ntc = 3 (does not divide 256, so a
      workgroup's consecutive tiles change channel block): 349 images (88 pixel tiles, 264 tiles), and
      352 images for the layouts 349 (a prime) cannot be cut into
  B3  3x3 32 -> 32, 32-channel blocks on the several-taps-per-stage path: 1025 images (65600 pixels)
  B4  the fold, K = 320 (256 + 64), Cout = 64: 1028 images (65792 pixels, 257 tiles)
  sconv  <8,32,s2> forward at 21 x 224^2 (1029 tiles) and <32,32,bnb> kind 1 at 21 x 112^2 (263424
      pixels): more than 1024 tiles, a second tile for every occupancy

in two kinds of segment layout.  Carried sums: one segment (three equal ones where the batch
divides), a workgroup's tiles in one segment.  Attribution: the most segments the predicates admit
(seg_m >= 256, seg_m % 64 == 0, whole images): one 256-pixel tile per segment where M % 256 == 0 (515
in B1, 88 in B2, 257 in B4), else the smallest straddling segment the batch divides into (448 pixels
x 147 in B1, 320 x 205 in B3) — every tile's sums checked nearly on their own, a dropped, doubled or
misfiled tile loud.  Reference, bars and how a case runs: _convref.py."""
import pytest
import torch

import _convref as cr
import _hip
import _kernels
import _tail
from test_tune_table_gpu import FOLD_PREFIX as TUNE_FOLD_PREFIX

pytestmark = pytest.mark.gpu

ACT = (1, 1, 0)
# candidate 14's five compile-time epilogues <BK, TWO>: (kind, targets, res_mode)
K14 = [ACT, (3, 2, 1), (3, 1, 2), (0, 2, 2), (0, 1, 1)]
# candidate 10's run-time epilogue: ACT, bits with two targets, bf16 mask with the unpool residual
K10 = [ACT, (3, 2, 1), (0, 1, 2)]

# name, N, layouts (segments), C, Cout, R, pad
PSTREAM = [
    ("B1", 1029, (1, 3, 147), 64, 64, 1, 0),
    ("B1", 2060, (1, 515), 64, 64, 1, 0),
    ("B2", 349, (1,), 64, 320, 1, 0),
    ("B2", 352, (1, 88), 64, 320, 1, 0),
    ("B3", 1025, (1, 5, 205), 32, 32, 3, 1),
]


def _cases():
    fwd, plain, bnb = [], [], []
    for name, N, layouts, C, Co, R, pad in PSTREAM:
        multi = C % 64 != 0
        for cfg in ("10", "15") if not multi else ("10",):
            plain.append((name, (N, 1, 8, 8, C, Co, R, 1, pad), cfg))
        for G in layouts:
            for cfg in ("10", "15", "24", "25") if not multi else ("10", "24"):
                fwd.append((name, (N, G, 8, 8, C, Co, R, 1, pad), cfg))
            # the data gradient of the same instance: dY with C channels, dX / the BN with Cout
            for epi in (K10 if not multi else [ACT]):
                bnb.append((name, (N, G, 8, 8, Co, C, R, pad) + epi, "10"))
            if not multi:
                for epi in K14:
                    bnb.append((name, (N, G, 8, 8, Co, C, R, pad) + epi, "14"))
    return fwd, plain, bnb


FWD_CASES, PLAIN_CASES, BNB_CASES = _cases()
SCONV_FWD = [(21, G, 224, 224, 8, 32, 3, 2, 1) for G in (1, 3)]
SCONV_BNB = [(21, G, 112, 112, 32, 32, 3, 1) + ACT for G in (1, 3)]
# fold: N, G, H, W, Co (g channels), Ci (x / dx channels)
FOLD_SHAPES = [(1028, 1, 8, 8, 256, 64), (1028, 257, 8, 8, 256, 64)]
FOLD_FORMS = [("10", False), ("14", True), ("17", False), ("17", True), ("wg", False), ("wg", True)]
FOLD_PREFIX = dict(TUNE_FOLD_PREFIX, **{"17": "pstream_kernel<32,", "wg": "pstream_kernel<64,"})
PROBLEMS = sorted({("fwd", k) for _, k, _ in FWD_CASES} | {("bnb", k) for _, k, _ in BNB_CASES}
                  | {("fwd", k) for k in SCONV_FWD} | {("bnb", k) for k in SCONV_BNB}
                  | {("fold", k + (fused, form == "wg")) for k in FOLD_SHAPES for form, fused in FOLD_FORMS
                     if fused or form == "wg"})  # the plain fold without wg has no sums


def _id(v):
    return cr.ident(v) if isinstance(v, tuple) else str(v)


@pytest.mark.parametrize("name,key,cfg", FWD_CASES, ids=_id)
def test_persistent_forward_stats(name, key, cfg, dev):
    cr.run_fwd(cr.Fwd(key), cfg, dev, f"persistent {name} fwd {cr.ident(key)}")


@pytest.mark.parametrize("name,key,cfg", PLAIN_CASES, ids=_id)
def test_persistent_forward_plain(name, key, cfg, dev):
    cr.run_fwd(cr.Fwd(key), cfg, dev, f"persistent {name} plain {cr.ident(key)}", stats=False)


@pytest.mark.parametrize("name,key,cfg", BNB_CASES, ids=_id)
def test_persistent_dgrad_bn_reduce(name, key, cfg, dev):
    cr.run_bnb(cr.Bnb(key), cfg, dev, f"persistent {name} bnb {cr.ident(key)}")


@pytest.mark.parametrize("key", SCONV_FWD, ids=cr.ident)
def test_sconv_persistent_forward_stats(key, dev):
    cr.run_fwd(cr.Fwd(key), "20", dev, f"persistent sconv fwd {cr.ident(key)}")
    assert _kernels.last_kernel() == "sconv_kernel<8,32,s2>"


@pytest.mark.parametrize("key", SCONV_BNB, ids=cr.ident)
def test_sconv_persistent_dgrad_bn_reduce(key, dev):
    cr.run_bnb(cr.Bnb(key), "20", dev, f"persistent sconv bnb {cr.ident(key)}")
    assert _kernels.last_kernel() == "sconv_kernel<32,32,bnb>"


@pytest.mark.parametrize("form,fused", FOLD_FORMS, ids=_id)
@pytest.mark.parametrize("shape", FOLD_SHAPES, ids=cr.ident)
def test_persistent_fold(shape, form, fused, dev):
    """B4: [g | x] w_s^T + bias_s with per-segment weights on the streaming fold forms; `wg`: the same
    pass accumulates P_s = g_s^T x_s and Gram_s = x_s^T x_s in its loader waves
    (artsbir_conv1x1_dgrad_fold_wg).  P and Gram are neither statistics nor slots;
    their bars are set here.  P (16384 elements per segment, terms of both signs) is held per element to
    8 * 2^-24 * sum |term|, the floor of the sums' bar alone and the tighter of its two parts.  Gram's
    terms are products of the non-negative x and do not cancel, so any float32 accumulation of the
    65792 terms of an element drifts by tens of 2^-24 of the sum and the floor cannot hold: Gram is held
    to _tail.check_f32 as it stands, max |err| / max |ref| <= 8 x that of the sequential float32
    accumulation of the float64 terms in pixel order (Fold.xtx_seq)."""
    p = cr.Fold(shape + (fused, form == "wg"))
    N, G, H, W, Co, Ci = shape
    gd, xd, wd, bd = p.gr.to(dev, cr.BF), p.x.to(dev, cr.BF), p.w.to(dev, cr.BF), p.bias.to(dev)
    d = _hip.conv_desc(cr.BF, N, H, W, Ci, Co, 1, 1, 1, 0)
    desc, slots = None, None
    if fused:
        yd, prm = p.bnb.ys[0].to(dev, cr.BF), p.bnb.params[0].to(dev)
        slots = [torch.zeros(G, _hip.NSLOT, 2, Ci, device=dev) for _ in range(2)]
        desc = _hip.BnBwdDesc()
        desc.dtype, desc.kind, desc.pool, desc.ntarget = _hip.DT_BF16, 1, 0, 1
        desc.mask_bn = prm.data_ptr()
        desc.y[0], desc.mean[0], desc.istd[0] = yd.data_ptr(), prm.data_ptr(), prm[0, 1].data_ptr()
        desc.B, desc.H, desc.W, desc.C = N, H, W, Ci
    acc = [(torch.zeros(G, Co, Ci, device=dev), torch.zeros(G, Ci, Ci, device=dev)) for _ in range(2)]

    def launch(o, i):
        if fused:
            desc.slots[0] = slots[i].data_ptr()
        if form == "wg":
            _hip.call("artsbir_conv1x1_dgrad_fold_wg", d, gd.data_ptr(), xd.data_ptr(), wd.data_ptr(), bd.data_ptr(),
                      o.data_ptr(), desc, G, 4 * Ci, acc[i][0].data_ptr(), acc[i][1].data_ptr(), _hip.stream())
        else:
            _hip.call("artsbir_conv1x1_dgrad_fold", d, gd.data_ptr(), xd.data_ptr(), wd.data_ptr(), bd.data_ptr(),
                      o.data_ptr(), desc, G, 4 * Ci, _hip.stream())

    if form == "wg":
        dx = cr._twice(launch, (p.M, Ci), dev)  # the entry point takes no forced candidate
    else:
        with cr.forced(form):
            dx = cr._twice(launch, (p.M, Ci), dev)
    name = _kernels.last_kernel()
    tail = ("bnbk,fold,wg>" if fused else "<64,fold,wg>") if form == "wg" else "fold>"
    assert name.startswith(FOLD_PREFIX[form]) and name.endswith(tail) and ("bnbk" in name) == fused, (form, name)
    r = cr.Report(f"persistent B4 fold {cr.ident(shape)} {form} {name}")
    r.out("dx", dx.double().cpu(), p.ref)
    if fused:
        s = slots[0].double().sum(1).cpu().numpy()
        r.sums("sum g", s[:, 0], p.ref, G)
        r.sums("sum g xhat", s[:, 1], p.ref * p.bnb.xhat[0], G)
    if form == "wg":
        gtx, gmag = p.gtx()
        err = (acc[0][0].double().cpu() - gtx).abs()
        r.add("g^T x", err.max().item(), (err / (8 * cr.U32 * gmag).clamp_min(1e-300)).max().item())
    r.done()
    if form == "wg":
        _tail.check_f32(f"{r.label} x^T x", acc[0][1], p.xtx()[0], p.xtx_seq())
