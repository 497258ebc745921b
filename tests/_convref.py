"""Shared by the conv-tile parity tests (test infrastructure): test_conv_straddle_gpu.py,
test_conv_persistent_gpu.py, test_rstream_edges_gpu.py, test_conv_tiles_inputs.py, and
the masks / sums test_fused_gpu.py compares with.

The reference works in float64 on the CPU from the same bf16-rounded operands: the
im2col product (torch's float64 convolution), the residual (res_mode 1: same pixel,
2: a quarter of the 2x2-pooled pixel), the ReLU mask (kind 1 from
(y - mean) * scale + beta > 0, kind 0 from a bf16 mask, kind 3 from packed bits) and
the per-segment sums: sum y, sum y^2 of the forward, sum g, sum g * xhat_t of the
fused BN backward for one and two targets.

Bars (none measured on the code under test).  Outputs: atol 2e-2, rtol 1e-2 against
float64, the bar test_pgemm_gpu.py and test_hconv2_gpu.py hold these candidates to.
Sums, per segment and channel, replica slots added in float64:
    |sum - ref64| <= max(8 * e_seq, 8 * 2^-24 * sum |term|)
where e_seq is the error of a sequential float32 accumulation of the float64 terms
in pixel order (numpy.cumsum in float32, the worst plain order): _tail.check_f32's
idiom, its factor 8 over the reference's own f32 evaluation.  _tail.check_atomic_sum's
derived bound n * 2^-24 * sum |term| replaces it where it is tighter (n < 8 terms; no
segment here is that small, the minimum is taken all the same).

Every run forces its candidate through ARTSBIR_PGEMM_CFG and ASSERTS the kernel that
ran (a candidate that does not take its case fails, it is not skipped), starts its
output as NaN and launches twice: the stored outputs must repeat byte for byte.  Each
case prints one "PARITY" line (Report); profiles/conv_tiles_parity.txt is that table
as measured on an MI355X."""
import functools
import os
import re

import numpy as np
import torch
import torch.nn.functional as F

import _hip
import _kernels

U32 = 2.0 ** -24
BF = torch.bfloat16
ATOL, RTOL = 2e-2, 1e-2


def bf(x):
    """rounded to bf16, as float64"""
    return x.to(BF).double()


def nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous()


def flat(x):
    """NCHW -> [pixels][channels]"""
    return x.permute(0, 2, 3, 1).reshape(-1, x.shape[1])


def pack_bits(mask_nhwc):
    """[..., C] -> uint8 [..., C/8]: bit e of byte c = mask[..., 8c+e] > 0"""
    m = (mask_nhwc > 0).to(torch.uint8).reshape(*mask_nhwc.shape[:-1], -1, 8)
    return (m << torch.arange(8, dtype=torch.uint8, device=m.device)).sum(-1).to(torch.uint8)


def bnb_reference(d, kind, ys, means, istds, msc, msh, mask):
    """g = d*mask, sum g, sum g*xhat_t for one segment; tensors [n, C];
    kind 1 masks with the ReLU's BN applied as (y - mean) * scale + beta"""
    if kind == 1:
        keep = ((ys[0] - means[0]) * msc + msh) > 0
    else:
        keep = mask > 0
    g = torch.where(keep, d, torch.zeros_like(d))
    sums = []
    for y, m, s in zip(ys, means, istds):
        xhat = (y - m) * s
        sums.append((g.sum(0), (g * xhat).sum(0)))
    return g, sums


def residual(res, res_mode):
    """the residual term of a data gradient, NCHW: res_mode 1 the same pixel, 2 a quarter of
    the pixel of the 2x2-pooled tensor (AvgPool2d(2) backward)"""
    if res_mode == 1:
        return res
    return 0.25 * F.interpolate(res, scale_factor=2, mode="nearest")


# ---------------------------------------------------------------------------
# bars
def seg_sums(terms, nseg):
    """[M][C] float64 terms -> (ref [nseg][C], bar [nseg][C]); see the module docstring"""
    t = np.ascontiguousarray(terms.numpy() if isinstance(terms, torch.Tensor) else terms, dtype=np.float64)
    t = t.reshape(nseg, -1, t.shape[-1])
    n = t.shape[1]
    ref = t.sum(1)
    seq = np.cumsum(t, axis=1, dtype=np.float32)[:, -1].astype(np.float64)
    mag = np.abs(t).sum(1)
    bar = np.maximum(8 * np.abs(seq - ref), 8 * U32 * mag)
    return ref, np.minimum(bar, n * U32 * mag)


class Report:
    """the checks of one case: one "PARITY" line (pytest -s) with, per checked quantity, the kernel's
    largest error and (in brackets) the largest error / bar; done() prints it, then asserts every bar"""

    def __init__(self, label):
        self.label, self.parts, self.missed = label, [], []

    def add(self, name, err, worst):
        self.parts.append(f"{name} {err:.2e} ({worst:.2e})")
        if not worst <= 1.0:
            self.missed.append((name, err, worst))

    def out(self, name, got, ref):
        """a stored bf16 result [M][C] against float64"""
        assert torch.isfinite(got).all(), (self.label, name)
        err = (got - ref).abs()
        self.add(name, err.max().item(), (err / (ATOL + RTOL * ref.abs())).max().item())

    def sums(self, name, got, terms, nseg):
        """got [nseg][C] (float64) against the float64 sums of terms [M][C]"""
        got = np.asarray(got, dtype=np.float64)
        ref, bar = seg_sums(terms, nseg)
        assert got.shape == ref.shape, (got.shape, ref.shape)
        assert np.isfinite(got).all(), (self.label, name)
        err = np.abs(got - ref)
        self.add(name, float(err.max()), float((err / np.maximum(bar, 1e-300)).max()))

    def done(self):
        print(f"PARITY {self.label}: " + " | ".join(self.parts))
        assert not self.missed, (self.label, self.missed)


def sensitivity(term_sets, nseg, slice_px):
    """The condition on a case's inputs: taking any single slice of slice_px pixels (one wave's share
    of a tile) out of the float64 sums, or crediting it to the neighbouring segment, moves some
    checked sum of some channel by more than 4 x its bar.  Either change moves a segment's sum by
    the slice's own sum, so:  min over slices of  max over sums, channels of  |slice sum| / (4 bar)."""
    ratio = None
    for terms in term_sets:
        t = np.ascontiguousarray(terms.numpy(), dtype=np.float64)
        M, C = t.shape
        seg_m = M // nseg
        assert seg_m % slice_px == 0 or nseg == 1
        _, bar = seg_sums(t, nseg)
        pad = (-M) % slice_px
        if pad:
            t = np.concatenate([t, np.zeros((pad, C))])
        s = np.abs(t.reshape(-1, slice_px, C).sum(1))                  # [slices][C]
        seg = np.minimum(np.arange(s.shape[0]) * slice_px // seg_m, nseg - 1)
        r = (s / np.maximum(4 * bar[seg], 1e-300)).max(1)
        ratio = r if ratio is None else np.maximum(ratio, r)
    return float(ratio.min())


# ---------------------------------------------------------------------------
# problems: inputs and float64 results on the CPU.  The expensive part (the float64 convolution)
# depends on the shape alone and is computed once; the segment layouts share it.
def _zones(N):
    """image -> one of three statistical zones: the inputs' means differ along the batch
    whatever the segment layout, so a sum credited to another segment moves far"""
    return (torch.arange(N) * 3 // N).double()


@functools.lru_cache(maxsize=3)
def _fwd_raw(N, H, W, C, Co, R, stride, pad):
    g = torch.Generator().manual_seed(1000 * H + 10 * W + 7 * C + Co + N + 31 * R)
    x = torch.randn(N, C, H, W, generator=g).double()
    x += 0.5 * _zones(N).view(-1, 1, 1, 1) + 0.25 * torch.randn(1, C, 1, 1, generator=g).double()
    x = bf(x)
    w = bf(torch.randn(Co, C, R, R, generator=g) / (C * R * R) ** 0.5)
    y = flat(F.conv2d(x, w, stride=stride, padding=pad))
    return x, w, y


@functools.lru_cache(maxsize=3)
def _dgrad_raw(N, H, W, Ci, Co, R, pad):
    """dY [N][Co][H][W], w [Co][Ci][R][R], and the raw data gradient [M][Ci] (float64)"""
    g = torch.Generator().manual_seed(2000 * H + 10 * W + 7 * Ci + Co + N + 31 * R)
    dy = bf(torch.randn(N, Co, H, W, generator=g))
    w = bf(torch.randn(Co, Ci, R, R, generator=g) / (Co * R * R) ** 0.5)
    return dy, w, flat(torch.nn.grad.conv2d_input((N, Ci, H, W), w, dy, stride=1, padding=pad))


class Fwd:
    """forward convolution with per-segment statistics: key (N, G, H, W, C, Co, R, stride, pad)"""

    def __init__(self, key):
        self.key = key
        N, G, H, W, C, Co, R, stride, pad = key
        self.x, self.w, self.y = _fwd_raw(N, H, W, C, Co, R, stride, pad)
        self.G, self.M = G, self.y.shape[0]
        self.slice_px = 64

    def term_sets(self):
        return [self.y, self.y * self.y]


class Bnb:
    """data gradient with the fused BN-backward reduction:
    key (N, G, H, W, Ci, Co, R, pad, kind, ntarget, res_mode); Ci: the BN's (dX) channels"""

    def __init__(self, key, slice_px=64):
        self.key = key
        N, G, H, W, Ci, Co, R, pad, kind, nt, rm = key
        self.dy, self.w, d = _dgrad_raw(N, H, W, Ci, Co, R, pad)
        g = torch.Generator().manual_seed(17 + 3 * G + 5 * kind + 7 * nt + 11 * rm + N + Ci)
        self.res = None
        if rm:
            self.res = bf(torch.randn(N, Ci, *((H, W) if rm == 1 else (H // 2, W // 2)), generator=g))
            d = d + flat(residual(self.res, rm))
        per = N // G
        M = d.shape[0]
        seg_m = M // G
        zone = (torch.arange(N) // per % 3).double().view(-1, 1, 1, 1)  # the segment of each image, mod 3
        self.ys = [flat(bf(torch.randn(N, Ci, H, W, generator=g).double() + 0.5 * zone)) for _ in range(nt)]
        self.mask = flat(bf(torch.randn(N, Ci, H, W, generator=g)))
        # a BN parameter block per segment and target (mean, istd, scale, beta): means shifted and
        # istd scaled by the segment (mod 3: neighbours differ, values stay O(1)), |scale| >= 1/4.
        # The kind-1 ReLU threshold stays within 0.8 standard deviations of y's mean (mean within
        # 0.3, beta within half a scale), so every channel keeps a fifth of its pixels or more:
        # the sums' bar scales with sum |g|, and the f32 GEMM's own rounding of each g (2^-24 of
        # its K products) has no room in it where a channel keeps a handful of values
        k3 = (torch.arange(G) % 3).view(-1, 1)
        self.params = []
        for _ in range(nt):
            p = torch.randn(G, 4, Ci, generator=g)
            p[:, 0] = 0.6 * torch.rand(G, Ci, generator=g) - 0.3 + 0.5 * k3
            p[:, 1] = (p[:, 1].abs() + 0.5) * (1 + 0.5 * k3)
            p[:, 2] = torch.where(p[:, 2] < 0, p[:, 2] - 0.25, p[:, 2] + 0.25)
            p[:, 3] = p[:, 2] * (torch.rand(G, Ci, generator=g) - 0.5)
            self.params.append(p)
        p64 = [p.double() for p in self.params]
        rows = lambda v: v.repeat_interleave(seg_m, 0)  # noqa: E731  [G][Ci] -> [M][Ci]
        if kind == 1:
            # no ReLU decision within rounding of its threshold: move such y by whole bf16 steps
            y0 = self.ys[0]
            for _ in range(8):
                pre = (y0 - rows(p64[0][:, 0])) * rows(p64[0][:, 2]) + rows(p64[0][:, 3])
                amb = pre.abs() < 1e-3
                if not amb.any():
                    break
                y0[amb] = bf(y0[amb] + torch.clamp(y0[amb].abs() / 64, min=0.0625))
            assert not amb.any()
            keep = pre > 0
        else:
            keep = self.mask > 0
        self.keep = keep
        self.g = torch.where(keep, d, torch.zeros_like(d))
        self.xhat = [(y - rows(p[:, 0])) * rows(p[:, 1]) for y, p in zip(self.ys, p64)]
        self.G, self.M = G, M
        self.slice_px = slice_px

    def term_sets(self):
        return [self.g] + [self.g * xh for xh in self.xhat]


_XTX_SEQ = {}


class Fold:
    """the folded BN backward's data gradient dx = [g | x] w_s^T + bias_s with weights and bias per
    segment s (artsbir_conv1x1_dgrad_fold): key (N, G, H, W, Co, Ci, fused, wg); fused: the kind-1
    mask and sums of a Bnb problem's BN on top; wg: P_s = g_s^T x_s and Gram_s = x_s^T x_s as well"""

    def __init__(self, key):
        self.key = key
        N, G, H, W, Co, Ci, fused, wg = key
        g = torch.Generator().manual_seed(29 + N + 3 * G + Co + Ci)
        self.G, self.M = G, N * H * W
        seg_m = self.M // G
        self.gr = bf(torch.randn(self.M, Co, generator=g))
        zone = _zones(N).repeat_interleave(H * W).view(-1, 1)
        self.x = bf(torch.relu(torch.randn(self.M, Ci, generator=g)).double() + 0.5 * zone)
        # consecutive segments' weights differ by factors 1, 2, 3 and their biases by whole units
        k3 = (torch.arange(G) % 3).double()
        self.w = bf(torch.randn(G, Ci, Co + Ci, generator=g).double() / (Co + Ci) ** 0.5 * (1 + k3).view(-1, 1, 1))
        self.bias = torch.randn(G, Ci, generator=g) + k3.float().view(-1, 1)
        a = torch.cat([self.gr, self.x], 1).view(G, seg_m, Co + Ci)
        self.ref = (torch.bmm(a, self.w.transpose(1, 2)) + self.bias.double().view(G, 1, Ci)).view(self.M, Ci)
        self.bnb = None
        if fused:
            self.bnb = Bnb((N, G, H, W, Ci, 64, 1, 0, 1, 1, 0))
            self.ref = torch.where(self.bnb.keep, self.ref, torch.zeros_like(self.ref))
        self.wg = wg
        self.slice_px = 64

    def _tx(self, a):
        G = self.G
        a, x = a.view(G, self.M // G, -1), self.x.view(G, self.M // G, -1)
        return torch.bmm(a.transpose(1, 2), x), torch.bmm(a.abs().transpose(1, 2), x.abs())

    def gtx(self):
        """(g_s^T x_s, |g_s|^T |x_s|), each [G][Co][Ci]"""
        return self._tx(self.gr)

    def xtx(self):
        return self._tx(self.x)

    def xtx_seq(self):
        """Gram [G][Ci][Ci] by a sequential float32 accumulation of the float64 terms in pixel order
        (numpy.cumsum in float32), eight rows' terms at a time; shared by the cases of one shape"""
        key = self.key[:6]
        if key not in _XTX_SEQ:
            Ci, G = self.x.shape[1], self.G
            seq = []
            for k0 in range(0, Ci, 8):
                t = (self.x[:, k0:k0 + 8, None] * self.x[:, None, :]).numpy().reshape(G, self.M // G, -1)
                seq.append(torch.from_numpy(np.cumsum(t, axis=1, dtype=np.float32)[:, -1]).double().view(G, -1, Ci))
            _XTX_SEQ.clear()
            _XTX_SEQ[key] = torch.cat(seq, 1)
        return _XTX_SEQ[key]

    def term_sets(self):
        sets = []
        if self.bnb is not None:
            sets += [self.ref, self.ref * self.bnb.xhat[0]]
        if self.wg:  # the terms of four rows of P (the loader pass that drops a slice drops it from Gram too)
            sets += [(self.gr[:, :4, None] * self.x[:, None, :]).reshape(self.M, -1)]
        return sets


PROBLEM_TYPES = {"fwd": Fwd, "bnb": Bnb, "bnb16": lambda key: Bnb(key, 16), "fold": Fold}


# ---------------------------------------------------------------------------
# running a forced candidate
class forced:
    """ARTSBIR_PGEMM_CFG = cfg for the block"""

    def __init__(self, cfg):
        self.cfg = cfg

    def __enter__(self):
        self.old = os.environ.get("ARTSBIR_PGEMM_CFG")
        os.environ["ARTSBIR_PGEMM_CFG"] = self.cfg

    def __exit__(self, *exc):
        if self.old is None:
            os.environ.pop("ARTSBIR_PGEMM_CFG", None)
        else:
            os.environ["ARTSBIR_PGEMM_CFG"] = self.old


def assert_kernel(cfg, refused=False, pattern=None):
    """the candidate's kernel ran; refused: the predicate must have left the case to another one"""
    name = _kernels.last_kernel()
    pat = pattern or _kernels.CONV[cfg]
    if refused:
        assert not re.match(pat, name), (cfg, name, "the predicate should refuse this case")
    else:
        assert re.match(pat, name), (cfg, name, pat)
    return name


def _twice(launch, out_shape, dev):
    outs = []
    for i in range(2):
        o = torch.full(out_shape, float("nan"), device=dev, dtype=BF)
        launch(o, i)
        outs.append(o)
    torch.cuda.synchronize()
    assert torch.equal(outs[0].view(torch.int16), outs[1].view(torch.int16)), "stored output differs between two calls"
    return outs[0]


def run_fwd(p, cfg, dev, tag, stats=True, refused=False):
    """p: Fwd.  artsbir_conv2d_fwd_seg (stats) or the plain forward under candidate cfg"""
    N, G, H, W, C, Co, R, stride, pad = p.key
    xd = nhwc(p.x).to(dev, BF)
    wd = p.w.permute(0, 2, 3, 1).contiguous().to(dev, BF)
    d = _hip.conv_desc(BF, N, H, W, C, Co, R, R, stride, pad)
    st = [torch.zeros(G, _hip.NSLOT, 2, Co, device=dev) for _ in range(2)] if stats else None

    def launch(o, i):
        if stats:
            _hip.call("artsbir_conv2d_fwd_seg", d, xd.data_ptr(), wd.data_ptr(), o.data_ptr(), G, st[i].data_ptr(),
                      _hip.stream())
        else:
            _hip.call("artsbir_conv2d_fwd", d, xd.data_ptr(), wd.data_ptr(), o.data_ptr(), Co, 0, 0, None, None, None, 0,
                      None, _hip.stream())

    with forced(cfg):
        y = _twice(launch, (p.M, Co), dev)
        name = assert_kernel(cfg, refused)
    r = Report(f"{tag} cfg {cfg} {name}")
    r.out("y", y.double().cpu(), p.y)
    if stats:
        s = st[0].double().sum(1).cpu().numpy()  # [G][2][Co]
        r.sums("sum y", s[:, 0], p.y, G)
        r.sums("sum y^2", s[:, 1], p.y * p.y, G)
    r.done()


def run_bnb(p, cfg, dev, tag, refused=False):
    """p: Bnb.  artsbir_conv2d_dgrad_bnb under candidate cfg"""
    N, G, H, W, Ci, Co, R, pad, kind, nt, rm = p.key
    dyd = nhwc(p.dy).to(dev, BF)
    wd = p.w.flip(2, 3).permute(1, 2, 3, 0).contiguous().to(dev, BF)  # [Ci][R][S][Co]
    resd = nhwc(p.res).to(dev, BF) if p.res is not None else None
    yds = [y.to(dev, BF) for y in p.ys]
    prm = [q.to(dev) for q in p.params]
    slots = [[torch.zeros(G, _hip.NSLOT, 2, Ci, device=dev) for _ in range(nt)] for _ in range(2)]
    maskd = None
    if kind == 0:
        maskd = p.mask.to(dev, BF)
    elif kind == 3:
        maskd = pack_bits(p.mask.to(dev, BF))
    desc = _hip.BnBwdDesc()
    desc.dtype, desc.kind, desc.pool, desc.ntarget = _hip.DT_BF16, kind, 0, nt
    desc.mask = maskd.data_ptr() if maskd is not None else None
    desc.mask_bn = prm[0].data_ptr() if kind == 1 else None
    for t in range(nt):
        desc.y[t] = yds[t].data_ptr()
        desc.mean[t] = prm[t][0, 0].data_ptr()
        desc.istd[t] = prm[t][0, 1].data_ptr()
    d = _hip.conv_desc(BF, N, H, W, Ci, Co, R, R, 1, pad)

    def launch(o, i):
        for t in range(nt):
            desc.slots[t] = slots[i][t].data_ptr()
        _hip.call("artsbir_conv2d_dgrad_bnb", d, dyd.data_ptr(), wd.data_ptr(), o.data_ptr(),
                  resd.data_ptr() if resd is not None else None, rm, desc, G, 4 * Ci, _hip.stream())

    with forced(cfg):
        dx = _twice(launch, (p.M, Ci), dev)
        name = assert_kernel(cfg, refused)
    r = Report(f"{tag} cfg {cfg} {name}")
    got = dx.double().cpu()
    r.out("dx", got, p.g)
    # the fused kernels sum the f32 result; the route a refusal leaves the case to stores g and sums
    # the stored values in a pass of its own, so there the terms are the stored bf16 g
    gs = got if refused else p.g
    for t in range(nt):
        s = slots[0][t].double().sum(1).cpu().numpy()  # [G][2][Ci]
        r.sums(f"sum g [{t}]", s[:, 0], gs, G)
        r.sums(f"sum g xhat_{t}", s[:, 1], gs * p.xhat[t], G)
    r.done()


def ident(key):
    return "-".join(str(v) for v in key)
