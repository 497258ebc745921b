"""The halo-tiled 3x3 convolution (candidate 21, conv3x3.hip) at the edges of its
tilings: forward with per-segment BN statistics and the data gradient with the
fused BN-backward reduction against float64 references on the same bf16
operands; the persistent grid with a ragged last round and with fewer tiles than
workgroups; the deterministic mode through the encoder.

Bars.  Outputs: test_pgemm_gpu.py's for candidate 21 (atol 2e-2, rtol 1e-2 on a
bf16 result).  Forward sums: test_conv_fwd_segment_stats' (atol 5e-2, rtol 1e-3).
Reduction slots: test_bn_bwd_gpu.py's atomic bar (check_atomic_sum: any order of n
f32 terms, n * 2^-24 * sum |term|) with the float64 g and g * xhat as the terms.
Every launch runs twice: y / dX are stored values and must repeat byte for byte
(the sums are f32 atomics and repeat only up to their order)."""
import os

import pytest
import torch
import torch.nn.functional as F

import _hip
import _kernels

pytestmark = pytest.mark.gpu

U32 = 2.0 ** -24
CHANNELS = [(64, 64), (32, 32), (32, 64), (64, 32)]  # C in, Cout of the forward conv
SIZES = [(56, 56), (16, 16), (32, 32), (24, 24), (40, 40), (24, 56)]
BATCHES = [3, 6]  # three segments: one and two images each
# tile counts against the persistent grid (256 CUs x workgroups per CU), one segment:
# N, H, W, C, Cout
GRID_CASES = [
    (7, 56, 56, 64, 64),     # 196 tiles: fewer than workgroups
    (10, 56, 56, 64, 64),    # 280 tiles on 256 workgroups: one or two tiles each
    (19, 56, 56, 64, 64),    # 532 tiles: two or three each (both parities of the tile count)
    (40, 56, 56, 32, 32),    # 1120 tiles: ragged for up to 4 workgroups per CU
    (12, 112, 112, 32, 32),  # 16 x 16 tiles, 588 of them
    (1, 24, 24, 64, 32),     # 6 tiles
]


@pytest.fixture
def cfg21():
    old = os.environ.get("ARTSBIR_PGEMM_CFG")
    os.environ["ARTSBIR_PGEMM_CFG"] = "21"
    yield
    if old is None:
        os.environ.pop("ARTSBIR_PGEMM_CFG", None)
    else:
        os.environ["ARTSBIR_PGEMM_CFG"] = old


def _nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous()


def _bf(x):
    return x.bfloat16().double()


def _require_hconv():
    k = _kernels.last_kernel()
    assert k.startswith("hconv_kernel<"), k


def _forward(N, G, H, W, C, Co, dev):
    g = torch.Generator().manual_seed(1000 * H + 10 * W + C + Co + N)
    x = torch.randn(N, C, H, W, generator=g)
    x[N // G:] += 0.5  # segments with different statistics
    x = _bf(x)
    w = _bf(torch.randn(Co, C, 3, 3, generator=g) / (C * 9) ** 0.5)
    ref = F.conv2d(x, w, padding=1)  # float64
    y = torch.full((N * H * W, Co), float("nan"), device=dev, dtype=torch.bfloat16)
    stats = torch.zeros(G, _hip.NSLOT, 2, Co, device=dev)
    d = _hip.conv_desc(torch.bfloat16, N, H, W, C, Co, 3, 3, 1, 1)
    xd = _nhwc(x).to(dev, torch.bfloat16)
    wd = w.permute(0, 2, 3, 1).contiguous().to(dev, torch.bfloat16)
    _hip.call("artsbir_conv2d_fwd_seg", d, xd.data_ptr(), wd.data_ptr(), y.data_ptr(), G, stats.data_ptr(), _hip.stream())
    y2 = torch.full_like(y, float("nan"))
    stats2 = torch.zeros_like(stats)
    _hip.call("artsbir_conv2d_fwd_seg", d, xd.data_ptr(), wd.data_ptr(), y2.data_ptr(), G, stats2.data_ptr(), _hip.stream())
    torch.cuda.synchronize()
    _require_hconv()
    assert torch.equal(y.view(torch.int16), y2.view(torch.int16)), "y differs between two calls"
    out = y.double().cpu().view(N, H, W, Co).permute(0, 3, 1, 2)
    err = (out - ref).abs().max().item()
    print(f"HCONV2 fwd N={N} {H}x{W} {C}->{Co}: {_kernels.last_kernel()} max |err| {err:.3e}")
    assert torch.isfinite(out).all()
    assert torch.allclose(out, ref, atol=2e-2, rtol=1e-2), err
    s = stats.double().sum(1).cpu()
    for k in range(G):
        r2 = ref[k * N // G:(k + 1) * N // G].permute(0, 2, 3, 1).reshape(-1, Co)
        e1 = (s[k, 0] - r2.sum(0)).abs().max().item()
        e2 = (s[k, 1] - (r2 * r2).sum(0)).abs().max().item()
        print(f"HCONV2   segment {k}: sum err {e1:.3e}, sum of squares err {e2:.3e}")
        assert torch.allclose(s[k, 0], r2.sum(0), atol=5e-2, rtol=1e-3), k
        assert torch.allclose(s[k, 1], (r2 * r2).sum(0), atol=5e-2, rtol=1e-3), k


def _dgrad_bnb(N, G, H, W, Ci, Co, dev):
    """data gradient of a Ci -> Co forward conv (dY with Co channels -> dX with Ci), masked by the ReLU of the
    BN over y (kind 1), with sum g and sum g * xhat per segment"""
    g = torch.Generator().manual_seed(2000 * H + 10 * W + Ci + Co + N)
    dy = _bf(torch.randn(N, Co, H, W, generator=g))
    w = _bf(torch.randn(Co, Ci, 3, 3, generator=g) / (Co * 9) ** 0.5)
    draw = torch.nn.grad.conv2d_input((N, Ci, H, W), w, dy, stride=1, padding=1)
    yv = _bf(torch.randn(N, Ci, H, W, generator=g))
    params = torch.randn(G, 4, Ci, generator=g)  # per segment: mean, istd, scale, beta
    params[:, 1] = params[:, 1].abs() + 0.5
    params[:, 2] = torch.where(params[:, 2] < 0, params[:, 2] - 0.25, params[:, 2] + 0.25)  # |scale| >= 1/4
    per = N // G
    p64 = params.double()
    seg = lambda k: slice(k * per, (k + 1) * per)  # noqa: E731
    # no ReLU decision within rounding of its threshold: move such y by whole bf16 steps
    for _ in range(8):
        amb = torch.zeros_like(yv, dtype=torch.bool)
        for k in range(G):
            pre = (yv[seg(k)] - p64[k, 0].view(1, -1, 1, 1)) * p64[k, 2].view(1, -1, 1, 1) + p64[k, 3].view(1, -1, 1, 1)
            amb[seg(k)] = pre.abs() < 1e-3
        if not amb.any():
            break
        yv[amb] = _bf(yv[amb] + 0.0625)
    assert not amb.any()
    wdflip = w.flip(2, 3).permute(1, 2, 3, 0).contiguous().to(dev, torch.bfloat16)  # [Ci][R][S][Co]
    dyd = _nhwc(dy).to(dev, torch.bfloat16)
    yd = _nhwc(yv).to(dev, torch.bfloat16)
    pdev = params.to(dev)
    slots = torch.zeros(G, _hip.NSLOT, 2, Ci, device=dev)
    dx = torch.full((N * H * W, Ci), float("nan"), device=dev, dtype=torch.bfloat16)
    desc = _hip.BnBwdDesc()
    desc.dtype = _hip.DT_BF16
    desc.kind = 1
    desc.pool = 0
    desc.mask = None
    desc.mask_bn = pdev[0].data_ptr()
    desc.ntarget = 1
    desc.y[0] = yd.data_ptr()
    desc.mean[0] = pdev[0, 0].data_ptr()
    desc.istd[0] = pdev[0, 1].data_ptr()
    desc.slots[0] = slots.data_ptr()
    d = _hip.conv_desc(torch.bfloat16, N, H, W, Ci, Co, 3, 3, 1, 1)
    _hip.call("artsbir_conv2d_dgrad_bnb", d, dyd.data_ptr(), wdflip.data_ptr(), dx.data_ptr(), None, 0, desc, G, 4 * Ci,
              _hip.stream())
    dx2 = torch.full_like(dx, float("nan"))
    slots2 = torch.zeros_like(slots)
    desc.slots[0] = slots2.data_ptr()
    _hip.call("artsbir_conv2d_dgrad_bnb", d, dyd.data_ptr(), wdflip.data_ptr(), dx2.data_ptr(), None, 0, desc, G, 4 * Ci,
              _hip.stream())
    torch.cuda.synchronize()
    _require_hconv()
    assert torch.equal(dx.view(torch.int16), dx2.view(torch.int16)), "dX differs between two calls"
    got = dx.double().cpu()
    assert torch.isfinite(got).all()
    flat = lambda t: t.permute(0, 2, 3, 1).reshape(-1, Ci)  # noqa: E731
    n = per * H * W
    tot = slots.double().sum(1).cpu()  # [G][2][Ci]
    for k in range(G):
        sl = slice(k * n, (k + 1) * n)
        ys = flat(yv)[sl]
        keep = ((ys - p64[k, 0]) * p64[k, 2] + p64[k, 3]) > 0
        gref = torch.where(keep, flat(draw)[sl], torch.zeros_like(ys))
        xhat = (ys - p64[k, 0]) * p64[k, 1]
        err = (got[sl] - gref).abs().max().item()
        assert torch.allclose(got[sl], gref, atol=2e-2, rtol=1e-2), (k, err)
        for m, terms in enumerate((gref, gref * xhat)):
            bound = n * U32 * terms.abs().sum(0)
            e = (tot[k, m] - terms.sum(0)).abs()
            worst = (e / bound.clamp_min(1e-300)).max().item()
            print(f"HCONV2 bnb N={N} {H}x{W} {Co}->{Ci} segment {k} sum {m}: {_kernels.last_kernel()} "
                  f"max |dx err| {err:.3e}, max err/bound {worst:.3e}")
            assert (e <= bound).all(), (k, m, worst)


@pytest.mark.parametrize("N", BATCHES)
@pytest.mark.parametrize("hw", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("ch", CHANNELS, ids=lambda c: f"{c[0]}to{c[1]}")
def test_hconv_forward_stats(ch, hw, N, dev, cfg21):
    _forward(N, 3, hw[0], hw[1], ch[0], ch[1], dev)


@pytest.mark.parametrize("N", BATCHES)
@pytest.mark.parametrize("hw", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("ch", CHANNELS, ids=lambda c: f"{c[0]}to{c[1]}")
def test_hconv_dgrad_bn_reduce(ch, hw, N, dev, cfg21):
    _dgrad_bnb(N, 3, hw[0], hw[1], ch[0], ch[1], dev)


@pytest.mark.parametrize("case", GRID_CASES, ids=lambda c: "x".join(map(str, c)))
def test_hconv_persistent_grid(case, dev, cfg21):
    N, H, W, C, Co = case
    _forward(N, 1, H, W, C, Co, dev)
    _dgrad_bnb(N, 1, H, W, Co, C, dev)  # the data gradient of the same instance: dY with C channels


def test_hconv_deterministic_mode(dev, cfg21):
    """Deterministic mode (engine.set_deterministic): the encoder's step, whose stem and layer-1 3x3
    convolutions run candidate 21 forward and backward, twice on the same inputs: loss, embeddings,
    BN running statistics and the gradient of every BatchNorm parameter (the finalised reduction
    slots of the backward, fed by this kernel's dX) byte-identical.  The mode takes the sums out of the
    convolutions' epilogues into fixed-order reductions; the fused sums of the default mode are f32
    atomics and repeat only up to their order.  The weight gradients of the convolutions are split-K
    f32 atomics in either mode (bench.py documents their run-to-run difference) and are not compared."""
    import engine
    import losses
    import models

    def run():
        torch.manual_seed(11)
        m = models.ModifiedResNet((1, 1, 1, 1), 32, heads=32, input_resolution=64, width=64)
        m.compute_dtype = torch.bfloat16
        m = m.to(dev)
        g = torch.Generator(device=dev).manual_seed(3)
        xs = [torch.randn(6, 3, 64, 64, device=dev, generator=g) + i for i in range(3)]
        m.train()
        _hip.TRACE = trace = []
        try:
            outs = m.forward_branches(xs)
            loss = losses.TripletMarginLoss(margin=0.2)(*outs)
            loss.backward()
            torch.cuda.synchronize()
        finally:
            _hip.TRACE = None
        assert any(k and k.startswith("hconv_kernel<") for _, k, _ in trace), "no hconv launch in the step"
        blobs = [loss.detach().cpu().numpy().tobytes()] + [o.detach().float().cpu().numpy().tobytes() for o in outs]
        blobs += [v.float().cpu().numpy().tobytes() for k, v in sorted(m.state_dict().items()) if "running" in k]
        for _, mod in sorted(m.named_modules()):
            if hasattr(mod, "running_mean"):  # dgamma, dbeta: the finalised fixed-order reduction slots
                blobs += [p.grad.float().cpu().numpy().tobytes() for p in (mod.weight, mod.bias)]
        return blobs

    old = engine.set_deterministic(True)
    try:
        a = run()
        b = run()
    finally:
        engine.set_deterministic(old)
    assert len(a) == len(b)
    for i, (u, v) in enumerate(zip(a, b)):
        assert u == v, f"blob {i} differs between two deterministic steps"
