"""The Bottleneck tail fused into the next block's conv1 forward
(artsbir_block_out_conv1x1_fwd, csrc/bstream.hip): the streaming kernel against
artsbir_block_out_mask (out and mask bits, bit for bit) and a CPU f32 1x1 conv of
the stored `out` (y1 and bn1's per-segment sums); the entry point's fallback to
the two launches; and the engine's wiring (which transitions make the fused call,
the backward untouched)."""
import pytest
import torch

import _hip
import _kernels

pytestmark = pytest.mark.gpu

NSLOT = _hip.NSLOT
FUSED = "artsbir_block_out_conv1x1_fwd"


def _inputs(K, N, nseg, per_seg, H, W, two, dtype=torch.bfloat16, seed=11):
    """y3, the second operand, per-segment BN blocks [nseg][4][K] (mean, istd,
    scale, beta) and conv1's weight [N][K] scaled by 1/sqrt(K); all values are
    bf16 values; segments 1.. are shifted and scaled apart from segment 0"""
    g = torch.Generator().manual_seed(seed + K + N + 7 * nseg + H)
    B = nseg * per_seg
    rows = B * H * W
    y3 = torch.randn(rows, K, generator=g)
    r = torch.randn(rows, K, generator=g)
    seg_rows = rows // nseg
    for s in range(1, nseg):
        y3[s * seg_rows:(s + 1) * seg_rows] = y3[s * seg_rows:(s + 1) * seg_rows] * (1.0 + s) + 0.75 * s
        r[s * seg_rows:(s + 1) * seg_rows] -= 0.5 * s

    def bn():
        blk = torch.empty(nseg, 4, K)
        for s in range(nseg):
            blk[s, 0] = 0.3 * torch.randn(K, generator=g) + 0.75 * s          # mean
            blk[s, 1] = (0.5 + torch.rand(K, generator=g)) / (1.0 + s)         # istd
            blk[s, 2] = blk[s, 1] * (0.5 + torch.rand(K, generator=g))         # scale = gamma * istd
            blk[s, 3] = 0.3 * torch.randn(K, generator=g) - 0.2 * s            # beta
        return blk

    w = torch.randn(N, K, generator=g) / K ** 0.5
    return dict(B=B, H=H, W=W, K=K, N=N, nseg=nseg, rows=rows, dtype=dtype, y3=y3.to(dtype), r=r.to(dtype), bn3=bn(),
                bnd=bn() if two else None, w=w.to(dtype))


def _dev(c, dev):
    return {k: (v.to(dev).contiguous() if torch.is_tensor(v) else v) for k, v in c.items()}


def _run_pair(c, dev, bits=True):
    """artsbir_block_out_mask, then artsbir_conv2d_fwd_seg of its output"""
    out = torch.empty_like(c["y3"])
    mb = torch.zeros(c["rows"] * c["K"] // 8, dtype=torch.uint8, device=dev) if bits else None
    two = c["bnd"] is not None
    dt = _hip.dtype_code(c["dtype"])
    _hip.call("artsbir_block_out_mask", dt, c["y3"].data_ptr(), c["bn3"].data_ptr(), c["r"].data_ptr() if two else None,
              c["bnd"].data_ptr() if two else None, None if two else c["r"].data_ptr(), c["rows"], c["K"], c["nseg"],
              out.data_ptr(), mb.data_ptr() if bits else None, _hip.stream())
    y1 = torch.empty(c["rows"], c["N"], dtype=c["dtype"], device=dev)
    stats = torch.zeros(c["nseg"], NSLOT, 2, c["N"], device=dev)
    d = _hip.conv_desc(c["dtype"], c["B"], c["H"], c["W"], c["K"], c["N"], 1, 1, 1, 0)
    _hip.call("artsbir_conv2d_fwd_seg", d, out.data_ptr(), c["w"].data_ptr(), y1.data_ptr(), c["nseg"], stats.data_ptr(),
              _hip.stream())
    torch.cuda.synchronize()
    return out, mb, y1, stats, _kernels.last_kernel()


def _run_fused(c, dev, bits=True):
    out = torch.empty_like(c["y3"])
    mb = torch.zeros(c["rows"] * c["K"] // 8, dtype=torch.uint8, device=dev) if bits else None
    y1 = torch.empty(c["rows"], c["N"], dtype=c["dtype"], device=dev)
    stats = torch.zeros(c["nseg"], NSLOT, 2, c["N"], device=dev)
    two = c["bnd"] is not None
    d = _hip.conv_desc(c["dtype"], c["B"], c["H"], c["W"], c["K"], c["N"], 1, 1, 1, 0)
    _hip.call(FUSED, d, c["y3"].data_ptr(), c["bn3"].data_ptr(), c["r"].data_ptr() if two else None,
              c["bnd"].data_ptr() if two else None, None if two else c["r"].data_ptr(), c["w"].data_ptr(), c["nseg"],
              out.data_ptr(), mb.data_ptr() if bits else None, y1.data_ptr(), stats.data_ptr(), _hip.stream())
    torch.cuda.synchronize()
    return out, mb, y1, stats, _kernels.last_kernel()


def _check_conv(c, out, y1, stats):
    """y1 and the slot sums against a CPU f32 1x1 conv of the stored out (the bars
    of tests/test_fused_gpu.py::test_conv_fwd_segment_stats)"""
    ref = out.float().cpu() @ c["w"].float().cpu().t()
    got = y1.float().cpu()
    print(f"y1 max abs err {(got - ref).abs().max().item():.3e}")
    assert torch.allclose(got, ref, atol=3e-2, rtol=1e-2), (got - ref).abs().max()
    s = stats.sum(1).cpu()
    seg_rows = c["rows"] // c["nseg"]
    for k in range(c["nseg"]):
        r2 = ref[k * seg_rows:(k + 1) * seg_rows]
        print(f"segment {k}: sum err {(s[k, 0] - r2.sum(0)).abs().max().item():.3e} "
              f"sumsq err {(s[k, 1] - (r2 * r2).sum(0)).abs().max().item():.3e}")
        assert torch.allclose(s[k, 0], r2.sum(0), atol=5e-2, rtol=1e-3), k
        assert torch.allclose(s[k, 1], (r2 * r2).sum(0), atol=5e-2, rtol=1e-3), k


# per segment: 2 images of 8x8 (8 blocks of 16 pixels: a workgroup of one block per
# wave, at nseg 3 three workgroups), or one image of 36x36 (81 blocks: 243 in all
# at nseg 3 — workgroups of 61 blocks, 7-8 per wave, the last one a block short,
# the second and the third with a segment change inside their range; at nseg 1
# two workgroups of 41 and 40)
SHAPES = {"8x8": (2, 8, 8), "36x36": (1, 36, 36)}


@pytest.mark.parametrize("nseg", [1, 3])
@pytest.mark.parametrize("two", [False, True], ids=["idn", "down"])
@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("KN", [(256, 64), (256, 128), (512, 128)])
def test_stream_kernel(KN, shape, two, nseg, dev):
    K, N = KN
    per_seg, H, W = SHAPES[shape]
    c = _dev(_inputs(K, N, nseg, per_seg, H, W, two), dev)
    out, mb, y1, stats, name = _run_fused(c, dev)
    if not name.startswith("bstream_kernel<"):
        pytest.skip(f"the streaming kernel does not take this case (the fallback ran {name})")
    out_r, mb_r, _, _, _ = _run_pair(c, dev)
    # the shared expression: identical bits
    assert torch.equal(out.view(torch.int16), out_r.view(torch.int16))
    assert torch.equal(mb, mb_r)
    _check_conv(c, out, y1, stats)
    # without the mask bits: the same out and y1
    out2, _, y12, _, name2 = _run_fused(c, dev, bits=False)
    assert name2 == name
    assert torch.equal(out2.view(torch.int16), out.view(torch.int16))
    assert torch.equal(y12.view(torch.int16), y1.view(torch.int16))


@pytest.mark.parametrize("case", ["K128", "f32"])
def test_fallback_runs_the_pair(case, dev):
    """a shape outside the predicate and an f32 call: the two launches' result, and
    artsbir_last_kernel() names the pair's conv kernel"""
    if case == "K128":
        c = _dev(_inputs(128, 32, 3, 2, 8, 8, True), dev)
    else:
        c = _dev(_inputs(256, 64, 3, 2, 8, 8, False, dtype=torch.float32), dev)
    out_r, mb_r, y1_r, st_r, name_r = _run_pair(c, dev)
    out, mb, y1, st, name = _run_fused(c, dev)
    assert not name.startswith("bstream_kernel<")
    assert name == name_r
    assert torch.equal(out, out_r)
    assert torch.equal(mb, mb_r)
    assert torch.equal(y1, y1_r)  # the same kernel on the same input
    _check_conv(c, out, y1, st)


def _train_step_traces(m, elements, dev, fuse):
    """one training step; the forward's and the backward's call traces"""
    import engine
    import losses
    old = engine.FUSE_BLOCK_CONV1[0]
    engine.FUSE_BLOCK_CONV1[0] = fuse
    fwd, bwd = [], []
    try:
        m.train()
        _hip.TRACE = fwd
        outs = m.forward_branches([e.to(dev) for e in elements])
        loss = losses.TripletMarginLoss(margin=0.2)(*outs)
        for p in m.parameters():
            p.grad = None
        _hip.TRACE = bwd
        loss.backward()
        torch.cuda.synchronize()
    finally:
        _hip.TRACE = None
        engine.FUSE_BLOCK_CONV1[0] = old
    return fwd, bwd


def test_engine_defers_the_tail(dev):
    """ModifiedResNet((2,2,1,1), 64) at 64x64, three branches of 4 images, bf16,
    atomic statistics: with the switch on every block that has a successor leaves
    its tail to the successor's fused call; the backward runs the same calls"""
    import engine
    import models
    assert not engine.DETERMINISTIC
    torch.manual_seed(0)
    m = models.ModifiedResNet((2, 2, 1, 1), 64, heads=32, input_resolution=64, width=64).to(dev)
    m.compute_dtype = torch.bfloat16
    g = torch.Generator().manual_seed(3)
    elements = [torch.randn(4, 3, 64, 64, generator=g) for _ in range(3)]
    _train_step_traces(m, elements, dev, False)  # packs the weights, tunes the kernels: not part of either trace
    f_off, b_off = _train_step_traces(m, elements, dev, False)
    f_on, b_on = _train_step_traces(m, elements, dev, True)
    nblocks, transitions = 6, 5
    assert sum(t[0] == FUSED for t in f_off) == 0
    assert sum(t[0] == "artsbir_block_out_colsum" for t in f_off) == nblocks
    assert sum(t[0] == FUSED for t in f_on) == transitions
    assert sum(t[0] == "artsbir_block_out_colsum" for t in f_on) == nblocks - transitions
    # 256->64 and 256->128 at 16x16, 512->128 at 8x8 stream; 512->256 and 1024->512 run the pair
    assert sum(t[0] == FUSED and t[1].startswith("bstream_kernel<") for t in f_on) == 3
    # one fused call stands for a block_out and a conv forward
    assert len(f_on) == len(f_off) - transitions
    assert b_on == b_off


def test_c2_transitions_stream(dev):
    """the C2 network (what bench.py times) at 4 triplets: every 56x56 and 28x28
    block -> block transition with conv1 K -> N of 256 -> 64, 256 -> 128 or
    512 -> 128 runs the streaming kernel.  With layers (3, 4, 6, 3) those are six:
    layer 1 b0 -> b1 (the producer has a downsample BN) and b1 -> b2, layer 1 b2 ->
    layer 2 b0, layer 2 b0 -> b1 (downsample producer), b1 -> b2, b2 -> b3; the
    next one, layer 2 b3 -> layer 3 b0, is 512 -> 256 and runs the pair"""
    import models
    m = models.ModifiedResNet((3, 4, 6, 3), 512, heads=32, input_resolution=224, width=64).to(dev)
    m.compute_dtype = torch.bfloat16
    m.train()
    g = torch.Generator().manual_seed(3)
    elements = [torch.randn(4, 3, 224, 224, generator=g).to(dev) for _ in range(3)]
    trace = []
    _hip.TRACE = trace
    try:
        with torch.no_grad():
            m.forward_branches(elements)
        torch.cuda.synchronize()
    finally:
        _hip.TRACE = None
    fused = [(t[1], t[2].split(" ")[1]) for t in trace if t[0] == FUSED]
    assert len(fused) == 15
    assert fused[:7] == [("bstream_kernel<two>", "12x56x56x256->64"), ("bstream_kernel<idn>", "12x56x56x256->64"),
                         ("bstream_kernel<idn>", "12x56x56x256->128"), ("bstream_kernel<two>", "12x28x28x512->128"),
                         ("bstream_kernel<idn>", "12x28x28x512->128"), ("bstream_kernel<idn>", "12x28x28x512->128"),
                         (fused[6][0], "12x28x28x512->256")], fused
    assert not any(k.startswith("bstream_kernel<") for k, _ in fused[6:]), fused
