"""Forward BatchNorm statistics and the element-wise forward kernels
(csrc/elementwise.hip) called on raw pointers against float64.

artsbir_bn_stats_det: per segment s of y [nseg][rows][C] the sums  sum_r y  and
  sum_r y^2  in f64 in a fixed order, stored as f32 hi/lo pairs in slots 0 / 1 of
  stats + s * seg_stride ([32][2][C]), slots 2 .. 31 zero.  Bar per channel:
  |hi + lo - ref| <= (2^-47 + rows 2^-53) sum|term|  (derived: the square of an f32 is
  exact in f64, the pair keeps 48 bits).  With |mean| / std = 1000 the moments that
  artsbir_bn_finalize_seg takes from those slots keep mean and istd to 4 * 2^-24.
artsbir_bn_finalize (one segment): mean = S1 / n, var = max(S2 / n - mean^2, 0),
  istd = 1 / sqrt(var + eps), scale = gamma istd, running = (1 - m) running + m new
  (variance unbiased), num_batches_tracked += 1; eval: from the running statistics.
  It adds the 32 slots in index order, _seg in four quarters, so it is held to the
  float64 formula at rtol 2e-7 (tests/test_bn_finalize_gpu.py's bar) and to _seg
  bit for bit only on hi/lo slots, where both orders are exact.
artsbir_act_pool / _colsum:  out = avgpool_p( relu?( (x - mean) * scale + beta ) ),
  segment s with the parameter block bn + s * 4 C = {mean, istd, scale, beta}.
artsbir_block_out / _mask / _colsum:  out = relu( bn3(y3) + (bnd(yd) | identity) ),
  mask bit e of byte c = stored out[row][8 c + e] > 0, colsum[s] = column sums of
  the stored output spread over 32 replica rows.
Outputs are held to _tail.check against an f32 restatement, the mask bits to exact
equality with the packed stored output, the column sums to _tail.check_atomic_sum.
Every output buffer carries a sentinel tail."""
import numpy as np
import pytest
import torch

from _tail import (NSLOT, SENT, bf16_round, check, check_atomic_sum, check_det_sum, check_exact, pack_bits, tail_intact,
                   to_dev, with_tail)

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16]
DT_IDS = ["f32", "bf16"]
EPS = float(np.float32(1e-5))
MOM = float(np.float32(0.1))


def _rnd(dtype, a):
    a = np.asarray(a, dtype=np.float32)
    return bf16_round(a) if dtype == torch.bfloat16 else a


# ------------------------------------------------------------------ bn_stats_det
def _stats_det(y, dtype, dev, stride_extra=64):
    """y [nseg][rows][C] numpy -> slots [nseg][32][2][C] f32 (gaps, tail and repeat checked)"""
    import _hip
    nseg, rows, C = y.shape
    stride = 2 * NSLOT * C + stride_extra
    dy = to_dev(y, dev, dtype)
    outs = []
    for _ in range(2):
        st = with_tail(nseg * stride, 2 * NSLOT * C, torch.float32, dev)
        st[:nseg * stride].view(nseg, stride)[:, :2 * NSLOT * C] = 7.0  # the kernel must zero slots 2 .. 31 itself
        _hip.call("artsbir_bn_stats_det", _hip.dtype_code(dtype), dy.data_ptr(), nseg, rows, C, st.data_ptr(), stride,
                  _hip.stream())
        torch.cuda.synchronize()
        assert tail_intact(st, nseg * stride), "stats written past the last segment's 32 slots"
        a = st[:nseg * stride].view(nseg, stride).cpu().numpy()
        assert (a[:, 2 * NSLOT * C:] == SENT).all(), "stats written between two segments"
        outs.append((st, a[:, :2 * NSLOT * C].reshape(nseg, NSLOT, 2, C).copy()))
    assert outs[0][1].tobytes() == outs[1][1].tobytes(), "bn_stats_det is not reproducible"
    return outs[0][0], stride, outs[0][1]


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("nseg", [1, 3])
@pytest.mark.parametrize("C", [8, 64, 72, 200])
@pytest.mark.parametrize("rows", [1, 15, 16, 17, 1000])
def test_bn_stats_det(rows, C, nseg, dtype, dev):
    rng = np.random.default_rng(rows * 1009 + C * 7 + nseg)
    y = _rnd(dtype, rng.normal(0, 1, (nseg, rows, C)) * rng.uniform(0.5, 2, C) + rng.normal(0, 2, C))
    _, _, sl = _stats_det(y, dtype, dev)
    assert (sl[:, 2:] == 0).all(), "slots 2 .. 31 must be zero"
    tot = sl[:, :2].astype(np.float64).sum(1)  # hi + lo  [nseg][2][C]
    y64 = y.astype(np.float64)
    tag = f"bn_stats_det rows{rows} C{C} nseg{nseg} {'bf16' if dtype == torch.bfloat16 else 'f32'}"
    check_det_sum(f"{tag} sum y", tot[:, 0], y64.sum(1), np.abs(y64).sum(1), rows, 2.0 ** -47)
    check_det_sum(f"{tag} sum y^2", tot[:, 1], (y64 * y64).sum(1), (y64 * y64).sum(1), rows, 2.0 ** -47)


def test_bn_stats_det_large_mean(dev):
    """|mean| / std = 1000: E[y^2] - mean^2 cancels six digits; from the hi/lo sums the
    cancellation costs 1e6 * 2^-47, far below one f32 rounding"""
    import _hip
    rows, C, nseg = 1000, 64, 2
    rng = np.random.default_rng(11)
    y = (rng.normal(0, 1, (nseg, rows, C)) + 1000.0 * np.sign(rng.normal(0, 1, C))).astype(np.float32)
    st, stride, _ = _stats_det(y, torch.float32, dev)
    gamma, beta = torch.ones(C, device=dev), torch.zeros(C, device=dev)
    out = with_tail(nseg * 4 * C, C, torch.float32, dev)
    _hip.call("artsbir_bn_finalize_seg", st.data_ptr(), nseg, stride, C, float(rows), gamma.data_ptr(), beta.data_ptr(),
              None, None, None, MOM, EPS, 1, out.data_ptr(), _hip.stream())
    torch.cuda.synchronize()
    assert tail_intact(out, nseg * 4 * C)
    o = out[:nseg * 4 * C].view(nseg, 4, C).cpu().numpy().astype(np.float64)
    y64 = y.astype(np.float64)
    mean, istd = y64.mean(1), 1.0 / np.sqrt(y64.var(1) + EPS)
    assert (np.abs(mean) / y64.std(1) > 800).all()  # the case is what it says
    e_m, e_i = np.abs(o[:, 0] / mean - 1).max(), np.abs(o[:, 1] / istd - 1).max()
    print(f"PARITY {'bn_stats_det -> finalize_seg, |mean|/std = 1000':<58s} f32  rel err mean={e_m:.3e} istd={e_i:.3e} "
          f"bar={4 * 2.0 ** -24:.3e}")
    assert e_m <= 4 * 2.0 ** -24 and e_i <= 4 * 2.0 ** -24, (e_m, e_i)


# ------------------------------------------------------------------- bn_finalize
def _finalize_ref(stats, count, gamma, beta, rmean, rvar, train):
    """float64 formula; stats [32][2][C] added in index order"""
    if train:
        s = np.zeros(stats.shape[1:])
        for k in range(stats.shape[0]):
            s += stats[k].astype(np.float64)
        mean = s[0] / count
        var = np.maximum(s[1] / count - mean * mean, 0.0)
        rm = ((1 - MOM) * rmean.astype(np.float64) + MOM * mean).astype(np.float32)
        rv = ((1 - MOM) * rvar.astype(np.float64) + MOM * var * count / (count - 1)).astype(np.float32)
    else:
        mean, var, rm, rv = rmean.astype(np.float64), rvar.astype(np.float64), rmean, rvar
    istd = (1.0 / np.sqrt(var + EPS)).astype(np.float32)
    return np.stack([mean.astype(np.float32), istd, gamma * istd, beta]), rm, rv


def _finalize_run(dev, stats_dev, C, count, gamma, beta, rmean, rvar, train, seg):
    import _hip
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    g, b, rm, rv = t(gamma), t(beta), t(rmean), t(rvar)
    nbt = torch.full((1,), 5, dtype=torch.int64, device=dev)
    out = with_tail(4 * C, C, torch.float32, dev)
    if seg:
        _hip.call("artsbir_bn_finalize_seg", stats_dev.data_ptr(), 1, 2 * NSLOT * C, C, count, g.data_ptr(), b.data_ptr(),
                  rm.data_ptr(), rv.data_ptr(), nbt.data_ptr(), MOM, EPS, train, out.data_ptr(), _hip.stream())
    else:
        o = out.data_ptr()
        _hip.call("artsbir_bn_finalize", stats_dev.data_ptr(), C, count, g.data_ptr(), b.data_ptr(), rm.data_ptr(),
                  rv.data_ptr(), nbt.data_ptr(), MOM, EPS, train, o, o + 4 * C, o + 8 * C, o + 12 * C, _hip.stream())
    torch.cuda.synchronize()
    assert tail_intact(out, 4 * C)
    return out[:4 * C].view(4, C).cpu().numpy(), rm.cpu().numpy(), rv.cpu().numpy(), int(nbt.item())


@pytest.mark.parametrize("train", [1, 0], ids=["train", "eval"])
@pytest.mark.parametrize("C", [8, 72, 300])
def test_bn_finalize(C, train, dev):
    rng = np.random.default_rng(C + train)
    count = 1234.0
    mean_t, var_t = rng.normal(0, 2, C), rng.uniform(0.1, 3, C)
    w = rng.dirichlet(np.ones(NSLOT), size=C).T  # [32][C]: uneven shares of the slots
    stats = np.stack([mean_t * count * w, (var_t + mean_t ** 2) * count * w], 1)
    stats = np.ascontiguousarray(stats, dtype=np.float32)  # [32][2][C] in memory, whatever order stack chose
    gamma = rng.uniform(0.5, 1.5, C).astype(np.float32)
    beta = rng.normal(0, 0.5, C).astype(np.float32)
    rmean = rng.normal(0, 1, C).astype(np.float32)
    rvar = rng.uniform(0.5, 2, C).astype(np.float32)
    sd = torch.from_numpy(stats).to(dev)
    o, rm, rv, nbt = _finalize_run(dev, sd, C, count, gamma, beta, rmean, rvar, train, seg=False)
    exp, erm, erv = _finalize_ref(stats, count, gamma, beta, rmean, rvar, train)
    tag = f"bn_finalize C{C} {'train' if train else 'eval'}"
    for label, a, b in ((f"{tag} block", o, exp), (f"{tag} running mean", rm, erm), (f"{tag} running var", rv, erv)):
        rel = float((np.abs(a.astype(np.float64) - b) / np.maximum(np.abs(b), 1e-30)).max())
        print(f"PARITY {label:<58s} f32  max rel err={rel:.3e} bar=2e-7")
        np.testing.assert_allclose(a, b, rtol=2e-7, atol=1e-30)
    assert nbt == 5 + train
    if not train:
        assert rm.tobytes() == rmean.tobytes() and rv.tobytes() == rvar.tobytes()


@pytest.mark.parametrize("train", [1, 0], ids=["train", "eval"])
def test_bn_finalize_equals_seg_on_hi_lo_slots(train, dev):
    """on bn_stats_det's slots (hi, lo, zeros) both summation orders are exact: bit for bit"""
    C, rows = 72, 333
    rng = np.random.default_rng(3)
    y = (rng.normal(0, 1, (1, rows, C)) * 1.5 + rng.normal(0, 2, C)).astype(np.float32)
    st, _, _ = _stats_det(y, torch.float32, dev, stride_extra=0)
    gamma = rng.uniform(0.5, 1.5, C).astype(np.float32)
    beta = rng.normal(0, 0.5, C).astype(np.float32)
    rmean = rng.normal(0, 1, C).astype(np.float32)
    rvar = rng.uniform(0.5, 2, C).astype(np.float32)
    a = _finalize_run(dev, st, C, float(rows), gamma, beta, rmean, rvar, train, seg=False)
    b = _finalize_run(dev, st, C, float(rows), gamma, beta, rmean, rvar, train, seg=True)
    tag = f"bn_finalize == _seg {'train' if train else 'eval'}"
    check_exact(f"{tag} block", a[0], b[0])
    check_exact(f"{tag} running mean", a[1], b[1])
    check_exact(f"{tag} running var", a[2], b[2])
    assert a[3] == b[3] == 5 + train


# ---------------------------------------------------------------------- act_pool
def _blocks(rng, nseg, C):
    """[nseg][4][C] parameter blocks with mean != 0 and scale != istd"""
    mean = rng.normal(0, 1, (nseg, C))
    istd = rng.uniform(0.2, 4, (nseg, C))
    scale = istd * rng.uniform(0.5, 1.5, (nseg, C)) * np.where(rng.random((nseg, C)) < 0.1, -1, 1)
    beta = rng.normal(0, 0.5, (nseg, C))
    return np.stack([mean, istd, scale, beta], 1).astype(np.float32)


def _affine(x, blk):
    """x [nseg][...][C], blk [nseg][4][C] in one float type"""
    ex = (slice(None),) + (None,) * (x.ndim - 2)
    return (x - blk[:, 0][ex]) * blk[:, 2][ex] + blk[:, 3][ex]


def _act_pool_ref(x, blk, relu, P):
    """x [nseg][Bs][H][W][C] -> [nseg][Bs][H/P][W/P][C] in x's float type, the quad added in
    (dy, dx) order"""
    a = _affine(x, blk) if blk is not None else x
    if relu:
        a = np.maximum(a, a.dtype.type(0))
    if P == 1:
        return a
    acc = a[:, :, 0::2, 0::2] + a[:, :, 0::2, 1::2]
    acc = acc + a[:, :, 1::2, 0::2]
    acc = acc + a[:, :, 1::2, 1::2]
    return acc * a.dtype.type(0.25)


def _colsum_check(tag, cs, nseg, C, stored):
    """cs: the device buffer [nseg][32][C] + tail; stored [nseg][rows][C]: the kernel's output"""
    assert tail_intact(cs, nseg * NSLOT * C), "colsum written past its end"
    got = cs[:nseg * NSLOT * C].view(nseg, NSLOT, C).double().sum(1).cpu().numpy()
    s64 = np.asarray(stored, dtype=np.float64)
    check_atomic_sum(f"{tag} colsum", got, s64.sum(1), np.moveaxis(s64, 1, 0).reshape(s64.shape[1], -1))


# relu, bn, pool, Bs (images per segment), H, W, C, nseg
ACT_CASES = [
    (1, 1, 0, 1, 50, 45, 8, 1),      # RL 256: 2250 units, two workgroups of 2048, a ragged second
    (1, 1, 1, 1, 30, 26, 24, 1),     # C/8 = 3 does not divide 256: RL 85, 780 units over 680-unit workgroups
    (1, 1, 2, 2, 12, 10, 24, 3),     # 60 quads: one ragged trip
    (1, 1, 2, 1, 32, 36, 72, 3),     # C/8 = 9: RL 28, 288 quads over 224-unit workgroups; H != W
    (0, 1, 1, 2, 9, 11, 256, 3),     # relu 0 with bn; 198 units = 3 * 64 + 6
    (0, 0, 2, 1, 6, 10, 256, 1),     # bn NULL, relu 0: a plain average pool
    (0, 0, 0, 1, 5, 7, 256, 3),      # bn NULL, relu 0, no pool: a copy
    (1, 1, 0, 1, 3, 7, 2048, 1),     # RL 1: 21 units over 8-unit workgroups
    (1, 1, 2, 1, 6, 14, 2048, 3),    # 21 quads
    (1, 1, 0, 1, 3, 5, 2056, 1),     # C/8 = 257: the generic kernel and its colsum pass
    (1, 1, 2, 1, 4, 6, 2056, 3),
]


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("relu,bn,pool,Bs,H,W,C,nseg", ACT_CASES)
def test_act_pool(relu, bn, pool, Bs, H, W, C, nseg, dtype, dev):
    import _hip
    rng = np.random.default_rng(pool * 100003 + H * 1009 + W * 31 + C + nseg)
    P = 2 if pool == 2 else 1
    x = _rnd(dtype, rng.normal(0, 1.5, (nseg, Bs, H, W, C)))
    blk = _blocks(rng, nseg, C) if bn else None
    ref64 = _act_pool_ref(x.astype(np.float64), None if blk is None else blk.astype(np.float64), relu, P)
    ref32 = _act_pool_ref(x, blk, relu, P)
    rows = Bs * (H // P) * (W // P)
    n = nseg * rows * C
    dx = to_dev(x, dev, dtype)
    dblk = None if blk is None else torch.from_numpy(blk).to(dev)
    pb = None if blk is None else dblk.data_ptr()
    tag = f"act_pool relu{relu} bn{bn} pool{pool} {nseg}x{Bs}x{H}x{W}x{C}"
    out = with_tail(n, C, dtype, dev)
    _hip.call("artsbir_act_pool", _hip.dtype_code(dtype), dx.data_ptr(), pb, relu, pool, nseg * Bs, H, W, C, nseg,
              out.data_ptr(), _hip.stream())
    torch.cuda.synchronize()
    assert tail_intact(out, n)
    check(tag, dtype, out[:n].float().cpu().numpy().reshape(ref64.shape), ref64, ref32)
    out2 = with_tail(n, C, dtype, dev)
    cs = with_tail(nseg * NSLOT * C, C, torch.float32, dev)
    cs[:nseg * NSLOT * C] = 0
    _hip.call("artsbir_act_pool_colsum", _hip.dtype_code(dtype), dx.data_ptr(), pb, relu, pool, nseg * Bs, H, W, C, nseg,
              out2.data_ptr(), cs.data_ptr(), _hip.stream())
    torch.cuda.synchronize()
    assert tail_intact(out2, n)
    stored = out2[:n].float().cpu().numpy()
    check(f"{tag} (colsum form)", dtype, stored.reshape(ref64.shape), ref64, ref32)
    _colsum_check(tag, cs, nseg, C, stored.reshape(nseg, rows, C))


# --------------------------------------------------------------------- block_out
# downsample form?, seg_rows, C, nseg
BLOCK_CASES = [
    (1, 2250, 8, 1),       # RL 256: two workgroups of 2048 rows, a ragged second
    (0, 2 * 25, 8, 3),
    (1, 6 * 49, 72, 3),    # C/8 = 9: RL 28, 294 rows over 224-row workgroups
    (0, 3 * 49, 256, 3),   # 147 = 2 * 64 + 19
    (1, 3 * 49, 256, 1),
    (1, 2 * 25, 2048, 3),  # RL 1: 50 rows over 8-row workgroups
    (0, 2 * 25, 2048, 1),
    (1, 2 * 25, 2056, 3),  # the generic kernel and its colsum pass
    (0, 3 * 7, 2056, 1),
]


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("down,seg_rows,C,nseg", BLOCK_CASES)
def test_block_out(down, seg_rows, C, nseg, dtype, dev):
    import _hip
    rng = np.random.default_rng(down * 100003 + seg_rows * 101 + C + nseg)
    y3 = _rnd(dtype, rng.normal(0, 1.5, (nseg, seg_rows, C)))
    b3, bd = _blocks(rng, nseg, C), _blocks(rng, nseg, C)
    z3 = _affine(y3.astype(np.float64), b3.astype(np.float64))
    # the residual: a third of the elements cancel bn3(y3) to about zero (either sign, some as
    # closely as the stored type allows), so the ReLU edge of the stored value is exercised
    want = np.where(rng.random(z3.shape) < 1 / 3, -z3 * (1 + rng.choice([0.0, 1e-3, -1e-3, 1e-6, -1e-6], z3.shape)),
                    rng.normal(0, 1.5, z3.shape))
    if down:
        res = _rnd(dtype, (want - bd[:, 3][:, None]) / bd[:, 2][:, None].astype(np.float64) + bd[:, 0][:, None])
    else:
        res = _rnd(dtype, want)

    def ref(y3, res, b3, bd):
        r = _affine(res, bd) if down else res
        return np.maximum(_affine(y3, b3) + r, y3.dtype.type(0))
    ref64 = ref(y3.astype(np.float64), res.astype(np.float64), b3.astype(np.float64), bd.astype(np.float64))
    ref32 = ref(y3, res, b3, bd)
    assert ((np.abs(ref64) < 1e-2) & (ref64 > 0)).mean() > 0.02  # the case is what it says

    n = nseg * seg_rows * C
    code = _hip.dtype_code(dtype)
    dy3, dres = to_dev(y3, dev, dtype), to_dev(res, dev, dtype)
    db3, dbd = torch.from_numpy(b3).to(dev), torch.from_numpy(bd).to(dev)
    yd, pbd, idn = (dres.data_ptr(), dbd.data_ptr(), None) if down else (None, None, dres.data_ptr())
    tag = f"block_out {'down' if down else 'idn'} {nseg}x{seg_rows}x{C}"

    def outputs():
        out = with_tail(n, C, dtype, dev)
        bits = with_tail(n // 8, C, torch.uint8, dev, fill=0xA5)
        cs = with_tail(nseg * NSLOT * C, C, torch.float32, dev)
        cs[:nseg * NSLOT * C] = 0
        return out, bits, cs

    def stored_of(out, label):
        torch.cuda.synchronize()
        assert tail_intact(out, n)
        st = out[:n].float().cpu().numpy().reshape(nseg, seg_rows, C)
        check(label, dtype, st, ref64, ref32)
        return st

    def bits_check(bits, st, label):
        assert tail_intact(bits, n // 8, fill=0xA5)
        check_exact(label, bits[:n // 8].cpu().numpy().reshape(nseg, seg_rows, C // 8), pack_bits(st))

    out, bits, cs = outputs()
    _hip.call("artsbir_block_out", code, dy3.data_ptr(), db3.data_ptr(), yd, pbd, idn, nseg * seg_rows, C, nseg,
              out.data_ptr(), _hip.stream())
    stored_of(out, tag)
    out, bits, cs = outputs()
    _hip.call("artsbir_block_out_mask", code, dy3.data_ptr(), db3.data_ptr(), yd, pbd, idn, nseg * seg_rows, C, nseg,
              out.data_ptr(), bits.data_ptr(), _hip.stream())
    st = stored_of(out, f"{tag} (mask form)")
    bits_check(bits, st, f"{tag} mask bits")
    out, bits, cs = outputs()
    _hip.call("artsbir_block_out_colsum", code, dy3.data_ptr(), db3.data_ptr(), yd, pbd, idn, nseg * seg_rows, C, nseg,
              out.data_ptr(), bits.data_ptr(), cs.data_ptr(), _hip.stream())
    st = stored_of(out, f"{tag} (colsum form)")
    bits_check(bits, st, f"{tag} mask bits (colsum form)")
    _colsum_check(tag, cs, nseg, C, st)
