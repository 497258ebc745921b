"""BatchNorm backward, reduce and apply (artsbir_bn_bwd_reduce / artsbir_bn_bwd_apply,
csrc/elementwise.hip) called on raw pointers against float64.

Per segment s and target t (tensors [nseg][B][H][W][C], n = B*H*W pixels):
  g     = d * [mask > 0]                                   kind 0
        = d * [bit]                                        kind 3 (mask packed as bits)
        = d                                                kind 2
        = up(d) / pool^2 * [(y_0 - mean) * scale + beta > 0]   kind 1, the mask_bn block of target 0
  xhat_t = (y_t - mean_t) * istd_t
  reduce:  sum g  and  sum g * xhat_t   per channel, spread over the 32 replica slots
           (the test adds the slots itself); deterministic mode: one f64 sum as an
           f32 hi/lo pair in slots 0 / 1, slots 2 .. 31 zero
  apply:   dy_t = c1 * (g - c2 - xhat_t * c3),  gout = g
The shapes follow launch_bnb's geometry (one lane per 8 channels, RL = 256 / (C/8)
unit lanes, UN units per trip with a clamped tail, the slot index blockIdx.x % 32,
per-segment pointer advance); parameter, coefficient and slot strides are above the
minimum and the gaps hold NaN / a sentinel.  Every output carries a sentinel tail;
the slots' tail is a whole further slot block.

Bars.  g / gout: exact.  Deterministic sums: (2 * 2^-24 + n 2^-53) sum|g xhat| and
(2^-47 + n 2^-53) sum|g|, derived (y - mean is formed in f32, the rest in f64).  Atomic
sums: _tail.check_atomic_sum.  dy: _tail.check against an f32 restatement, the apply
fed with coefficients from the float64 sums.  The chain reduce -> bn_bwd_finalize_seg
-> apply is compared with torch float64 autograd of relu(batch_norm(y, training=True))
(dy, dgamma, dbeta): _tail.check in deterministic mode, in atomic mode every element
widened by what the sums' derived bound moves it, |c1| (b1 + |xhat| b2) / n."""
import ctypes
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from _tail import (NSLOT, SENT, atomic_bound, bf16_round, check, check_atomic_sum, check_det_sum, check_exact,
                   check_f32, check_widened, pack_bits, tail_intact, to_dev, with_tail)

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16]
DT_IDS = ["f32", "bf16"]
EPS = float(np.float32(1e-5))

# name: kind, pool, B (per segment), H, W, C, nseg, ntarget
CASES = {
    "k0_1x7x7x2048_t2": (0, 0, 1, 7, 7, 2048, 1, 2),      # RL 1; 49 reduce workgroups; apply UN 2, last workgroup 1 unit
    "k0_2x11x13x64_s3_t1": (0, 0, 2, 11, 13, 64, 3, 1),   # RL 32, 286 units: 256 + 30; UN 4
    "k0_2x11x13x64_s3_t2": (0, 0, 2, 11, 13, 64, 3, 2),   # UN 2
    "k3_2x11x13x64_s3_t1": (3, 0, 2, 11, 13, 64, 3, 1),   # the same data as k0, mask as bits (advance by /8)
    "k3_2x11x13x64_s3_t2": (3, 0, 2, 11, 13, 64, 3, 2),
    "k1p0_3x30x30x8_s2": (1, 0, 3, 30, 30, 8, 2, 1),      # CG 1, RL 256; 2700 units: two apply workgroups
    "k1p2_2x6x10x128_s3": (1, 2, 2, 6, 10, 128, 3, 1),    # H != W quads, d advancing by full / 4
    "k1p2_1x14x14x512": (1, 2, 1, 14, 14, 512, 1, 1),
    "k2_2x9x9x256_s1": (2, 0, 2, 9, 9, 256, 1, 1),        # load8_last of the apply
    "k2_2x9x9x256_s3": (2, 0, 2, 9, 9, 256, 3, 2),
}
CHAIN = ["k0_2x11x13x64_s3_t2", "k3_2x11x13x64_s3_t2", "k1p0_3x30x30x8_s2", "k1p2_2x6x10x128_s3", "k1p2_1x14x14x512",
         "k2_2x9x9x256_s3"]


def _rnd(dtype, a):
    a = np.asarray(a, dtype=np.float32)
    return bf16_round(a) if dtype == torch.bfloat16 else a


class Case:
    pass


@functools.lru_cache(maxsize=None)
def _case(name, bf16):
    """inputs (f32 numpy, representable in the compute dtype) and the float64 reference, built once"""
    dtype = torch.bfloat16 if bf16 else torch.float32
    kind, pool, B, H, W, C, nseg, nt = CASES[name]
    c = Case()
    c.name, c.dtype, c.kind, c.pool, c.B, c.H, c.W, c.C, c.nseg, c.nt = name, dtype, kind, pool, B, H, W, C, nseg, nt
    P = 2 if pool == 2 else 1
    n = B * H * W
    c.n, c.P = n, P
    rng = np.random.default_rng(B * 1000003 + H * 10007 + W * 101 + C + 7 * nseg)  # not the kind: k3 shares k0's data
    cm = rng.normal(0, 1, (nt, 1, 1, C))
    cs = rng.uniform(0.5, 2, (nt, 1, 1, C))
    draw = lambda shape, t: _rnd(dtype, rng.normal(0, 1, shape) * cs[t, 0, 0] + cm[t, 0, 0])  # noqa: E731
    y = np.stack([draw((nseg, n, C), t) for t in range(nt)])  # [nt][nseg][n][C]
    c.gamma = rng.uniform(0.5, 1.5, (nt, C)).astype(np.float32)
    c.beta = rng.normal(0, 0.5, (nt, C)).astype(np.float32)

    def params(y):
        y64 = y.astype(np.float64)
        mean = y64.mean(2).astype(np.float32)                                # [nt][nseg][C]
        istd = (1.0 / np.sqrt(y64.var(2) + EPS)).astype(np.float32)
        return mean, istd, c.gamma[:, None, :] * istd                         # scale: the f32 product
    mean, istd, scale = params(y)
    c.rounds = 0
    if kind == 1:  # unambiguous ReLU decisions: redraw what lies within 2^-10 of the channel's scale of zero
        for c.rounds in range(1, 20):
            y64 = y[0].astype(np.float64)
            bn = (y64 - mean[0][:, None]) * scale[0][:, None] + c.beta[0]
            lim = 2.0 ** -10 * (np.abs(scale[0]) * y64.std(1) + np.abs(c.beta[0]))[:, None]
            amb = np.abs(bn) < lim
            if not amb.any():
                break
            y[0][amb] = draw((nseg, n, C), 0)[amb]
            mean, istd, scale = params(y)
        assert not amb.any(), "the redraw loop did not end"
    c.y, c.mean, c.istd, c.scale = y, mean, istd, scale
    y64 = y.astype(np.float64)
    xhat = (y64 - mean[:, :, None]) * istd[:, :, None].astype(np.float64)    # with the f32 parameters the kernel reads
    bnv = xhat * c.gamma[:, None, None].astype(np.float64) + c.beta[:, None, None]
    c.d = _rnd(dtype, rng.normal(0, 1, (nseg, n // (P * P), C)))
    d64 = c.d.astype(np.float64)
    c.mask = c.bits = None
    if kind in (0, 3):   # the block output relu(sum_t bn_t(y_t)) as the kernels store it
        c.mask = _rnd(dtype, np.maximum(bnv.sum(0), 0.0))
        assert ((c.mask > 0) == (bnv.sum(0) > 0)).all()
        c.bits = pack_bits(c.mask)
        c.dec = c.mask > 0
        g = d64 * c.dec
    elif kind == 2:
        g = d64
    else:
        m32, s32, h32, y32 = mean[0][:, None], scale[0][:, None], c.beta[0], y[0]
        dec64 = (y32.astype(np.float64) - m32) * s32.astype(np.float64) + h32 > 0
        diff = (y32 - m32).astype(np.float32)
        dec32 = ((diff * s32).astype(np.float32) + h32).astype(np.float32) > 0
        decfma = diff.astype(np.float64) * s32.astype(np.float64) + h32.astype(np.float64) > 0  # one rounding: the sign is exact
        assert (dec64 == dec32).all() and (dec64 == decfma).all(), "ambiguous ReLU decision left in the inputs"
        up = d64
        if P == 2:
            up = d64.reshape(nseg, B, H // 2, 1, W // 2, 1, C)
            up = np.broadcast_to(up, (nseg, B, H // 2, 2, W // 2, 2, C)).reshape(nseg, n, C) * 0.25
        c.dec = dec64
        g = up * dec64
    c.g, c.xhat = g, xhat
    c.t1 = g                                   # terms of sum g          [nseg][n][C]
    c.t2 = g[None] * xhat                      # terms of sum g * xhat   [nt][nseg][n][C]
    c.S1 = g.sum(1)                            # [nseg][C]
    c.S2 = c.t2.sum(2)                         # [nt][nseg][C]
    # the apply's coefficients from the reference sums, rounded to the f32 the kernel reads
    c.coef = np.stack([np.stack([c.gamma[t][None] * istd[t], (c.S1 / n).astype(np.float32),
                                 (c.S2[t] / n).astype(np.float32)], 1) for t in range(nt)]).astype(np.float32)  # [nt][nseg][3][C]
    c1, c2, c3 = (c.coef[:, :, i][:, :, None].astype(np.float64) for i in range(3))
    c.dy64 = c1 * (g[None] - c2 - xhat * c3)
    g32 = g.astype(np.float32)
    f = lambda a: a[:, :, None]  # noqa: E731
    c.dy32 = f(c.coef[:, :, 0]) * (g32[None] - f(c.coef[:, :, 1]) - (y - f(mean)) * f(istd) * f(c.coef[:, :, 2]))
    return c


class Bufs:
    """device buffers of one launch and the descriptor that points at them"""

    def __init__(self, c, dev, det=False, cstride=None, inplace=False, gout=True):
        import _hip
        C, nseg, nt, n, dt = c.C, c.nseg, c.nt, c.n, c.dtype
        self.c = c
        self.pstride, self.sstride = 4 * C + 64, 2 * NSLOT * C + 128
        self.cstride = 3 * C + 32 if cstride is None else cstride
        self.full = nseg * n * C
        self.keep = []
        desc = _hip.BnBwdDesc()
        desc.dtype, desc.kind, desc.pool, desc.ntarget = _hip.dtype_code(dt), c.kind, c.pool, nt
        self.d = to_dev(c.d, dev, dt)
        if c.P == 2:  # NaN up to the full-resolution size: a segment advance by `full` reads it, inside the buffer
            self.d = torch.cat([self.d, torch.full((self.full - self.d.numel(),), float("nan"), dtype=dt, device=dev)])
        if inplace:  # g over d: d gets a sentinel tail of its own
            self.d = torch.cat([self.d, with_tail(0, C, dt, dev)])
        desc.d = self.d.data_ptr()
        if c.kind == 0:
            self.keep.append(to_dev(c.mask, dev, dt))
            desc.mask = self.keep[-1].data_ptr()
        elif c.kind == 3:
            bits = torch.from_numpy(c.bits.reshape(-1).copy()).to(dev)
            # ones up to one byte per element: an advance by `full` instead of `full / 8` stays inside the buffer
            self.keep.append(torch.cat([bits, torch.full((self.full - bits.numel(),), 0xFF, dtype=torch.uint8, device=dev)]))
            desc.mask = self.keep[-1].data_ptr()
        self.slots, self.dy = [], []
        for t in range(nt):
            prm = np.full((nseg, self.pstride), np.nan, np.float32)
            prm[:, :C], prm[:, C:2 * C], prm[:, 2 * C:3 * C], prm[:, 3 * C:4 * C] = c.mean[t], c.istd[t], c.scale[t], c.beta[t]
            p = torch.from_numpy(prm).to(dev)
            co = np.full((nseg, self.cstride), np.nan, np.float32)
            co[:, :3 * C] = c.coef[t].reshape(nseg, 3 * C)
            cf = torch.from_numpy(co).to(dev)
            sl = with_tail(nseg * self.sstride, 2 * NSLOT * C, torch.float32, dev)
            sl[:nseg * self.sstride].view(nseg, self.sstride)[:, :2 * NSLOT * C] = 7.0 if det else 0.0
            yt = to_dev(c.y[t], dev, dt)
            dy = with_tail(self.full, C, dt, dev)
            self.keep += [p, cf, yt]
            self.slots.append(sl)
            self.dy.append(dy)
            desc.y[t], desc.mean[t], desc.istd[t] = yt.data_ptr(), p.data_ptr(), p.data_ptr() + 4 * C
            desc.slots[t], desc.coef[t], desc.dy[t] = sl.data_ptr(), cf.data_ptr(), dy.data_ptr()
            if t == 0 and c.kind == 1:
                desc.mask_bn = p.data_ptr()
        self.gout = None
        if inplace:
            self.gout = self.d
        elif gout:
            self.gout = with_tail(self.full, C, dt, dev)
        if self.gout is not None:
            desc.gout = self.gout.data_ptr()
        desc.B, desc.H, desc.W, desc.C, desc.nseg = c.B, c.H, c.W, C, nseg
        desc.pstride, desc.cstride, desc.sstride = self.pstride, self.cstride, self.sstride
        self.desc = desc

    def run(self, entry):
        import _hip
        _hip.call(entry, ctypes.byref(self.desc), _hip.stream())
        torch.cuda.synchronize()

    def slot_arrays(self):
        """per target [nseg][NSLOT][2][C] f32, after checking the gaps and the tail"""
        c, out = self.c, []
        for sl in self.slots:
            assert tail_intact(sl, c.nseg * self.sstride), "reduce wrote past the last segment's slots"
            a = sl[:c.nseg * self.sstride].view(c.nseg, self.sstride).cpu().numpy()
            assert (a[:, 2 * NSLOT * c.C:] == SENT).all(), "reduce wrote between two segments' slots"
            out.append(a[:, :2 * NSLOT * c.C].reshape(c.nseg, NSLOT, 2, c.C).copy())
        return out

    def g_out(self):
        assert tail_intact(self.gout, self.full), "gout written past its end"
        return self.gout[:self.full].float().cpu().numpy().reshape(self.c.nseg, self.c.n, self.c.C)

    def dy_out(self, t):
        assert tail_intact(self.dy[t], self.full), "dy written past its end"
        return self.dy[t][:self.full].float().cpu().numpy().reshape(self.c.nseg, self.c.n, self.c.C)


class deterministic:
    """artsbir_set_deterministic is process-global: set, and restore the previous value"""

    def __init__(self, on):
        self.on = on

    def __enter__(self):
        import _hip
        self.old = _hip.lib().artsbir_set_deterministic(1 if self.on else 0)

    def __exit__(self, *exc):
        import _hip
        _hip.lib().artsbir_set_deterministic(self.old)


def _check_sums(tag, c, slots, det):
    """slots: per target [nseg][NSLOT][2][C]"""
    for t, a in enumerate(slots):
        tot = a.astype(np.float64).sum(1)  # [nseg][2][C]: the replica slots added by the test
        if det:
            assert (a[:, 2:] == 0).all(), "deterministic mode: slots 2 .. 31 must be zero"
            check_det_sum(f"{tag} t{t} sum g", tot[:, 0], c.S1, np.abs(c.t1).sum(1), c.n, 2.0 ** -47)
            check_det_sum(f"{tag} t{t} sum g*xhat", tot[:, 1], c.S2[t], np.abs(c.t2[t]).sum(1), c.n, 2 * 2.0 ** -24)
        else:
            cols = lambda x: np.moveaxis(x, 1, 0).reshape(c.n, -1)  # noqa: E731  [n][nseg*C]
            check_atomic_sum(f"{tag} t{t} sum g", tot[:, 0], c.S1, cols(c.t1))
            check_atomic_sum(f"{tag} t{t} sum g*xhat", tot[:, 1], c.S2[t], cols(c.t2[t]))


@pytest.mark.parametrize("det", [False, True], ids=["atomic", "det"])
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("name", list(CASES))
def test_bn_bwd_reduce(name, dtype, det, dev):
    c = _case(name, dtype == torch.bfloat16)
    tag = f"reduce {name} {'det' if det else 'atomic'}"
    with deterministic(det):
        b = Bufs(c, dev, det=det, gout=c.P == 1)
        b.run("artsbir_bn_bwd_reduce")
        slots = b.slot_arrays()
        _check_sums(tag, c, slots, det)
        if c.P == 1:
            check_exact(f"{tag} gout", b.g_out(), c.g)
        if det:  # a second call on the same inputs: bit-identical slots
            b2 = Bufs(c, dev, det=True, gout=False)
            b2.run("artsbir_bn_bwd_reduce")
            for a, a2 in zip(slots, b2.slot_arrays()):
                assert a.tobytes() == a2.tobytes(), "deterministic reduce is not reproducible"
        if c.kind == 0:  # g written in place over d
            b3 = Bufs(c, dev, det=det, inplace=True)
            b3.run("artsbir_bn_bwd_reduce")
            _check_sums(f"{tag} in place", c, b3.slot_arrays(), det)
            check_exact(f"{tag} gout in place", b3.g_out(), c.g)


@pytest.mark.parametrize("gout", [False, True], ids=["nogout", "gout"])
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("name", list(CASES))
def test_bn_bwd_apply(name, dtype, gout, dev):
    c = _case(name, dtype == torch.bfloat16)
    tag = f"apply {name}"
    b = Bufs(c, dev, gout=gout)
    b.run("artsbir_bn_bwd_apply")
    for t in range(c.nt):
        check(f"{tag} dy{t}", dtype, b.dy_out(t), c.dy64[t], c.dy32[t])
    if gout:
        check_exact(f"{tag} gout", b.g_out(), c.g)


@pytest.mark.parametrize("det", [False, True], ids=["atomic", "det"])
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("nt", [1, 2])
def test_bn_bwd_kind3_equals_kind0(nt, dtype, det, dev):
    """the bit mask packed by the test against the tensor mask, on the same data: the
    same g, so bit-identical dy, gout and (fixed order) sums"""
    c0 = _case(f"k0_2x11x13x64_s3_t{nt}", dtype == torch.bfloat16)
    c3 = _case(f"k3_2x11x13x64_s3_t{nt}", dtype == torch.bfloat16)
    assert c0.y.tobytes() == c3.y.tobytes() and c0.d.tobytes() == c3.d.tobytes()
    with deterministic(det):
        outs = []
        for c in (c0, c3):
            b = Bufs(c, dev, det=det)
            b.run("artsbir_bn_bwd_reduce")
            sl, g = b.slot_arrays(), b.g_out()
            b = Bufs(c, dev)
            b.run("artsbir_bn_bwd_apply")
            outs.append((sl, g, [b.dy_out(t) for t in range(nt)], b.g_out()))
    (s0, g0, dy0, ga0), (s3, g3, dy3, ga3) = outs
    check_exact(f"kind 3 == kind 0 t{nt} reduce gout", g3, g0)
    check_exact(f"kind 3 == kind 0 t{nt} apply gout", ga3, ga0)
    for t in range(nt):
        check_exact(f"kind 3 == kind 0 t{nt} dy{t}", dy3[t], dy0[t])
        if det:
            assert s0[t].tobytes() == s3[t].tobytes()


# ----------------------------------------------------------------------- chain
@functools.lru_cache(maxsize=None)
def _chain_ref(name, bf16, ftype):
    """torch autograd of the forward the kernels' backward belongs to, in ftype:
    -> dy [nt][nseg][n][C], dgamma [nt][C], dbeta [nt][C]"""
    c = _case(name, bf16)
    shp = (c.nseg, c.B, c.H, c.W, c.C)
    ys = [torch.tensor(c.y[t].reshape(shp), dtype=ftype, requires_grad=True) for t in range(c.nt)]
    gam = [torch.tensor(c.gamma[t], dtype=ftype, requires_grad=True) for t in range(c.nt)]
    bet = [torch.tensor(c.beta[t], dtype=ftype, requires_grad=True) for t in range(c.nt)]
    d = torch.tensor(c.d.reshape(c.nseg, c.B, c.H // c.P, c.W // c.P, c.C), dtype=ftype).permute(0, 1, 4, 2, 3)
    L = 0
    for s in range(c.nseg):
        z = sum(F.batch_norm(ys[t][s].permute(0, 3, 1, 2), None, None, gam[t], bet[t], True, 0.0, EPS)
                for t in range(c.nt))
        if c.kind != 2:
            z = torch.relu(z)
            if ftype == torch.float64:  # the graph's ReLU decisions are the kernels'
                assert ((z > 0).permute(0, 2, 3, 1).reshape(c.n, c.C).numpy() == c.dec[s]).all()
        if c.P == 2:
            z = F.avg_pool2d(z, 2)
        L = L + (z * d[s]).sum()
    grads = torch.autograd.grad(L, ys + gam + bet)
    dy = np.stack([g.reshape(c.nseg, c.n, c.C).numpy() for g in grads[:c.nt]])
    dg = np.stack([g.numpy() for g in grads[c.nt:2 * c.nt]])
    db = np.stack([g.numpy() for g in grads[2 * c.nt:]])
    return dy, dg, db


@pytest.mark.parametrize("det", [False, True], ids=["atomic", "det"])
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("name", CHAIN)
def test_bn_bwd_chain(name, dtype, det, dev):
    """reduce -> artsbir_bn_bwd_finalize_seg -> apply, as the engine runs them"""
    import _hip
    bf = dtype == torch.bfloat16
    c = _case(name, bf)
    C, nseg, nt, n = c.C, c.nseg, c.nt, c.n
    dy64, dg64, db64 = _chain_ref(name, bf, torch.float64)
    dy32, dg32, db32 = _chain_ref(name, bf, torch.float32)
    rng = np.random.default_rng(5)
    dg0, db0 = rng.normal(0, 1, (nt, C)).astype(np.float32), rng.normal(0, 1, (nt, C)).astype(np.float32)
    tag = f"chain {name} {'det' if det else 'atomic'}"
    with deterministic(det):
        b = Bufs(c, dev, det=det, cstride=3 * C, gout=c.P == 2)  # finalize_seg writes coef[s][3][C]
        gout, b.desc.gout = b.desc.gout, None  # only the apply writes g at pool 2; the reduce refuses it
        b.run("artsbir_bn_bwd_reduce")
        b.desc.gout = gout
        keep = []
        for t in range(nt):
            coef = with_tail(nseg * 3 * C, C, torch.float32, dev)
            gm = torch.from_numpy(c.gamma[t]).to(dev)
            dgb = torch.from_numpy(np.stack([dg0[t], db0[t]])).to(dev)
            _hip.call("artsbir_bn_bwd_finalize_seg", b.slots[t].data_ptr(), nseg, b.sstride, C, float(n), gm.data_ptr(),
                      b.desc.istd[t], b.pstride, dgb[0].data_ptr(), dgb[1].data_ptr(), coef.data_ptr(), _hip.stream())
            b.desc.coef[t] = coef.data_ptr()
            keep.append((coef, gm, dgb))
        b.run("artsbir_bn_bwd_apply")
    for t in range(nt):
        coef, _, dgb = keep[t]
        assert tail_intact(coef, nseg * 3 * C)
        dgb = dgb.cpu().numpy()
        ref_g, ref_b = dg0[t].astype(np.float64) + dg64[t], db0[t].astype(np.float64) + db64[t]
        f32_g, f32_b = dg0[t] + dg32[t], db0[t] + db32[t]
        if det:
            check(f"{tag} dy{t}", dtype, b.dy_out(t), dy64[t], dy32[t])
            check_f32(f"{tag} dgamma{t}", dgb[0], ref_g, f32_g)
            check_f32(f"{tag} dbeta{t}", dgb[1], ref_b, f32_b)
        else:
            b1 = atomic_bound(np.moveaxis(c.t1, 1, 0))       # [nseg][C]
            b2 = atomic_bound(np.moveaxis(c.t2[t], 1, 0))
            c1 = np.abs(c.coef[t][:, 0].astype(np.float64))  # [nseg][C]
            extra = c1[:, None] * (b1[:, None] + np.abs(c.xhat[t]) * b2[:, None]) / n
            check_widened(f"{tag} dy{t}", dtype, b.dy_out(t), dy64[t], dy32[t], extra)
            check_widened(f"{tag} dgamma{t}", torch.float32, dgb[0], ref_g, f32_g, b2.sum(0))
            check_widened(f"{tag} dbeta{t}", torch.float32, dgb[1], ref_b, f32_b, b1.sum(0))
    if c.P == 2:
        check_exact(f"{tag} gout", b.g_out(), c.g)


@pytest.mark.parametrize("det", [False, True], ids=["atomic", "det"])
def test_bn_bwd_finalize_equals_seg(det, dev):
    """artsbir_bn_bwd_finalize (one segment) on the slots of a reduce == _seg with nseg 1, bit for bit"""
    import _hip
    c = _case("k0_1x7x7x2048_t2", False)
    C = c.C
    with deterministic(det):
        b = Bufs(c, dev, det=det, gout=False)
        b.run("artsbir_bn_bwd_reduce")
    rng = np.random.default_rng(6)
    init = rng.normal(0, 1, (2, C)).astype(np.float32)
    gm = torch.from_numpy(c.gamma[0]).to(dev)
    outs = []
    for seg in (False, True):
        coef = with_tail(3 * C, C, torch.float32, dev)
        dgb = torch.from_numpy(init).to(dev)
        if seg:
            _hip.call("artsbir_bn_bwd_finalize_seg", b.slots[0].data_ptr(), 1, b.sstride, C, float(c.n), gm.data_ptr(),
                      b.desc.istd[0], b.pstride, dgb[0].data_ptr(), dgb[1].data_ptr(), coef.data_ptr(), _hip.stream())
        else:
            _hip.call("artsbir_bn_bwd_finalize", b.slots[0].data_ptr(), C, float(c.n), gm.data_ptr(), b.desc.istd[0],
                      dgb[0].data_ptr(), dgb[1].data_ptr(), coef.data_ptr(), _hip.stream())
        torch.cuda.synchronize()
        assert tail_intact(coef, 3 * C)
        outs.append((coef[:3 * C].cpu().numpy(), dgb.cpu().numpy()))
    check_exact("bn_bwd_finalize == _seg coef", outs[0][0], outs[1][0])
    check_exact("bn_bwd_finalize == _seg dgamma, dbeta", outs[0][1], outs[1][1])
    assert (outs[0][1] != init).any()
