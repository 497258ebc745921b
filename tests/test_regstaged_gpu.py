"""Float64 parity of the register-staged kernels of csrc/gemm.hip, called on their own:
conv_gemm_kernel<T,128,64|128> through artsbir_conv2d_fwd / _fwd_seg / _fwd_act / _dgrad and
artsbir_gemm_nt, wgrad_kernel<T,64|128,128> through artsbir_conv2d_wgrad and artsbir_gemm_tn.

The reference, the bars and the case tables are in _regstaged_ref.py; test_regstaged_inputs.py
(CPU) holds the tables to the code paths they claim and the data to its sensitivity condition.
f32 reaches these kernels through the dtype; bf16 is forced with ARTSBIR_PGEMM_CFG=-2 /
ARTSBIR_WGRAD_CFG=-1 (restored by a fixture).  After every launch the kernel that ran is asserted
by its exact name.  Outputs start as NaN (accumulated ones from random values) inside buffers
whose row gaps and tails hold a sentinel that must survive; inputs carry NaN in their row gaps
and tails, which must reach no output.  Convolution outputs (no atomics) are launched twice and
must repeat byte for byte.  Each case prints one "PARITY" line; profiles/regstaged_parity.txt is
that table as measured on an MI355X.

Not covered: the 2^22-pixel / 2^30-byte offset caps of launch_wgrad_tile, which no test-sized
shape reaches.

One finding.  conv_gemm_kernel<f32,...> accumulated all of K in one chain of MFMAs, and two f32
cases missed the bar of sum y^2: fwd-f32-1x9x7x64x136x5x5x1x2-stats (K 1600, 63 pixels) by
1.81 bars and seg-f32-3x7x5x64x72x3x3x1x1-stats-seg3 (K 576, 35 per segment) by 1.04.  The sum
itself was a faithful sum of the accumulators (0.24 bars from the float64 sum of the stored y^2);
the rest was y's rounding, that of a sequential f32 accumulation over K (rms 8.9 units of 2^-24,
numpy.cumsum in float32 gives the same), squared and summed over a short segment.  The kernel now
sums each K-step on its own and adds the steps (rms 2 units); the two cases stand at 0.41 and 0.43."""
import os

import pytest
import torch

import _convref as cr
import _hip
import _kernels
import _regstaged_ref as rr
from _tail import SENT, tail_intact, with_tail

pytestmark = pytest.mark.gpu

TAIL = 64
NAN = float("nan")


@pytest.fixture
def forced_old():
    """bf16 cases force the register-staged candidates; the variables are read per call"""
    old = {k: os.environ.get(k) for k in ("ARTSBIR_PGEMM_CFG", "ARTSBIR_WGRAD_CFG")}
    os.environ["ARTSBIR_PGEMM_CFG"] = "-2"
    os.environ["ARTSBIR_WGRAD_CFG"] = "-1"
    yield
    for k, v in old.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v


def _rows(x2d, ld, dtype, dev):
    """x2d [rows][cols] in a flat buffer of rows * ld + TAIL elements; the row gaps and the tail hold NaN"""
    rows, cols = x2d.shape
    buf = with_tail(rows * ld, TAIL, dtype, dev, fill=NAN)
    buf[:rows * ld].view(rows, ld)[:, :cols] = x2d.to(dev, dtype)
    return buf


def _vec(v, dev):
    """an f32 parameter vector with a NaN tail (None -> None)"""
    return None if v is None else _rows(v.view(1, -1), v.numel(), torch.float32, dev)


def _out(rows, cols, ld, dtype, dev, prev=None):
    """an output of rows x cols at row stride ld: NaN (or prev) where the kernel writes, the sentinel in the
    row gaps and the tail"""
    buf = with_tail(rows * ld, TAIL, dtype, dev)
    buf[:rows * ld].view(rows, ld)[:, :cols] = NAN if prev is None else prev.to(dev, dtype)
    return buf


def _read_out(buf, rows, cols, ld, what):
    body = buf[:rows * ld].view(rows, ld)
    assert tail_intact(buf, rows * ld), f"{what}: the sentinel after the output was overwritten"
    if ld > cols:
        assert bool((body[:, cols:].float() == SENT).all()), f"{what}: a row gap of the output was overwritten"
    got = body[:, :cols].double().cpu()
    assert torch.isfinite(got).all(), f"{what}: NaN / unwritten output"
    return got


def _ptr(t):
    return None if t is None else t.data_ptr()


def _worst(err, bar):
    return float((err / bar.clamp_min(1e-300)).max())


# ---------------------------------------------------------------------------
@pytest.mark.parametrize("case", rr.CONV_CASES, ids=[c.id for c in rr.CONV_CASES])
def test_conv_gemm_kernel(case, dev, forced_old):
    p = rr.problem(case)
    api, dt, geo, opts = case
    T, OT = rr.DT[dt], rr.DT[p.out_dt]
    M, Co = p.M, p.Co
    x = _rows(p.x2d, p.lda, T, dev)
    w = _rows(p.w2d, p.K, T, dev)
    bias = _vec(p.bias, dev)
    sc, sh, in_relu = (_vec(p.aff[0], dev), _vec(p.aff[1], dev), p.aff[2]) if p.aff else (None, None, 0)
    res = _rows(p.res2d, Co, T, dev) if p.res2d is not None else None
    nst = p.nseg * _hip.NSLOT * 2 * Co
    d = _hip.conv_desc(T, *geo)
    outs, stats = [], []
    for i in range(2):
        y = _out(M, Co, p.ldy, OT, dev, p.prev)
        st = None
        if p.y_stats is not None:
            st = with_tail(nst, _hip.NSLOT * 2 * Co, torch.float32, dev)
            st[:nst] = 0
        ys, ss, s = y.data_ptr(), _ptr(st), _hip.stream()
        if api == "fwd":
            _hip.call("artsbir_conv2d_fwd", d, x.data_ptr(), w.data_ptr(), ys, p.ldy, p.out_f32, p.acc, _ptr(bias),
                      _ptr(sc), _ptr(sh), in_relu, ss, s)
        elif api == "seg":
            _hip.call("artsbir_conv2d_fwd_seg", d, x.data_ptr(), w.data_ptr(), ys, p.nseg, ss, s)
        elif api == "act":
            _hip.call("artsbir_conv2d_fwd_act", d, x.data_ptr(), w.data_ptr(), ys, _ptr(bias), _ptr(res), p.res_mode,
                      p.relu, s)
        elif api == "dgrad":
            _hip.call("artsbir_conv2d_dgrad", d, x.data_ptr(), w.data_ptr(), ys, _ptr(res), p.res_mode, s)
        else:
            _hip.call("artsbir_gemm_nt", _hip.dtype_code(T), M, Co, p.K, x.data_ptr(), p.lda, w.data_ptr(), ys, p.ldy,
                      p.out_f32, p.acc, _ptr(bias), ss, s)
        assert _kernels.last_kernel() == rr.conv_kernel(dt, Co), (_kernels.last_kernel(), rr.conv_kernel(dt, Co))
        outs.append(y)
        stats.append(st)
    torch.cuda.synchronize()
    itype = torch.int32 if OT == torch.float32 else torch.int16
    assert torch.equal(outs[0].view(itype), outs[1].view(itype)), "the stored output differs between two launches"

    r = cr.Report(f"{case.id} {rr.conv_kernel(dt, Co)}")
    got = _read_out(outs[0], M, Co, p.ldy, case.id)
    err = (got - p.ref).abs()
    r.add("y", err.max().item(), _worst(err, p.bar))
    if p.y_stats is not None:
        for st in stats:
            assert tail_intact(st, nst), "the slots after the last segment's were written"
        s = stats[0][:nst].view(p.nseg, _hip.NSLOT, 2, Co).double().sum(1).cpu().numpy()   # [nseg][2][Co]
        for j, (name, terms) in enumerate(p.stats_sums()):
            r.sums(name, s[:, j], terms, p.nseg)
    r.done()


def test_seven_by_seven_is_refused(dev):
    """49 filter taps do not fit the 32-bit validity mask: -1 with the error set, nothing launched"""
    d = _hip.conv_desc(torch.float32, 1, 9, 9, 8, 8, 7, 7, 1, 3)
    x = torch.zeros(81 * 8, device=dev)
    w = torch.zeros(8 * 49 * 8, device=dev)
    y = with_tail(81 * 8, TAIL, torch.float32, dev)
    before = _kernels.last_kernel()
    rc = _hip.lib().artsbir_conv2d_fwd(d, x.data_ptr(), w.data_ptr(), y.data_ptr(), 8, 0, 0, None, None, None, 0, None,
                                       _hip.stream())
    torch.cuda.synchronize()
    assert rc == -1
    assert "at most 32 filter taps" in _hip.lib().artsbir_last_error().decode()
    assert _kernels.last_kernel() == before
    assert bool((y == SENT).all())


# ---------------------------------------------------------------------------
@pytest.mark.parametrize("case", rr.WGRAD_CASES, ids=[c.id for c in rr.WGRAD_CASES])
def test_wgrad_kernel(case, dev, forced_old):
    p = rr.problem(case)
    api, dt, geo, opts = case
    T = rr.DT[dt]
    M, Co, K = p.M, p.Co, p.K
    dy = _rows(p.dy, p.ldd, T, dev)
    x = _rows(p.x2d, p.ldx, T, dev)
    sc, sh, in_relu = (_vec(p.aff[0], dev), _vec(p.aff[1], dev), p.aff[2]) if p.aff else (None, None, 0)
    dw = _out(Co, K, K, torch.float32, dev, p.prev)
    if api == "conv":
        d = _hip.conv_desc(T, *geo)
        _hip.call("artsbir_conv2d_wgrad", d, dy.data_ptr(), x.data_ptr(), _ptr(sc), _ptr(sh), in_relu, dw.data_ptr(),
                  _hip.stream())
    else:
        _hip.call("artsbir_gemm_tn", _hip.dtype_code(T), M, Co, K, dy.data_ptr(), p.ldd, x.data_ptr(), p.ldx,
                  dw.data_ptr(), _hip.stream())
    assert _kernels.last_kernel() == rr.wgrad_kernel(dt, Co), (_kernels.last_kernel(), rr.wgrad_kernel(dt, Co))
    torch.cuda.synchronize()
    r = cr.Report(f"{case.id} {rr.wgrad_kernel(dt, Co)} splits {p.splits} x {p.m_per_split}")
    got = _read_out(dw, Co, K, K, case.id)
    err = (got - p.ref).abs()
    r.add("dw", err.max().item(), _worst(err, p.bar))
    r.done()
