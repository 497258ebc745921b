"""Shared bars of the step's-tail parity tests (test infrastructure): the attention
pool, token, head, loss and Adam kernels against float64 restatements.

Every f32 output is held to  e_hip <= max(8 * e_f32, 8 * 2^-24)  with
  e_x = max|x - ref64| / max|ref64|
where e_f32 is the error of an f32 CPU restatement of the same formula (numpy /
torch f32, or the torch CPU op the reference calls).  The factor 8 over the f32
restatement's own error covers the kernels' different summation order (wave
shuffles, four-wave partials) and the hardware fast exponential of the attention
softmax.  A bf16 output is computed in f32 from bf16-rounded inputs and rounded
once, so it is held elementwise to  2^-8 |ref64| + (the f32 bar) * max|ref64|.
Where the reference is identically zero
(a gradient that cancels exactly, e.g. d cos / dx at D = 1) e_x has no scale; the
same factor is then applied to the absolute errors: max|hip| <= 8 max|f32|, so an
exact zero of the f32 restatement must be met exactly.
Each check prints one "PARITY" line (pytest -s); profiles/r8_tail_parity.txt is
that table as measured on an MI355X."""
import numpy as np
import torch

U32 = 2.0 ** -24


def f64(x):
    if isinstance(x, torch.Tensor):
        return x.detach().to("cpu", torch.float64).numpy()
    return np.asarray(x, dtype=np.float64)


def bf16_round(a):
    """f32 numpy array rounded to bf16 (round to nearest even), as f32"""
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(torch.bfloat16).float().numpy()


def _errors(hip, ref64, f32):
    hip, ref64, f32 = f64(hip), f64(ref64), f64(f32)
    assert hip.shape == ref64.shape == f32.shape, (hip.shape, ref64.shape, f32.shape)
    assert np.isfinite(hip).all(), "non-finite kernel output"
    scale = float(np.abs(ref64).max()) if ref64.size else 0.0
    if scale == 0.0:  # an all-zero reference: absolute errors
        amax = lambda a: float(np.abs(a).max()) if a.size else 0.0  # noqa: E731
        return hip, ref64, 0.0, amax(hip), amax(f32)
    e_hip = float(np.abs(hip - ref64).max()) / scale
    e_f32 = float(np.abs(f32 - ref64).max()) / scale
    return hip, ref64, scale, e_hip, e_f32


def check_f32(label, hip, ref64, f32, quiet=False):
    """assert the f32 bar; returns (e_hip, e_f32)"""
    hip, ref64, scale, e_hip, e_f32 = _errors(hip, ref64, f32)
    bar = max(8 * e_f32, 8 * U32)
    if not quiet:
        shown = f"bar={bar:.3e}" if scale else "zero reference: absolute errors, bar=8*e_f32"
        print(f"PARITY {label:<58s} f32  e_hip={e_hip:.3e} e_f32={e_f32:.3e} {shown}")
    if scale == 0.0:
        assert e_hip <= 8 * e_f32, (label, "absolute, zero reference", e_hip, e_f32)
    else:
        assert e_hip <= bar, (label, e_hip, e_f32, bar)
    return e_hip, e_f32


def check_bf16(label, hip, ref64, f32):
    """assert the elementwise bf16 bar around the f32 bar; returns (e_hip, e_f32)"""
    hip, ref64, scale, e_hip, e_f32 = _errors(hip, ref64, f32)
    bar = max(8 * e_f32, 8 * U32)
    print(f"PARITY {label:<58s} bf16 e_hip={e_hip:.3e} e_f32={e_f32:.3e} bar=2^-8|ref|+{bar:.3e}*max")
    if scale == 0.0:
        assert e_hip <= 8 * e_f32, (label, "absolute, zero reference", e_hip, e_f32)
        return e_hip, e_f32
    excess = np.abs(hip - ref64) - (2.0 ** -8 * np.abs(ref64) + bar * scale)
    assert excess.max() <= 0, (label, float(excess.max()), e_hip, e_f32)
    return e_hip, e_f32


def check(label, dtype, hip, ref64, f32):
    return (check_bf16 if dtype == torch.bfloat16 else check_f32)(label, hip, ref64, f32)


def check_atomic_sum(label, hip, ref64, terms64):
    """a one-row operand's gradient: the sum of terms64 [n][D] over the n rows by
    f32 atomics in arbitrary order.  Worst-case bound of any summation order of n
    f32 terms, per column:  n * 2^-24 * sum_r |term_r[d]|  (derived, not measured)"""
    hip, ref64, terms64 = f64(hip).reshape(-1), f64(ref64).reshape(-1), f64(terms64)
    n = terms64.shape[0]
    bound = n * U32 * np.abs(terms64).sum(0)
    err = np.abs(hip - ref64)
    worst = float((err / np.maximum(bound, 1e-300)).max())
    print(f"PARITY {label:<58s} f32  atomic sum of n={n}: max err/bound={worst:.3e}")
    assert (err <= bound).all(), (label, worst)


# ---------------------------------------------------------------------------
# Additions for the BatchNorm / element-wise / layout parity tests
# (tests/test_bn_bwd_gpu.py, test_bn_elementwise_gpu.py, test_layout_gpu.py;
# profiles/r11_bn_parity.txt is their table).  The bars above are unchanged.
SENT = -768.0  # exact in bf16 and f32
NSLOT = 32


def to_dev(a, dev, dtype=torch.float32):
    """numpy array -> flat contiguous device tensor of `dtype` (values are expected to
    be representable, so the conversion is exact)"""
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev).to(dtype).reshape(-1).contiguous()


def with_tail(n, tail, dtype, dev, fill=SENT):
    """a flat buffer of n + tail elements, all `fill`"""
    return torch.full((n + tail,), fill, dtype=dtype, device=dev)


def tail_intact(buf, n, fill=SENT):
    return bool((buf[n:].float() == fill).all().item())


def pack_bits(mask):
    """numpy [..., C] -> uint8 [..., C/8]: bit e of byte c = mask[..., 8c+e] > 0 (the
    layout of tests/test_fused_gpu.py::_pack_bits)"""
    m = (np.asarray(mask) > 0).astype(np.uint8).reshape(*mask.shape[:-1], -1, 8)
    return (m << np.arange(8, dtype=np.uint8)).sum(-1).astype(np.uint8)


def check_exact(label, hip, ref):
    """bit-for-value equality (a select / copy / exact scaling of stored values)"""
    hip, ref = f64(hip), f64(ref)
    assert hip.shape == ref.shape, (hip.shape, ref.shape)
    bad = int((hip != ref).sum()) if hip.size else 0
    print(f"PARITY {label:<58s} exact mismatches={bad} of {hip.size}")
    assert bad == 0, (label, bad, float(np.abs(hip - ref).max()))


def check_det_sum(label, hip64, ref64, abs_terms_sum, n, rel):
    """a fixed-order f64 sum of n terms stored as an f32 hi/lo pair:
    |hip - ref| <= (rel + n * 2^-53) * sum |term|  per channel (derived, worst case)"""
    hip64, ref64, a = f64(hip64).reshape(-1), f64(ref64).reshape(-1), f64(abs_terms_sum).reshape(-1)
    assert np.isfinite(hip64).all(), label
    bound = (rel + n * 2.0 ** -53) * a
    err = np.abs(hip64 - ref64)
    worst = float((err / np.maximum(bound, 1e-300)).max())
    print(f"PARITY {label:<58s} f64  fixed-order sum of n={n}: max err/bound={worst:.3e}")
    assert (err <= bound).all(), (label, worst)


def atomic_bound(terms64):
    """check_atomic_sum's bound of the sum over axis 0 of terms64 [n][...]"""
    terms64 = f64(terms64)
    return terms64.shape[0] * U32 * np.abs(terms64).sum(0)


def check_widened(label, dtype, hip, ref64, f32, extra):
    """check()'s bar with every element's allowance widened by extra (same shape as
    ref64, >= 0): what a derived bound on an input of the kernel can move that element"""
    hip, ref64, scale, e_hip, e_f32 = _errors(hip, ref64, f32)
    extra = f64(extra)
    assert extra.shape == ref64.shape and (extra >= 0).all()
    bar = max(8 * e_f32, 8 * U32)
    allow = bar * scale + extra
    name = "f32 "
    if dtype == torch.bfloat16:
        allow = allow + 2.0 ** -8 * np.abs(ref64)
        name = "bf16"
    worst = float((np.abs(hip - ref64) / np.maximum(allow, 1e-300)).max())
    print(f"PARITY {label:<58s} {name} e_hip={e_hip:.3e} e_f32={e_f32:.3e} bar={bar:.3e}*max+derived: "
          f"max err/allowed={worst:.3e}")
    assert worst <= 1.0, (label, worst, e_hip, e_f32)
