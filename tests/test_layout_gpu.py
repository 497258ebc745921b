"""Layout and parameter-packing kernels (csrc/elementwise.hip) called on raw pointers:
exact equality with numpy / torch restatements of the formulas in include/artsbir.h.

artsbir_pack_input   out[b][h][w][c] = (T) x[b][c][h][w] for c < Cin, 0 for Cin <= c < 8
artsbir_cast         y[i] = (TO) x[i]  (bf16: round to nearest even), vector path only when
                     both pointers are 16-byte aligned
artsbir_pack_weight  mode 0: dst[co][r][s][ci'] = src[co][ci'][r][s] (ci' < Ci), 0 up to ci_pad
                     mode 1: dst[((ci R + r) S + s) ldo + co] = src[co][ci][R-1-r][S-1-s]
artsbir_pack_weights a device table of such entries in one launch (mode 2: an f32 copy of
                     Co elements), entry i starting at block blk0[i]
artsbir_unpack_wgrad dst[co][ci][r][s] += src[co][r][s][ci], src rows of Cp >= Ci channels
artsbir_bn_fold      w_out = w gamma / sqrt(var + eps), bias = beta - mean gamma / sqrt(var + eps)
                     (f32 arithmetic: _tail.check_f32 against float64)
Every output buffer carries a sentinel tail; gaps of a strided output stay at the sentinel."""
import ctypes

import numpy as np
import pytest
import torch

from _tail import SENT, check_exact, check_f32, tail_intact, with_tail

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16]
DT_IDS = ["f32", "bf16"]


def _bits(t):
    """a CPU tensor's bit patterns (so -0 != +0 and every NaN-free value compares exactly)"""
    t = t.contiguous()
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16).numpy()


# -------------------------------------------------------------------- pack_input
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("B,Cin,H,W", [(2, 1, 5, 9), (3, 3, 7, 4), (1, 8, 3, 11), (2, 3, 37, 29)])
def test_pack_input(B, Cin, H, W, dtype, dev):
    import _hip
    rng = np.random.default_rng(B * 1009 + Cin * 31 + H)
    x = torch.from_numpy(rng.normal(0, 1, (B, Cin, H, W)).astype(np.float32))
    n = B * H * W * 8
    out = with_tail(n, 8, dtype, dev)
    _hip.call("artsbir_pack_input", _hip.dtype_code(dtype), x.to(dev).data_ptr(), B, Cin, H, W, out.data_ptr(),
              _hip.stream())
    torch.cuda.synchronize()
    assert tail_intact(out, n)
    exp = torch.zeros(B, H, W, 8)
    exp[..., :Cin] = x.permute(0, 2, 3, 1)
    check_exact(f"pack_input {B}x{Cin}x{H}x{W} {dtype}", _bits(out[:n].cpu().view(B, H, W, 8)), _bits(exp.to(dtype)))


# -------------------------------------------------------------------------- cast
def _cast_values(n, src):
    """n f32 values: signed zeros, infinities, f32 subnormals, exact bf16 ties in both
    directions, the largest finite f32, then random ones"""
    special = np.array([0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x00000001, 0x80000001, 0x007FFFFF, 0x00400000,
                        0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000,  # ties: to even down / up
                        0x3F808001, 0x3F807FFF, 0x7F7FFFFF, 0xFF7FFFFF, 0x7F7F8000, 0x00008000, 0x00018000],
                       dtype=np.uint32).view(np.float32)
    rng = np.random.default_rng(n)
    v = np.concatenate([special, (rng.normal(0, 1, n) * 10.0 ** rng.integers(-6, 6, n)).astype(np.float32)])
    v = np.roll(v, 3)[:n] if n >= 8 else v[[8, 1, 2, 9, 6, 14, 10][:n]]
    t = torch.from_numpy(np.ascontiguousarray(v))
    return t.to(src)  # a bf16 source: the rounded values


@pytest.mark.parametrize("soff,doff", [(0, 0), (1, 0), (0, 1), (1, 1)], ids=["aligned", "src+1", "dst+1", "both+1"])
@pytest.mark.parametrize("n", [1, 7, 8, 9, 8 * 256 * 3 + 5])
@pytest.mark.parametrize("dst", DTYPES, ids=["to_f32", "to_bf16"])
@pytest.mark.parametrize("src", DTYPES, ids=["f32", "bf16"])
def test_cast(src, dst, n, soff, doff, dev):
    import _hip
    x = _cast_values(n, src)
    xs = torch.zeros(n + 1, dtype=src, device=dev)
    xs[soff:soff + n] = x.to(dev)
    y = with_tail(1 + n, 16, dst, dev)  # one leading sentinel for the offset destination
    _hip.call("artsbir_cast", _hip.dtype_code(src), xs.data_ptr() + soff * xs.element_size(), _hip.dtype_code(dst),
              y.data_ptr() + doff * y.element_size(), n, _hip.stream())
    torch.cuda.synchronize()
    assert tail_intact(y, doff + n) and bool((y[:doff].float() == SENT).all()), "cast wrote outside [0, n)"
    check_exact(f"cast {src}->{dst} n={n} src+{soff} dst+{doff}", _bits(y[doff:doff + n].cpu()), _bits(x.to(dst)))


# ------------------------------------------------------------------- pack_weight
def _pack_ref(src, ci_pad, mode, ldo, fill):
    """index by index, as the header states it; untouched elements stay at `fill`"""
    Co, Ci, R, S = src.shape
    if mode == 0:
        dst = np.full((Co, R, S, ci_pad), fill, np.float32)
        for co in range(Co):
            for r in range(R):
                for s in range(S):
                    for ci in range(ci_pad):
                        dst[co, r, s, ci] = src[co, ci, r, s] if ci < Ci else 0.0
        return dst.reshape(-1)
    dst = np.full((Ci * R * S * ldo,), fill, np.float32)
    for ci in range(Ci):
        for r in range(R):
            for s in range(S):
                dst[((ci * R + r) * S + s) * ldo:((ci * R + r) * S + s) * ldo + Co] = src[:, ci, R - 1 - r, S - 1 - s]
    return dst


def _as(dtype, a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("Co,Ci,RS,ci_pad", [(8, 3, 1, 8), (72, 3, 3, 8), (130, 3, 3, 8), (130, 3, 1, 8), (72, 16, 3, 16)])
def test_pack_weight(Co, Ci, RS, ci_pad, mode, dtype, dev):
    import _hip
    rng = np.random.default_rng(Co * 101 + Ci * 7 + RS + mode)
    src = rng.normal(0, 1, (Co, Ci, RS, RS)).astype(np.float32)
    ldo = Co + 6
    exp = _pack_ref(src, ci_pad, mode, ldo, SENT)
    dst = with_tail(exp.size, 64, dtype, dev)
    _hip.call("artsbir_pack_weight", _hip.dtype_code(dtype), torch.from_numpy(src).to(dev).data_ptr(), Co, Ci, RS, RS,
              ci_pad, mode, ldo, dst.data_ptr(), _hip.stream())
    torch.cuda.synchronize()
    assert tail_intact(dst, exp.size)
    check_exact(f"pack_weight mode{mode} {Co}x{Ci}x{RS}x{RS} pad{ci_pad} {dtype}", _bits(dst[:exp.size].cpu()),
                _bits(_as(dtype, exp)))


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_pack_weights_table(dtype, dev):
    """against the numpy restatements, not against artsbir_pack_weight"""
    import _hip
    # Co, Ci, R = S, ci_pad, mode, ldo
    entries = [(72, 3, 3, 8, 0, 0),      # 5184 elements: six blocks, the last partial
               (128, 5, 1, 8, 0, 0),     # exactly 1024 elements
               (130, 3, 3, 8, 1, 136),   # K = 27, Co = 130: 3 x 1 ragged tiles, ldo > Co
               (72, 24, 3, 24, 1, 72),   # K = 216: 2 x 4 tiles, ragged both ways
               (1030, 1, 1, 1, 2, 0),    # a bias of more than one block
               (9, 3, 1, 8, 0, 0)]       # the last entry ends on a partial block
    rng = np.random.default_rng(17)
    tab = (_hip.PackDesc * len(entries))()
    keep, blk = [], 0
    for i, (Co, Ci, RS, ci_pad, mode, ldo) in enumerate(entries):
        if mode == 2:
            src = rng.normal(0, 1, (Co,)).astype(np.float32)
            exp, dt = src.copy(), torch.float32
            nblk = -(-Co // 1024)
        else:
            src = rng.normal(0, 1, (Co, Ci, RS, RS)).astype(np.float32)
            exp, dt = _pack_ref(src, ci_pad, mode, ldo, SENT), dtype
            nblk = -(-exp.size // 1024) if mode == 0 else -(-Co // 64) * -(-(Ci * RS * RS) // 64)
        dsrc = torch.from_numpy(src).to(dev)
        dst = with_tail(exp.size, 64, dt, dev)
        tab[i].src, tab[i].dst = dsrc.data_ptr(), dst.data_ptr()
        tab[i].Co, tab[i].Ci, tab[i].R, tab[i].S, tab[i].ci_pad, tab[i].mode = Co, Ci, RS, RS, ci_pad, mode
        tab[i].ldo, tab[i].blk0 = ldo, blk
        blk += nblk
        keep.append((dsrc, dst, exp, dt))
    raw = np.frombuffer(bytes(tab), dtype=np.uint8).copy()
    dtab = torch.from_numpy(raw).to(dev)
    _hip.call("artsbir_pack_weights", _hip.dtype_code(dtype), dtab.data_ptr(), len(entries), blk, _hip.stream())
    torch.cuda.synchronize()
    for i, (_, dst, exp, dt) in enumerate(keep):
        assert tail_intact(dst, exp.size), i
        check_exact(f"pack_weights entry {i} mode{entries[i][4]} {dtype}", _bits(dst[:exp.size].cpu()), _bits(_as(dt, exp)))


# ------------------------------------------------------------------ unpack_wgrad
@pytest.mark.parametrize("Co,Ci,RS,Cp", [(8, 3, 3, 8), (72, 3, 1, 8), (5, 24, 3, 32), (130, 16, 1, 16)])
def test_unpack_wgrad(Co, Ci, RS, Cp, dev):
    import _hip
    rng = np.random.default_rng(Co + Ci + RS)
    src = rng.normal(0, 1, (Co, RS, RS, Cp)).astype(np.float32)
    dst0 = rng.normal(0, 1, (Co, Ci, RS, RS)).astype(np.float32)  # pre-filled: the kernel accumulates
    n = dst0.size
    dst = with_tail(n, 64, torch.float32, dev)
    dst[:n] = torch.from_numpy(dst0.reshape(-1)).to(dev)
    _hip.call("artsbir_unpack_wgrad", torch.from_numpy(src).to(dev).data_ptr(), Co, Ci, RS, RS, Cp, dst.data_ptr(),
              _hip.stream())
    torch.cuda.synchronize()
    assert tail_intact(dst, n)
    exp = dst0 + src[..., :Ci].transpose(0, 3, 1, 2)  # one f32 addition per element
    check_exact(f"unpack_wgrad {Co}x{Ci}x{RS}x{RS} Cp{Cp}", dst[:n].cpu().numpy().reshape(dst0.shape), exp)


# ----------------------------------------------------------------------- bn_fold
@pytest.mark.parametrize("Co,K", [(1, 1), (1, 4608), (64, 27), (2048, 1), (64, 4608), (2048, 27), (2048, 4608)])
def test_bn_fold(Co, K, dev):
    import _hip
    rng = np.random.default_rng(Co * 7 + K)
    w = rng.normal(0, 1, (Co, K)).astype(np.float32)
    gamma = rng.uniform(0.5, 1.5, Co).astype(np.float32)
    beta = rng.normal(0, 0.5, Co).astype(np.float32)
    mean = rng.normal(0, 2, Co).astype(np.float32)
    var = rng.uniform(0.05, 3, Co).astype(np.float32)
    eps = np.float32(1e-5)
    t = lambda a: torch.from_numpy(a).to(dev)  # noqa: E731
    dw, dg, db, dm, dv = t(w), t(gamma), t(beta), t(mean), t(var)
    wo = with_tail(Co * K, 64, torch.float32, dev)
    bo = with_tail(Co, 64, torch.float32, dev)
    _hip.call("artsbir_bn_fold", dw.data_ptr(), Co, K, dg.data_ptr(), db.data_ptr(), dm.data_ptr(), dv.data_ptr(),
              float(eps), wo.data_ptr(), bo.data_ptr(), _hip.stream())
    torch.cuda.synchronize()
    assert tail_intact(wo, Co * K) and tail_intact(bo, Co)
    sc64 = gamma.astype(np.float64) / np.sqrt(var.astype(np.float64) + float(eps))
    sc32 = gamma / np.sqrt(var + eps)
    check_f32(f"bn_fold {Co}x{K} w", wo[:Co * K].cpu().numpy().reshape(Co, K), w.astype(np.float64) * sc64[:, None],
              w * sc32[:, None])
    check_f32(f"bn_fold {Co}x{K} bias", bo[:Co].cpu().numpy(), beta.astype(np.float64) - mean.astype(np.float64) * sc64,
              beta - mean * sc32)
