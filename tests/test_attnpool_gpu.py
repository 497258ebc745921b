"""Attention-pool core and token kernels called on their own, against float64.

artsbir_attnpool_fwd / _bwd (csrc/attnpool.hip): per image and head one query
against T tokens, head_dim 64, each lane owning tokens `lane` and `lane + 64`:
  s_t = q_h . k_t / 8,  p = softmax_t(s),  o = sum_t p_t v_t
  dp_t = dO_h . v_t,  ds = p * (dp - sum p dp),  dq = sum_t ds_t k_t / 8,
  dK_t = ds_t q / 8,  dV_t = p_t dO
at token counts on both sides of 64 and 128 and head counts that leave the
four-wave head stride on a partial round.  The backward runs once on the kernel's
own saved P (as the engine feeds it) and once on the reference P, so a forward
error cannot hide a backward one.  Every output buffer carries a sentinel tail.

artsbir_tokens_fwd / _bwd / _bwd_ex (csrc/elementwise.hip):
  tok[b][0] = mean_p h[b][p] + pos[0],  tok[b][1+p] = h[b][p] + pos[1+p]
  dh[b][p] = dtok[b][1+p] + dtok[b][0] / P
  dh[b][p] = dtok[b][1+p] + (dtok[b][0] + d0[b]) / P        (_ex)
The bars are tests/_tail.py's."""
import numpy as np
import pytest
import torch

from _tail import bf16_round, check, check_f32

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16]
DT_IDS = ["f32", "bf16"]
SENT = -768.0  # exact in bf16


# ------------------------------------------------------------------ references
def ref_fwd(q, kv, heads):
    """q [B][C], kv [B][T][2C] in one float type -> P [B][heads][T], O [B][C]"""
    B, C = q.shape
    T = kv.shape[1]
    k = kv[:, :, :C].reshape(B, T, heads, 64)
    v = kv[:, :, C:].reshape(B, T, heads, 64)
    s = np.einsum("bhd,bthd->bht", q.reshape(B, heads, 64), k) * q.dtype.type(0.125)
    p = np.exp(s - s.max(-1, keepdims=True))
    p = p / p.sum(-1, keepdims=True)
    o = np.einsum("bht,bthd->bhd", p, v).reshape(B, C)
    return p, o


def ref_bwd(q, kv, p, do, heads):
    """-> dQ [B][C], dKV [B][T][2C]"""
    B, C = q.shape
    T = kv.shape[1]
    k = kv[:, :, :C].reshape(B, T, heads, 64)
    v = kv[:, :, C:].reshape(B, T, heads, 64)
    qh, doh = q.reshape(B, heads, 64), do.reshape(B, heads, 64)
    eighth = q.dtype.type(0.125)
    dp = np.einsum("bhd,bthd->bht", doh, v)
    ds = p * (dp - (p * dp).sum(-1, keepdims=True))
    dq = (np.einsum("bht,bthd->bhd", ds, k) * eighth).reshape(B, C)
    dk = (np.einsum("bht,bhd->bthd", ds, qh) * eighth).reshape(B, T, C)
    dv = np.einsum("bht,bhd->bthd", p, doh).reshape(B, T, C)
    return dq, np.concatenate([dk, dv], -1)


def _dev(a, dev, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev).to(dtype).contiguous()


def _with_tail(n, tail, dtype, dev):
    """a flat buffer of n + tail elements, all SENT"""
    return torch.full((n + tail,), SENT, dtype=dtype, device=dev)


def _tail_intact(buf, n):
    return bool((buf[n:].float() == SENT).all().item())


def _run_fwd(q, kv, heads, dtype, dev):
    import _hip
    B, C = q.shape
    T = kv.shape[1]
    dq_, dkv_ = _dev(q, dev), _dev(kv, dev, dtype)
    P = _with_tail(B * heads * T, T, torch.float32, dev)
    O = _with_tail(B * C, C, dtype, dev)
    _hip.call("artsbir_attnpool_fwd", _hip.dtype_code(dtype), dq_.data_ptr(), dkv_.data_ptr(), B, C, heads, T,
              P.data_ptr(), O.data_ptr(), _hip.stream())
    torch.cuda.synchronize()
    assert _tail_intact(P, B * heads * T) and _tail_intact(O, B * C), "forward wrote past its outputs"
    return P[:B * heads * T].view(B, heads, T), O[:B * C].view(B, C)


def _run_bwd(q, kv, p_dev, do, heads, dtype, dev):
    import _hip
    B, C = q.shape
    T = kv.shape[1]
    dq_, dkv_, ddo = _dev(q, dev), _dev(kv, dev, dtype), _dev(do, dev)
    dQ = _with_tail(B * C, C, dtype, dev)
    dKV = _with_tail(B * T * 2 * C, 2 * C, dtype, dev)  # one sentinel token row
    _hip.call("artsbir_attnpool_bwd", _hip.dtype_code(dtype), dq_.data_ptr(), dkv_.data_ptr(), p_dev.data_ptr(),
              ddo.data_ptr(), B, C, heads, T, dQ.data_ptr(), dKV.data_ptr(), _hip.stream())
    torch.cuda.synchronize()
    assert _tail_intact(dQ, B * C) and _tail_intact(dKV, B * T * 2 * C), "backward wrote at t >= T"
    return dQ[:B * C].view(B, C), dKV[:B * T * 2 * C].view(B, T, 2 * C)


def _inputs(B, heads, T, dtype, qscale=1.0):
    C = 64 * heads
    rng = np.random.default_rng(B * 100003 + heads * 1009 + T)
    q = (rng.normal(0, qscale, (B, C))).astype(np.float32)
    kv = rng.normal(0, 1, (B, T, 2 * C)).astype(np.float32)
    do = rng.normal(0, 1, (B, C)).astype(np.float32)
    if dtype == torch.bfloat16:  # the kernel's bf16 operand; the reference sees the rounded values
        kv = bf16_round(kv)
    return q, kv, do


def _compare(tag, B, heads, T, dtype, dev, qscale=1.0):
    q, kv, do = _inputs(B, heads, T, dtype, qscale)
    q64, kv64, do64 = q.astype(np.float64), kv.astype(np.float64), do.astype(np.float64)
    P, O = _run_fwd(q, kv, heads, dtype, dev)
    p64, o64 = ref_fwd(q64, kv64, heads)
    p32, o32 = ref_fwd(q, kv, heads)
    check_f32(f"{tag} P", P, p64, p32)
    check(f"{tag} O", dtype, O, o64, o32)
    # softmax rows sum to one (the kernel's P summed in f64)
    check_f32(f"{tag} sum_t P", P.double().sum(-1), np.ones((B, heads)), p32.sum(-1, dtype=np.float32))
    # backward on the kernel's own saved P ...
    p_own = P.contiguous()
    dQ, dKV = _run_bwd(q, kv, p_own, do, heads, dtype, dev)
    pn = p_own.cpu().numpy()
    dq64, dkv64 = ref_bwd(q64, kv64, pn.astype(np.float64), do64, heads)
    dq32, dkv32 = ref_bwd(q, kv, pn, do, heads)
    check(f"{tag} dQ  (own P)", dtype, dQ, dq64, dq32)
    check(f"{tag} dKV (own P)", dtype, dKV, dkv64, dkv32)
    # ... and on the reference P (rounded to the f32 the kernel reads)
    pr = p64.astype(np.float32)
    dQ, dKV = _run_bwd(q, kv, _dev(pr, dev), do, heads, dtype, dev)
    dq64, dkv64 = ref_bwd(q64, kv64, pr.astype(np.float64), do64, heads)
    dq32, dkv32 = ref_bwd(q, kv, pr, do, heads)
    check(f"{tag} dQ  (ref P)", dtype, dQ, dq64, dq32)
    check(f"{tag} dKV (ref P)", dtype, dKV, dkv64, dkv32)
    return P, p64


CASES = [(1, 1, 1), (2, 1, 2), (3, 2, 63), (2, 3, 64), (2, 4, 65), (2, 5, 82), (1, 8, 127), (2, 8, 128), (3, 32, 50)]


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("B,heads,T", CASES)
def test_attnpool_core(B, heads, T, dtype, dev):
    _compare(f"attnpool B{B} h{heads} T{T}", B, heads, T, dtype, dev)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_attnpool_large_logits(dtype, dev):
    """q scaled so the scores span about +-60: without the max subtraction exp()
    overflows; with it the softmax is finite and close to one-hot"""
    B, heads, T = 2, 5, 82
    P, p64 = _compare(f"attnpool large-logit B{B} h{heads} T{T}", B, heads, T, dtype, dev, qscale=20.0)
    s_span = np.log(p64.max(-1)) - np.log(np.maximum(p64.min(-1), 1e-300))
    assert s_span.max() > 60.0, s_span.max()  # the case is what it says
    assert torch.isfinite(P).all()
    assert (P.max(-1).values.cpu().numpy() > 0.5 * p64.max(-1)).all()


# ---------------------------------------------------------------------- tokens
# (3, 2, 696): B*C/8 = 261 and B*P*C/8 = 522, one and two 256-thread blocks plus a ragged rest
TOKEN_CASES = [(1, 1, 8), (2, 4, 72), (3, 81, 512), (2, 121, 2048), (3, 2, 696)]


def _round_for(dtype, a):
    return bf16_round(a) if dtype == torch.bfloat16 else a


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("B,P,C", TOKEN_CASES)
def test_tokens_fwd(B, P, C, dtype, dev):
    import _hip
    rng = np.random.default_rng(B * 7919 + P * 31 + C)
    h = _round_for(dtype, rng.normal(0, 1, (B, P, C)).astype(np.float32))
    pos = rng.normal(0, 0.5, (P + 1, C)).astype(np.float32)
    dh_, dpos = _dev(h, dev, dtype), _dev(pos, dev)
    n = B * (P + 1) * C
    tok = _with_tail(n, C, dtype, dev)
    _hip.call("artsbir_tokens_fwd", _hip.dtype_code(dtype), dh_.data_ptr(), dpos.data_ptr(), B, P, C, tok.data_ptr(),
              _hip.stream())
    torch.cuda.synchronize()
    assert _tail_intact(tok, n)

    def ref(h, pos):
        out = np.empty((B, P + 1, C), h.dtype)
        out[:, 0] = h.sum(1, dtype=h.dtype) / h.dtype.type(P) + pos[0]
        out[:, 1:] = h + pos[1:]
        return out
    check(f"tokens_fwd B{B} P{P} C{C}", dtype, tok[:n].view(B, P + 1, C), ref(h.astype(np.float64), pos.astype(np.float64)),
          ref(h, pos))


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("B,P,C", TOKEN_CASES)
def test_tokens_bwd(B, P, C, dtype, dev):
    import _hip
    rng = np.random.default_rng(B * 7907 + P * 37 + C)
    dtok = rng.normal(0, 1, (B, P + 1, C)).astype(np.float32)  # f32 in, compute dtype out
    ddtok = _dev(dtok, dev)
    n = B * P * C
    dh = _with_tail(n, C, dtype, dev)
    _hip.call("artsbir_tokens_bwd", _hip.dtype_code(dtype), ddtok.data_ptr(), B, P, C, dh.data_ptr(), _hip.stream())
    torch.cuda.synchronize()
    assert _tail_intact(dh, n)

    def ref(d):
        return d[:, 1:] + d[:, :1] / d.dtype.type(P)
    check(f"tokens_bwd B{B} P{P} C{C}", dtype, dh[:n].view(B, P, C), ref(dtok.astype(np.float64)), ref(dtok))


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("B,P,C", TOKEN_CASES)
def test_tokens_bwd_ex(B, P, C, dtype, dev):
    """dtok in the compute dtype, d0 in f32.  d0 and dtok[:, 0] are large, of opposite
    sign and nearly cancel, so (dtok0 + d0) / P differs visibly from dtok0 / P + d0 / P
    or from a sum rounded to the compute dtype before the division"""
    import _hip
    rng = np.random.default_rng(B * 7901 + P * 41 + C)
    dtok = rng.normal(0, 1, (B, P + 1, C)).astype(np.float32)
    dtok[:, 0] *= 1024.0
    dtok = _round_for(dtype, dtok)
    d0 = (-dtok[:, 0] * (1.0 + 0.01 * rng.normal(0, 1, (B, C)))).astype(np.float32)
    ddtok, dd0 = _dev(dtok, dev, dtype), _dev(d0, dev)
    n = B * P * C
    dh = _with_tail(n, C, dtype, dev)
    _hip.call("artsbir_tokens_bwd_ex", _hip.dtype_code(dtype), ddtok.data_ptr(), dd0.data_ptr(), B, P, C, dh.data_ptr(),
              _hip.stream())
    torch.cuda.synchronize()
    assert _tail_intact(dh, n)

    def ref(d, e):
        return d[:, 1:] + ((d[:, 0] + e) / d.dtype.type(P))[:, None]
    check(f"tokens_bwd_ex B{B} P{P} C{C}", dtype, dh[:n].view(B, P, C), ref(dtok.astype(np.float64), d0.astype(np.float64)),
          ref(dtok, d0))
