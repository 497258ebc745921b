"""Direct float64 parity of the ViT row and elementwise kernels (csrc/vit.hip)
and of the fp8 quantiser's forms (csrc/fp8.hip), one dispatch form per case.

Every case calls the C entry point itself, so that its shape, dtype and pointer
alignment pin the kernel the launcher selects (the form is named in the
parametrisation id or the docstring; these entry points record no kernel name,
so artsbir_last_kernel() has nothing to assert).  The references are
oracle.encoder.layernorm_fp32 / quick_gelu and plain torch in float64, on the
same (for bf16: bf16-rounded) inputs.

Tolerances:
  f32 storage   relative L2 < 1e-5 and max |got - ref| <= 1e-5 max |ref|
                (the same formulas in f32 on the CPU sit at <= 1.6e-7 LayerNorm,
                7e-9 QuickGELU, 9e-7 its derivative in the max norm)
  bf16 storage  every element within one bf16 ulp: |got - ref| <= 2^-7 |ref| + 1e-5
                (the f32 formula rounded to bf16 uses <= 0.50 of that)
  f32 column sums  relative L2 < 1e-4; over at most 8 terms the derived bound
                terms * 2^-24 * sum |terms|
  copies and single f32 adds  bit for bit

A misaligned operand is buf[1:] of a flat buffer with one extra element: the
natural 4- / 2-byte alignment stays, the 16-byte alignment (the vector forms'
condition) does not."""
import functools

import pytest
import torch

from oracle import encoder as oenc

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
DTYPES = [pytest.param(F32, id="f32"), pytest.param(BF16, id="bf16")]
EPS = 1e-5
SENT = -7.0  # sentinel: exact in f32 and bf16, no kernel output here equals it over a whole tail


def _code(dtype):
    import _hip
    return _hip.DT_BF16 if dtype == BF16 else _hip.DT_F32


def _mis(t):
    """a copy of t (on its device) whose storage starts one element past a 16-B boundary"""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == t.element_size()
    return v


def _sentinel(n, pad, dtype, dev, mis=False):
    """(flat buffer of n + pad sentinels, optionally misaligned)"""
    buf = torch.full((n + pad + 1,), SENT, dtype=dtype, device=dev)
    out = buf[1:] if mis else buf[:-1]
    assert (out.data_ptr() % 16 != 0) == mis
    return out


def _tail_untouched(buf, n):
    return bool((buf[n:] == SENT).all())


def _bits(t):
    return t.contiguous().view({4: torch.int32, 2: torch.int16, 1: torch.uint8}[t.element_size()])


def _biteq(a, b):
    a, b = a.cpu(), b.cpu()
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _check(got, ref, dtype, what):
    """the storage tolerance of dtype (module docstring); ref is float64"""
    got = got.detach().double().cpu().reshape(ref.shape)
    assert torch.isfinite(got).all(), what
    diff = (got - ref).abs()
    if dtype == F32:
        l2 = (diff.norm() / ref.norm()).item()
        mx = diff.max().item() / ref.abs().max().item()
        print(what, "f32 rel-L2 %.3g max-norm %.3g" % (l2, mx))
        assert l2 < 1e-5, (what, "rel-L2", l2)
        assert mx <= 1e-5, (what, "max-norm", mx)
    else:
        bound = 2.0 ** -7 * ref.abs() + 1e-5
        worst = (diff / bound).max().item()
        print(what, "bf16 worst |got - ref| / bound %.3g" % worst)
        assert worst <= 1.0, (what, "bf16 ulp bound used", worst, int((diff > bound).sum()))


def _check_sum(got, ref, what, tol=1e-4):
    """an f32 column sum (ACCUMULATED onto initial contents that ref includes),
    relative to the reference's norm"""
    e = ((got.detach().double().cpu() - ref).norm() / ref.norm()).item()
    print(what, "sum rel-L2 %.3g" % e)
    assert e < tol, (what, e)


def _rand(g, *shape, dtype=F32, scale=1.0):
    """CPU values already rounded to dtype, as float32"""
    return (torch.randn(*shape, generator=g) * scale).to(dtype).float()


# --------------------------------------------------------------- LayerNorm forward
@functools.lru_cache(maxsize=None)
def _ln_fwd_case(dtype, rows, C, small_head=0):
    """inputs (rounded to dtype) and the float64 LayerNorm; small_head: that many
    leading rows scaled by 1e-4 (their variance falls below eps, their outputs
    shrink towards beta)"""
    g = torch.Generator().manual_seed(100003 * C + 17 * rows + (dtype == BF16))
    x = torch.randn(rows, C, generator=g) + 0.5 * torch.randn(rows, 1, generator=g)
    if small_head:
        x[:small_head] *= 1e-4
    x = x.to(dtype).float()
    gam = 1 + 0.1 * torch.randn(C, generator=g)
    bet = 0.1 * torch.randn(C, generator=g)
    ref = oenc.layernorm_fp32(x.double(), gam.double(), bet.double(), EPS)
    return x, gam, bet, ref


LN_FWD = [
    # (C, row counts, misaligned operand, form)
    (8, (1, 5), None, "v1-one-lane"), (264, (1, 5), None, "v1-partial"), (512, (1, 5), None, "v1-full-chunk"),
    (520, (1, 5), None, "v2-one-lane"), (768, (1, 5, 37), None, "v2-half-chunk"), (1024, (1, 5), None, "v2-full-chunk"),
    (100, (1, 5), None, "scalar-C%8"), (1001, (1, 5), None, "scalar-C%8"), (1280, (1, 5), None, "scalar-C>1024"),
    (768, (1, 5), "x", "scalar-misaligned-x"), (768, (1, 5), "gamma", "scalar-misaligned-gamma"),
]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C,rowset,mis,form", LN_FWD, ids=[f"C{c[0]}-{c[3]}" for c in LN_FWD])
def test_layernorm_fwd_forms(C, rowset, mis, form, dtype, dev):
    """artsbir_layernorm_fwd: layernorm_v_kernel<T, 1> (C <= 512) and <T, 2> with a
    full, partial or single-lane last chunk, layernorm_kernel<T> for C % 8 != 0,
    C > 1024 or a misaligned x / gamma; rows not a multiple of the 4 per block;
    rows past `rows` of the output stay untouched"""
    import _hip
    for rows in rowset:
        x, gam, bet, ref = _ln_fwd_case(dtype, rows, C)
        X, G, B = x.to(dev, dtype), gam.to(dev), bet.to(dev)
        if mis == "x":
            X = _mis(X)
        if mis == "gamma":
            G = _mis(G)
        y = _sentinel(rows * C, 3 * C, dtype, dev)
        _hip.call("artsbir_layernorm_fwd", _code(dtype), X.data_ptr(), G.data_ptr(), B.data_ptr(), rows, C, EPS,
                  y.data_ptr(), _hip.stream())
        _check(y[:rows * C], ref, dtype, f"layernorm_fwd {form} rows={rows} C={C}")
        assert _tail_untouched(y, rows * C), (rows, C)


def _slot_maxima(y, rows):
    """what vt_block_amax leaves: max |y| per block of 4 rows, folded into slot block & 4095"""
    rm = y.float().abs().amax(1).cpu()
    blocks = (rows + 3) // 4
    rm = torch.cat([rm, torch.zeros(4 * blocks - rows)]).view(blocks, 4).amax(1)
    slots = torch.zeros(4096)
    slots.scatter_reduce_(0, torch.arange(blocks) & 4095, rm, "amax")
    return slots


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rows,C,form", [(5, 768, "early-return-waves"), (37, 512, "v1"),
                                         (4 * 4096 + 5, 8, "slot-wrap")], ids=lambda v: str(v))
def test_layernorm_fwd_pmax(rows, C, form, dtype, dev):
    """artsbir_layernorm_fwd_pmax: y bit-equal to the plain call; every one of the
    4096 slots holds, as float bits, max |stored y| of the blocks folded into it, so
    their maximum is y.abs().max() exactly.  rows = 5: three waves of the second
    block return early through the barrier.  rows = 4 * 4096 + 5: blocks 4096 and
    4097 wrap into slots 0 and 1, and the first 4 * 4096 rows are scaled down so that
    the tensor's maximum lies in them"""
    import _hip
    wrap = rows > 4 * 4096
    x, gam, bet, ref = _ln_fwd_case(dtype, rows, C, 4 * 4096 if wrap else 0)
    X, G, B = x.to(dev, dtype), gam.to(dev), bet.to(dev)
    y0 = torch.empty_like(X)
    _hip.call("artsbir_layernorm_fwd", _code(dtype), X.data_ptr(), G.data_ptr(), B.data_ptr(), rows, C, EPS,
              y0.data_ptr(), _hip.stream())
    y = torch.empty_like(X)
    pm = torch.zeros(4096, dtype=torch.int32, device=dev)
    _hip.call("artsbir_layernorm_fwd_pmax", _code(dtype), X.data_ptr(), G.data_ptr(), B.data_ptr(), rows, C, EPS,
              y.data_ptr(), pm.data_ptr(), _hip.stream())
    assert _biteq(y, y0)
    _check(y, ref, dtype, f"layernorm_fwd_pmax {form}")
    got = pm.view(torch.float32).cpu()
    assert got.max().item() == y.float().abs().max().item()
    assert torch.equal(got, _slot_maxima(y, rows))
    if wrap:
        assert int(y.float().abs().amax(1).argmax()) >= 4 * 4096  # the maximum came through a wrapped block


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C,mis", [(100, False), (1280, False), (768, True)],
                         ids=["C100", "C1280", "misaligned-x"])
def test_layernorm_fwd_pmax_rejects_scalar_forms(C, mis, dtype, dev):
    """the fused amax exists in the vector kernel only: a shape or pointer that
    needs layernorm_kernel is an error, and nothing is written"""
    import _hip
    rows = 5
    x, gam, bet, _ = _ln_fwd_case(dtype, rows, C)
    X, G, B = x.to(dev, dtype), gam.to(dev), bet.to(dev)
    if mis:
        X = _mis(X)
    y = _sentinel(rows * C, 0, dtype, dev)
    pm = torch.zeros(4096, dtype=torch.int32, device=dev)
    with pytest.raises(_hip.HipError):
        _hip.call("artsbir_layernorm_fwd_pmax", _code(dtype), X.data_ptr(), G.data_ptr(), B.data_ptr(), rows, C, EPS,
                  y.data_ptr(), pm.data_ptr(), _hip.stream())
    torch.cuda.synchronize()
    assert _tail_untouched(y, 0) and int(pm.abs().max()) == 0


# -------------------------------------------------------------- LayerNorm backward
@functools.lru_cache(maxsize=None)
def _ln_bwd_case(dtype, rows, C):
    """inputs (rounded to dtype) and float64 autograd of layernorm_fp32:
    dx without the residual, dgamma, dbeta"""
    g = torch.Generator().manual_seed(200003 * C + 31 * rows + (dtype == BF16))
    x = (torch.randn(rows, C, generator=g) + 0.5 * torch.randn(rows, 1, generator=g)).to(dtype).float()
    gam = 1 + 0.1 * torch.randn(C, generator=g)
    dy = _rand(g, rows, C, dtype=dtype)
    res = _rand(g, rows, C, dtype=dtype)
    init = torch.randn(4, C, generator=g)  # non-zero contents of dgamma, dbeta, dres_sum, dx_sum
    xr = x.double().requires_grad_(True)
    gr = gam.double().requires_grad_(True)
    br = torch.zeros(C, dtype=torch.float64, requires_grad=True)
    (oenc.layernorm_fp32(xr, gr, br, EPS) * dy.double()).sum().backward()
    return x, gam, dy, res, init, xr.grad, gr.grad, br.grad


def _ln_bwd_run(dev, dtype, rows, C, with_res, sums, mis_x=False, alias=False):
    """one call of artsbir_layernorm_bwd(_sums) checked against float64: dx in the
    storage tolerance, dgamma / dbeta (/ dres_sum / dx_sum) = initial + gradient"""
    import _hip
    x, gam, dy, res, init, dx_ref, dg_ref, db_ref = _ln_bwd_case(dtype, rows, C)
    want_dx = dx_ref + res.double() if with_res else dx_ref
    X, Dy, G = x.to(dev, dtype), dy.to(dev, dtype), gam.to(dev)
    if mis_x:
        X = _mis(X)
    Rs = res.to(dev, dtype).clone() if with_res else None  # dx may be written here
    dx = Rs if alias else _sentinel(rows * C, C, dtype, dev)
    acc = init.to(dev).clone()
    dg, db, rsum, xsum = acc[0], acc[1], acc[2], acc[3]
    what = f"layernorm_bwd {dtype} rows={rows} C={C} res={with_res} sums={sums} mis={mis_x} alias={alias}"
    if sums:
        _hip.call("artsbir_layernorm_bwd_sums", _code(dtype), X.data_ptr(), G.data_ptr(), Dy.data_ptr(), rows, C, EPS,
                  _hip.ptr(Rs), dx.data_ptr(), dg.data_ptr(), db.data_ptr(), rsum.data_ptr() if with_res else None,
                  xsum.data_ptr(), _hip.stream())
    else:
        _hip.call("artsbir_layernorm_bwd", _code(dtype), X.data_ptr(), G.data_ptr(), Dy.data_ptr(), rows, C, EPS,
                  _hip.ptr(Rs), dx.data_ptr(), dg.data_ptr(), db.data_ptr(), _hip.stream())
    _check(dx.reshape(-1)[:rows * C], want_dx, dtype, what + " dx")
    if not alias:
        assert _tail_untouched(dx, rows * C), what
    i64 = init.double()

    def acc_check(got, k, grad, name):
        # initial + gradient, the error measured against the gradient alone
        e = ((got.double().cpu() - i64[k] - grad).norm() / grad.norm()).item()
        print(what, name, "rel-L2 %.3g" % e)
        assert e < 1e-4, (what, name, e)
    acc_check(dg, 0, dg_ref, "dgamma")
    acc_check(db, 1, db_ref, "dbeta")
    if sums:
        if with_res:
            acc_check(rsum, 2, res.double().sum(0), "dres_sum")
        else:
            assert torch.equal(rsum.cpu(), init[2])
        acc_check(xsum, 3, want_dx.sum(0), "dx_sum")  # the f32 values, before dx's rounding to its storage
    else:
        assert torch.equal(acc[2:].cpu(), init[2:])


LN_BWD_SCALAR = [(3, 100, 2), (37, 100, 2), (8200, 100, 2), (3, 250, 4), (37, 250, 4), (3, 500, 8), (37, 500, 8),
                 (3, 700, 12), (37, 700, 12), (3, 1001, 16), (37, 1001, 16)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rows,C,cpl", LN_BWD_SCALAR, ids=[f"rows{r}-C{c}-CPL{k}" for r, c, k in LN_BWD_SCALAR])
def test_layernorm_bwd_scalar_form(rows, C, cpl, dtype, dev):
    """layernorm_bwd_kernel<T, CPL> (C % 8 != 0), CPL = 2, 4, 8, 12, 16, with and
    without dres; rows = 8200: more than the 2048-block cap covers, so waves stride"""
    assert (C + 63) // 64 <= cpl and C % 8
    for with_res in (True, False):
        _ln_bwd_run(dev, dtype, rows, C, with_res, False)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rows", [3, 37])
def test_layernorm_bwd_scalar_form_misaligned_x(rows, dtype, dev):
    """C = 768 with a misaligned x: layernorm_bwd_kernel<T, 12> on a vector shape"""
    for with_res in (True, False):
        _ln_bwd_run(dev, dtype, rows, 768, with_res, False, mis_x=True)


LN_BWD_V = ([(F32, c) for c in (8, 264, 512, 520, 1024)] + [(BF16, c) for c in (264, 520)])


@pytest.mark.parametrize("rows", [1, 37, 2100])
@pytest.mark.parametrize("dtype,C", LN_BWD_V, ids=[f"{'f32' if d == F32 else 'bf16'}-C{c}-NCH{1 if c <= 512 else 2}"
                                                    for d, c in LN_BWD_V])
def test_layernorm_bwd_8col_form(dtype, C, rows, dev):
    """layernorm_bwd_v_kernel<T, NCH, SUMS>: NCH = 1 (C <= 512) and 2, f32 and bf16,
    with the column sums and without, with dres and with dres == NULL; rows = 2100:
    past the 512-block cap, waves stride and prefetch their next row"""
    for with_res in (True, False):
        for sums in (False, True):
            _ln_bwd_run(dev, dtype, rows, C, with_res, sums)


LN_BWD_C4 = [(1, 256), (5, 256), (4101, 256), (1, 512), (5, 512), (1, 768), (5, 768), (1, 1024), (5, 1024)]


@pytest.mark.parametrize("rows,C", LN_BWD_C4, ids=[f"rows{r}-NC{c // 256}" for r, c in LN_BWD_C4])
def test_layernorm_bwd_4col_form(rows, C, dev):
    """layernorm_bwd_c4_kernel<NC, SUMS, 2> (bf16, C = 256 NC), with and without
    dres and the sums; rows = 4101 at 512 blocks of 4 waves: waves 0-4 walk three
    rows, the whole cur <- n1 <- n2 rotation"""
    for with_res in (True, False):
        for sums in (False, True):
            _ln_bwd_run(dev, BF16, rows, C, with_res, sums)


@pytest.mark.parametrize("dtype,C,sums,form", [(F32, 700, False, "scalar"), (F32, 520, True, "8col"),
                                               (BF16, 768, True, "4col")], ids=["scalar", "8col", "4col"])
def test_layernorm_bwd_dx_may_alias_dres(dtype, C, sums, form, dev):
    """include/artsbir.h: dx may alias dres"""
    _ln_bwd_run(dev, dtype, 37, C, True, sums, alias=True)


@pytest.mark.parametrize("dtype", DTYPES)
def test_layernorm_bwd_rejects(dtype, dev):
    """C > 1024; the column sums on a scalar-form shape; dres_sum without dres —
    each an error that writes nothing"""
    import _hip
    st = _hip.stream()
    rows = 3
    for C, sums, with_res in [(1032, False, True), (100, True, True), (264, True, False)]:
        X = torch.randn(rows, C, device=dev).to(dtype)
        Dy, Rs = torch.randn_like(X), torch.randn_like(X)
        G = torch.ones(C, device=dev)
        dx = _sentinel(rows * C, 0, dtype, dev)
        acc = torch.full((4, C), SENT, device=dev)
        with pytest.raises(_hip.HipError):
            if sums:
                _hip.call("artsbir_layernorm_bwd_sums", _code(dtype), X.data_ptr(), G.data_ptr(), Dy.data_ptr(), rows,
                          C, EPS, Rs.data_ptr() if with_res else None, dx.data_ptr(), acc[0].data_ptr(),
                          acc[1].data_ptr(), acc[2].data_ptr(), acc[3].data_ptr(), st)
            else:
                _hip.call("artsbir_layernorm_bwd", _code(dtype), X.data_ptr(), G.data_ptr(), Dy.data_ptr(), rows, C,
                          EPS, Rs.data_ptr(), dx.data_ptr(), acc[0].data_ptr(), acc[1].data_ptr(), st)
        torch.cuda.synchronize()
        assert _tail_untouched(dx, 0) and bool((acc == SENT).all()), (C, sums, with_res)


# ----------------------------------------------------------------------- QuickGELU
FIXED = [-100.0, -60.0, -20.0, -1e-30, 0.0, 1e-30, 20.0, 60.0, 100.0]


@functools.lru_cache(maxsize=None)
def _gelu_case(dtype, n):
    """x = 3 randn with the fixed values from element 1 on, as many as fit (element
    0 stays random: quickgelu(-100) is 1e-72, no scale for a relative error), and,
    where they fit twice, at the tail, which the n % 8 remainder loop handles; dy;
    float64 y, dx; `body` marks the random entries"""
    g = torch.Generator().manual_seed(300007 + 2 * n + (dtype == BF16))
    x = 3 * torch.randn(n, generator=g)
    body = torch.ones(n, dtype=torch.bool)
    k = min(n - 1, len(FIXED))
    x[1:1 + k] = torch.tensor(FIXED[:k])
    body[1:1 + k] = False
    if n >= 2 * len(FIXED):
        x[-len(FIXED):] = torch.tensor(FIXED)
        body[-len(FIXED):] = False
    x = x.to(dtype).float()
    dy = _rand(g, n, dtype=dtype)
    xr = x.double().requires_grad_(True)
    y = oenc.quick_gelu(xr)
    (y * dy.double()).sum().backward()
    return x, dy, y.detach(), xr.grad, body


def _check_gelu(got, ref, body, dtype, what):
    """the storage tolerance over everything, and again over the random entries
    alone: next to |x| = 100 the max-norm and L2 scales would hide an error of
    1e-3 in an ordinary element"""
    _check(got, ref, dtype, what)
    if body.any():
        _check(got.detach().cpu()[body], ref[body], dtype, what + " (random entries)")


GELU_N = [1, 7, 8, 1000, 1003, 8 * 256 * 3 + 5]
GELU = [(n, None) for n in GELU_N] + [(1003, "x"), (1003, "out")]


def _gelu_id(c):
    n, mis = c
    form = "scalar-only" if n < 8 or mis else "vec" if n % 8 == 0 else "vec+tail"
    return f"n{n}-{form}" + (f"-misaligned-{mis}" if mis else "")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,mis", GELU, ids=[_gelu_id(c) for c in GELU])
def test_quickgelu_fwd_bwd_forms(n, mis, dtype, dev):
    """artsbir_quickgelu and artsbir_quickgelu_bwd: the 8-wide loop, its n % 8 tail,
    n < 8, and n8 = 0 for a misaligned input or output; saturating inputs give finite
    outputs; nothing past n is written.  n = 8 * 256 * 3 + 5: three blocks and a tail"""
    import _hip
    st = _hip.stream()
    x, dy, y_ref, dx_ref, body = _gelu_case(dtype, n)
    X, Dy = x.to(dev, dtype), dy.to(dev, dtype)
    if mis == "x":
        X = _mis(X)
    y = _sentinel(n, 16, dtype, dev, mis == "out")
    _hip.call("artsbir_quickgelu", _code(dtype), X.data_ptr(), n, y.data_ptr(), st)
    _check_gelu(y[:n], y_ref, body, dtype, f"quickgelu n={n} mis={mis}")
    assert _tail_untouched(y, n)
    dx = _sentinel(n, 16, dtype, dev, mis == "out")
    _hip.call("artsbir_quickgelu_bwd", _code(dtype), X.data_ptr(), Dy.data_ptr(), n, dx.data_ptr(), st)
    _check_gelu(dx[:n], dx_ref, body, dtype, f"quickgelu_bwd n={n} mis={mis}")
    assert _tail_untouched(dx, n)


GELU_SUM = [(1, 8, "one-thread"), (3, 1032, "second-column-block-one-thread"), (7, 3072, "4-rows+tail-gridy7"),
            (4099, 8, "gridy1024-one-trip+tail"), (4 * 341 + 7, 3072, "gridy341-one-trip+tail")]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rows,C,form", GELU_SUM, ids=[f"{r}x{c}-{f}" for r, c, f in GELU_SUM])
def test_quickgelu_bwd_sum(rows, C, form, dtype, dev):
    """artsbir_quickgelu_bwd_sum: dx bit-equal to artsbir_quickgelu_bwd on the same
    operands (the same arithmetic) and within the storage tolerance of float64;
    dsum = its non-zero initial contents + the column sums of the f32 dx"""
    import _hip
    st = _hip.stream()
    n = rows * C
    x, dy, _, dx_ref, body = _gelu_case(dtype, n)
    X, Dy = x.to(dev, dtype), dy.to(dev, dtype)
    dx0 = torch.empty_like(X)
    _hip.call("artsbir_quickgelu_bwd", _code(dtype), X.data_ptr(), Dy.data_ptr(), n, dx0.data_ptr(), st)
    dx = _sentinel(n, C, dtype, dev)
    init = torch.randn(C, generator=torch.Generator().manual_seed(rows + C))
    dsum = init.to(dev).clone()
    _hip.call("artsbir_quickgelu_bwd_sum", _code(dtype), X.data_ptr(), Dy.data_ptr(), rows, C, dx.data_ptr(),
              dsum.data_ptr(), st)
    assert _biteq(dx[:n], dx0)
    assert _tail_untouched(dx, n)
    _check_gelu(dx[:n], dx_ref, body, dtype, f"quickgelu_bwd_sum {rows}x{C} dx")
    _check_sum(dsum, init.double() + dx_ref.view(rows, C).sum(0), f"quickgelu_bwd_sum {rows}x{C} dsum")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("why", ["C100", "no-dsum", "misaligned-x"])
def test_quickgelu_bwd_sum_rejects(why, dtype, dev):
    import _hip
    rows, C = 3, 100 if why == "C100" else 104
    X = torch.randn(rows * C, device=dev).to(dtype)
    Dy = torch.randn_like(X)
    if why == "misaligned-x":
        X = _mis(X)
    dx = _sentinel(rows * C, 0, dtype, dev)
    dsum = torch.full((C,), SENT, device=dev)
    with pytest.raises(_hip.HipError):
        _hip.call("artsbir_quickgelu_bwd_sum", _code(dtype), X.data_ptr(), Dy.data_ptr(), rows, C, dx.data_ptr(),
                  None if why == "no-dsum" else dsum.data_ptr(), _hip.stream())
    torch.cuda.synchronize()
    assert _tail_untouched(dx, 0) and bool((dsum == SENT).all())


# ------------------------------------------------------------ patch and token kernels
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,R,patch", [(2, 64, 16), (3, 28, 14), (1, 32, 32), (2, 96, 32), (2, 6, 1)],
                         ids=lambda v: str(v))
def test_vit_patchify_bit_for_bit(B, R, patch, dtype, dev):
    """artsbir_vit_patchify = unfold / permute / reshape of the image (a copy; for
    bf16 torch's cast of it), patch 16, 14, 32 and 1"""
    import _hip
    img = torch.randn(B, 3, R, R, generator=torch.Generator().manual_seed(B * 1000 + R + patch))
    P, K = (R // patch) ** 2, 3 * patch * patch
    ref = img.unfold(2, patch, patch).unfold(3, patch, patch).permute(0, 2, 3, 1, 4, 5).reshape(B * P, K).to(dtype)
    out = _sentinel(B * P * K, 64, dtype, dev)
    Img = img.to(dev)
    _hip.call("artsbir_vit_patchify", _code(dtype), Img.data_ptr(), B, R, patch, out.data_ptr(), _hip.stream())
    assert _biteq(out[:B * P * K].view(B * P, K), ref)
    assert _tail_untouched(out, B * P * K)


def test_vit_patchify_rejects_ragged_resolution(dev):
    import _hip
    img = torch.randn(1, 3, 30, 30, device=dev)
    out = _sentinel(3 * 30 * 30, 0, F32, dev)
    with pytest.raises(_hip.HipError):
        _hip.call("artsbir_vit_patchify", _hip.DT_F32, img.data_ptr(), 1, 30, 16, out.data_ptr(), _hip.stream())
    torch.cuda.synchronize()
    assert _tail_untouched(out, 0)


TOKENS = [(1, 1, 8), (3, 4, 100), (2, 49, 768)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,P,E", TOKENS, ids=lambda v: str(v))
def test_vit_tokens_bit_for_bit(B, P, E, dtype, dev):
    """artsbir_vit_tokens: class embedding / patch rows, sequence-first, plus the
    positional embedding: one f32 add per element, then the cast"""
    import _hip
    g = torch.Generator().manual_seed(B * 100 + P * 10 + E)
    patches = torch.randn(B * P, E, generator=g).to(dtype)
    cls, pos = torch.randn(E, generator=g), torch.randn(P + 1, E, generator=g)
    ref = (torch.cat([cls.expand(1, B, E), patches.float().view(B, P, E).transpose(0, 1)]) + pos[:, None]).to(dtype)
    n = (P + 1) * B * E
    out = _sentinel(n, 64, dtype, dev)
    Pt, Cl, Po = patches.to(dev), cls.to(dev), pos.to(dev)
    _hip.call("artsbir_vit_tokens", _code(dtype), Pt.data_ptr(), Cl.data_ptr(), Po.data_ptr(), B, P, E, out.data_ptr(),
              _hip.stream())
    assert _biteq(out[:n].view(P + 1, B, E), ref)
    assert _tail_untouched(out, n)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,P,E", TOKENS, ids=lambda v: str(v))
def test_vit_tokens_bwd(B, P, E, dtype, dev):
    """artsbir_vit_tokens_bwd: dpatches = the transposed dtok[1:] bit for bit; dpos
    and dcls ACCUMULATED onto non-zero contents: initial + sum_b dtok within
    B 2^-24 sum_b |dtok| per element (B f32 additions, each rounding a partial sum
    of at most sum_b |dtok| + |initial|; the initial contents are kept two orders
    below the gradients, inside the last addition's share); dcls takes token 0
    only; a second call on the same inputs gives the same bits (fixed order)"""
    import _hip
    g = torch.Generator().manual_seed(B * 100 + P * 10 + E + 1)
    dtok = torch.randn(P + 1, B, E, generator=g).to(dtype)
    init_pos, init_cls = 0.01 * torch.randn(P + 1, E, generator=g), 0.01 * torch.randn(E, generator=g)
    D = dtok.to(dev)
    outs = []
    for _ in range(2):
        dpat = _sentinel(B * P * E, 64, dtype, dev)
        dpos, dcls = init_pos.to(dev).clone(), init_cls.to(dev).clone()
        _hip.call("artsbir_vit_tokens_bwd", _code(dtype), D.data_ptr(), B, P, E, dpat.data_ptr(), dcls.data_ptr(),
                  dpos.data_ptr(), _hip.stream())
        outs.append((dpat.cpu(), dpos.cpu(), dcls.cpu()))
    dpat, dpos, dcls = outs[0]
    assert _biteq(dpat[:B * P * E].view(B, P, E), dtok[1:].transpose(0, 1).contiguous())
    assert _tail_untouched(dpat, B * P * E)
    s, sa = dtok.double().sum(1), dtok.double().abs().sum(1)
    bound = B * 2.0 ** -24 * sa
    assert ((dpos.double() - (init_pos.double() + s)).abs() <= bound).all()
    assert ((dcls.double() - (init_cls.double() + s[0])).abs() <= bound[0]).all()
    for a, b in zip(outs[0], outs[1]):
        assert _biteq(a, b)


# -------------------------------------------------------------------- fp8 quantiser
def _fp8_ref(x):
    """torch's RNE e4m3fn cast of the IEEE f32 quotient x / (amax / 448), and the scale"""
    xf = x.float().cpu()
    amax = xf.abs().max()
    s = amax / 448.0 if amax > 0 else torch.tensor(1.0)
    return (xf / s).to(torch.float8_e4m3fn).view(torch.uint8), s


def _fp8_check(x, pmax=None):
    import vit
    q, s = vit._fp8(x, pmax)
    want, ws = _fp8_ref(x)
    bad = int((q.cpu() != want).sum())
    assert bad == 0, (bad, x.numel())
    assert s.item() == ws.item(), (s.item(), ws.item())
    return q, s


FP8_BIG = 8 * (3 * 524288 + 1000) + 5


@pytest.mark.parametrize("dtype,n,mis", [(BF16, FP8_BIG, False), (F32, 1, False), (BF16, 1, False), (F32, 7, False),
                                         (BF16, 7, False), (F32, 1003, False), (BF16, 1003, False),
                                         (F32, 1003, True), (BF16, 1003, True)],
                         ids=["bf16-main-loop-12590917", "f32-n1", "bf16-n1", "f32-n7", "bf16-n7", "f32-n1003",
                              "bf16-n1003", "f32-n1003-misaligned", "bf16-n1003-misaligned"])
def test_fp8_quantiser_forms(dtype, n, mis, dev):
    """artsbir_quantize_fp8 code for code against torch's float8_e4m3fn cast.
    n = 12 590 917 (bf16, 25 MB): 2048 blocks, threads 0-999 take one trip of four
    chunks in flight with the non-temporal store, every thread then up to three
    single chunks, five elements the scalar tail.  n < 8, n % 8 != 0, and n8 = 0 for
    a misaligned x"""
    g = torch.Generator().manual_seed(n + (dtype == BF16))
    x = (torch.randn(n, generator=g) * (0.05 + torch.rand(n, generator=g))).to(dtype).to(dev)
    if mis:
        x = _mis(x)
    _fp8_check(x)


@pytest.mark.parametrize("dtype", DTYPES)
def test_fp8_quantiser_all_zero(dtype, dev):
    """an all-zero tensor: scale exactly 1 (not 0 / 0), codes 0x00, and 0x80 for -0.0"""
    import vit
    x = torch.zeros(1003, dtype=dtype)
    x[5] = -0.0
    x[1001] = -0.0
    q, s = vit._fp8(x.to(dev))
    want = torch.zeros(1003, dtype=torch.uint8)
    want[5] = want[1001] = 0x80
    assert torch.equal(q.cpu(), want)
    assert s.item() == 1.0


@pytest.mark.parametrize("dtype", DTYPES)
def test_fp8_quantiser_pmax_last_slot(dtype, dev):
    """artsbir_quantize_fp8_pmax with hand-filled partial maxima whose maximum sits in
    slot 4095: the codes and scale of the plain call"""
    import vit
    g = torch.Generator().manual_seed(4095)
    x = torch.randn(37, 264, generator=g).to(dtype).to(dev)
    amax = x.float().abs().max().cpu()
    part = torch.rand(4096, generator=g) * amax * 0.99
    part[4095] = amax
    pm = part.view(torch.int32).to(dev)
    q1, s1 = _fp8_check(x, pm)
    q0, s0 = _fp8_check(x)
    assert torch.equal(q0, q1) and torch.equal(s0, s1)


# ------------------------------------------------------- f32 attention, lane boundaries
@pytest.mark.parametrize("L,N,heads,masked", [(64, 2, 1, False), (65, 1, 2, True), (128, 1, 1, False),
                                              (129, 2, 2, True), (256, 1, 1, True), (1, 2, 3, False)],
                         ids=lambda v: str(v))
def test_f32_attention_lane_boundaries(L, N, heads, masked, dev):
    """mha_fwd_kernel, mha_bwd_q_kernel, mha_bwd_kv_kernel (DT_F32: lane l owns keys
    l, l + 64, l + 128, l + 192) at L = 64, 65, 128, 129, 256 and 1 against float64
    autograd; the mask is causal -inf plus finite noise"""
    import _hip
    g = torch.Generator().manual_seed(2000 + L)
    st = _hip.stream()
    E = 64 * heads
    qkv = torch.randn(L * N, 3 * E, generator=g)
    dO = torch.randn(L * N, E, generator=g)
    mask = None
    if masked:
        mask = torch.full((L, L), float("-inf")).triu(1) + 0.5 * torch.randn(L, L, generator=g)
    qr = qkv.double().requires_grad_(True)
    q, k, vv = qr.view(L, N, 3 * E).split(E, dim=-1)

    def hd(t):
        return t.reshape(L, N, heads, 64).permute(1, 2, 0, 3)
    s = (hd(q) / 8.0) @ hd(k).transpose(-1, -2)
    if mask is not None:
        s = s + mask.double()
    lse_ref = torch.logsumexp(s, dim=-1)  # [N, heads, L]
    o = (torch.softmax(s, dim=-1) @ hd(vv)).permute(2, 0, 1, 3).reshape(L * N, E)
    (o * dO.double()).sum().backward()
    Q, DO = qkv.to(dev), dO.to(dev)
    M = mask.to(dev) if mask is not None else None
    out = _sentinel(L * N * E, 64, F32, dev)
    lse = _sentinel(L * N * heads, 16, F32, dev)
    _hip.call("artsbir_mha_fwd_lse", _hip.DT_F32, Q.data_ptr(), L, N, heads, _hip.ptr(M), out.data_ptr(),
              lse.data_ptr(), st)
    _check(out[:L * N * E], o.detach(), F32, f"mha_fwd L={L} out")
    assert _tail_untouched(out, L * N * E) and _tail_untouched(lse, L * N * heads)
    lse_got = lse[:L * N * heads].view(L, N, heads).permute(1, 2, 0).double().cpu()
    lse_err = (lse_got - lse_ref.detach()).abs().max().item()
    print("mha_fwd L=%d lse abs %.3g" % (L, lse_err))
    assert lse_err < 1e-5, lse_err
    dq = _sentinel(L * N * 3 * E, 64, F32, dev)
    dsc = torch.empty(L * N * heads, device=dev)
    _hip.call("artsbir_mha_bwd", _hip.DT_F32, Q.data_ptr(), out.data_ptr(), DO.data_ptr(), lse.data_ptr(), L, N,
              heads, _hip.ptr(M), dq.data_ptr(), dsc.data_ptr(), st)
    assert _tail_untouched(dq, L * N * 3 * E)
    got = dq[:L * N * 3 * E].view(L * N, 3 * E)
    for part, sl in (("dq", slice(0, E)), ("dk", slice(E, 2 * E)), ("dv", slice(2 * E, 3 * E))):
        ref = qr.grad[:, sl]
        if L == 1 and part != "dv":  # one key: p = 1, ds = dp - D = 0 up to the rounding of D = dO . O
            assert ref.abs().max().item() < 1e-12
            assert got[:, sl].abs().max().item() <= 1e-6, part
        else:
            _check(got[:, sl], ref, F32, f"mha_bwd L={L} {part}")


def test_attention_rejects_L257(dev):
    """L > 256 is an error from both entry points (four keys per lane), in f32 and bf16"""
    import _hip
    L, N, heads, E = 257, 1, 1, 64
    st = _hip.stream()
    for dtype in (F32, BF16):
        Q = torch.randn(L * N, 3 * E, device=dev).to(dtype)
        out = _sentinel(L * N * E, 0, dtype, dev)
        dq = _sentinel(L * N * 3 * E, 0, dtype, dev)
        lse = torch.zeros(L * N * heads, device=dev)
        dsc = torch.zeros(L * N * heads, device=dev)
        with pytest.raises(_hip.HipError):
            _hip.call("artsbir_mha_fwd_lse", _code(dtype), Q.data_ptr(), L, N, heads, None, out.data_ptr(),
                      lse.data_ptr(), st)
        with pytest.raises(_hip.HipError):
            _hip.call("artsbir_mha_bwd", _code(dtype), Q.data_ptr(), out.data_ptr(), out.data_ptr(), lse.data_ptr(),
                      L, N, heads, None, dq.data_ptr(), dsc.data_ptr(), st)
        torch.cuda.synchronize()
        assert _tail_untouched(out, 0) and _tail_untouched(dq, 0)
