"""Conditions on the INPUTS of test_regstaged_gpu.py, checked on the CPU.

Case claims: the launchers' arithmetic restated in Python (_regstaged_ref: decoder, the tile from Cout,
splits / m_per_split of launch_wgrad_tile, the store form from nv and ldy) says that every case reaches
the path its table row names, and that the tables together reach every decoder x dtype x tile, every
store form and both split conditions.

Reference: the float64 sums built from F.unfold agree with torch's own float64 conv2d / conv2d_input /
conv2d_weight (so the (r, s, ci) order of Xcol is the kernels' and torch's, not this file's invention).

Sensitivity: in every case, leaving out any single 16-byte chunk position of the reduction (one EPC
group of k of a convolution; one EPC-pixel unit of one tap, or one whole tap, of a weight gradient),
crediting it to the neighbouring filter tap, or (three segments) crediting its share of a segment's
sum to the neighbouring segment moves at least one checked output past 4 x its bar.  A case that
missed this would get different data, never a wider bar."""
import pytest

import _regstaged_ref as rr


def _ids(cases):
    return [c.id for c in cases]


# ---------------------------------------------------------------------------
# claims
def _kernel_C(case):
    return case.geo[4] if case.api == "dgrad" else case.geo[3]


def test_decoder_rows_reach_what_they_name():
    reached = set()
    for geo, dec32, dec16, tile in rr.DECODER_ROWS:
        C, Co = geo[3], geo[4]
        assert rr.decoder(C, "f32") == dec32, geo
        assert rr.decoder(C, "bf16") == dec16, geo
        assert (64 if Co <= 64 else 128) == tile, geo
        reached |= {("f32", dec32, tile), ("bf16", dec16, tile)}
    want = {(dt, d, t) for dt in ("f32", "bf16") for d in ("divides", "uniform", "generic") for t in (64, 128)}
    assert reached == want, want - reached
    # the issue's channel counts and their forms
    forms = {dt: {g[3]: rr.decoder(g[3], dt) for g, *_ in rr.DECODER_ROWS} for dt in ("f32", "bf16")}
    assert forms["f32"] == {8: "divides", 16: "divides", 32: "uniform", 96: "uniform", 64: "uniform",
                            24: "generic", 40: "generic", 48: "generic"}
    assert forms["bf16"] == {8: "divides", 16: "divides", 32: "divides", 64: "uniform",
                             24: "generic", 40: "generic", 48: "generic", 96: "generic"}


def test_filter_geometries_and_tiles_of_the_decoder_rows():
    geos = {g[5:] for g, *_ in rr.DECODER_ROWS}
    for want in [(3, 3, 1, 1), (3, 3, 2, 1), (1, 1, 2, 0), (5, 5, 1, 2), (1, 7, 1, 0), (3, 1, 1, 1), (4, 8, 1, 1)]:
        assert want in geos, want
    # R != S in every decoder of both dtypes
    for dt in ("f32", "bf16"):
        assert {rr.decoder(g[3], dt) for g, *_ in rr.DECODER_ROWS if g[5] != g[6]} == {"divides", "uniform", "generic"}
    ms, ks = [], []
    for g, *_ in rr.DECODER_ROWS:
        N, H, W, C, Co, R, S, st, pd = g
        Ho, Wo = (H + 2 * pd - R) // st + 1, (W + 2 * pd - S) // st + 1
        ms.append((N * Ho * Wo, Ho * Wo))
        ks.append(R * S * C)
        assert N * Ho * Wo * Co * R * S * C <= 5e7
    assert any(m < 128 for m, _ in ms)
    assert any(m > 128 and m % 128 and 128 % hw for m, hw in ms)   # tiles cross images, the last is partial
    assert any(k % 32 and k % 64 for k in ks) and 216 in ks
    assert max(g[5] * g[6] for g, *_ in rr.DECODER_ROWS) == 32     # bit 31 of rmask


def test_epilogue_shapes_and_store_forms():
    for name, shape in (("U", rr.SHAPE_U), ("G", rr.SHAPE_G)):
        assert (rr.decoder(shape[3], "f32"), rr.decoder(shape[3], "bf16")) == rr.SHAPE_DEC[name]
    reached = set()
    for opts, co, claim in rr.FWD_EPILOGUES:
        got = rr.store_paths(co, co + rr._extra(opts, "ld"), "f32out" in opts, "acc" in opts)
        assert got == claim, (opts, co, got)
        reached |= got
    assert reached == {"vec", "scalar-tail", "scalar-ld", "acc-vec", "acc-scalar-tail", "acc-scalar-ld"}
    couts = {c.geo[4] for c in rr.CONV_CASES if c.api == "fwd"}
    assert {5, 20, 64, 72, 136} <= couts
    # ldy = Cout + 8 and Cout + 3 through the convolution and through the dense entry point's ldc
    for api in ("fwd", "nt"):
        assert {o for c in rr.CONV_CASES if c.api == api for o in c.opts} >= {"ld+8", "ld+3"}
    # every epilogue on a uniform-tap and on a generic-decoder shape, in both dtypes
    for dt in ("f32", "bf16"):
        for api, rows in (("fwd", [r[0] for r in rr.FWD_EPILOGUES]), ("act", [r[0] for r in rr.ACT_EPILOGUES]),
                          ("seg", [("stats", "seg3")])):
            for opts in rows:
                decs = {rr.decoder(c.geo[3], dt) for c in rr.CONV_CASES if (c.api, c.dt, c.opts) == (api, dt, opts)}
                assert decs == {"uniform", "generic"}, (dt, api, opts, decs)


def test_dgrad_and_dense_rows():
    for dt in ("f32", "bf16"):
        dg = [c for c in rr.CONV_CASES if c.api == "dgrad" and c.dt == dt]
        assert {c.opts for c in dg} == {(), ("res1",), ("res2",)}
        assert {(c.geo[5], c.geo[8]) for c in dg} == {(3, 1), (1, 0)}
        assert all(c.geo[3] != c.geo[4] for c in dg)
        assert {rr.decoder(_kernel_C(c), dt) for c in dg} == {"divides", "uniform", "generic"} - \
            ({"divides"} if dt == "f32" else set())
        for c in dg:
            if c.opts == ("res2",):
                N, H, W = c.geo[:3]
                assert H % 2 == 0 and W % 2 == 0 and H // 2 != W // 2 and (N * H * W) % 128
        nt = [c for c in rr.CONV_CASES if c.api == "nt" and c.dt == dt]
        assert {c.geo[3] for c in nt} >= {24, 40, 2048}
        assert all(rr._extra(c.opts, "lda") > 0 for c in nt)
        assert any({"bias", "stats"} <= set(c.opts) for c in nt)


def test_wgrad_rows_reach_what_they_name():
    for dt in ("f32", "bf16"):
        epc, bk = rr.EPC[dt], rr.BK[dt]
        cases = [c for c in rr.WGRAD_CASES if c.dt == dt]
        conv = [c for c in cases if c.api == "conv"]
        assert {c.geo[4] for c in conv} == {8, 64, 72, 136}
        assert {c.geo[3] * c.geo[5] * c.geo[6] for c in conv} >= {72, 216, 1152, 200}
        maps, ms, mid_row, mid_img, partial = set(), set(), False, False, False
        for c in cases:
            N, H, W, C, Co, R, S, st, pd = c.geo
            Ho, Wo = (H + 2 * pd - R) // st + 1, (W + 2 * pd - S) // st + 1
            M, K = N * Ho * Wo, R * S * C
            splits, mps = rr.wgrad_splits(dt, M, Co, K)
            assert mps % bk == 0 and (splits - 1) * mps < M <= splits * mps
            assert M * Co * K <= 5e7
            ms.add(M)
            if c.api == "conv":
                maps.add((Ho, Wo, st))
                if splits >= 2:
                    assert M >= 16 * bk or splits == 2
                    mid_row |= mps % Wo != 0
                    mid_img |= mps % (Ho * Wo) != 0 and mps % Wo != 0
                    partial |= M % mps != 0 and M % epc != 0
        assert {(1, 1, 1), (2, 2, 1), (3, 5, 1), (7, 5, 1), (9, 14, 1), (5, 4, 2)} <= maps
        assert any(c.geo[5:] == (1, 1, 2, 0) for c in conv)
        assert any(Ho * Wo < epc and N * Ho * Wo > 2 * epc for (N, Ho, Wo) in
                   [(c.geo[0], (c.geo[1] + 2 * c.geo[8] - c.geo[5]) // c.geo[7] + 1,
                     (c.geo[2] + 2 * c.geo[8] - c.geo[6]) // c.geo[7] + 1) for c in conv])
        assert mid_row and mid_img and partial
        assert any(M >= 16 * bk and rr.wgrad_splits(dt, M, 8, 72)[0] >= 2 for M in ms)
        assert 1 in ms and any(1 < M < bk for M in ms)
        assert {c.opts for c in conv} >= {("aff0",), ("aff1",)}
        tn = [c for c in cases if c.api == "tn"]
        assert {c.geo[0] for c in tn} >= {37, 600}
        assert all(rr._extra(c.opts, "ldd") and rr._extra(c.opts, "ldx") for c in tn)
    # the issue's example: f32, M = 595 on 7x5 maps splits into 224-pixel ranges
    assert rr.wgrad_splits("f32", 595, 136, 216) == (3, 224)
    assert rr.wgrad_splits("bf16", 1134, 8, 72) == (3, 384) and rr.wgrad_splits("f32", 1134, 8, 72) == (5, 256)


# ---------------------------------------------------------------------------
# per case: the reference against torch's own float64 operator, and the sensitivity of the data
@pytest.mark.parametrize("case", rr.CONV_CASES, ids=_ids(rr.CONV_CASES))
def test_conv_case(case):
    p = rr.problem(case)
    assert rr.decoder(p.C, case.dt) in ("divides", "uniform", "generic")
    assert p.M * p.Co * p.K <= 5e7
    if p.aff is not None:
        assert (p.aff[1] > 0).any() and (p.aff[1] < 0).any()
    ref = p.torch_ref()
    scale = p.ref.abs().max().item()
    assert (ref - p.ref).abs().max().item() <= 1e-12 * max(scale, 1.0)
    assert ((p.bar > 0) | (p.ref == 0)).all()  # an all-padding pixel: exactly zero, bar zero
    s = p.sensitivity()
    print(f"SENSITIVITY {case.id}: " + " ".join(f"{k}={v:.2e}" for k, v in s.items() if v is not None))
    assert s["drop"] > 1.0, s
    assert (s["tap"] is None) == (p.R * p.S == 1) and (s["tap"] is None or s["tap"] > 1.0), s
    assert (s["seg"] is None) == (p.nseg == 1) and (s["seg"] is None or s["seg"] > 1.0), s


@pytest.mark.parametrize("case", rr.WGRAD_CASES, ids=_ids(rr.WGRAD_CASES))
def test_wgrad_case(case):
    p = rr.problem(case)
    assert (p.splits, p.m_per_split) == rr.wgrad_splits(case.dt, p.M, p.Co, p.K)
    if p.aff is not None:
        assert (p.aff[1] > 0).any() and (p.aff[1] < 0).any()
    ref = p.torch_ref()
    assert (ref - p.ref).abs().max().item() <= 1e-12 * max(p.ref.abs().max().item(), 1.0)
    assert (p.bar > 0).all()
    s = p.sensitivity()
    print(f"SENSITIVITY {case.id}: " + " ".join(f"{k}={v:.2e}" for k, v in s.items() if v is not None))
    assert s["drop"] > 1.0 and s["whole"] > 1.0, s
    assert (s["tap"] is None) == (p.R * p.S == 1) and (s["tap"] is None or s["tap"] > 1.0), s


def test_case_ids_are_unique():
    ids = _ids(rr.CONV_CASES) + _ids(rr.WGRAD_CASES)
    assert len(ids) == len(set(ids))
    # no row of the tables is dropped on the way to the parametrisation
    assert len(rr.CONV_CASES) == 2 * (len(rr.DECODER_ROWS) + 2 * (len(rr.FWD_EPILOGUES) + len(rr.ACT_EPILOGUES) + 1)
                                      + len(rr.DGRAD_ROWS) + len(rr.NT_ROWS))
    assert len(rr.WGRAD_CASES) == 2 * (len(rr.WGRAD_ROWS) + len(rr.TN_ROWS))
