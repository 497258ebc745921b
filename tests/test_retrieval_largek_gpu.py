"""Exact top-k for k > 64 vs the float64 oracle (oracle/retrieval.py): indices and
ranks bit-equal, keys at rtol 1e-12.

65 <= k <= 1024 is still one call of artsbir_pairwise_l2_topk: the chunk lists of
the scan give a per-query cut, a second scan pass collects the rows under it (at
most C = 2 k + 2048 per query), knn_lk_select_kernel sorts their exact keys and
knn_lk_exhaustive_kernel answers the queries whose buffer overflowed or stayed
short.  A gallery of at most C rows is sorted whole.  k > 1024 is knn.py's plain
path (artsbir_knn_exact_keys + a stable sort)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from oracle import retrieval as oret

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _case(N, D, Q, k, metric, noise=0.5):
    """inputs and the oracle's answers, computed once per case and never modified"""
    g, qs, pos = oret.synthetic_gallery(N, D, Q, noise=noise)
    return (g, qs, pos) + _oracle(g, qs, pos, k, metric)


def _oracle(g, qs, pos, k, metric="euclidean"):
    idx, dist, ranks = [], [], []
    for i, q in enumerate(qs):
        d = oret.distances(q, g, metric)
        ti, td = oret.topk(d, k)
        idx.append(ti)
        dist.append(td)
        ranks.append(oret.rank_of(d, pos[i]) if pos[i] >= 0 else -1)
    return np.array(idx), np.array(dist), np.array(ranks)


def _stat():
    """(queries answered by the select path, by the exhaustive fallback) since the last read"""
    import _hip
    torch.cuda.synchronize()
    out = (ctypes.c_longlong * 2)()
    assert _hip.lib().artsbir_knn_largek_stat_read(out, 1) == 0
    return int(out[0]), int(out[1])


def _t(x, dev):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dev)


def _check(out, ri, rd, rr=None, pos=None, atol=0.0):
    idx, dist, rank = out[0], out[1], out[2]
    np.testing.assert_array_equal(idx.cpu().numpy(), ri)
    np.testing.assert_allclose(dist.cpu().numpy(), rd, rtol=1e-12, atol=atol)
    if rr is not None:
        r = rank.cpu().numpy()
        m = pos >= 0
        np.testing.assert_array_equal(r[m], rr[m])


# (5000, 128, 32, 1024): 40 tiles x 16 list items < k, no cut exists (exhaustive
# kernel); (300, ...): N <= C, sorted whole; D = 768 takes knn_scan_kernel in bf16 too
SHAPES = [(20000, 64, 64, 65), (20000, 512, 48, 100), (20000, 64, 64, 1000), (5000, 128, 32, 1024),
          (300, 128, 20, 200), (4000, 768, 24, 100),
          # the collect-mode v2 scan at Dp = 128 and 256 (the cases above reach it at Dp = 64 and 512 only)
          (6000, 128, 24, 100), (6000, 256, 24, 100)]


@pytest.mark.parametrize("metric", ["euclidean", "cosine"])
@pytest.mark.parametrize("compute", ["bf16", "f32"])
@pytest.mark.parametrize("N,D,Q,k", SHAPES)
def test_largek_matches_oracle(compute, metric, N, D, Q, k, dev):
    import knn
    g, qs, pos, ri, rd, rr = _case(N, D, Q, k, metric)
    _stat()
    out = knn.knn(_t(qs, dev), _t(g, dev), k, _t(pos, dev), compute=compute, metric=metric)
    sel, fb = _stat()
    _check(out, ri, rd, rr, pos)
    assert sel + fb == Q
    if (N, k) != (5000, 1024):
        # i.i.d. rows: the candidates fit 2 k + 2048, so the select path
        # itself gave these answers, not the exhaustive kernel behind it
        assert (sel, fb) == (Q, 0)


@pytest.mark.parametrize("k", [100, 601])
def test_largek_ties_across_the_k_boundary(k, dev):
    """every row three times: sorted keys come in triples, and entries k and k + 1
    (1-based; 100 / 101 and 601 / 602) share one, so the lower index must win"""
    import knn
    rng = np.random.Generator(np.random.PCG64(21))
    base = rng.standard_normal((400, 64), dtype=np.float32)
    g = np.concatenate([base, base, base])[rng.permutation(1200)]
    at = np.array([5, 333, 777, 1199])
    qs = g[at] + np.float32(0.01) * rng.standard_normal((4, 64), dtype=np.float32)
    pos = at.astype(np.int64)
    ri, rd, rr = _oracle(g, qs, pos, k)
    assert (rd[:, k - 1] == np.sort(np.stack([oret.distances(q, g) for q in qs]), 1)[:, k]).all()  # a tie at the cut
    _check(knn.knn(_t(qs, dev), _t(g, dev), k, _t(pos, dev)), ri, rd, rr, pos)


@pytest.mark.parametrize("metric", ["euclidean", "cosine"])
def test_largek_near_ties_duplicates_and_scaled_rows(metric, dev):
    """the construction of test_knn_near_ties_duplicates_and_scaled_rows at k = 128 (N =
    3000 > C = 2304: cut + collect + select).  atol 1e-15 as there: the cosine key of a
    scaled copy is 1 - (1 - O(2^-53)), whose f64 rounding depends on the summation order"""
    import knn
    rng = np.random.Generator(np.random.PCG64(11))
    base = rng.standard_normal((3000, 128), dtype=np.float32)
    g = base.copy()
    g[1000:1040] = base[0:40]
    g[1040:1080] = base[0:40] * np.float32(2.5)
    g[1080:1120] = np.nextafter(base[0:40], np.float32(np.inf))
    g[1200] = 0.0
    qs = base[0:40] + np.float32(0.05) * rng.standard_normal((40, 128), dtype=np.float32)
    qs[5] = 0.0
    pos = np.arange(40, dtype=np.int64)
    pos[7] = 1200
    ri, rd, rr = _oracle(g, qs, pos, 128, metric)
    _check(knn.knn(_t(qs, dev), _t(g, dev), 128, _t(pos, dev), metric=metric), ri, rd, rr, pos, atol=1e-15)


@pytest.mark.parametrize("k", [100, 1024])
def test_largek_natural_overflow(k, dev):
    """6000 identical rows: every row is under any cut, more than C of them (k = 1024:
    the lists hold 47 x 16 < k items, no cut): the exhaustive kernel answers, rows 0..k-1"""
    import knn
    rng = np.random.Generator(np.random.PCG64(4))
    g = np.repeat(rng.standard_normal((1, 64), dtype=np.float32), 6000, axis=0)
    qs = rng.standard_normal((6, 64), dtype=np.float32)
    _stat()
    idx, dist, _, _ = knn.knn(_t(qs, dev), _t(g, dev), k)
    assert _stat() == (0, 6)
    np.testing.assert_array_equal(idx.cpu().numpy(), np.tile(np.arange(k), (6, 1)))
    d = dist.cpu().numpy()
    assert (d == d[:, :1]).all()
    np.testing.assert_allclose(d[:, 0], [oret.distances(q, g[:1])[0] for q in qs], rtol=1e-12)


def test_largek_forced_fallback(dev):
    import _hip
    import knn
    N, D, Q, k = 5000, 64, 40, 200
    g, qs, pos, ri, rd, rr = _case(N, D, Q, k, "euclidean")
    q, gg, p = _t(qs, dev), _t(g, dev), _t(pos, dev)
    _stat()
    ref = knn.knn(q, gg, k, p)
    assert _stat() == (Q, 0)
    old = _hip.lib().artsbir_knn_set_cand_cap(8)
    try:
        out = knn.knn(q, gg, k, p)
        assert _stat() == (0, Q)
    finally:
        _hip.lib().artsbir_knn_set_cand_cap(old)
    _check(out, ri, rd, rr, pos)
    for a, b in zip(out, ref):
        assert torch.equal(a, b)


@pytest.mark.parametrize("N", [70, 129, 1024])
def test_largek_k_equal_n_and_n_minus_1(N, dev):
    import knn
    for k in (N, N - 1):
        g, qs, pos, ri, rd, rr = _case(N, 64, 9, k, "euclidean", 1.0)
        _check(knn.knn(_t(qs, dev), _t(g, dev), k, _t(pos, dev)), ri, rd, rr, pos)


def test_largek_single_query_missing_and_far_positives(dev):
    import knn
    g, qs, pos, ri, rd, rr = _case(3000, 64, 40, 200, "euclidean", 3.0)  # the positive deep in the list
    assert rr.max() > 200
    pos = pos.copy()
    pos[::7] = -1
    out = knn.knn(_t(qs, dev), _t(g, dev), 200, _t(pos, dev))
    _check(out, ri, rd, rr, pos)
    one = knn.knn(_t(qs[3:4], dev), _t(g, dev), 200, _t(pos[3:4], dev))  # Q = 1
    _check(one, ri[3:4], rd[3:4], rr[3:4], pos[3:4])
    none = knn.knn(_t(qs, dev), _t(g, dev), 200)  # no positives at all
    assert none[2] is None and none[3] is None
    _check(none, ri, rd)


def test_largek_shards_on_one_gpu(dev):
    """ragged shards 4000 / 0 / 3700 / 1300 with rows duplicated across shards, k = 200:
    per-shard calls, device merge == oracle == host merge, summed ranks == oracle"""
    import knn
    N, D, Q, k = 9000, 256, 50, 200
    g, qs, pos = oret.synthetic_gallery(N, D, Q, noise=1.5)
    g = g.copy()
    g[4100:4160] = g[20:80]   # copies of shard 0 rows in shard 2 ...
    g[7800:7860] = g[20:80]   # ... and in shard 3
    qs[:10] = g[20:30] + np.float32(0.01)
    pos = pos.copy()
    pos[:10] = np.arange(7800, 7810)
    pos[::9] = -1
    ri, rd, rr = _oracle(g, qs, pos, k)
    q, gg, p = _t(qs, dev), _t(g, dev), _t(pos, dev)
    bounds = [0, 4000, 4000, 7700, N]
    shards = [(b0, gg[b0:b1].contiguous()) for b0, b1 in zip(bounds[:-1], bounds[1:])]
    dpos = torch.stack([knn.shard_positive_distances(q, sh, b0, p) for b0, sh in shards if len(sh)]).max(dim=0).values
    outs = [knn.knn(q, sh, k, p, g_base=b0, dpos=dpos) for b0, sh in shards]
    assert (outs[1][0] == -1).all() and torch.isinf(outs[1][1]).all()  # the empty shard
    all_d, all_i = torch.stack([o[1] for o in outs]), torch.stack([o[0] for o in outs])
    mi, md = knn.merge_topk_device(all_d, all_i, k)
    hi, hd = knn.merge_topk(list(all_i.cpu()), list(all_d.cpu()), k)
    assert torch.equal(mi.cpu(), hi) and torch.equal(md.cpu(), hd)
    _check((mi, md, sum(o[2] for o in outs)), ri, rd, rr, pos)


def test_largek_shard_shorter_than_k(dev):
    import knn
    g, qs, pos, ri, rd, rr = _case(150, 64, 12, 150, "euclidean", 1.0)
    q, gg, p = _t(qs, dev), _t(g, dev), _t(pos, dev)
    dpos = knn.shard_positive_distances(q, gg, 1000, p + 1000)
    idx, dist, rank, _ = knn.knn(q, gg, 200, p + 1000, g_base=1000, dpos=dpos)
    idx, dist = idx.cpu().numpy(), dist.cpu().numpy()
    np.testing.assert_array_equal(idx[:, :150], ri + 1000)
    np.testing.assert_allclose(dist[:, :150], rd, rtol=1e-12)
    assert (idx[:, 150:] == -1).all() and np.isinf(dist[:, 150:]).all()
    np.testing.assert_array_equal(rank.cpu().numpy(), rr)


def test_topk_merge_device_large_k(dev):
    """artsbir_topk_merge at nshard = 8, k = 500 == merge_topk, with ties and empties"""
    import knn
    rng = np.random.Generator(np.random.PCG64(3))
    ns, Q, k = 8, 5, 500
    d = np.round(rng.random((ns, Q, k)) * 64) / 64  # many exact ties
    i = rng.permutation(ns * Q * k).reshape(ns, Q, k).astype(np.int64)
    i[1, :, 300:] = -1
    d[1, :, 300:] = np.inf
    i[5] = -1
    d[5] = np.inf
    td, ti = torch.from_numpy(d), torch.from_numpy(i)
    hi, hd = knn.merge_topk(list(ti), list(td), k)
    di, dd = knn.merge_topk_device(td.to(dev), ti.to(dev), k)
    assert torch.equal(di.cpu(), hi) and torch.equal(dd.cpu(), hd)


@pytest.mark.parametrize("metric", ["euclidean", "cosine"])
@pytest.mark.parametrize("N,k", [(2000, 1500), (1100, 1100)])
def test_any_k_plain_path(N, k, metric, dev):
    import knn
    g, qs, pos, ri, rd, rr = _case(N, 64, 10, k, metric, 1.0)
    out = knn.knn(_t(qs, dev), _t(g, dev), k, _t(pos, dev), metric=metric)
    _check(out, ri, rd, rr, pos)
    np.testing.assert_allclose(out[3].cpu().numpy(), [oret.distances(q, g[p:p + 1], metric)[0] for q, p in zip(qs, pos)],
                               rtol=1e-12)


def test_get_topk_images_k_100(dev):
    import inference
    g, qs, pos, ri, rd, rr = _case(5000, 64, 40, 200, "euclidean")
    paths = [f"gallery/{i:05d}.jpg" for i in range(len(g))]
    got = inference.get_topk_images(100, paths, _t(qs[0], dev), _t(g, dev), "euclidean")
    assert len(got) == 100
    assert [p for p, _ in got] == [paths[i] for i in ri[0, :100]]
    np.testing.assert_allclose([d for _, d in got], rd[0, :100], rtol=1e-12)
