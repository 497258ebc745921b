#!/usr/bin/env python3
"""Whole-call time of knn.knn at several k on the gallery and queries of
bench.retrieval_leg (1M x 512, 10k queries, top-k + rank of the positive):

    python tools/knn_largek_bench.py [--reps R] [--n N] [--q Q] [k ...]   (default k: 10 64 100 1000)

Each k is warmed up once, then R calls are timed one by one with device events
(the k are interleaved rep by rep, so a drift of the machine hits all of them
alike); one JSON line per k with the median, the minimum and the maximum, and
for k > 64 the queries answered by the select path / the exhaustive fallback.
ARTSBIR_LIB=<path> times another build of the library (the parent commit's, for
the k <= 64 comparison): entry points it lacks are dropped from the ctypes table
and k beyond its limit is skipped.  The per-kernel split of one call comes from a
kernel trace of this script with --reps 1, in a run of its own."""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "art-sbir_amd"))

import torch  # noqa: E402

import _hip  # noqa: E402
import knn  # noqa: E402

NEW = ("artsbir_knn_set_cand_cap", "artsbir_knn_largek_stat_read", "artsbir_knn_exact_keys")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--q", type=int, default=10_000)
    ap.add_argument("--d", type=int, default=512)
    ap.add_argument("k", type=int, nargs="*", default=[10, 64, 100, 1000])
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("knn_largek_bench: no GPU (there is no CPU timing of this path)")
    dev = torch.device("cuda:0")
    handle = ctypes.CDLL(_hip.LIB_PATH)
    has_large = all(hasattr(handle, n) for n in NEW)
    if not has_large:
        for n in NEW:
            _hip.SIGNATURES.pop(n, None)
    lib = _hip.lib()
    ks = [k for k in args.k if has_large or k <= knn.KMAX]
    N, D, Q = args.n, args.d, args.q
    gal = torch.randn(N, D, device=dev, generator=torch.Generator(device=dev).manual_seed(7))
    pos = (torch.arange(Q, device=dev, dtype=torch.int64) * 7919) % N
    qs = gal[pos] + 0.5 * torch.randn(Q, D, device=dev, generator=torch.Generator(device=dev).manual_seed(8))

    def stat():
        if not has_large:
            return None
        torch.cuda.synchronize()
        out = (ctypes.c_longlong * 2)()
        lib.artsbir_knn_largek_stat_read(out, 1)
        return [int(out[0]), int(out[1])]

    counts = {}
    for k in ks:  # warm-up of every shape, and the path each query took
        stat()
        knn.knn(qs, gal, k, pos)
        counts[k] = stat()
    ms = {k: [] for k in ks}
    for _ in range(args.reps):
        for k in ks:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            knn.knn(qs, gal, k, pos)
            e1.record()
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1))
    for k in ks:
        t = ms[k]
        r = {"lib": os.path.relpath(_hip.LIB_PATH, ROOT), "N": N, "D": D, "Q": Q, "k": k, "reps": len(t),
             "ms_median": round(statistics.median(t), 3), "ms_min": round(min(t), 3), "ms_max": round(max(t), 3)}
        if k > knn.KMAX and counts[k] is not None:
            r["select_queries"], r["fallback_queries"] = counts[k]
        print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
