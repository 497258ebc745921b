#!/usr/bin/env python3
"""What the cross-batch memory adds to the selection: losses.select_negatives on
[B, D] f32 embeddings with ids, alone (M = 0: artsbir_mine_negatives, the `select`
column of tools/mining_bench.py) and over a full ring of M rows (artsbir_mine_pool),
timed with device events after warm-up.  The forms alternate on the same device and
the medians are compared; every raw run is printed.

    python tools/xbm_bench.py [--runs 40] [--out profiles/xbm_bench.txt]

For M > 0 the time the ring adds (median minus the M = 0 median) is set against the
derived bound of its arithmetic: B M D pair terms of three f32 vector operations
(subtract, add eps, fused multiply-add; the cosine key has one, its bound is a third)
at the chip's unpacked f32 vector rate, a quarter of the 157.3 TFLOP/s packed-FMA peak;
with every operation packed (two anchors an instruction, as the scan issues them) the
bound is half of that, so 50 % of the printed rate is the packed limit's."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "art-sbir_amd"))

import torch  # noqa: E402

import losses  # noqa: E402

SIZES = [(384, 512), (384, 1024)]
RINGS = [0, 4096, 16384, 65536]
VALU_OPS = 157.3e12 / 4  # unpacked f32 vector operations per second
C2_STEP_MS = 88.77


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def bound_ms(B, M, D, metric):
    return 1e3 * B * M * D * (3 if metric == "euclidean" else 1) / VALU_OPS


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--metric", default="euclidean", choices=["euclidean", "cosine"])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("xbm_bench needs the GPU: there is no CPU path to time")
    dev = torch.device("cuda:0")
    lines = [f"# {torch.cuda.get_device_name(0)}; {args.metric}; ms per selection, device events, {args.runs} "
             f"alternating runs after {args.warmup} warm-up"]
    for mode in ("hardest", "semihard"):
        for B, D in SIZES:
            g = torch.Generator(device="cpu").manual_seed(B + D)
            a = torch.randn(B, D, generator=g)
            p = a + 0.7 * torch.randn(B, D, generator=g)
            n = torch.randn(B, D, generator=g)
            a, p, n = (t.to(dev) for t in (a, p, n))
            ids = torch.arange(2 * B, device=dev)
            forms, rings = {}, {}
            for M in RINGS:
                if M:
                    memory = losses.CrossBatchMemory(M, D, dev)
                    memory.enqueue(torch.randn(M, D, generator=g).to(dev), torch.arange(2 * B, 2 * B + M, device=dev))
                    rings[M] = memory
                forms[M] = (lambda m: lambda: losses.select_negatives(a, p, n, mode, args.metric, cand_ids=ids,
                                                                      memory=m))(rings.get(M))
            for _ in range(args.warmup):
                for fn in forms.values():
                    fn()
            times = {M: [] for M in forms}
            for r in range(args.runs):
                for M, fn in forms.items():
                    times[M].append(timed(fn))
                lines.append(f"raw {mode} B={B} D={D} run={r} " + " ".join(f"M{M}={times[M][-1]:.4f}" for M in forms))
            med = {M: statistics.median(v) for M, v in times.items()}
            for M in RINGS:
                text = f"median {mode} B={B} D={D} M={M} select={med[M]:.4f} min={min(times[M]):.4f}"
                if M:
                    added, bound = med[M] - med[0], bound_ms(B, M, D, args.metric)
                    sel = forms[M]()[0]
                    text += (f" ring={added:.4f} bound={bound:.4f} unpacked / {bound / 2:.4f} packed"
                             f" ({100 * bound / added:.1f} % / {50 * bound / added:.1f} % of the bound's rate)"
                             f" {100 * added / C2_STEP_MS:.2f} % of the {C2_STEP_MS} ms C2 step"
                             f" from_memory={float((sel >= 2 * B).float().mean()):.3f}")
                lines.append(text)
            del rings, forms
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
