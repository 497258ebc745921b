#!/usr/bin/env python3
"""What in-batch negative mining adds to the loss tail: forward + backward of
losses.MinedNegatives(TripletMarginLoss) against plain TripletMarginLoss on [B, D]
f32 embeddings, timed with device events after warm-up.  The two forms alternate on
the same device and the medians are compared; the mining kernels alone (selection,
gather, scatter) are timed the same way.

    python tools/mining_bench.py [--runs 40] [--out profiles/mining_bench.txt]

The limit: the added time at B = 384, D = 512 stays under 1 % of the C2 step."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "art-sbir_amd"))

import torch  # noqa: E402

import _hip  # noqa: E402
import losses  # noqa: E402

SIZES = [(384, 512), (384, 1024)]
C2_STEP_MS = 88.77


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def tail(loss_fn, a, p, n):
    def run():
        for t in (a, p, n):
            t.grad = None
        loss_fn(a, p, n).backward()
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mining_bench needs the GPU: there is no CPU path to time")
    dev = torch.device("cuda:0")
    lines = [f"# {torch.cuda.get_device_name(0)}; ms per call, device events, {args.runs} alternating runs "
             f"after {args.warmup} warm-up"]
    for mode in ("hardest", "semihard"):
        for B, D in SIZES:
            g = torch.Generator(device="cpu").manual_seed(B + D)
            a = torch.randn(B, D, generator=g)
            p = a + 0.7 * torch.randn(B, D, generator=g)
            n = torch.randn(B, D, generator=g)
            a, p, n = (t.to(dev).requires_grad_(True) for t in (a, p, n))
            plain = losses.TripletMarginLoss(0.2)
            mined = losses.MinedNegatives(losses.TripletMarginLoss(0.2), mode)
            ids = torch.arange(2 * B, device=dev)
            sel = losses.select_negatives(a, p, n, mode)[0]
            out, dp, dn = (torch.empty(B, D, device=dev) for _ in range(3))
            forms = {
                "plain": tail(plain, a, p, n),
                "mined": tail(mined, a, p, n),
                "select": lambda: losses.select_negatives(a, p, n, mode, cand_ids=ids),
                "gather": lambda: _hip.call("artsbir_rows_gather2", p.data_ptr(), n.data_ptr(), sel.data_ptr(), B, D,
                                            out.data_ptr(), _hip.stream()),
                "scatter": lambda: _hip.call("artsbir_rows_scatter2", out.data_ptr(), sel.data_ptr(), B, D,
                                             dp.data_ptr(), dn.data_ptr(), _hip.stream()),
            }
            for _ in range(args.warmup):
                for fn in forms.values():
                    fn()
            times = {k: [] for k in forms}
            for r in range(args.runs):
                for k, fn in forms.items():
                    times[k].append(timed(fn))
                lines.append(f"raw {mode} B={B} D={D} run={r} " + " ".join(f"{k}={times[k][-1]:.4f}" for k in forms))
            med = {k: statistics.median(v) for k, v in times.items()}
            added = med["mined"] - med["plain"]
            lines.append(f"median {mode} B={B} D={D} " + " ".join(f"{k}={v:.4f}" for k, v in med.items()) +
                         f" added={added:.4f} ({100 * added / C2_STEP_MS:.3f} % of the {C2_STEP_MS} ms C2 step)"
                         f" mined_fraction={mined.mined_fraction():.3f}")
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
