#!/usr/bin/env python3
"""losses.info_nce with gradients (one artsbir_info_nce call and the backward's three
multiplies) on [B, D] f32 embeddings with ids, over the batch alone (M = 0) and with a full
ring of M rows, against the torch composition of the same loss on the same device:
normalise, matmul, masked logsumexp in the stable form, autograd backward.  The parent of
this kernel has no such path, so the composition is the baseline.  Device events after
warm-up; the two forms alternate and the medians are compared; every raw run is printed.

    python tools/infonce_bench.py [--runs 20] [--out profiles/infonce_bench.txt]

The derived bound: four products of 2 B C D flops with C = 2B + M (the logits twice, W C^
over C, W^T A^ over 2B only) at the 157.3 TFLOP/s f32 matrix peak."""
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
F32_MATRIX = 157.3e12
C2_STEP_MS = 88.77
TAU = 0.07


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def bound_ms(B, M, D):
    C = 2 * B + M
    return 1e3 * (3 * 2 * B * C * D + 2 * B * 2 * B * D) / F32_MATRIX


def composition(a, p, n, ids, mem, mem_ids):
    """the same loss by torch ops: the stable form, f32"""
    norm = lambda x: x / x.norm(dim=1, keepdim=True).clamp_min(1e-8)  # noqa: E731
    B = a.shape[0]
    pool = torch.cat((p, n) if mem is None else (p, n, mem))
    pool_ids = ids if mem is None else torch.cat((ids, mem_ids))
    z = norm(a) @ norm(pool).T / TAU
    rows = torch.arange(B, device=a.device)
    neg = pool_ids[None, :] != ids[:B, None]
    neg[rows, rows] = False
    L = torch.logsumexp(z.masked_fill(~neg, float("-inf")), dim=1)
    return torch.nn.functional.softplus(L - z[rows, rows]).mean()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("infonce_bench needs the GPU: there is no CPU path to time")
    dev = torch.device("cuda:0")
    lines = [f"# {torch.cuda.get_device_name(0)}; tau {TAU}; ms per loss + gradients, device events, {args.runs} "
             f"alternating runs after {args.warmup} warm-up"]
    for B, D in SIZES:
        g = torch.Generator(device="cpu").manual_seed(B + D)
        a = torch.randn(B, D, generator=g)
        p = a + 3.0 * torch.randn(B, D, generator=g)
        n = torch.randn(B, D, generator=g)
        leaves = [t.to(dev).requires_grad_(True) for t in (a, p, n)]
        ids = torch.arange(2 * B, device=dev)
        for M in RINGS:
            memory = mem = mem_ids = None
            if M:
                memory = losses.CrossBatchMemory(M, D, dev)
                memory.enqueue(torch.randn(M, D, generator=g).to(dev), torch.arange(2 * B, 2 * B + M, device=dev))
                mem, mem_ids = memory.mem, memory.mem_ids

            def kernel():
                for t in leaves:
                    t.grad = None
                losses.info_nce(*leaves, temperature=TAU, cand_ids=ids, memory=memory).backward()

            def torch_ops():
                for t in leaves:
                    t.grad = None
                composition(*leaves, ids, mem, mem_ids).backward()

            forms = {"kernel": kernel, "torch": torch_ops}
            for _ in range(args.warmup):
                for fn in forms.values():
                    fn()
            # the two forms compute the same thing
            kernel()
            lk, gk = float(losses.info_nce(*leaves, temperature=TAU, cand_ids=ids, memory=memory)), leaves[0].grad.clone()
            torch_ops()
            lt, gt = float(composition(*leaves, ids, mem, mem_ids)), leaves[0].grad
            agree = float((gk - gt).abs().max() / gt.abs().max())
            times = {k: [] for k in forms}
            for r in range(args.runs):
                for k, fn in forms.items():
                    times[k].append(timed(fn))
                lines.append(f"raw B={B} D={D} M={M} run={r} " + " ".join(f"{k}={times[k][-1]:.4f}" for k in forms))
            med = {k: statistics.median(v) for k, v in times.items()}
            bound = bound_ms(B, M, D)
            lines.append(f"median B={B} D={D} M={M} kernel={med['kernel']:.4f} min={min(times['kernel']):.4f} "
                         f"torch={med['torch']:.4f} min={min(times['torch']):.4f} torch/kernel={med['torch'] / med['kernel']:.2f} "
                         f"bound={bound:.4f} ({100 * bound / med['kernel']:.1f} % of the bound's rate) "
                         f"{100 * med['kernel'] / C2_STEP_MS:.2f} % of the {C2_STEP_MS} ms C2 step "
                         f"loss kernel={lk:.6f} torch={lt:.6f} max|da - da_torch|/max={agree:.2e}")
            del memory, mem, mem_ids
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
