#!/usr/bin/env python3
"""The C2 training step (ResNet-50, 512-d, bf16, 384 triplets, bench.py's model,
batch and tuning table) through train.triplet_train with the given negatives and
with --negatives hardest / semihard, alternating on the same device: ms per step
from device events recorded as the loop fetches each batch.  With --memory_size M the
forms are --negatives hardest alone and with a cross-batch memory of M rows, filled
with random rows ahead of the first step so that every timed step scans all M.  With
--negatives all the forms are the given negatives and the InfoNCE loss over the batch
(losses.InfoNCELoss, cosine) and, with --memory_size M, over the batch and a full ring too.

    python tools/mining_step.py [--steps 10] [--warmup 3] [--negatives all] [--memory_size M] [--out FILE]"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "art-sbir_amd"))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import _hip  # noqa: E402
import bench  # noqa: E402  (the C2 constants and the tuning table)
import models  # noqa: E402
import optim  # noqa: E402
import train  # noqa: E402


class ResidentLoader:
    """one device-resident batch `steps` times; an event before every fetch"""
    sampler = None

    def __init__(self, batch, steps, batch_size):
        self.batch, self.steps, self.batch_size, self.events = batch, steps, batch_size, []

    def __len__(self):
        return self.steps

    def __iter__(self):
        for _ in range(self.steps):
            ev = torch.cuda.Event(enable_timing=True)
            ev.record()
            self.events.append(ev)
            yield self.batch


def run(negatives, batch, args, dev, memory_size=0):
    torch.manual_seed(1234)
    model = models.ModifiedResNet(bench.LAYERS, bench.OUT_DIM, heads=bench.HEADS, input_resolution=bench.RES,
                                  width=bench.WIDTH).to(dev)
    model.compute_dtype = torch.bfloat16
    opt = optim.Adam(model.parameters(), lr=1e-5, weight_decay=0.002)
    loss_fn = train.make_loss("cosine" if negatives == "all" else "euclidean", False, "Synthetic", 0.2, negatives,
                              memory_size)
    B = batch[0].shape[0]
    if memory_size:  # a full ring from the first step on (768 rows a step would take M / 768 steps)
        loss_fn.memory.enqueue(torch.randn(memory_size, bench.OUT_DIM, device=dev))
    if negatives != "given":
        batch = batch + [torch.arange(B, device=dev), torch.arange(B, 2 * B, device=dev)]
    loader = ResidentLoader(batch, args.warmup + args.steps + 1, B)
    out = train.triplet_train(model, 1, loader, ResidentLoader(batch, 1, B), loss_fn, opt, False)
    torch.cuda.synchronize()
    ev = loader.events[args.warmup:]
    ms = [ev[i].elapsed_time(ev[i + 1]) for i in range(len(ev) - 1)]
    return statistics.median(ms), min(ms), out, ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=384)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--memory_size", type=int, default=0)
    ap.add_argument("--negatives", default=None, choices=["all"],
                    help="all: time the InfoNCE loss against the given negatives")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mining_step needs the GPU")
    dev = torch.device("cuda:0")
    if os.path.exists(bench.TUNE_CACHE):
        _hip.lib().artsbir_tune_load(bench.TUNE_CACHE.encode())
    g = torch.Generator(device=dev).manual_seed(100)
    B, R = args.batch, bench.RES
    sketch = (torch.rand(B, 1, R, R, device=dev, generator=g) >= 0.1).float().expand(B, 3, R, R)
    pos, neg = (torch.rand(B, 3, R, R, device=dev, generator=g) for _ in range(2))
    mean = torch.tensor(models.CLIP_MEAN, device=dev)[None, :, None, None]
    std = torch.tensor(models.CLIP_STD, device=dev)[None, :, None, None]
    batch = [((t - mean) / std).contiguous() for t in (sketch, pos, neg)]
    lines = []
    forms = [("given", 0), ("hardest", 0), ("semihard", 0)]
    if args.memory_size:
        forms = [("hardest", 0), ("hardest", args.memory_size)]
    if args.negatives == "all":
        forms = [("given", 0), ("all", 0)] + ([("all", args.memory_size)] if args.memory_size else [])
    for r in range(args.rounds):
        for negatives, memory_size in forms:
            med, best, out, ms = run(negatives, batch, args, dev, memory_size)
            extra = f" mined_fraction={out['mined_fraction'][0]:.3f}" if "mined_fraction" in out else ""
            if "memory_fraction" in out:
                extra += f" memory_size={memory_size} memory_fraction={out['memory_fraction'][0]:.3f}"
            if "positive_probability" in out:
                extra += f" memory_size={memory_size} positive_probability={out['positive_probability'][0]:.4f}"
            lines.append(f"C2 step B={B} round={r} negatives={negatives:<8s} median={med:.2f} ms min={best:.2f} ms "
                         f"over {args.steps} steps train_loss={out['train_losses'][0]:.5f}{extra}")
            print(lines[-1], flush=True)
            if args.negatives == "all":  # every step of the run
                lines.append(f"raw round={r} negatives={negatives} memory_size={memory_size} ms=" +
                             " ".join(f"{v:.2f}" for v in ms))
                print(lines[-1], flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
