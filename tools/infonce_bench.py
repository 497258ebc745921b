#!/usr/bin/env python3
"""losses.info_nce with gradients (one artsbir_info_nce call and the backward's three
multiplies) on [B, D] f32 embeddings with ids, over the batch alone (M = 0) and with a full
ring of M rows, against the torch composition of the same loss on the same device:
normalise, matmul, masked logsumexp in the stable form, autograd backward.  The parent of
this kernel has no such path, so the composition is the baseline.  Device events after
warm-up; the two forms alternate and the medians are compared; every raw run is printed.

    python tools/infonce_bench.py [--runs 20] [--out profiles/infonce_bench.txt]
    python tools/infonce_bench.py --pool-out profiles/infonce_gather_bench.txt [--parent-lib OLD.so]

--pool-out times the raw entry points instead (no autograd around them), forward plus
gradients: artsbir_info_nce of this tree's library against the same call of --parent-lib (a
build of the parent commit, loaded beside it) at B = 384, D = 512 / 1024, M = 0 / 65536, with
the outputs of the two compared byte for byte; and artsbir_info_nce_pool at the shape of 8
ranks x 384 triplets (B = 384, Nc = 6144, pos0 = 768, D = 512, M = 0 / 65536) against
artsbir_info_nce at the same total candidate count (B = 384, M = 5376 filled).

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


class Raw:
    """buffers of one shape and the raw calls on them.  batch(lib): artsbir_info_nce with
    p = cand[:B], n = cand[B:2B]; pool(lib): artsbir_info_nce_pool over all Nc rows"""

    def __init__(self, B, Nc, pos0, D, M, dev, seed):
        import _hip
        g = torch.Generator(device="cpu").manual_seed(seed)
        self.B, self.Nc, self.pos0, self.D, self.M = B, Nc, pos0, D, M
        self.a = torch.randn(B, D, generator=g).to(dev)
        self.cand = torch.randn(Nc, D, generator=g).to(dev)
        self.cand[pos0:pos0 + B] = self.a + 3.0 * torch.randn(B, D, generator=g).to(dev)
        self.ids = torch.arange(Nc, device=dev)
        self.mem = self.mem_ids = self.state = None
        if M:
            self.mem = torch.randn(M, D, generator=g).to(dev)
            self.mem_ids = torch.arange(Nc, Nc + M, device=dev)
            self.state = torch.tensor([0, M], dtype=torch.int64, device=dev)
        lib = _hip.lib()
        nbytes = max(lib.artsbir_info_nce_workspace(B, D, M, 1), lib.artsbir_info_nce_pool_workspace(B, Nc, D, M, 1))
        self.ws, self.nbytes = torch.empty(nbytes, dtype=torch.uint8, device=dev), nbytes
        f = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=dev)  # noqa: E731
        self.out = dict(loss=f(1), rows=f(B), q=f(B), da=f(B, D), dcand=f(Nc, D))
        self.stream = _hip.stream()

    def _ring(self):
        from _hip import ptr
        return ptr(self.ids), ptr(self.mem), ptr(self.mem_ids), ptr(self.state), self.M

    def batch(self, lib):
        from _hip import ptr
        o, B, D = self.out, self.B, self.D
        rc = lib.artsbir_info_nce(ptr(self.a), ptr(self.cand), ptr(self.cand[B:]), B, D, 1.0 / TAU, 1e-8, *self._ring(),
                                  ptr(o["loss"]), ptr(o["rows"]), ptr(o["q"]), ptr(o["da"]), ptr(o["dcand"]),
                                  ptr(o["dcand"][B:]), ptr(self.ws), self.nbytes, self.stream)
        assert rc == 0, lib.artsbir_last_error()

    def pool(self, lib):
        from _hip import ptr
        o = self.out
        rc = lib.artsbir_info_nce_pool(ptr(self.a), ptr(self.cand), self.B, self.Nc, self.pos0, self.D, 1.0 / TAU, 1e-8,
                                       *self._ring(), ptr(o["loss"]), ptr(o["rows"]), ptr(o["q"]), ptr(o["da"]),
                                       ptr(o["dcand"]), ptr(self.ws), self.nbytes, self.stream)
        assert rc == 0, lib.artsbir_last_error()

    def snapshot(self, rows):
        torch.cuda.synchronize()
        return [self.out[k].clone() for k in ("loss", "rows", "q", "da")] + [self.out["dcand"][:rows].clone()]


def load_beside(path):
    """a second build of the library beside the one _hip holds: its own symbols first"""
    import ctypes

    import _hip
    lib = ctypes.CDLL(os.path.abspath(path), mode=os.RTLD_LOCAL | os.RTLD_DEEPBIND)
    for name in ("artsbir_info_nce", "artsbir_info_nce_workspace"):
        fn = getattr(lib, name)
        fn.argtypes = _hip.SIGNATURES[name]
        fn.restype = _hip._RESTYPES.get(name, ctypes.c_int)
    lib.artsbir_last_error.restype = ctypes.c_char_p
    return lib


def alternate(forms, runs, warmup, tag, lines):
    """forms: name -> callable; alternating timed runs -> name -> (median, min, max, quartiles' distance)"""
    for _ in range(warmup):
        for fn in forms.values():
            fn()
    times = {k: [] for k in forms}
    for r in range(runs):
        for k, fn in forms.items():
            times[k].append(timed(fn))
        lines.append(f"raw {tag} run={r} " + " ".join(f"{k}={times[k][-1]:.4f}" for k in forms))
    out = {}
    for k, v in times.items():
        qs = statistics.quantiles(v, n=4)
        out[k] = (statistics.median(v), min(v), max(v), qs[2] - qs[0])
    return out


def pool_bench(args, dev):
    import _hip
    lib = _hip.lib()
    lines = [f"# {torch.cuda.get_device_name(0)}; tau {TAU}; ms per raw call, forward plus gradients, with ids; device "
             f"events, {args.runs} alternating runs after {args.warmup} warm-up; spread = the distance of the quartiles"]
    if args.parent_lib:
        parent = load_beside(args.parent_lib)
        lines.append("# artsbir_info_nce: this tree's library against the parent commit's, B = 384")
        for D in (512, 1024):
            for M in (0, 65536):
                raw = Raw(384, 768, 0, D, M, dev, seed=D + M)
                raw.batch(parent)
                want = raw.snapshot(768)
                raw.batch(lib)
                got = raw.snapshot(768)
                same = all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(want, got))
                st = alternate({"new": lambda: raw.batch(lib), "parent": lambda: raw.batch(parent)}, args.runs,
                               args.warmup, f"batch D={D} M={M}", lines)
                diff = st["new"][0] - st["parent"][0]
                spread = max(st["new"][3], st["parent"][3])
                lines.append(f"median batch B=384 D={D} M={M} new={st['new'][0]:.4f} (min {st['new'][1]:.4f} max "
                             f"{st['new'][2]:.4f} spread {st['new'][3]:.4f}) parent={st['parent'][0]:.4f} (min "
                             f"{st['parent'][1]:.4f} max {st['parent'][2]:.4f} spread {st['parent'][3]:.4f}) new-parent="
                             f"{diff:+.4f} ({100 * diff / st['parent'][0]:+.2f} %) "
                             f"{'inside' if abs(diff) <= spread else 'OUTSIDE'} the spread; outputs the same bytes: {same}")
                del raw
    lines.append("# artsbir_info_nce_pool at 8 ranks x 384 (B = 384, Nc = 6144, pos0 = 768, D = 512) against "
                 "artsbir_info_nce at the same 6144 candidates (B = 384, M = 5376 filled)")
    pool0, pool64k, batch = Raw(384, 6144, 768, 512, 0, dev, 1), Raw(384, 6144, 768, 512, 65536, dev, 2), \
        Raw(384, 768, 0, 512, 5376, dev, 3)
    st = alternate({"pool_M0": lambda: pool0.pool(lib), "pool_M65536": lambda: pool64k.pool(lib),
                    "batch_M5376": lambda: batch.batch(lib)}, args.runs, args.warmup, "pool D=512", lines)
    for k, (med, lo, hi, spread) in st.items():
        lines.append(f"median {k} B=384 D=512 {med:.4f} (min {lo:.4f} max {hi:.4f} spread {spread:.4f}) "
                     f"{100 * med / C2_STEP_MS:.2f} % of the {C2_STEP_MS} ms C2 step")
    lines.append(f"pool_M0 - batch_M5376 = {st['pool_M0'][0] - st['batch_M5376'][0]:+.4f} ms: the dc^ kernel over 8x the "
                 f"rows and the finish pass; the collectives are not in these figures (one GPU): per rank the all-gather "
                 f"receives and the reduce-scatter sends 2 B D 4 world = {2 * 384 * 512 * 4 * 8} bytes at D = 512, world 8")
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.pool_out)), exist_ok=True)
    with open(args.pool_out, "w") as f:
        f.write(text + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--pool-out", default=None, help="time the raw batch and pool entry points instead; write here")
    ap.add_argument("--parent-lib", default=None, help="a build of the parent commit's library to alternate with")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("infonce_bench needs the GPU: there is no CPU path to time")
    dev = torch.device("cuda:0")
    if args.pool_out:
        return pool_bench(args, dev)
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
