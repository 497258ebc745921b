#!/usr/bin/env python3
"""Microbenchmark of the Bottleneck tail + next conv1 forward at the C2 step's
56x56 and 28x28 transitions (384 images per segment, three BN segments, both
residual forms): the pair artsbir_block_out_mask + artsbir_conv2d_fwd_seg (the
committed tune table loaded) against the one call artsbir_block_out_conv1x1_fwd.

Each is timed REPS times with events after a warm-up, the two interleaved; the
pair's spread is max - min of its timings.  A shape belongs in the C predicate
(bstream_shape, csrc/bstream.hip) only if the fused median is below the pair's
median by more than that spread.  Results are not checked here
(tests/test_block_conv1_gpu.py)."""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "art-sbir_amd"))

import torch  # noqa: E402

import _hip  # noqa: E402

TUNE_CACHE = os.path.join(ROOT, "profiles", "tune_r6.txt")
SHAPES = [  # images, H, W, K (block channels), N (conv1 outputs)
    (1152, 56, 56, 256, 64),
    (1152, 56, 56, 256, 128),
    (1152, 28, 28, 512, 128),
]
G = 3
REPS = int(os.environ.get("REPS", "9"))


def once(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3


def main():
    dev = torch.device("cuda:0")
    st = _hip.stream()
    if _hip.lib().artsbir_tune_load(TUNE_CACHE.encode()) < 0:
        raise SystemExit(f"cannot load {TUNE_CACHE}")
    print(f"# {torch.cuda.get_device_name(0)}; library {os.path.relpath(_hip.LIB_PATH, ROOT)}; {REPS} timings each, interleaved; us")
    for (B, H, W, K, N) in SHAPES:
        rows = B * H * W
        y3 = torch.randn(rows, K, device=dev).bfloat16()
        r = torch.randn(rows, K, device=dev).bfloat16()
        w = (torch.randn(N, K, device=dev) / K ** 0.5).bfloat16()
        bn3 = torch.rand(G, 4, K, device=dev) + 0.5
        bnd = torch.rand(G, 4, K, device=dev) + 0.5
        out = torch.empty_like(y3)
        bits = torch.empty(rows * K // 8, dtype=torch.uint8, device=dev)
        y1 = torch.empty(rows, N, device=dev, dtype=torch.bfloat16)
        stats = torch.zeros(G, _hip.NSLOT, 2, N, device=dev)
        d = _hip.conv_desc(torch.bfloat16, B, H, W, K, N, 1, 1, 1, 0)
        nb_fused = 2 * (3 * rows * K + N * K + rows * N) + rows * K // 8
        nb_pair = nb_fused + 2 * rows * K
        for two in (False, True):
            yd, pd, idn = (r.data_ptr(), bnd.data_ptr(), None) if two else (None, None, r.data_ptr())

            def pair():
                _hip.call("artsbir_block_out_mask", _hip.DT_BF16, y3.data_ptr(), bn3.data_ptr(), yd, pd, idn, rows, K,
                          G, out.data_ptr(), bits.data_ptr(), st)
                _hip.call("artsbir_conv2d_fwd_seg", d, out.data_ptr(), w.data_ptr(), y1.data_ptr(), G,
                          stats.data_ptr(), st)

            def fused():
                _hip.call("artsbir_block_out_conv1x1_fwd", d, y3.data_ptr(), bn3.data_ptr(), yd, pd, idn, w.data_ptr(),
                          G, out.data_ptr(), bits.data_ptr(), y1.data_ptr(), stats.data_ptr(), st)

            def conv_only():
                _hip.call("artsbir_conv2d_fwd_seg", d, out.data_ptr(), w.data_ptr(), y1.data_ptr(), G,
                          stats.data_ptr(), st)

            for fn in (pair, fused, pair, fused):
                fn()
            torch.cuda.synchronize()
            pair()
            kp = _hip.lib().artsbir_last_kernel().decode()
            fused()
            kf = _hip.lib().artsbir_last_kernel().decode()
            tp, tf, tc = [], [], []
            for _ in range(REPS):
                tp.append(once(pair))
                tf.append(once(fused))
                tc.append(once(conv_only))
            mp, mf = statistics.median(tp), statistics.median(tf)
            spread = max(tp) - min(tp)
            form = "downsample" if two else "identity"
            print(f"== {B}x{H}x{W} {K}->{N} {form}: pair {nb_pair / 1e9:.2f} GB, fused {nb_fused / 1e9:.2f} GB")
            print(f"  pair  block_out + {kp:30s} min {min(tp):7.1f} med {mp:7.1f} max {max(tp):7.1f}  spread {spread:5.1f}"
                  f"  ({nb_pair / mp / 1e3:5.0f} GB/s; its conv alone med {statistics.median(tc):7.1f})")
            print(f"  fused {kf:42s} min {min(tf):7.1f} med {mf:7.1f} max {max(tf):7.1f}"
                  f"  ({nb_fused / mf / 1e3:5.0f} GB/s)")
            print(f"  fused - pair {mf - mp:+8.1f} us ({(mf / mp - 1) * 100:+.1f} %): "
                  f"{'faster by more than the spread' if mf < mp - spread else 'NOT faster by more than the spread'}",
                  flush=True)
        del y3, r, out, bits, y1


if __name__ == "__main__":
    main()
