"""bench.py end to end on the GPU at --steps 2 --warmup 1: what a plain run does
and prints, what --full brings back, and --dump-outputs (the last timed step
under DIR/timed/, the repeatable replayed step under DIR/).  Three benchmark
processes in all (one shared reference run, two cases), at the benchmark's own
batch: its shapes are the ones in the committed autotuner table.

Bounds.  The timed (atomic BatchNorm sums) mode is not repeatable: loss_step0 is
held to the 5e-2 that tests/test_c2_gpu.py gives the atomic mode's loss.  The
loss after the three steps is compared with the reference run's to 30 %: at
these seeds it falls by about half per step (0.21, 0.13, 0.06), so timed steps
that started from another state, or one step more or fewer, miss that by far,
while two honest runs differed by 7.5 %.  The replayed step runs in the
deterministic mode: its forward arrays must be identical bits in both cases
(which differ in what ran before it); its gradients may differ by f32 summation
order (1e-3 rel. L2 allows for a bf16 rounding flip here and there), its
parameters by Adam's first update taken with the other sign, 2 lr."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")
NAMES = ["bn_running_stats", "embedding_negative", "embedding_positive", "embedding_sketch", "grads_sample", "loss",
         "params_sample"]
LEGS = ["embed", "retrieval", "c5", "preprocess", "cpu_baseline"]
NO_LEGS = ["--no-cpu-baseline", "--no-c5", "--no-retrieval", "--no-preprocess", "--no-embed"]
LR = 1e-5


def _bench(*argv):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", "2", "--warmup", "1", *argv], env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    return lines[0]


def _check_line(line):
    assert line["unit"] == "triplet-images/s" and line["higher_is_better"] is True and line["dtype"] == "bf16"
    assert line["steps"] == 2 and line["warmup"] == 1 and line["n_gpus"] == 1
    assert len(line["allocator"]["step_ms"]) == 2
    assert 20.0 < line["ms_per_step"] < 500.0, line["ms_per_step"]
    # value is the images of the timed steps over their time
    assert abs(line["value"] - 3 * 384 * 1e3 / line["ms_per_step"]) < 1e-3 * line["value"]
    assert np.isfinite(line["loss"]) and np.isfinite(line["loss_step0"])


@pytest.fixture(scope="module")
def plain(dev):
    return _bench()


def test_plain_run_times_the_steps_and_nothing_else(plain):
    _check_line(plain)
    assert [k for k in LEGS if k in plain] == []
    assert plain["roofline"] is None and plain["loss_step0_f32"] is None


_replays = {}


@pytest.mark.parametrize("full", [False, True], ids=["plain", "full"])
def test_dump_outputs(plain, tmp_path, full):
    line = _bench("--dump-outputs", str(tmp_path), *((["--full"] + NO_LEGS) if full else []))
    _check_line(line)
    assert [k for k in LEGS if k in line] == []
    if full:  # what --full brings back, less the legs switched off again
        assert line["roofline"]["kernel"] and line["roofline"]["launches"] > 0
        assert abs(line["loss_step0"] - line["loss_step0_f32"]) < 5e-2 * line["loss_step0_f32"]
    else:
        assert line["roofline"] is None and line["loss_step0_f32"] is None
    # the option does not change what the timed steps compute
    assert abs(line["loss_step0"] - plain["loss_step0"]) < 5e-2 * plain["loss_step0"]
    assert abs(line["loss"] - plain["loss"]) < 0.3 * plain["loss"], (line["loss"], plain["loss"])

    assert sorted(os.listdir(tmp_path)) == sorted([n + ".npy" for n in NAMES] + ["timed"])
    assert sorted(os.listdir(tmp_path / "timed")) == [n + ".npy" for n in NAMES]
    replay = {n: np.load(tmp_path / (n + ".npy")) for n in NAMES}
    timed = {n: np.load(tmp_path / "timed" / (n + ".npy")) for n in NAMES}
    total = 0
    for d in (replay, timed):
        for n, a in d.items():
            assert a.dtype == np.float32 and np.isfinite(a).all(), n
            total += a.nbytes
        assert d["loss"].shape == (1,) and d["embedding_sketch"].shape == (384, 512)
        assert d["embedding_positive"].shape == d["embedding_negative"].shape == (384, 512)
        assert d["params_sample"].shape == d["grads_sample"].shape and np.abs(d["grads_sample"]).max() > 0
    assert total <= 64e6
    # DIR/timed is the last timed step: its loss is the line's
    assert timed["loss"][0] == np.float32(line["loss"])
    # the replayed step starts from the initial state: its loss is the first step's (another reduction mode)
    assert abs(replay["loss"][0] - line["loss_step0"]) < 5e-2 * line["loss_step0"]
    assert not np.array_equal(replay["params_sample"], timed["params_sample"])
    _replays[full] = replay
    if len(_replays) == 2:
        a, b = _replays[False], _replays[True]
        for n in ("loss", "embedding_sketch", "embedding_positive", "embedding_negative", "bn_running_stats"):
            assert np.array_equal(a[n], b[n]), n
        ga, gb = a["grads_sample"].astype(np.float64), b["grads_sample"].astype(np.float64)
        assert np.linalg.norm(ga - gb) < 1e-3 * np.linalg.norm(ga)
        assert np.abs(a["params_sample"].astype(np.float64) - b["params_sample"]).max() <= 2 * LR * 1.05
