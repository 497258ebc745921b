"""bench.py --dump-outputs: dump_outputs writes the loss, the three embeddings,
the BatchNorm running statistics and one fixed sample of every parameter and
of its gradient as float32 .npy files.  CPU only: the function is handed a small
torch model in place of the benchmark's (it reads tensors, it launches nothing);
the sample's indices must not depend on the run, since the dumps of two builds
are compared element for element."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _model_and_step(seed):
    torch.manual_seed(seed)
    m = torch.nn.Sequential(torch.nn.Linear(300, 200), torch.nn.BatchNorm1d(200), torch.nn.Linear(200, 8))
    with torch.no_grad():  # element i holds i / 65536 - 0.5 (exact in float32): a value tells its position
        m[0].weight.copy_((torch.arange(60000.0) / 65536 - 0.5).reshape(200, 300))
    outs = [m(torch.randn(4, 300)) for _ in range(3)]
    loss = torch.nn.functional.triplet_margin_loss(*outs, margin=0.2)
    loss.backward()
    return m, loss, outs


def test_dump_outputs_files_and_sample(tmp_path, monkeypatch):
    import bench
    monkeypatch.setattr(bench, "DUMP_SAMPLE", 2000)
    m, loss, outs = _model_and_step(0)
    # the process's random state must not move the sample
    torch.manual_seed(99)
    bench.dump_outputs(str(tmp_path / "a"), loss, [o.bfloat16() for o in outs], m)
    torch.manual_seed(7)
    torch.rand(5)
    bench.dump_outputs(str(tmp_path / "b"), loss, [o.bfloat16() for o in outs], m)
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == ["bn_running_stats.npy", "embedding_negative.npy", "embedding_positive.npy",
                     "embedding_sketch.npy", "grads_sample.npy", "loss.npy", "params_sample.npy"]
    a = {n: np.load(tmp_path / "a" / n) for n in names}
    for n in names:
        assert a[n].dtype == np.float32, n
        assert np.array_equal(a[n], np.load(tmp_path / "b" / n)), n
    assert a["loss.npy"].shape == (1,) and a["loss.npy"][0] == np.float32(loss.item())
    for n, o in zip(("sketch", "positive", "negative"), outs):
        assert np.array_equal(a[f"embedding_{n}.npy"], o.detach().bfloat16().float().numpy())
    # running_mean | running_var in full (num_batches_tracked is no float buffer)
    assert np.array_equal(a["bn_running_stats.npy"], torch.cat([m[1].running_mean, m[1].running_var]).numpy())
    # Linear(300, 200).weight has 60000 > 2000 elements: sampled; the other five tensors are whole
    n_whole = 200 + 200 + 200 + 8 * 200 + 8
    assert a["params_sample.npy"].shape == a["grads_sample.npy"].shape == (2000 + n_whole,)
    w, g = m[0].weight.detach().reshape(-1).numpy(), m[0].weight.grad.reshape(-1).numpy()
    # the sampled positions, read back from the values
    idx = np.rint((a["params_sample.npy"][:2000].astype(np.float64) + 0.5) * 65536).astype(np.int64)
    assert idx.min() >= 0 and idx.max() < 60000 and len(set(idx.tolist())) > 1900
    assert np.array_equal(w[idx], a["params_sample.npy"][:2000])
    assert np.array_equal(a["grads_sample.npy"][:2000], g[idx])  # the gradient is sampled at the same positions
    assert np.array_equal(a["params_sample.npy"][2000:2200], m[0].bias.detach().numpy())
    assert np.array_equal(a["grads_sample.npy"][-8:], m[2].bias.grad.numpy())


def test_steps_below_one_is_refused():
    import subprocess
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 2 and "--steps must be at least 1" in r.stderr
