"""The unforced path of the GEMM launchers (csrc/gemm.hip on csrc/tune.h): with
ARTSBIR_PGEMM_CFG / ARTSBIR_WGRAD_CFG unset, the first call of a shape that is in
no table times the candidates, stores its choice under the shape's key and
launches it; later calls launch the stored choice; ARTSBIR_TUNE=0 stores the
static choice without trial runs.  The trial runs of a weight gradient must go
to the scratch buffer: the caller's dW is accumulated into exactly once.

The table is process-wide and other tests add to it, so only the presence and
content of this file's own lines are asserted.  Shapes: a 1x1 convolution
(models.py:198 Bottleneck conv1 in miniature), 96 -> 40 channels, two images of
6 x 6 (tuned) and 10 x 10 (ARTSBIR_TUNE=0) pixels, bf16."""
import os

import pytest
import torch

import _hip
import _kernels
from test_tune_table_gpu import _close

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
N, C, COUT = 2, 96, 40
# convolution candidates (gemm.hip tune_conv) and the "none ran" value -2
CONV_CANDS = {-2, 0, 1, 2, 3, 4, 5, 10, 11, 12, 13, 14, 15, 16, 18, 19, 20, 21, 22, 24, 25, 26}
# weight-gradient candidates (gemm.hip tune_wgrad): the register-staged kernel,
# pwgrad_num_cfgs() = 9 tile shapes x 4 split levels + 4 halo variants
# (pwgrad.hip), pw256 at three split levels
WGRAD_CANDS = {-1} | set(range(40)) | {100, 101, 102}


@pytest.fixture
def unforced():
    keys = ("ARTSBIR_PGEMM_CFG", "ARTSBIR_WGRAD_CFG", "ARTSBIR_TUNE")
    old = {k: os.environ.pop(k, None) for k in keys}
    yield
    for k, v in old.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v


def _operands(hw, dev):
    gen = torch.Generator(device=dev).manual_seed(1000 + hw)
    x = torch.randn(N, hw, hw, C, device=dev, generator=gen).to(BF)
    w = (torch.randn(COUT, C, device=dev, generator=gen) * C ** -0.5).to(BF)
    dy = torch.randn(N * hw * hw, COUT, device=dev, generator=gen).to(BF)
    return x, w, dy


def _table_lines(tmp_path):
    path = str(tmp_path / "tune.txt")
    assert _hip.lib().artsbir_tune_save(path.encode()) == 0
    with open(path) as f:
        return f.read().splitlines()


def _entry(lines, prefix):
    """the choice of the one line that starts with prefix (a whole key)"""
    hits = [ln for ln in lines if ln.startswith(prefix)]
    assert len(hits) == 1, (prefix, hits)
    rest = hits[0][len(prefix):]
    assert rest.lstrip("-").isdigit(), hits[0]
    return int(rest)


def _conv(hw, dev):
    """y = conv1x1(x, w) through artsbir_conv2d_fwd, checked against the f64
    product of the bf16 operands; returns the kernel that ran"""
    x, w, _ = _operands(hw, dev)
    M = N * hw * hw
    y = torch.full((M, COUT), float("nan"), dtype=BF, device=dev)
    d = _hip.conv_desc(BF, N, hw, hw, C, COUT, 1, 1, 1, 0)
    _hip.call("artsbir_conv2d_fwd", d, x.data_ptr(), w.data_ptr(), y.data_ptr(), COUT, 0, 0, None, None, None, 0,
              None, _hip.stream())
    torch.cuda.synchronize()
    ref = x.reshape(M, C).double().cpu() @ w.double().cpu().T
    _close(y.double().cpu(), ref, f"conv {hw}x{hw}")
    return _kernels.last_kernel()


def _wgrad(hw, dev):
    """dW (zeroed) += dy^T x through artsbir_conv2d_wgrad against the f32 product.
    Every product of two bf16 values is exact in f32, so the two sides differ
    only in the order and rounding of 72 (or 200) f32 additions per element: at
    most (M - 1) roundings of one ulp (2^-23; the MFMA accumulator need not round
    to nearest) in the kernel and of half an ulp in the reference, each relative
    to a partial sum bounded by sum |dy| |x|.  A trial run that reached dW would
    be off by a whole multiple of the result."""
    x, _, dy = _operands(hw, dev)
    M = N * hw * hw
    dw = torch.zeros(COUT, C, device=dev)
    d = _hip.conv_desc(BF, N, hw, hw, C, COUT, 1, 1, 1, 0)
    _hip.call("artsbir_conv2d_wgrad", d, dy.data_ptr(), x.data_ptr(), None, None, 0, dw.data_ptr(), _hip.stream())
    torch.cuda.synchronize()
    xf, dyf, got = x.reshape(M, C).float().cpu(), dy.float().cpu(), dw.cpu()
    ref = dyf.T @ xf
    bound = (M - 1) * (2.0 ** -23 + 2.0 ** -24) * (dyf.abs().T @ xf.abs())
    excess = ((got - ref).abs() - bound).max().item()
    print(f"wgrad {hw}x{hw}: max |err| {(got - ref).abs().max().item():.3e}, min bound {bound.min().item():.3e}")
    assert excess <= 0, (hw, excess, _kernels.last_kernel())


def test_conv_first_call_tunes_and_stores_its_choice(dev, unforced, tmp_path):
    prefix = "c 72 6 6 96 40 1 1 1 0 6 6 0 0 1 0 "
    name = _conv(6, dev)
    lines = _table_lines(tmp_path)
    choice = _entry(lines, prefix)
    print("conv choice", choice, name)
    assert choice in CONV_CANDS, choice
    assert (choice == -2) == name.startswith("conv_gemm_kernel<"), (choice, name)
    assert _conv(6, dev) == name
    assert _entry(_table_lines(tmp_path), prefix) == choice


def test_wgrad_first_call_tunes_into_the_scratch_buffer(dev, unforced, tmp_path):
    _wgrad(6, dev)
    choice = _entry(_table_lines(tmp_path), "w 72 6 6 96 40 1 1 1 0 1 96 40 96 ")
    print("wgrad choice", choice, _kernels.last_kernel())
    assert choice in WGRAD_CANDS, choice
    _wgrad(6, dev)  # the stored choice: again one accumulation into a fresh dW


def test_tune_off_stores_the_static_choice(dev, unforced, tmp_path):
    os.environ["ARTSBIR_TUNE"] = "0"
    _conv(10, dev)
    _wgrad(10, dev)
    assert _kernels.last_kernel().startswith("wgrad_kernel<")
    lines = _table_lines(tmp_path)
    assert _entry(lines, "w 200 10 10 96 40 1 1 1 0 1 96 40 96 ") == -1
    assert _entry(lines, "c 200 10 10 96 40 1 1 1 0 10 10 0 0 1 0 ") in CONV_CANDS
