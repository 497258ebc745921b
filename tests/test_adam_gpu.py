"""optim.Adam (the one-launch artsbir_adam_step of csrc/loss_optim.hip) past its
first step: the three torch.optim.Adam steps recorded in tests/golden/loss_adam.npz,
ten steps over many tensors whose sizes sit on the 4096-element chunk edges with
non-default betas / eps and with and without weight decay (float64
oracle.numpy_ref.adam_step as the reference, torch.optim.Adam on CPU f32 clones as
the yardstick, tests/_tail.py's bar), sentinel gaps around every parameter and
gradient, optimizer state_dicts exchanged with torch.optim.Adam in both
directions, and parameters without a gradient."""
import copy
import os

import numpy as np
import pytest
import torch

from _tail import check_f32, f64
from oracle import numpy_ref

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "loss_adam.npz")


def _check_golden(p, opt, gold):
    st = opt.state[p]
    # the bars tests/test_oracle.py holds the float64 restatement to on this fixture
    np.testing.assert_allclose(p.detach().cpu().numpy(), gold["w3"], rtol=0, atol=2e-6)
    np.testing.assert_allclose(st["exp_avg"].cpu().numpy(), gold["m3"], rtol=0, atol=1e-6)
    np.testing.assert_allclose(st["exp_avg_sq"].cpu().numpy(), gold["v3"], rtol=1e-4, atol=1e-8)
    assert float(st["step"]) == 3.0


def test_golden_three_steps_same_pointers(dev):
    """p.grad.copy_(): every pointer stays, the block table is built once and reused"""
    import optim
    gold = np.load(GOLDEN)
    p = torch.nn.Parameter(torch.from_numpy(gold["w0"]).to(dev))
    opt = optim.Adam([p], lr=1e-3, weight_decay=0.002)
    p.grad = torch.zeros_like(p)
    entries = []
    for s in range(3):
        p.grad.copy_(torch.from_numpy(gold["grads"][s]))
        opt.step()
        entries.append(opt._tables[id(opt.param_groups[0])][1])
    torch.cuda.synchronize()
    assert entries[1] is entries[0] and entries[2] is entries[0]  # the cache hit
    _check_golden(p, opt, gold)


def test_golden_three_steps_fresh_gradients(dev):
    """a new p.grad tensor every step (the earlier ones kept alive, so the address
    differs) and zero_grad(set_to_none=True) in between: the table must be rebuilt"""
    import optim
    gold = np.load(GOLDEN)
    p = torch.nn.Parameter(torch.from_numpy(gold["w0"]).to(dev))
    opt = optim.Adam([p], lr=1e-3, weight_decay=0.002)
    alive, ptrs, entries = [], [], []
    for s in range(3):
        g = torch.from_numpy(gold["grads"][s]).to(dev)
        alive.append(g)
        ptrs.append(g.data_ptr())
        p.grad = g
        opt.step()
        entries.append(opt._tables[id(opt.param_groups[0])][1])
        opt.zero_grad(set_to_none=True)
        assert p.grad is None
    torch.cuda.synchronize()
    assert len(set(ptrs)) == 3
    assert entries[1] is not entries[0] and entries[2] is not entries[1]
    for s in range(3):  # step() leaves the gradients as they were
        assert torch.equal(alive[s].cpu(), torch.from_numpy(gold["grads"][s]))
    _check_golden(p, opt, gold)


# ------------------------------------------------------- many tensors, chunk edges
SHAPES = [(1,), (7,), (4095,), (4096,), (4097,), (3 * 4096 + 5,), (33, 129), (0,)]
GAP = 4096 + 37  # sentinel elements before, between and after the tensors: more than one chunk
P_SENT, G_SENT = 12345.678, -8765.4321


def _flat_views(fill, dev):
    """one flat buffer holding every tensor of SHAPES with GAP sentinels around each:
    -> buffer, [views], bool mask of the sentinel positions"""
    numels = [int(np.prod(s)) for s in SHAPES]
    total = GAP + sum(n + GAP for n in numels)
    buf = torch.full((total,), fill, dtype=torch.float32, device=dev)
    mask = torch.ones(total, dtype=torch.bool)
    views, off = [], GAP
    for s, n in zip(SHAPES, numels):
        views.append(buf[off:off + n].view(s))
        mask[off:off + n] = False
        off += n + GAP
    return buf, views, mask.to(dev)


def _cat(ts):
    """the one launch's output: every tensor's elements in one f64 vector.  The bar is
    taken over it, not per tensor: exp_avg is a difference of terms that can cancel
    far below its operands, and in a tensor of one or seven elements neither
    max|ref64| nor the torch yardstick's error is a population to measure against"""
    return np.concatenate([f64(t).reshape(-1) for t in ts])


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("weight_decay", [0.0, 0.01], ids=["wd0", "wd0.01"])
def test_many_tensors_ten_steps(weight_decay, dev):
    import optim
    assert optim.CHUNK == 4096 and GAP > optim.CHUNK
    hp = dict(lr=3e-3, betas=(0.8, 0.95), eps=1e-6, weight_decay=weight_decay)
    rng = np.random.default_rng(2024)
    w0 = [rng.normal(0, 1, s).astype(np.float32) for s in SHAPES]
    pbuf, pviews, pmask = _flat_views(P_SENT, dev)
    gbuf, gviews, gmask = _flat_views(G_SENT, dev)
    params = []
    for v, w in zip(pviews, w0):
        v.copy_(torch.from_numpy(w))
        params.append(torch.nn.Parameter(v))
    for p, v, gv in zip(params, pviews, gviews):
        assert p.data_ptr() == v.data_ptr()
        p.grad = gv
    opt = optim.Adam(params, **hp)
    cpu = [torch.nn.Parameter(torch.from_numpy(w).clone()) for w in w0]
    topt = torch.optim.Adam(cpu, **hp)
    w64 = [w.astype(np.float64) for w in w0]
    m64 = [np.zeros(s) for s in SHAPES]
    v64 = [np.zeros(s) for s in SHAPES]
    f32_eps = float(np.float32(hp["eps"]))  # the kernel takes f32 hyper-parameters
    b1, b2 = (float(np.float32(b)) for b in hp["betas"])
    nblocks = sum((int(np.prod(s)) + optim.CHUNK - 1) // optim.CHUNK for s in SHAPES)
    for step in range(1, 11):
        grads = [rng.normal(0, 1, s).astype(np.float32) for s in SHAPES]
        for gv, cp, g in zip(gviews, cpu, grads):
            gv.copy_(torch.from_numpy(g))
            cp.grad = torch.from_numpy(g).clone()
        g_before = gbuf.clone()
        opt.step()
        topt.step()
        torch.cuda.synchronize()
        assert torch.equal(_bits(gbuf), _bits(g_before)), "step() changed a gradient or its surroundings"
        assert opt._tables[id(opt.param_groups[0])][1][2] == nblocks
        for i, s in enumerate(SHAPES):
            w64[i], m64[i], v64[i] = numpy_ref.adam_step(
                w64[i], grads[i].astype(np.float64), m64[i], v64[i], step, lr=float(np.float32(hp["lr"])),
                wd=float(np.float32(weight_decay)), b1=b1, b2=b2, eps=f32_eps)
            st = opt.state[params[i]]
            assert st["exp_avg"].shape == params[i].shape and st["exp_avg_sq"].shape == params[i].shape
            assert float(st["step"]) == step
        quiet = step != 10  # the table keeps the last step; every step is asserted
        tag = f"adam 8 tensors wd={weight_decay} step {step}"
        check_f32(f"{tag} param", _cat(params), _cat(w64), _cat(cpu), quiet)
        for key, ref in (("exp_avg", m64), ("exp_avg_sq", v64)):
            check_f32(f"{tag} {key}", _cat(opt.state[p][key] for p in params), _cat(ref),
                      _cat(topt.state[c][key] for c in cpu), quiet)
    # every sentinel around the parameters and the gradients is bit-unchanged
    assert torch.equal(_bits(pbuf[pmask]), _bits(torch.full_like(pbuf[pmask], P_SENT)))
    assert torch.equal(_bits(gbuf[gmask]), _bits(torch.full_like(gbuf[gmask], G_SENT)))
    # and the parameters moved
    assert all(not np.allclose(p.detach().cpu().numpy(), w) for p, w in zip(params[:-1], w0[:-1]))


# ----------------------------------------------------------- state interchange
def _three_steps(make_opt, params, grads):
    opt = make_opt(params)
    for s in range(3):
        for p, g in zip(params, grads[s]):
            p.grad = g.to(p.device).clone()
        opt.step()
    return opt


def _interchange_data():
    rng = np.random.default_rng(77)
    shapes = [(5,), (4097,), (3, 11)]
    w0 = [torch.from_numpy(rng.normal(0, 1, s).astype(np.float32)) for s in shapes]
    grads = [[torch.from_numpy(rng.normal(0, 1, s).astype(np.float32)) for s in shapes] for _ in range(4)]
    return w0, grads


HP = dict(lr=2e-3, betas=(0.85, 0.97), eps=1e-7, weight_decay=0.01)


def _ref_four_steps(w0, grads):
    out = []
    for i, w in enumerate(w0):
        w, m, v = w.numpy().astype(np.float64), np.zeros(w.shape), np.zeros(w.shape)
        for s in range(4):
            w, m, v = numpy_ref.adam_step(w, grads[s][i].numpy().astype(np.float64), m, v, s + 1,
                                          lr=float(np.float32(HP["lr"])), wd=float(np.float32(HP["weight_decay"])),
                                          b1=float(np.float32(HP["betas"][0])), b2=float(np.float32(HP["betas"][1])),
                                          eps=float(np.float32(HP["eps"])))
        out.append((w, m, v))
    return out


def _check_step4(tag, opt, params, ref, yard_opt, yard_params):
    assert all(float(opt.state[p]["step"]) == 4.0 for p in params)
    check_f32(f"{tag} param", _cat(params), _cat(r[0] for r in ref), _cat(yard_params))
    for k, key in ((1, "exp_avg"), (2, "exp_avg_sq")):
        check_f32(f"{tag} {key}", _cat(opt.state[p][key] for p in params), _cat(r[k] for r in ref),
                  _cat(yard_opt.state[p][key] for p in yard_params))


def _torch_four_steps(w0, grads):
    cpu = [torch.nn.Parameter(w.clone()) for w in w0]
    topt = _three_steps(lambda ps: torch.optim.Adam(ps, **HP), cpu, grads)
    for p, g in zip(cpu, grads[3]):
        p.grad = g.clone()
    topt.step()
    return topt, cpu


def test_torch_adam_loads_hip_state_dict(dev):
    """three HIP steps, then torch.optim.Adam over CPU clones loads the HIP optimizer's
    state_dict(); both take step 4 on the same gradient"""
    import optim
    w0, grads = _interchange_data()
    params = [torch.nn.Parameter(w.to(dev)) for w in w0]
    opt = _three_steps(lambda ps: optim.Adam(ps, **HP), params, grads)
    cpu = [torch.nn.Parameter(p.detach().cpu().clone()) for p in params]
    topt = torch.optim.Adam(cpu, lr=1.0)  # every hyper-parameter comes from the loaded state
    topt.load_state_dict(copy.deepcopy(opt.state_dict()))  # as a saved checkpoint: nothing shared
    for p in cpu:
        assert topt.state[p]["exp_avg"].device.type == "cpu" and float(topt.state[p]["step"]) == 3.0
    assert topt.param_groups[0]["lr"] == HP["lr"] and tuple(topt.param_groups[0]["betas"]) == HP["betas"]
    for p, c, g in zip(params, cpu, grads[3]):
        p.grad = g.to(dev)
        c.grad = g.clone()
    opt.step()
    topt.step()
    torch.cuda.synchronize()
    ref = _ref_four_steps(w0, grads)
    yard_opt, yard = _torch_four_steps(w0, grads)
    _check_step4("adam hip->torch: hip", opt, params, ref, yard_opt, yard)
    _check_step4("adam hip->torch: torch on hip state", topt, cpu, ref, yard_opt, yard)


def test_hip_adam_loads_torch_state_dict(dev):
    """the other direction: a fresh optim.Adam loads a torch optimizer's three-step state_dict()"""
    import optim
    w0, grads = _interchange_data()
    cpu = [torch.nn.Parameter(w.clone()) for w in w0]
    topt = _three_steps(lambda ps: torch.optim.Adam(ps, **HP), cpu, grads)
    params = [torch.nn.Parameter(c.detach().to(dev)) for c in cpu]
    opt = optim.Adam(params, lr=1.0)
    opt.load_state_dict(copy.deepcopy(topt.state_dict()))
    for p in params:
        assert opt.state[p]["exp_avg"].is_cuda and opt.state[p]["exp_avg_sq"].is_cuda
    for p, g in zip(params, grads[3]):
        p.grad = g.to(dev)
    opt.step()
    torch.cuda.synchronize()
    ref = _ref_four_steps(w0, grads)
    yard_opt, yard = _torch_four_steps(w0, grads)
    _check_step4("adam torch->hip", opt, params, ref, yard_opt, yard)


# ------------------------------------------------- skipped and late parameters
def test_parameter_without_gradient_is_skipped_and_a_late_one_raises(dev):
    import optim
    rng = np.random.default_rng(3)
    a0, b0 = (torch.from_numpy(rng.normal(0, 1, 100).astype(np.float32)) for _ in range(2))
    a, b = torch.nn.Parameter(a0.to(dev)), torch.nn.Parameter(b0.to(dev))
    opt = optim.Adam([a, b], lr=1e-2)
    for _ in range(2):
        a.grad = torch.from_numpy(rng.normal(0, 1, 100).astype(np.float32)).to(dev)
        opt.step()
    torch.cuda.synchronize()
    assert torch.equal(b.detach().cpu(), b0) and len(opt.state[b]) == 0  # untouched, no state
    assert not torch.equal(a.detach().cpu(), a0) and float(opt.state[a]["step"]) == 2.0
    # torch.optim.Adam would start b at its own step 1; the one-launch kernel has one
    # bias correction per group, so this is refused (documented in optim.py)
    a.grad = torch.ones_like(a)
    b.grad = torch.ones_like(b)
    with pytest.raises(RuntimeError, match="different Adam steps"):
        opt.step()
