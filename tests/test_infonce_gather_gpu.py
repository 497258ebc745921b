"""losses.info_nce(gather=True) and train.py --gather_negatives with two ranks on the real
kernels.  The test box has one GPU, so the two ranks share it over gloo
(ARTSBIR_DIST_BACKEND, as tests/test_train_ddp_gpu.py): the collective code is the same
torch.distributed API RCCL serves in a real run, with all_reduce and a slice in place of
reduce_scatter_tensor.  The children are spawned (never exec'ed), each joined under its own
time limit; a child that does not exit 0 fails the test there."""
import hashlib
import os
import socket

import numpy as np
import pytest
import torch.multiprocessing as mp

import _infonce_pool_ref as pref
from _tail import check_f32

pytestmark = pytest.mark.gpu

WORLD, B, D, M, FILLED, TAU = 2, 33, 65, 64, 40, 0.07
TRAIN = ["--layers", "1,1,1,1", "--width", "16", "--resolution", "64", "--output_dim", "32", "-b", "4",
         "--synthetic_n", "40", "-e", "1", "--no_save", "--negatives", "all", "--loss_type", "cosine",
         "--gather_negatives", "--memory_size", "64"]


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _setup(rank, port, tmp):
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "art-sbir_amd"))
    sys.path.insert(0, root)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), WORLD_SIZE=str(WORLD), RANK=str(rank),
                      LOCAL_RANK=str(rank), ARTSBIR_DIST_BACKEND="gloo")
    os.chdir(tmp)


def _spawn(target, tmp, limit):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=target, args=(r, port, str(tmp), q)) for r in range(WORLD)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(timeout=limit)
    codes = [p.exitcode for p in procs]
    for p in procs:
        if p.exitcode is None:
            p.kill()
    assert codes == [0] * WORLD, codes
    return [v[1:] for v in sorted((q.get(timeout=5) for _ in range(WORLD)), key=lambda v: v[0])]


def _rank_rows(r):
    """rank r's (a, p, n, ids); rank 1's n[2] carries the photo of rank 0's anchor 4"""
    rng = np.random.default_rng(300 + r)
    a = rng.standard_normal((B, D)).astype(np.float32)
    p = (a + 3.0 * rng.standard_normal((B, D))).astype(np.float32)
    n = rng.standard_normal((B, D)).astype(np.float32)
    ids = np.arange(1000 * r, 1000 * r + 2 * B, dtype=np.int64)
    if r == 1:
        ids[B + 2] = 4
    return a, p, n, ids


def _ring_rows():
    """the ring before the step, the same on every rank; slot 7 is the photo of rank 1's anchor 0"""
    rng = np.random.default_rng(9)
    ids = np.arange(5000, 5000 + FILLED, dtype=np.int64)
    ids[7] = 1000
    return rng.standard_normal((FILLED, D)).astype(np.float32), ids


def _loss_entry(rank, port, tmp, q):
    _setup(rank, port, tmp)
    import torch
    import torch.distributed as dist
    import ddp
    import losses
    ddp.init_distributed()
    try:
        dev = torch.device("cuda", torch.cuda.current_device())
        a, p, n, ids = _rank_rows(rank)
        memory = losses.CrossBatchMemory(M, D, device=dev)
        ring, ring_ids = _ring_rows()
        memory.enqueue(torch.from_numpy(ring).to(dev), torch.from_numpy(ring_ids).to(dev), gathered=True)  # no collective
        leaves = [torch.from_numpy(x).to(dev).requires_grad_(True) for x in (a, p, n)]
        loss = losses.info_nce(*leaves, temperature=TAU, cand_ids=torch.from_numpy(ids).to(dev), memory=memory, gather=True)
        (loss * float(rank + 2)).backward()  # a rank-local gout
        with torch.no_grad():  # the eval loss stays local and touches no collective
            local = losses.info_nce(*leaves, temperature=TAU, cand_ids=torch.from_numpy(ids).to(dev), gather=True)
        torch.cuda.synchronize()
        q.put((rank, loss.item(), local.item(), [t.grad.cpu().numpy() for t in leaves], memory.filled()))
    finally:
        if dist.is_initialized():
            dist.destroy_process_group()


def test_gathered_loss_and_gradients_world2(tmp_path):
    res = _spawn(_loss_entry, tmp_path, 120)
    every = [_rank_rows(r) for r in range(WORLD)]
    G = np.concatenate([np.concatenate([e[1], e[2]]) for e in every])
    ids_G = np.concatenate([e[3] for e in every])
    ring, ring_ids = _ring_rows()
    mem = np.zeros((M, D), np.float32)
    mem[:FILLED] = ring
    mids = np.full(M, -1, np.int64)
    mids[:FILLED] = ring_ids
    calls = {dt: [pref.info_nce_pool(every[r][0], G, r * 2 * B, TAU, ids_G, mem, mids, FILLED, dtype=dt)
                  for r in range(WORLD)] for dt in (np.float64, np.float32)}
    # d(sum_s (s + 2) loss_s) / d(rank r's rows): the weighted sum of the ranks' dG, in either precision
    dG = {dt: sum(dt(s + 2) * c["dcand"] for s, c in enumerate(cs)) for dt, cs in calls.items()}
    for r, (loss, local, (da, dp, dn), filled) in enumerate(res):
        c64, c32 = calls[np.float64][r], calls[np.float32][r]
        check_f32(f"gather world2 rank{r} loss", np.array([loss]), np.array([c64["loss"]]), np.array([c32["loss"]]))
        check_f32(f"gather world2 rank{r} da", da, (r + 2) * c64["da"], np.float32(r + 2) * c32["da"])
        lo = r * 2 * B
        check_f32(f"gather world2 rank{r} dp", dp, dG[np.float64][lo:lo + B], dG[np.float32][lo:lo + B])
        check_f32(f"gather world2 rank{r} dn", dn, dG[np.float64][lo + B:lo + 2 * B], dG[np.float32][lo + B:lo + 2 * B])
        alone = [pref.info_nce_pool(every[r][0], G[lo:lo + 2 * B], 0, TAU, every[r][3], dtype=dt)["loss"]
                 for dt in (np.float64, np.float32)]
        check_f32(f"gather world2 rank{r} no_grad loss", np.array([local]), np.array([alone[0]]), np.array([alone[1]]))
        assert filled == FILLED  # info_nce alone does not feed the ring
    # the planted collisions carry weight
    assert calls[np.float64][0]["loss"] != pref.info_nce_pool(every[0][0], G, 0, TAU, None, mem, None, FILLED)["loss"]


def _train_entry(rank, port, tmp, q):
    _setup(rank, port, tmp)
    import torch
    import torch.distributed as dist
    import losses
    import train
    seen, counts = [], dict(gather=0, reduce=0)
    inner_train, inner_gather, inner_reduce = train.triplet_train, losses._gather_ranks, losses._reduce_rows

    def keep_model(model, *a, **kw):
        seen.append(model)
        return inner_train(model, *a, **kw)

    def count_gather(rows, ids):
        counts["gather"] += 1
        return inner_gather(rows, ids)

    def count_reduce(rows):
        counts["reduce"] += 1
        return inner_reduce(rows)

    train.triplet_train, losses._gather_ranks, losses._reduce_rows = keep_model, count_gather, count_reduce
    try:
        training, _ = train.main(TRAIN)
        flat = torch.cat([p.detach().float().reshape(-1) for p in seen[0].parameters()]).cpu().numpy()
        # a digest, not the weights: a child that has put more than a pipe's buffer into the
        # queue does not exit until the parent reads it, and the parent joins first
        q.put((rank, hashlib.sha256(flat.tobytes()).hexdigest(), bool(np.isfinite(flat).all()), flat.size,
               training["train_losses"][0], counts))
    finally:
        if dist.is_initialized():
            dist.destroy_process_group()


def test_train_main_world2_gather_negatives(tmp_path):
    (w0, ok0, n0, l0, c0), (w1, ok1, n1, l1, c1) = _spawn(_train_entry, tmp_path, 240)
    assert np.isfinite(l0) and np.isfinite(l1)
    assert ok0 and ok1 and n0 == n1 > 0 and w0 == w1  # finite, and the same bytes on both ranks
    # one all-gather and one backward collective per training step, the same on both ranks;
    # the ring is fed with the gathered rows (no gather of its own)
    assert c0 == c1 and c0["gather"] == c0["reduce"] > 0
