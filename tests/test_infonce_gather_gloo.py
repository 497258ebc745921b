"""losses.info_nce(gather=True) / losses.InfoNCELoss(gather=True) over CPU gloo at world 2
and 4: the protocol code itself (one all-gather of cat(p, n), the pool call at
pos0 = rank 2B, the backward's sum of the gathered rows' gradients over the ranks and this
rank's slice of it, the ring fed with the gathered rows) with the float64 restatement
tests/_infonce_pool_ref.py standing in for the kernel and a numpy ring (tests/_xbm_ref.py)
for the device ring, against torch float64 autograd of sum_s loss_s."""
import numpy as np
import pytest
import torch
import torch.distributed as dist

import _infonce_pool_ref as pref
import _xbm_ref as xref
from test_ddp_gloo import _run

D, M, TAU = 6, 8, 0.07


def _rank_rows(r, B):
    """rank r's (a, p, n, ids): seeded per rank; rank 1's n[0] carries the photo of rank 0's p[0]"""
    rng = np.random.default_rng(100 + r)
    a = rng.standard_normal((B, D)).astype(np.float32)
    p = (a + 3.0 * rng.standard_normal((B, D))).astype(np.float32)
    n = rng.standard_normal((B, D)).astype(np.float32)
    ids = np.arange(1000 * r, 1000 * r + 2 * B, dtype=np.int64)
    if r == 1:
        ids[B] = 0
    return a, p, n, ids


def _ring0():
    """the ring before the step: 5 of 8 slots filled, slot 3 the photo of rank 0's anchor 1"""
    rng = np.random.default_rng(7)
    ring = xref.Ring(M, D)
    ring.enqueue(rng.standard_normal((5, D)).astype(np.float32), np.array([50, 51, 52, 1, 54], np.int64))
    return ring


class _CpuMemory:
    """stands in for losses.CrossBatchMemory on the CPU: the ring rule of tests/_xbm_ref.py"""

    def __init__(self):
        self.ring, self.size, self.calls = _ring0(), M, []

    def enqueue(self, rows, ids=None, gathered=False):
        self.calls.append((tuple(rows.shape), bool(gathered)))
        self.ring.enqueue(rows.numpy(), None if ids is None else ids.numpy())


class _Hooks:
    """the kernel stand-in and counting wrappers of the two collectives"""

    def __init__(self):
        self.kernel_calls, self.gathers, self.reduces = [], 0, 0

    def kernel(self, a, cand, pos0, temperature, cand_ids, memory, eps, with_grad):
        self.kernel_calls.append((tuple(a.shape), tuple(cand.shape), int(pos0), with_grad))
        ring = memory.ring if memory is not None else None
        r = pref.info_nce_pool(a.numpy(), cand.numpy(), int(pos0), temperature,
                               None if cand_ids is None else cand_ids.numpy(),
                               None if ring is None else ring.mem, None if ring is None else ring.ids,
                               0 if ring is None else ring.count, eps)
        t = lambda k: torch.from_numpy(np.asarray(r[k], np.float64))  # noqa: E731
        return t("loss"), t("rows"), t("q"), ((t("da"), t("dcand")) if with_grad else None)

    def all_gather(self, rows, ids):
        import losses
        self.gathers += 1
        return losses._gather_ranks(rows.double(), ids)  # f64 through the collective: the restatement's own precision

    def reduce_rows(self, rows):
        import losses
        self.reduces += 1
        return losses._reduce_rows(rows)

    def kw(self):
        return dict(kernel=self.kernel, all_gather=self.all_gather, reduce_rows=self.reduce_rows)


def _gathered(rank, B, with_ids, with_ring):
    import losses
    world = dist.get_world_size()
    every = [_rank_rows(r, B) for r in range(world)]
    a, p, n, ids = every[rank]
    G = np.concatenate([np.concatenate([e[1], e[2]]) for e in every])
    ids_G = np.concatenate([e[3] for e in every]) if with_ids else None
    ring = _ring0() if with_ring else None
    ring_kw = dict(mem=ring.mem, mem_ids=ring.ids if with_ids else None, count=ring.count) if with_ring else {}

    hooks, memory = _Hooks(), (_CpuMemory() if with_ring else None)
    fn = losses.InfoNCELoss(TAU, memory=memory, gather=True, **hooks.kw())
    leaves = [torch.from_numpy(x.astype(np.float64)).requires_grad_(True) for x in (a, p, n)]
    tids = torch.from_numpy(ids) if with_ids else None
    loss = fn(*leaves, cand_ids=tids)
    assert hooks.gathers == 1 and hooks.reduces == 0
    assert hooks.kernel_calls == [((B, D), (world * 2 * B, D), rank * 2 * B, True)]

    # each rank's loss is the restatement's for its pos0
    own = pref.info_nce_pool(a, G, rank * 2 * B, TAU, ids_G, **ring_kw)
    assert abs(loss.item() - own["loss"]) <= 1e-12 * abs(own["loss"])

    # the ring: one copy of the gathered rows, the same bytes on every rank, no second gather
    if with_ring:
        assert memory.calls == [((world * 2 * B, D), True)] and hooks.gathers == 1
        want = _ring0()
        want.enqueue(G, ids_G)
        assert np.array_equal(memory.ring.mem, want.mem) and np.array_equal(memory.ring.ids, want.ids)
        assert np.array_equal(memory.ring.state(), want.state())
        blob = torch.from_numpy(np.concatenate([memory.ring.mem.view(np.int32).ravel(),
                                                memory.ring.ids.astype(np.int32), memory.ring.state().astype(np.int32)]))
        blobs = [torch.empty_like(blob) for _ in range(world)]
        dist.all_gather(blobs, blob)
        assert all(torch.equal(b, blob) for b in blobs)

    # rank-local gout: rank r scales its loss by r + 2, so the backward's sum must weigh
    # every rank's dG by that rank's own factor
    weights = np.arange(world) + 2.0
    (loss * float(weights[rank])).backward()
    assert hooks.reduces == 1 and hooks.gathers == 1
    a_all = np.concatenate([e[0] for e in every])
    _, per, da_all, dG = pref.global_loss_textbook(a_all, G, B, TAU, ids_G, weights=weights, **ring_kw)
    assert abs(per[rank] - loss.item()) <= 1e-12 * abs(per[rank])
    lo = rank * 2 * B
    for name, got, want in (("da", leaves[0].grad, da_all[rank * B:(rank + 1) * B]), ("dp", leaves[1].grad, dG[lo:lo + B]),
                            ("dn", leaves[2].grad, dG[lo + B:lo + 2 * B])):
        assert got.shape == (B, D), name
        assert np.abs(got.numpy() - want).max() <= 1e-12 * np.abs(want).max(), (rank, name)

    # under torch.no_grad() the call is local: no collective, the ring neither read nor written
    before = (hooks.gathers, hooks.reduces, len(hooks.kernel_calls), None if memory is None else list(memory.calls))
    with torch.no_grad():
        local = fn(*leaves, cand_ids=tids)
    assert (hooks.gathers, hooks.reduces) == before[:2] and len(hooks.kernel_calls) == before[2] + 1
    assert hooks.kernel_calls[-1][:3] == ((B, D), (2 * B, D), 0)
    assert memory is None or memory.calls == before[3]
    alone = pref.info_nce_pool(a, np.concatenate([p, n]), 0, TAU, ids if with_ids else None)
    assert abs(local.item() - alone["loss"]) <= 1e-12 * abs(alone["loss"])
    # and gather=False with gradients enabled is the local loss too
    loc = losses.info_nce(*leaves, temperature=TAU, cand_ids=tids, gather=False, **hooks.kw())
    assert hooks.gathers == before[0] and abs(loc.item() - alone["loss"]) <= 1e-12 * abs(alone["loss"])
    dist.barrier()


@pytest.mark.parametrize("B", [3, 5])
@pytest.mark.parametrize("world", [2, 4])
def test_gathered_protocol_with_ids_and_ring(world, B):
    _run(_gathered, B, True, True, world=world)


def test_gathered_protocol_without_ids_or_ring():
    _run(_gathered, 3, False, False, world=2)
