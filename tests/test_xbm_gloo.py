"""losses._gather_ranks on CPU with the gloo backend at world size 2: what
CrossBatchMemory.enqueue puts into the ring under torch.distributed.run is every
rank's rows and ids, rank-major, and the same on both ranks."""
import torch
import torch.distributed as dist

from test_ddp_gloo import _run

R, D = 3, 4


def _rows(rank):
    return (torch.arange(R * D, dtype=torch.float32).reshape(R, D) + 100.0 * rank)


def _ids(rank):
    return torch.arange(R, dtype=torch.int64) + 10 * rank


def _gather(rank):
    import losses
    world = dist.get_world_size()
    rows, ids = losses._gather_ranks(_rows(rank), _ids(rank))
    want_rows = torch.cat([_rows(r) for r in range(world)])
    want_ids = torch.cat([_ids(r) for r in range(world)])
    assert rows.shape == (world * R, D) and rows.dtype == torch.float32 and torch.equal(rows, want_rows)
    assert ids.shape == (world * R,) and ids.dtype == torch.int64 and torch.equal(ids, want_ids)
    rows, ids = losses._gather_ranks(_rows(rank), None)  # no ids, on every rank alike
    assert ids is None and torch.equal(rows, want_rows)
    # identical on both ranks: rank 0's bytes, broadcast, are this rank's
    seen = rows.clone()
    dist.broadcast(seen, src=0)
    assert torch.equal(seen, rows)


def test_gather_ranks_is_rank_major_and_identical_on_both_ranks():
    _run(_gather, world=2)
