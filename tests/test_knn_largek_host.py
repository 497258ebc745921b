"""Host-side checks of the large-k retrieval path (no GPU): the workspace query of
artsbir_pairwise_l2_topk accepts k up to 1024, the new entry points are declared on
both sides of the boundary, and knn.py names the limit."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "artsbir.h")
NEW = ("artsbir_knn_set_cand_cap", "artsbir_knn_largek_stat_read", "artsbir_knn_exact_keys")


def test_workspace_accepts_large_k_and_grows_with_it():
    import _hip
    lib = _hip.lib()
    small = lib.artsbir_pairwise_l2_topk_workspace(_hip.DT_BF16, 100, 20000, 512, 65, 0)
    large = lib.artsbir_pairwise_l2_topk_workspace(_hip.DT_BF16, 100, 20000, 512, 1024, 0)
    assert small > 0 and large > 0
    assert large > small


@pytest.mark.parametrize("k", [0, 1025])
def test_workspace_rejects_k_outside_the_range(k):
    import _hip
    lib = _hip.lib()
    assert lib.artsbir_pairwise_l2_topk_workspace(_hip.DT_BF16, 100, 20000, 512, k, 0) == -1
    assert b"1024" in lib.artsbir_last_error()


def test_new_entry_points_declared_on_both_sides():
    import _hip
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, src), name
        assert name in _hip.SIGNATURES, name
        assert hasattr(_hip.lib(), name), name


def test_cand_cap_hook_returns_the_old_limit_and_ignores_nonpositive():
    import _hip
    lib = _hip.lib()
    old = lib.artsbir_knn_set_cand_cap(8)
    try:
        assert old > 0
        assert lib.artsbir_knn_set_cand_cap(0) == 8    # cap <= 0 leaves it
        assert lib.artsbir_knn_set_cand_cap(-3) == 8
        # the capacity is part of the workspace layout: smaller buffers with the limit set
        limited = lib.artsbir_pairwise_l2_topk_workspace(_hip.DT_BF16, 100, 20000, 512, 100, 0)
    finally:
        assert lib.artsbir_knn_set_cand_cap(old) == 8
    assert lib.artsbir_pairwise_l2_topk_workspace(_hip.DT_BF16, 100, 20000, 512, 100, 0) > limited


def test_knn_limits():
    import knn
    assert knn.KMAX == 64
    assert knn.KMAX_LARGE == 1024
