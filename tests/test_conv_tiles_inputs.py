"""A condition on the INPUTS of the conv-tile parity tests (test_conv_straddle_gpu.py,
test_conv_persistent_gpu.py, test_rstream_edges_gpu.py), checked on the CPU: in every case, taking
any single wave slice (64 pixels; 16 for rstream) out of the float64 sums, or crediting it to the
neighbouring segment, must move at least one checked sum of one channel by more than 4 x its bar —
so a kernel that dropped, doubled or misfiled one wave's share of one tile cannot pass.  A case that
missed this would get a per-channel offset or smaller segments, never a wider bar."""
import pytest

import _convref as cr
import test_conv_persistent_gpu as persistent
import test_conv_straddle_gpu as straddle
import test_rstream_edges_gpu as rstream

PROBLEMS = straddle.PROBLEMS + rstream.PROBLEMS + persistent.PROBLEMS


@pytest.mark.parametrize("kind,key", PROBLEMS, ids=lambda v: v if isinstance(v, str) else cr.ident(v))
def test_one_wave_slice_moves_a_sum_past_four_bars(kind, key):
    p = cr.PROBLEM_TYPES[kind](key)
    r = cr.sensitivity(p.term_sets(), p.G, p.slice_px)
    print(f"SENSITIVITY {kind} {cr.ident(key)}: min over slices of max |slice sum| / (4 bar) = {r:.3e}")
    assert r > 1.0, r
