"""The edges of rstream_kernel's two-set software pipeline (candidate 26, rstream.hip): a workgroup walks
a chunk of 32 sixteen-pixel blocks two at a time (operand sets a and b), keeps the BN-backward sums in
registers and flushes them when the block's BN segment changes.

  N = 37, one segment     37 blocks: chunks of 32 and 5 — an odd count ends the loop on the a set
                          (`if (blk + 1 >= b1) break`), a short last chunk next to a full one; with
                          C = 512 four workgroups (the XCD remap inactive), with C = 256 two
  N = 12, four segments   of three images: boundaries at blocks 3, 6 and 9, so a segment changes on
                          the odd (b-set) block and on the even one; four is RS_NSEG
  N = 128, C = 512        eight workgroups: the XCD remap active
Inputs are 4x4 images (one block each), contiguous NHWC, K in {64, 128} channels of dY and C in
{256, 512} of dX; every case with the bf16 mask and the mask bits (kinds 0 and 3), one and two
targets, res_mode 1 and 2.  The predicate must refuse five segments, a segment of 24 pixels and
a C that is no whole number of 256-channel workgroups: another kernel runs and the result is still
right.  For C = 384 no route exists at all (the separate reduction pass the refusal falls back to takes
C / 8 dividing 256 only): the entry point must say so, not launch rstream_kernel; C = 128 shows the
same refusal with a fallback that runs.  Reference and bars: _convref.py."""
import pytest

import _convref as cr
import _hip
import _kernels

pytestmark = pytest.mark.gpu

EPILOGUES = [(kind, nt, rm) for kind in (0, 3) for nt in (1, 2) for rm in (1, 2)]
# N, G, H, W, C (dX / BN channels), K (dY channels)
SHAPES = ([(37, 1, 4, 4, C, K) for C in (256, 512) for K in (64, 128)]
          + [(12, 4, 4, 4, C, K) for C in (256, 512) for K in (64, 128)]
          + [(128, 1, 4, 4, 512, K) for K in (64, 128)])
CASES = [(N, G, H, W, C, K, 1, 0) + e for (N, G, H, W, C, K) in SHAPES for e in EPILOGUES]
REFUSED = [
    (10, 5, 4, 4, 256, 64, 1, 0, 3, 1, 1),    # five segments: one more than the LDS table holds
    (10, 5, 4, 4, 256, 128, 1, 0, 0, 2, 2),
    (4, 4, 4, 6, 256, 64, 1, 0, 3, 1, 1),     # segments of 24 pixels: not whole 16-pixel blocks
    (4, 4, 4, 6, 256, 64, 1, 0, 0, 2, 2),
    (12, 1, 4, 4, 128, 64, 1, 0, 3, 1, 1),    # C = 128: not whole 256-channel workgroups
    (12, 4, 4, 4, 128, 128, 1, 0, 0, 2, 2),
]
NO_ROUTE = [(12, 1, 4, 4, 384, 64, 1, 0, 3, 1, 1), (12, 4, 4, 4, 384, 128, 1, 0, 0, 2, 2)]
SLICE = 16  # a wave's step is one 16-pixel block
PROBLEMS = sorted(("bnb16", k) for k in CASES)


@pytest.mark.parametrize("key", CASES, ids=cr.ident)
def test_rstream_pipeline_edges(key, dev):
    cr.run_bnb(cr.Bnb(key, SLICE), "26", dev, f"rstream {cr.ident(key)}")


@pytest.mark.parametrize("key", REFUSED, ids=cr.ident)
def test_rstream_refusals(key, dev):
    cr.run_bnb(cr.Bnb(key, SLICE), "26", dev, f"rstream refused {cr.ident(key)}", refused=True)


@pytest.mark.parametrize("key", NO_ROUTE, ids=cr.ident)
def test_rstream_refuses_c384(key, dev):
    with pytest.raises(_hip.HipError, match="C=384 unsupported"):
        cr.run_bnb(cr.Bnb(key, SLICE), "26", dev, f"rstream refused {cr.ident(key)}", refused=True)
    assert not _kernels.last_kernel().startswith("rstream_kernel"), _kernels.last_kernel()
