"""Host-code AddressSanitizer check of artsbir_block_out_conv1x1_fwd's argument
checks: tests/asan/block_conv1_asan.cpp, a stand-alone program linked against
the sanitized library of `make -C art-sbir_amd asan` (built by
__graft_entry__.build(), like tests/test_asan_host.py's).  It runs without a
GPU: every call is rejected before a launch."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "art-sbir_amd", "build_asan", "block_conv1_asan")


@pytest.mark.skipif(not os.path.exists(EXE), reason="ASan build absent: make -C art-sbir_amd asan")
def test_block_conv1_argument_checks_under_asan():
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1")
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "asan block_conv1 ok" in r.stdout
