"""The sequence-table stage under the emulator (tests/collapse_cases.py, emu_run): the product's own k_collapse_join,
k_collapse_scan, pair-form lane aligner and host orchestration run on the CPU, in a subprocess with dada2_amd._lib pointed at the
emulated library as in tests/test_emu_host_ends.py - collapse_pairs against the fixture's brute-force scan, the whole function
in batches of 8 against the plain-C restatement, nweval / nwhamming against the fixture's reference triples."""
import os
import subprocess
import sys

import pytest

from test_emu import CXX, ROOT, emu_lib  # noqa: F401  (the module-scoped fixture that builds the emulated library)

pytestmark = pytest.mark.skipif(not os.path.exists(CXX), reason="no host clang++ for the emulator build")


def test_emulated_collapse_pairs_whole_function_and_nweval(emu_lib):   # noqa: F811
    code = (
        "import sys\n"
        "sys.path[:0] = [%r, %r]\n"
        "from dada2_amd import _lib\n"
        "_lib.LIB_PATH = %r\n"
        "import collapse_cases as cc\n"
        "print(cc.emu_run())\n"
    ) % (ROOT, os.path.join(ROOT, "tests"), emu_lib)
    out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ), capture_output=True, text=True, timeout=900)
    assert out.returncode == 0 and out.stdout.startswith("ok "), out.stdout[-2000:] + out.stderr[-4000:]


def test_emulated_collapse_wraps_the_aligner_scratch_ring(emu_lib):   # noqa: F811
    """collapse_cases.ring_run: more than 512 pairs in one call of the pair-form lane aligner under DADA2HIP_NW_RING=4, the table
    against the restatement over the plain-C oracle, and the knob changes nothing."""
    code = (
        "import sys\n"
        "sys.path[:0] = [%r, %r]\n"
        "from dada2_amd import _lib\n"
        "_lib.LIB_PATH = %r\n"
        "import collapse_cases as cc\n"
        "from dada2_amd import api\n"
        "from oracle import cport\n"
        "print('ring: ok', cc.ring_run(api, cport))\n"
    ) % (ROOT, os.path.join(ROOT, "tests"), emu_lib)
    out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ), capture_output=True, text=True, timeout=900)
    assert out.returncode == 0 and out.stdout.startswith("ring: ok "), out.stdout[-2000:] + out.stderr[-4000:]
