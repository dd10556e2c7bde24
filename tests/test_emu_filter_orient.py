"""orient.fwd and matchIDs under the emulator (tests/filter_orient_cases.py, emu_run): the product's own host code - the barcode,
the oriented call through the two-slot pipeline, the chunk loop of dada2hip_filter_fastq_oriented and _paired_ex with its two
puts, its swapped pairs, the id split, the join and the remainders - and k_filter_orient and the oriented instances of
k_filter_scan, k_filter_ee and k_filter_kmers run on the CPU.  No case here makes a wave take a second read (that is
tests/test_gpu_filter_orient.py's batch of 131 073).  In a subprocess with dada2_amd._lib pointed at the emulated library, as
tests/test_emu_filter.py does."""
import os
import subprocess
import sys

import pytest

from test_emu import CXX, ROOT, emu_lib  # noqa: F401  (the module-scoped fixture that builds the emulated library)

pytestmark = pytest.mark.skipif(not os.path.exists(CXX), reason="no host clang++ for the emulator build")


def test_emulated_orient_and_match_ids(emu_lib):   # noqa: F811
    code = (
        "import sys\n"
        "sys.path[:0] = [%r, %r]\n"
        "from dada2_amd import _lib\n"
        "_lib.LIB_PATH = %r\n"
        "import filter_orient_cases as oc\n"
        "print(oc.emu_run())\n"
    ) % (ROOT, os.path.join(ROOT, "tests"), emu_lib)
    out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ), capture_output=True, text=True, timeout=900)
    assert out.returncode == 0 and out.stdout.startswith("ok "), out.stdout[-2000:] + out.stderr[-4000:]
