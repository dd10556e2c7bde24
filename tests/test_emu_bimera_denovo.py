"""isBimeraDenovo under the emulator (tests/bimera_denovo_cases.py, emu_run): k_bimera_worklist and k_bimera_fold run on the CPU on
arrays made up by hand - work lists against their definition, five-word records folded against a Python fold of chimera.cpp:29-50,
with maxima and flags carried in from earlier windows, empty slots, tossed parents and the compaction of the live list - and then
the product's own host code end to end on small cases: both aligner routes, a slot budget of one chunk, the per-sample table and
isShiftDenovo.  In a subprocess with dada2_amd._lib pointed at the emulated library, as tests/test_emu_pool.py does."""
import os
import subprocess
import sys

import pytest

from test_emu import CXX, ROOT, emu_lib  # noqa: F401  (the module-scoped fixture that builds the emulated library)

pytestmark = pytest.mark.skipif(not os.path.exists(CXX), reason="no host clang++ for the emulator build")


def test_emulated_worklist_fold_and_small_cases(emu_lib):   # noqa: F811
    code = (
        "import sys\n"
        "sys.path[:0] = [%r, %r]\n"
        "from dada2_amd import _lib\n"
        "_lib.LIB_PATH = %r\n"
        "import bimera_denovo_cases as bc\n"
        "print(bc.emu_run())\n"
    ) % (ROOT, os.path.join(ROOT, "tests"), emu_lib)
    out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ), capture_output=True, text=True, timeout=900)
    assert out.returncode == 0 and out.stdout.startswith("ok"), out.stdout[-2000:] + out.stderr[-4000:]
