"""removePrimers under the emulator (tests/primer_cases.py, emu_run): the product's own host code - the four patterns and their
plane selectors, the pieces and the two slots, the FASTQ reader and the writer with its reverse-complemented records and gzip
members - and k_primers run on the CPU, held to the cases of the GPU tests.  No case here makes a block take a second read (that
is tests/test_gpu_primers.py's batch past one piece and one sweep of the grid).  All of it in a subprocess with dada2_amd._lib
pointed at the emulated library, as in tests/test_emu_filter.py."""
import os
import subprocess
import sys

import pytest

from test_emu import CXX, ROOT, emu_lib  # noqa: F401  (the module-scoped fixture that builds the emulated library)

pytestmark = pytest.mark.skipif(not os.path.exists(CXX), reason="no host clang++ for the emulator build")


def test_emulated_remove_primers(emu_lib):   # noqa: F811
    code = (
        "import sys\n"
        "sys.path[:0] = [%r, %r]\n"
        "from dada2_amd import _lib\n"
        "_lib.LIB_PATH = %r\n"
        "import primer_cases as pc\n"
        "print(pc.emu_run())\n"
    ) % (ROOT, os.path.join(ROOT, "tests"), emu_lib)
    out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ), capture_output=True, text=True, timeout=900)
    assert out.returncode == 0 and out.stdout.startswith("ok "), out.stdout[-2000:] + out.stderr[-4000:]
