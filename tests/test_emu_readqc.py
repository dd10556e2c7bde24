"""The read diagnostics under the emulator (tests/readqc_cases.py, emu_run): the product's own host code - the pieces and the two
slots, a piece's table summed into the call's, the file reader without writers, the table that grows under later chunks, the two
numbers per read and the host's last word on them - and k_qprofile / k_complexity_win run on the CPU, held to the cases of the GPU
tests (the file cases in their lighter form).  No case here gives a block of k_qprofile a second group of reads per wave beyond a
few (that is tests/test_gpu_readqc.py's 70 000 reads).  All of it in a subprocess with dada2_amd._lib pointed at the emulated
library, as in tests/test_emu_primers.py."""
import os
import subprocess
import sys

import pytest

from test_emu import CXX, ROOT, emu_lib  # noqa: F401  (the module-scoped fixture that builds the emulated library)

pytestmark = pytest.mark.skipif(not os.path.exists(CXX), reason="no host clang++ for the emulator build")


def test_emulated_read_diagnostics(emu_lib):   # noqa: F811
    code = (
        "import sys\n"
        "sys.path[:0] = [%r, %r]\n"
        "from dada2_amd import _lib\n"
        "_lib.LIB_PATH = %r\n"
        "import readqc_cases as rc\n"
        "print(rc.emu_run())\n"
    ) % (ROOT, os.path.join(ROOT, "tests"), emu_lib)
    out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ), capture_output=True, text=True, timeout=900)
    assert out.returncode == 0 and out.stdout.rstrip().splitlines()[-1].startswith("ok "), out.stdout[-2000:] + out.stderr[-4000:]
