"""The resident form of the device dereplicator under the emulator (tests/derep_resident_cases.py, emu_run): the product's own
host code - the small rows' way down, the order's way up, the sample's shell, the input errors behind the kernel - and
k_dd_to_sample run on the CPU, held to the cases of the GPU test in their light form: both routes to a resident sample, the
derep objects' fields, the rows byte for byte, the runs field for field.  EMU_GUARD=1: every device buffer ends at an unmapped
page, so a word or a byte written past a row's stride stops the job.  Cases 1-3 once more on dirty memory, under both bytes of
tests/poison_cases.py.  Each job in a subprocess with dada2_amd._lib pointed at the emulated library, as in
tests/test_emu_derep_dev.py."""
import os
import subprocess
import sys

import pytest

from test_emu import CXX, ROOT, emu_lib  # noqa: F401  (the module-scoped fixture that builds the emulated library)

pytestmark = pytest.mark.skipif(not os.path.exists(CXX), reason="no host clang++ for the emulator build")


def emu_job(emu_lib, call):   # noqa: F811
    code = (
        "import sys\n"
        "sys.path[:0] = [%r, %r]\n"
        "from dada2_amd import _lib\n"
        "_lib.LIB_PATH = %r\n"
        "import derep_resident_cases as rc\n"
        "print(rc.%s)\n"
    ) % (ROOT, os.path.join(ROOT, "tests"), emu_lib, call)
    out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, EMU_GUARD="1"), capture_output=True, text=True, timeout=900)
    assert out.returncode == 0 and out.stdout.rstrip().splitlines()[-1].startswith("ok "), out.stdout[-2000:] + out.stderr[-4000:]


def test_emulated_resident_cases(emu_lib):   # noqa: F811
    emu_job(emu_lib, "emu_run()")


@pytest.mark.parametrize("byte", (0x5A, 0xFF))
def test_emulated_resident_rows_on_poisoned_memory(emu_lib, byte):   # noqa: F811
    emu_job(emu_lib, "emu_run(poison=%d)" % byte)
