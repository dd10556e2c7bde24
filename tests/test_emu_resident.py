"""One resident sample across changing options, error matrices, prior flags, a compare, an abort and the device-raised error, under
the emulator (tests/resident_cases.py, emu_run): the product's own host driver - the Run object kept on the handle, what
alloc_state and v2_alloc clear and what they leave, the aligner rings resized by band and class, the error matrix uploaded under
another stride, set_priors' two copies of the flags, the way out of a run that throws - and its kernels run on the CPU, in a
subprocess with dada2_amd._lib pointed at the emulated library as in tests/test_emu_pool.py.  The cut: the walk over the option
steps marked for the emulator, forward and reversed, on 153 uniques of 66-80 nt; the band steps on the lane kernels and on the wide
kernel; the err walk; the priors walk with a handful of flags; a compare between runs; an abort at the third poll and both inputs
of the device-raised error, each followed by runs on the same handle."""
import os
import subprocess
import sys

import pytest

from test_emu import CXX, ROOT, emu_lib  # noqa: F401  (the module-scoped fixture that builds the emulated library)

pytestmark = pytest.mark.skipif(not os.path.exists(CXX), reason="no host clang++ for the emulator build")


def test_emulated_resident_sample_across_options_errors_and_aborts(emu_lib, oracle_c):   # noqa: F811
    code = (
        "import sys\n"
        "sys.path[:0] = [%r, %r]\n"
        "from dada2_amd import _lib\n"
        "_lib.LIB_PATH = %r\n"
        "import resident_cases as rc\n"
        "print(rc.emu_run())\n"
    ) % (ROOT, os.path.join(ROOT, "tests"), emu_lib)
    out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ), capture_output=True, text=True, timeout=900)
    assert out.returncode == 0 and out.stdout.startswith("ok"), out.stdout[-2000:] + out.stderr[-4000:]
