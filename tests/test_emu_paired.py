"""The run-level mergePairs under the emulator (tests/paired_cases.py, emu_run): the product's own host code - the validation, the
per-sample tables, the order, the chunks, the throw-away samples - and the kernels k_mp_tally, k_mp_compact, k_nw_gen<pair>,
k_mp_eval and k_mp_consensus run on the CPU, held to the cases of the GPU test in their lighter form.  The emulator runs a wave's
lanes one after the other, so a lane that depended on what another lane of its wave wrote in the same launch would show here.  All
of it in a subprocess with dada2_amd._lib pointed at the emulated library, as in tests/test_emu_seqtables.py."""
import os
import subprocess
import sys

import pytest

from test_emu import CXX, ROOT, emu_lib  # noqa: F401  (the module-scoped fixture that builds the emulated library)

pytestmark = pytest.mark.skipif(not os.path.exists(CXX), reason="no host clang++ for the emulator build")


def test_emulated_run(emu_lib):   # noqa: F811
    code = (
        "import sys\n"
        "sys.path[:0] = [%r, %r]\n"
        "from dada2_amd import _lib\n"
        "_lib.LIB_PATH = %r\n"
        "import paired_cases as pc\n"
        "print(pc.emu_run())\n"
    ) % (ROOT, os.path.join(ROOT, "tests"), emu_lib)
    out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ), capture_output=True, text=True, timeout=900)
    assert out.returncode == 0 and out.stdout.rstrip().splitlines()[-1].startswith("ok "), out.stdout[-2000:] + out.stderr[-4000:]
