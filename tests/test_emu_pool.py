"""Priors by sequence and the pooled runs under the emulator (tests/pool_cases.py, emu_run): the product's own host code - the
packing of the prior sequences, their key and row tables, the choice between the LDS and the global path, the copy back into the
host mirror - and k_prior_match run on the CPU, in a subprocess with dada2_amd._lib pointed at the emulated library as in
tests/test_emu_species.py, and are held to the cases of the GPU tests: first_match and the flags equal to list.index / in on
every prior list, through LDS, through global memory and with blocks that stride; then one small pooled and one small
pseudo-pooled dada() against the restated pipeline on the reference's dada_uniques."""
import os
import subprocess
import sys

import pytest

from test_emu import CXX, ROOT, emu_lib  # noqa: F401  (the module-scoped fixture that builds the emulated library)

pytestmark = pytest.mark.skipif(not os.path.exists(CXX), reason="no host clang++ for the emulator build")


def test_emulated_prior_matching_and_pooled_runs(emu_lib, oracle_ref):   # noqa: F811
    code = (
        "import sys\n"
        "sys.path[:0] = [%r, %r]\n"
        "from dada2_amd import _lib\n"
        "_lib.LIB_PATH = %r\n"
        "import pool_cases as pc\n"
        "print(pc.emu_run())\n"
    ) % (ROOT, os.path.join(ROOT, "tests"), emu_lib)
    out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ), capture_output=True, text=True, timeout=900)
    assert out.returncode == 0 and out.stdout.startswith("ok"), out.stdout[-2000:] + out.stderr[-4000:]
