"""assignSpecies under the emulator (tests/species_cases.py, emu_run): the product's own host code - the packing of the references,
the fold of equal queries, the key and CSR tables, the re-run of a range whose candidates do not fit - and k_species_bitmap,
k_species_seed and k_species_verify run on the CPU, in a subprocess with dada2_amd._lib pointed at the emulated library as in
tests/test_emu_taxonomy.py, and are held to the cases of the GPU tests: the per-query lists of reference indices equal to the
restatement's."""
import os
import subprocess
import sys

import pytest

from test_emu import CXX, ROOT, emu_lib  # noqa: F401  (the module-scoped fixture that builds the emulated library)

pytestmark = pytest.mark.skipif(not os.path.exists(CXX), reason="no host clang++ for the emulator build")


def test_emulated_species_matching(emu_lib):   # noqa: F811
    code = (
        "import sys\n"
        "sys.path[:0] = [%r, %r]\n"
        "from dada2_amd import _lib\n"
        "_lib.LIB_PATH = %r\n"
        "import species_cases as sc\n"
        "print(sc.emu_run())\n"
    ) % (ROOT, os.path.join(ROOT, "tests"), emu_lib)
    out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ), capture_output=True, text=True, timeout=900)
    assert out.returncode == 0 and out.stdout.startswith("ok "), out.stdout[-2000:] + out.stderr[-4000:]
