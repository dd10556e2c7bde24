"""assignTaxonomy under the emulator (tests/taxonomy_cases.py, emu_run): the product's own host code - the model build with the
host's logf, the k-mer arrays, the uniform layout, the bootstrap counts - and k_tax_sums (slab and gather instance) and
k_tax_combine run on the CPU, in a subprocess with dada2_amd._lib pointed at the emulated library as in
tests/test_emu_collapse.py, and are held to the criteria of the GPU tests: the model table bit-equal to the restatement's, ntie
exact, every pick in its tie set, boot recounted, the two instances / two calls identical, another seed only at ties; three
cases also with the queries in chunks of 1 and 3 (DADA2HIP_TAX_CHUNK): identical outputs, the chunks counted from the launches."""
import os
import subprocess
import sys

import pytest

from test_emu import CXX, ROOT, emu_lib  # noqa: F401  (the module-scoped fixture that builds the emulated library)

pytestmark = pytest.mark.skipif(not os.path.exists(CXX), reason="no host clang++ for the emulator build")


def test_emulated_taxonomy_model_and_classifier(emu_lib):   # noqa: F811
    code = (
        "import sys\n"
        "sys.path[:0] = [%r, %r]\n"
        "from dada2_amd import _lib\n"
        "_lib.LIB_PATH = %r\n"
        "import taxonomy_cases as tc\n"
        "print(tc.emu_run())\n"
    ) % (ROOT, os.path.join(ROOT, "tests"), emu_lib)
    out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ), capture_output=True, text=True, timeout=900)
    assert out.returncode == 0 and out.stdout.startswith("ok "), out.stdout[-2000:] + out.stderr[-4000:]
