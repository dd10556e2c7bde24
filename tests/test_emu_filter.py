"""filterAndTrim under the emulator (tests/filter_cases.py, emu_run): the product's own host code - the word table of both
strands, the expected-error tables, the Shannon number, the FASTQ reader, the paired AND and the writer with its gzip members -
and k_filter_scan, k_filter_ee and k_filter_kmers run on the CPU.  The pieces and the two slots of a call run in the case
"pieces" alone (DADA2HIP_FILTER_PIECE from 1 to 299 reads and DADA2HIP_FILTER_PIECE_BYTES on 300 reads, 30 reads on files in
chunks of 100: the second piece, a slot used again, the stats summed over pieces, the cut by bytes, each counted from
upload_bytes); every other case is one piece in slot 0, and no case here makes a wave of k_filter_scan or a block of
k_filter_kmers take a second read (that is tests/test_gpu_filter.py's batch of 131 073).  All of it in a subprocess with
dada2_amd._lib pointed at the emulated library as in tests/test_emu_species.py, and are held to the cases of the GPU tests."""
import os
import subprocess
import sys

import pytest

from test_emu import CXX, ROOT, emu_lib  # noqa: F401  (the module-scoped fixture that builds the emulated library)

pytestmark = pytest.mark.skipif(not os.path.exists(CXX), reason="no host clang++ for the emulator build")


def test_emulated_filter_and_trim(emu_lib):   # noqa: F811
    code = (
        "import sys\n"
        "sys.path[:0] = [%r, %r]\n"
        "from dada2_amd import _lib\n"
        "_lib.LIB_PATH = %r\n"
        "import filter_cases as fc\n"
        "print(fc.emu_run())\n"
    ) % (ROOT, os.path.join(ROOT, "tests"), emu_lib)
    out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ), capture_output=True, text=True, timeout=900)
    assert out.returncode == 0 and out.stdout.startswith("ok "), out.stdout[-2000:] + out.stderr[-4000:]
