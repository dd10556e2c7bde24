"""The plain-C++ parts of the stages' shared host layer (dada2_amd/csrc/stage_plain.h), through tools/stage_plain_check.cpp: no
GPU, no library.  The piece cutter of the two-slot read pipeline: for every vector of 0..7 reads and 20 000 drawn vectors each of 8
and 9 reads, lengths in {0, 1, 7, 8, 9}, limits (reads, bytes) in {1, 2, 3} x {1, 8, 9, 64}, the pieces tile [0, n) in order, none
is empty, none exceeds the read limit, and one exceeds the byte limit only as a single read.  The prefix keys of
collapseNoMismatch's join and assignSpecies' seed: rows of 1, 15, 16, 17, 31, 32, 33 and 40 bases over six fixed patterns - two of
them equal in their first 32 bases and different behind, two equal through the shorter one's length - have the keys a bit-by-bit
restatement gives, the groups ascend by length, the keys ascend strictly inside a group, and every row's key is found in its group
by the device helper's lower bound, restated."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
pytestmark = pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which(HIPCC)), reason="no hipcc for the host build")


@pytest.fixture(scope="module")
def stage_plain_check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("stage_plain") / "stage_plain_check")
    subprocess.check_call([HIPCC, "-O2", "-std=c++17", "-Wall", "-x", "c++",
                           os.path.join(ROOT, "tools", "stage_plain_check.cpp"), "-o", exe])
    return exe


@pytest.mark.parametrize("which", ["pieces", "keys"])
def test_the_shared_layer_keeps_its_properties(stage_plain_check, which):
    out = subprocess.run([stage_plain_check, which], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "stage_plain_check: ok" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]
