"""The plain-C++ core of dada2hip_derep_combine (dada2_amd/csrc/pool_plain.h), through tools/pool_plain_check.cpp: no GPU, no
library, nothing loaded into Python.  The program is plain host C++, built with the address and undefined-behaviour sanitizers
and run on the CPU.  Hand-made
samples: a unique in all three samples, in the first and last only, in one; abundance ties settled by first appearance; a weak
hash under which every sequence of one length collides; a duplicate inside a sample; an abundance sum past INT32_MAX and one of
exactly INT32_MAX; no samples, samples without uniques.  Drawn samples: 300 sets of 1-5 samples of up to 40 short sequences
over two letters, against a restatement over std::map and std::stable_sort - first-appearance order, sums, the contributors in
sample order, the stable order, the renumbered indices, and map entries (NA stays NA, an entry that names no unique is refused)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
pytestmark = pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which(HIPCC)), reason="no hipcc for the host build")


@pytest.fixture(scope="module")
def pool_plain_check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("pool_plain") / "pool_plain_check")
    subprocess.check_call([HIPCC, "-O1", "-g", "-std=c++17", "-Wall", "-Xarch_host", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-x", "c++",
                           os.path.join(ROOT, "tools", "pool_plain_check.cpp"), "-o", exe])
    return exe


@pytest.mark.parametrize("which", ["hand", "drawn"])
def test_the_grouping_the_order_and_the_renumbering(pool_plain_check, which):
    out = subprocess.run([pool_plain_check, which], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "pool_plain_check: ok" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]
