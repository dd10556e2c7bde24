"""The plain-C++ core of matchIDs (dada2_amd/csrc/filter_ids_plain.h), through tools/filter_ids_check.cpp: no GPU, no library,
nothing loaded into Python.  The program is plain host C++, built with the address and undefined-behaviour sanitizers and run on
the CPU.  By hand: strsplit's rules (consecutive, leading and trailing separators, the six white-space characters, a literal
separator), the detection of the id field, the key (NA for a missing field, the old format's '#' on the forward ids only, an
empty field), the join with NA matching NA and a duplicate, the remainder.  Drawn: 2 000 pairs of id lists over a small
alphabet with separators, against a restatement over std::set<std::string>."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
pytestmark = pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which(HIPCC)), reason="no hipcc for the host build")


@pytest.fixture(scope="module")
def filter_ids_check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("filter_ids") / "filter_ids_check")
    subprocess.check_call([HIPCC, "-O1", "-g", "-std=c++17", "-Wall", "-Xarch_host", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-x", "c++",
                           os.path.join(ROOT, "tools", "filter_ids_check.cpp"), "-o", exe])
    return exe


@pytest.mark.parametrize("which", ["hand", "drawn"])
def test_the_split_the_key_and_the_join(filter_ids_check, which):
    out = subprocess.run([filter_ids_check, which], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "filter_ids_check: ok" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]
