"""The host loops of the boundary's marshalling (dada2_amd/csrc/hostsimd.cpp: quality rounding and 2-bit packing), every
compiled form against the scalar rules that tools/host_marshal.cpp restates: row lengths 1..70, 250, 251, 1510 (every tail
length of the 16-wide rounding body), the values at which the rounding rule can go wrong, values outside [0, 255.5) and NaN at
the first, a middle and the last position (the row is reported for redo), NaN behind a read's end (not looked at); packing
lengths 6..70, 250, 1510, every byte value at every position mod 32 (words identical, the invalid flag exactly for non-ACGT
bytes, padding words zero).  Every input array ends where an inaccessible page begins."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
pytestmark = pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which(HIPCC)), reason="no hipcc for the host build")


@pytest.fixture(scope="module")
def host_marshal(tmp_path_factory):
    """tools/host_marshal.cpp + hostsimd.cpp, built with the flags of the Makefile's hostsimd.o line."""
    exe = str(tmp_path_factory.mktemp("host_marshal") / "host_marshal")
    subprocess.check_call([HIPCC, "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-Wall", "-x", "c++",
                           os.path.join(ROOT, "tools", "host_marshal.cpp"), os.path.join(ROOT, "dada2_amd", "csrc", "hostsimd.cpp"),
                           "-lpthread", "-o", exe])
    return exe


@pytest.mark.parametrize("variant", ["scalar", "avx2", None])
def test_marshalling_forms_equal_the_scalar_rules(host_marshal, variant):
    argv = [host_marshal, "--check"] + (["--variant", variant] if variant else [])
    out = subprocess.run(argv, capture_output=True, text=True, timeout=300)
    if out.returncode == 77:
        pytest.skip(f"this CPU lacks {variant}")
    assert out.returncode == 0 and ": ok" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]


def test_an_unknown_variant_is_refused(host_marshal):
    out = subprocess.run([host_marshal, "--check", "--variant", "sse9"], capture_output=True, text=True, timeout=60)
    assert out.returncode == 2, out.stdout + out.stderr
