"""The file level of the read diagnostics (dada2_amd/csrc/derep.cpp: dada2hip_qprofile_fastq, dada2hip_complexity_fastq,
fq_run_chunks without writers), through tools/readqc_file_check.cpp: no GPU, no library, nothing loaded into Python.  The program
is derep.cpp itself with the device calls replaced by plain host stand-ins, built as host C++ with the address and
undefined-behaviour sanitizers and run on the CPU: 157 records whose lengths grow, shrink and vanish, plain and gzip, in chunks of
1, 7, 50, 1 000 and the default, with record limits below, inside and above the file - the table of every run against a direct
count (a later chunk with a longer read makes it grow), the complexities against the R loop written out, the maximum taken over
the profiled records only; an empty file; the record a bad letter's message names, and that a record past the limit is not looked
at; a directory, a missing file, a wrong offset, a window no read is longer than."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
pytestmark = pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which(HIPCC)), reason="no hipcc for the host build")


@pytest.fixture(scope="module")
def readqc_file_check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("readqc_file") / "readqc_file_check")
    subprocess.check_call([HIPCC, "-O1", "-g", "-std=c++17", "-w", "-I", os.path.join(ROOT, "tests", "emu"), "-Xarch_host",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-x", "c++",
                           os.path.join(ROOT, "tools", "readqc_file_check.cpp"), "-o", exe, "-lz", "-ldl", "-lpthread"])
    return exe


def test_the_file_level_on_host_stand_ins(readqc_file_check, tmp_path):
    out = subprocess.run([readqc_file_check, str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "readqc_file_check: ok" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]
