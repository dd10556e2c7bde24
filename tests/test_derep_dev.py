"""The device dereplicator's parts that need no GPU.

  * The finalisation (dada2_amd/csrc/derep_dev_plain.h: derepFastq's order from the first read index, the means from integer
    sums, the map's renumbering) through tools/derep_dev_plain_check.cpp - plain host C++ with a main of its own, built with the
    address and undefined-behaviour sanitizers, nothing of it loaded into Python.  The program's stand-in for the device numbers
    the uniques in an order that has nothing to do with arrival; cases 1-5 of tests/derep_dev_cases.py run against it exactly as
    they run on the card: against oracle.derep.derep_from_reads and the host's dada2hip_derep_fastq.
  * The library's side: the new entry points are exported and registered, the module refuses what it says it refuses, and
    dada2_amd.api has gained nothing."""
import os
import shutil
import subprocess
import types

import numpy as np
import pytest

import derep_dev_cases as dc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
needs_hipcc = pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which(HIPCC)), reason="no hipcc for the host build")


@pytest.fixture(scope="module")
def plain_check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("derep_dev_plain") / "derep_dev_plain_check")
    subprocess.check_call([HIPCC, "-O1", "-g", "-std=c++17", "-Wall", "-Xarch_host", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-x", "c++", os.path.join(ROOT, "tools", "derep_dev_plain_check.cpp"), "-o", exe])
    return exe


class PlainModule:
    """dada2_amd.dereplicate's derep_reads as the cases call it, served by the check program."""

    def __init__(self, exe, tmp):
        from dada2_amd import _lib
        self._lib, self.exe, self.tmp = _lib, exe, str(tmp)

    def derep_reads(self, seqs, quals, n=10 ** 6, qual_offset=0, device=0, stats=None):
        from dada2_amd.io import Derep
        quals = dc.qbytes(quals)
        if any(len(s) != len(q) for s, q in zip(seqs, quals)):
            raise ValueError("Every read needs as many quality characters as bases.")
        if qual_offset not in (0, 33, 64):
            raise self._lib.Dada2HipError(1, "dada2hip: the quality offset must be 33, 64 or 0 (Auto).")
        path = os.path.join(self.tmp, "reads.txt")
        with open(path, "wb") as fh:
            fh.write(b"%d %d %d\n" % (len(seqs), n, qual_offset))
            for s, q in zip(seqs, quals):
                fh.write(s.encode("latin-1") + b"\n" + q + b"\n")
        out = subprocess.run([self.exe, path], capture_output=True, timeout=120)
        if out.returncode == 3:
            raise self._lib.Dada2HipError(1, out.stdout.decode().strip())
        assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
        lines = out.stdout.decode("latin-1").split("\n")
        nu, maxlen, nreads, _ = (int(x) for x in lines[0].split())
        ab, sq = zip(*(lines[1 + 2 * k].split(" ", 1) for k in range(nu)))
        q = np.array([[int(lines[2 + 2 * k][16 * p:16 * p + 16], 16) for p in range(maxlen)] for k in range(nu)], dtype=np.uint64).view(np.float64)
        mp = np.array(lines[1 + 2 * nu].split(), dtype=np.int32)
        d = Derep(list(sq), np.array(ab, dtype=np.int32), q.reshape(nu, maxlen), mp)
        if stats is not None:
            stats.update(reads_in=nreads, uniques=nu)

        return types.SimpleNamespace(nuniques=nu, maxlen=maxlen, nreads=nreads, to_derep=lambda: d, close=lambda: None)


@needs_hipcc
@pytest.mark.parametrize("name", dc.CASE_NAMES[:5])
def test_the_finalisation_alone(plain_check, tmp_path, name):
    dc.CASES[name](PlainModule(plain_check, tmp_path), light=True)


def test_entry_points_are_exported_and_registered():
    from dada2_amd import _lib
    L = _lib.lib()
    for name in ("dada2hip_derep_reads", "dada2hip_filter_derep_fastq", "dada2hip_filter_derep_fastq_paired"):
        assert name in _lib.EXPORTS and getattr(L, name).argtypes is not None, name
    assert len(_lib.DEREP_STATS) <= _lib.DEREP_NSTATS


def test_refusals_and_api_untouched():
    from dada2_amd import api, dereplicate
    assert not hasattr(api, "derep_reads") and not hasattr(api, "filter_and_derep")
    dc._raises(NotImplementedError, lambda: dereplicate.filter_and_derep(dc.SAM1F, None, orient_fwd="ACGT"), "orient_fwd is not supported")
    dc._raises(NotImplementedError, lambda: dereplicate.filter_and_derep(dc.SAM1F, None, dc.SAM1R, None, match_ids=True), "match_ids")
    dc._raises(ValueError, lambda: dereplicate.derep_reads(["ACGT"], [b"III"]), "as many quality characters")
