"""The resident form of the device dereplicator: the parts that need no GPU.

  * The integer rounding (dada2_amd/csrc/derep_resident_plain.h) against the rule on doubles that the host route applies, through
    tools/derep_resident_plain_check.cpp - plain host C++ with a main of its own, built with the address and undefined-behaviour
    sanitizers, nothing of it loaded into Python: exhaustively for n up to 2 048, on 10^7 random (T, n), with the ties k + 1/2.
  * The library's side: the new entry points are exported and registered, an object without a quality matrix is refused by the
    combine with the one message, dada2hip_derep_qmax reads a full object's matrix, the module refuses what it says it refuses,
    and dada2_amd.api has gained no function."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import derep_dev_cases as dc
import derep_resident_cases as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
needs_hipcc = pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which(HIPCC)), reason="no hipcc for the host build")


@needs_hipcc
def test_the_integer_rounding_is_the_double_rounding(tmp_path):
    exe = str(tmp_path / "derep_resident_plain_check")
    subprocess.check_call([HIPCC, "-O1", "-g", "-std=c++17", "-Wall", "-Xarch_host", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-x", "c++", os.path.join(ROOT, "tools", "derep_resident_plain_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and out.stdout.rstrip().splitlines()[-1] == "ok", out.stdout[-2000:] + out.stderr[-4000:]
    counts = dict(zip(out.stdout.split()[0:6:2], (int(v) for v in out.stdout.split()[1:6:2])))
    # n = 1 .. 2 048 with every T in [-n, 95 n] is 96 n + 1 values each; 10^7 random draws; ties for the even n among them
    assert counts["exhaustive"] >= sum(96 * n + 1 for n in range(1, 2049)) and counts["random"] == 10 ** 7 and counts["ties"] > 10 ** 6, counts


def test_entry_points_are_exported_and_registered():
    from dada2_amd import _lib
    L = _lib.lib()
    for name in ("dada2hip_derep_reads_resident", "dada2hip_filter_derep_fastq_resident", "dada2hip_filter_derep_fastq_paired_resident",
                 "dada2hip_derep_has_quals", "dada2hip_derep_qmax", "dada2hip_sample_rows"):
        assert name in _lib.EXPORTS and getattr(L, name).argtypes is not None, name
    assert len(_lib.RESIDENT_STATS) <= _lib.RESIDENT_NSTATS and _lib.DEREP_NSTATS == 16 and len(_lib.SAMPLE_ROWS_GEOM) <= _lib.SAMPLE_ROWS_NGEOM
    hdr = open(os.path.join(ROOT, "include", "dada2hip.h")).read()
    knobs = open(os.path.join(ROOT, "dada2_amd", "csrc", "knobs.h")).read()
    assert "#define DADA2HIP_RESIDENT_NSTATS %d" % _lib.RESIDENT_NSTATS in hdr and "#define DADA2HIP_DEREP_NSTATS 16" in hdr
    assert "DADA2HIP_DD_SAMPLE_BLOCKS" in hdr and "DADA2HIP_DD_SAMPLE_BLOCKS" in knobs


def test_a_full_object_has_its_matrix_and_its_qmax(tmp_path):
    """The host dereplicator's object (no device touched): has_quals, and dada2hip_derep_qmax from the matrix."""
    from dada2_amd import _lib, api
    nd = api.NativeDerep(dc.SAM1F)
    try:
        L = _lib.lib()
        q = nd.to_derep().quals
        want = int(np.ceil(np.where(np.isnan(q), -np.inf, q).max()))
        assert L.dada2hip_derep_has_quals(nd._h) == 1 and bool(L.dada2hip_derep_quals(nd._h))
        assert L.dada2hip_derep_qmax(nd._h) == want == nd.qmax() and 30 <= want <= 41, (L.dada2hip_derep_qmax(nd._h), want)
    finally:
        nd.close()
    assert _lib.lib().dada2hip_derep_qmax(None) == 0 and _lib.lib().dada2hip_derep_has_quals(None) == 0


def test_the_combine_refuses_a_view_without_a_matrix():
    from dada2_amd import _lib, api
    full = api.Derep(["ACGTACGT", "ACGTACGA"], np.array([3, 1], np.int32), np.full((2, 8), 30.0), np.array([0, 0, 1, 0], np.int32))
    keep = []
    views = (_lib.CDerepView * 2)(api._derep_view(full, keep), api._derep_view(full, keep))
    views[1].quals = None
    h, eb = C.c_void_p(), C.create_string_buffer(2048)
    rcode = _lib.lib().dada2hip_derep_combine(2, views, C.byref(h), None, eb, 2048)
    assert rcode == 1 and not h and rc.NO_MATRIX in eb.value.decode() and "dada2hip_derep_reads" in eb.value.decode(), (rcode, eb.value)
    # ... and the sample entry says the same of a missing object's sibling: a null object is still "no derep object"
    rcode = _lib.lib().dada2hip_sample_from_derep(None, None, 0, C.byref(h), eb, 2048)
    assert rcode == 1 and b"no derep object" in eb.value


def test_refusals_and_api_untouched():
    from dada2_amd import api, dereplicate
    for name in ("derep_reads_resident", "filter_and_sample", "ResidentDerep"):
        assert hasattr(dereplicate, name) and not hasattr(api, name), name
    assert issubclass(dereplicate.ResidentDerep, api.NativeDerep)
    dc._raises(TypeError, lambda: dereplicate.ResidentDerep("reads.fastq"), "filter_and_sample")
    dc._raises(NotImplementedError, lambda: dereplicate.filter_and_sample(dc.SAM1F, None, orient_fwd="ACGT"), "orient_fwd is not supported by filter_and_sample")
    dc._raises(NotImplementedError, lambda: dereplicate.filter_and_sample(dc.SAM1F, None, dc.SAM1R, None, match_ids=True), "match_ids")
    dc._raises(ValueError, lambda: dereplicate.filter_and_sample([dc.SAM1F, dc.SAM1R], None), "one sample")
    dc._raises(ValueError, lambda: dereplicate.filter_and_sample(os.path.join(dc.GOLDEN, "missing.fastq")), "do not exist")
    dc._raises(ValueError, lambda: dereplicate.derep_reads_resident(["ACGT"], [b"III"]), "as many quality characters")
    dc._raises(ValueError, lambda: dereplicate.dada([], None), "ResidentDerep")
    assert rc.NO_MATRIX in dereplicate.NO_MATRIX and "filter_and_derep" in dereplicate.NO_MATRIX
