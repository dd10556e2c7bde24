"""The run-level mergePairs (dada2_amd.paired): the parts that need no GPU.

  * The cases of tests/paired_cases.py against a stand-in that serves paired.merge_pairs from the specification itself: every
    case's fact holds on the oracle's rows, and the cases' own arithmetic (counts, orders, chunk numbers) is right before a GPU
    sees them.
  * The host's part (dada2_amd/csrc/merge_plain.h: capacity, the checks of the maps, the message of an index past a table, the row
    order, the chunk cutter, the scan of the accepted lengths) through tools/merge_plain_check.cpp - plain host C++ with a main of
    its own, built with the address and undefined-behaviour sanitizers, nothing of it loaded into Python.
  * Every refusal that is decided before the device is touched, with the reference's message; the library's side of the new
    entry; dada2_amd.api has gained nothing.
The input forms, propagate_col, return_rejects, the verbose text, the sequence table and the just_concatenate goldens need the
device's tally: they run on the GPU and under the emulator (paired_cases.case_interface, case_concat)."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import paired_cases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
needs_hipcc = pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which(HIPCC)), reason="no hipcc for the host build")


def _capacity(nreads, ncF, ncR):
    cap = 64
    while cap < 2 * max(1, min(nreads, ncF * ncR)):
        cap *= 2
    return cap


class SpecModule:
    """dada2_amd.paired.merge_pairs as the cases call it, served by the specification; the stats by their definitions."""
    SERVED_BY_SPEC = True

    def merge_pairs(self, dadaF, derepF, dadaR, derepR, stats=None, device=0, **kw):
        from dada2_amd import _lib
        dF = list(dadaF.values()) if isinstance(dadaF, dict) else [dadaF] if not isinstance(dadaF, list) else dadaF
        dR = list(dadaR.values()) if isinstance(dadaR, dict) else [dadaR] if not isinstance(dadaR, list) else dadaR
        eF, eR = (derepF if isinstance(derepF, list) else [derepF]), (derepR if isinstance(derepR, list) else [derepR])
        for s in range(len(dF)):                                    # an index past a table: the first read that has one
            for side, dada, derep in (("forward", dF[s], eF[s]), ("reverse", dR[s], eR[s])):
                rmap, umap = np.asarray(derep.map), np.asarray(dada.map)
                past = np.flatnonzero(rmap >= umap.size)
                if past.size:
                    raise _lib.Dada2HipError(1, "%s (sample %d, read %d counted from 0: the %s derep-class map names unique %d of %d)"
                                             % (pc.NO_MATCH, s + 1, past[0], side, rmap[past[0]] + 1, umap.size))
            for side, dada, derep in (("forward", dF[s], eF[s]), ("reverse", dR[s], eR[s])):
                rmap, umap = np.asarray(derep.map), np.asarray(dada.map)
                v = np.where(rmap >= 0, umap[np.maximum(rmap, 0)], 0)
                past = np.flatnonzero(v > dada.nclust)
                if past.size:
                    raise _lib.Dada2HipError(1, "%s (sample %d, read %d counted from 0: the %s dada-class map names sequence %d of %d)"
                                             % (pc.NO_MATCH, s + 1, past[0], side, v[past[0]], dada.nclust))
            try:
                pc.spec_sample(dF[s], eF[s], dR[s], eR[s], just_concatenate=True)
            except pc.SpecError as e:
                raise _lib.Dada2HipError(1, "%s (sample %d: ...)" % (e, s + 1))
        names = dict(zip(dadaF, dF)) if isinstance(dadaF, dict) else dF
        got, messages = pc.spec_merge_pairs(names, eF, dict(zip(dadaR, dR)) if isinstance(dadaR, dict) else dR, eR, **kw)
        for m in messages:
            print(m)
        if stats is not None:
            every = [pc.spec_sample(dF[s], eF[s], dR[s], eR[s], **dict(kw, return_rejects=True, verbose=False)) for s in range(len(dF))]
            unique = sum(len(r) for r in every)
            chunk = min(int(os.environ.get("DADA2HIP_MERGE_CHUNK", 65536)), 65536)
            bits = int(os.environ.get("DADA2HIP_MERGE_HASH_BITS", 64))
            stats.update(samples=len(dF), read_pairs_in=sum(len(e.map) for e in eF), unique_pairs=unique,
                         pairs_na=sum(len(e.map) for e in eF) - sum(r["abundance"] for rows in every for r in rows),
                         chunks=-(-unique // chunk), accepted=sum(r["accept"] for rows in every for r in rows),
                         table_capacity=max(_capacity(len(eF[s].map), dF[s].nclust, dR[s].nclust) for s in range(len(dF))),
                         collisions=0 if bits >= 64 else unique * unique)
        return got


@pytest.mark.parametrize("name", [n for n in pc.CASE_NAMES if n not in ("interface", "concat")])
def test_cases_hold_on_the_specification(name):
    pc.CASES[name](SpecModule())


def test_concat_goldens_are_what_the_specification_gives():
    pc.case_concat(SpecModule())


# ---- the host's part, alone, under the sanitizers ------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def plain_check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("merge_plain") / "merge_plain_check")
    subprocess.check_call([HIPCC, "-O1", "-g", "-std=c++17", "-Wall", "-Xarch_host", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-x", "c++", os.path.join(ROOT, "tools", "merge_plain_check.cpp"), "-o", exe])
    return exe


def _plain(exe, tmp, sample, chunk=7, letters="ACGTTGCAAC"):
    dF, eF, dR, eR = sample
    path = os.path.join(str(tmp), "sample.txt")
    with open(path, "w") as fh:
        fh.write("%d %d %d %d %d %d\n" % (len(eF.map), len(dF.map), len(dR.map), dF.nclust, dR.nclust, chunk))
        for v in (eF.map, eR.map, dF.map, dR.map):
            fh.write(" ".join(str(int(x)) for x in v) + "\n")
        fh.write(letters + "\n")
    out = subprocess.run([exe, path], capture_output=True, text=True, timeout=300)
    assert out.returncode in (0, 3), (out.returncode, out.stdout[-1000:], out.stderr[-3000:])
    return out.returncode, out.stdout.rstrip("\n").split("\n")


@needs_hipcc
def test_host_part_alone_under_the_sanitizers(plain_check, tmp_path):
    rng = np.random.default_rng(5)
    c = pc._case(rng, np.concatenate([rng.integers(1, 8, 900), [-1, 7, 3]]), np.concatenate([rng.integers(1, 7, 900), [6, -1, 6]]), 7, 6)
    for na_by, chunk in (("both", 7), ("derep", 1), ("dada", 1000)):
        sample = pc.sample_of(c, na_by)
        want = pc.spec_sample(*sample, just_concatenate=True, return_rejects=True)
        code, lines = _plain(plain_check, tmp_path, sample, chunk)
        assert code == 0, lines
        P = len(want)
        assert lines[0] == "%d %d %d" % (_capacity(903, 7, 6), P, 2) and P == 42
        rows = [tuple(int(x) for x in ln.split()) for ln in lines[1:1 + P]]
        assert [r[:3] for r in rows] == [(w["forward"], w["reverse"], w["abundance"]) for w in want]
        fwd, rev = pc.denoised(sample[0], sample[1]), pc.denoised(sample[2], sample[3])
        assert all(fwd[r[3]] == r[0] and rev[r[3]] == r[1] and not ((fwd[:r[3]] == r[0]) & (rev[:r[3]] == r[1])).any() for r in rows)
        assert [int(x) for x in lines[1 + P].split()] == list(range(chunk, P, chunk)) + [P]
        off, at = [], 0
        for r in rows:
            off.append(at)
            at += (r[0] + r[1]) * (r[2] & 1)
        assert [int(x) for x in lines[2 + P].split()] == off and int(lines[3 + P]) == at
        assert lines[4 + P] == "GTTGCAACGT 1"
    assert _plain(plain_check, tmp_path, sample, letters="ACGNT")[1][-1] == "ANCGT 0"
    # the refusals: the maximum of a map against the dada-class object (:117-118), and an index past either table
    dF, eF, dR, eR = pc.sample_of(c)
    short = pc.derep_of(np.where(np.asarray(eF.map) == len(dF.map) - 1, 0, eF.map), len(dF.map))
    code, lines = _plain(plain_check, tmp_path, (dF, short, dR, eR))
    assert code == 3 and lines[0].startswith("error 1 " + pc.NO_MATCH + " (sample 1:"), lines
    rmap = np.array(eR.map)
    rmap[[500, 20]] = len(dR.map)
    code, lines = _plain(plain_check, tmp_path, (dF, eF, dR, pc.derep_of(rmap, len(dR.map))))
    assert code == 3 and "sample 1, read 20 counted from 0: the reverse derep-class map names unique %d of %d" % (len(dR.map) + 1, len(dR.map)) in lines[0]
    umap = np.array(dF.map)
    umap[2] = dF.nclust + 1
    first = int(np.flatnonzero(np.asarray(eF.map) == 2)[0])
    code, lines = _plain(plain_check, tmp_path, (pc.dada_of(dF.clustering["sequence"], dF.clustering["n0"], umap), eF, dR, eR))
    assert code == 3 and "read %d counted from 0: the forward dada-class map names sequence 8 of 7" % first in lines[0], lines
    empty = (pc.dada_of(["ACGT"], [1], []), pc.derep_of([], 0)) * 2
    code, lines = _plain(plain_check, tmp_path, empty)
    assert code == 3 and pc.NO_MATCH in lines[0]


# ---- refusals in front of the device ---------------------------------------------------------------------------------------------------

def _refused(fn, text):
    from dada2_amd import _lib
    with pytest.raises(_lib.Dada2HipError) as e:
        fn()
    assert text in str(e.value), str(e.value)
    return e.value


def test_refusals_with_the_reference_messages():
    from dada2_amd import paired
    rng = np.random.default_rng(6)
    dF, eF, dR, eR = pc.sample_of(pc._case(rng, [1, 2, 2], [2, 1, 2], 2, 2))
    not_dada = "dadaF and dadaR must be provided as dada-class objects or lists of dada-class objects."
    not_derep = "derepF and derepR must be provided as derep-class objects or as character vectors of filenames."
    _refused(lambda: paired.merge_pairs(eF, eF, dR, eR), not_dada)
    _refused(lambda: paired.merge_pairs([dF, 3], [eF, eF], [dR, dR], [eR, eR]), not_dada)
    _refused(lambda: paired.merge_pairs(dF, eF, {"a": "x"}, eR), not_dada)
    _refused(lambda: paired.merge_pairs(dF, dF, dR, eR), not_derep)
    _refused(lambda: paired.merge_pairs(dF, eF, dR, [eR.map]), not_derep)
    _refused(lambda: paired.merge_pairs([dF, dF], [eF, eF], [dR, dR], [eR]), "The dadaF/derepF/dadaR/derepR arguments must be the same length.")
    _refused(lambda: paired.merge_pairs([dF, dF], eF, [dR, dR], eR), "must be the same length.")
    floats = pc.derep_of([0, 1, 1], 2)
    floats.map = np.array([0.0, 1.0, 1.0])
    _refused(lambda: paired.merge_pairs(dF, floats, dR, eR), "Incorrect format of $map in derep-class arguments.")
    shorter = pc.derep_of([1, 0], 2)
    e = _refused(lambda: paired.merge_pairs([dF, dF], [eF, eF], {"x": dR, "y": dR}, [eR, shorter]), pc.NO_MATCH)
    assert "sample 2" in str(e) and e.code == 1
    e = _refused(lambda: paired.merge_pairs({"x": dF, "y": dF}, [eF, eF], [dR, dR], [eR, shorter]), pc.NO_MATCH)
    assert "sample 'y'" in str(e)
    with pytest.raises(ValueError, match="not an existing directory|No files found"):
        paired.merge_pairs(dF, os.path.join(ROOT, "tests", "emu"), dR, eR)


def test_library_refuses_in_front_of_the_device():
    """dada2hip_merge_run: a map longer than INT32_MAX is ERR_INPUT, a letter outside ACGT ERR_UNSUPPORTED, both with the sample -
    decided before a device is selected."""
    from dada2_amd import _lib
    L = _lib.lib()
    one = np.zeros(4, dtype=np.int32)
    ptr = (C.c_void_p * 1)(one.ctypes.data)
    ones = np.ones(1, dtype=np.int32)
    off = np.array([0, 4], dtype=np.int64)

    def call(nreads, fb=b"ACGT", rb=b"ACGT", concat=0, stats=None):
        n = np.array([nreads], dtype=np.int64)
        eb = C.create_string_buffer(1024)
        h = C.c_void_p(1)
        rc = L.dada2hip_merge_run(1, n.ctypes.data, C.cast(ptr, C.c_void_p), C.cast(ptr, C.c_void_p), ones.ctypes.data, C.cast(ptr, C.c_void_p),
                                  ones.ctypes.data, C.cast(ptr, C.c_void_p), ones.ctypes.data, fb, off.ctypes.data, ones.ctypes.data, ones.ctypes.data,
                                  rb, off.ctypes.data, ones.ctypes.data, 12, 0, 0, concat, 0, C.byref(h), stats, eb, 1024)
        assert h.value is None
        return rc, eb.value.decode()
    rc, msg = call(2**31)
    assert rc == 1 and "2^31 - 1 reads" in msg and "sample 1" in msg
    rc, msg = call(-1)
    assert rc == 1
    rc, msg = call(4, rb=b"ACNT")
    assert rc == 4 and "A/C/G/T only: sample 1, reverse sequence 1" in msg     # DADA2HIP_ERR_UNSUPPORTED
    rc, msg = call(4, fb=b"acgt")
    assert rc == 4 and "forward sequence 1" in msg
    assert L.dada2hip_merge_run_nsamples(None) == 0 and L.dada2hip_merge_run_nrow(None, 0) == 0 and L.dada2hip_merge_run_column(None, 0, 0) is None
    L.dada2hip_merge_run_free(None)


def test_module_stands_beside_api():
    from dada2_amd import _lib, api, paired
    assert not hasattr(api, "paired") and api.merge_pairs is not paired.merge_pairs
    assert "device" in api.merge_pairs.__code__.co_varnames and "propagate_col" not in api.merge_pairs.__code__.co_varnames
    assert len(paired.STATS) == 16 == _lib.MERGE_NSTATS and paired.STATS[-1] == "total_us"
    with open(os.path.join(ROOT, "include", "dada2hip.h")) as fh:
        assert "#define DADA2HIP_MERGE_NSTATS 16" in fh.read()
