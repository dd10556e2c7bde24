"""filterAndTrim without a device: the restatement of tests/filter_cases.py pinned to the reference's own compiled routines
(tests/golden/filter.npz: C_matchRef and C_matrixEE of src/filter.cpp, recorded by tests/golden/make_filter_golden.py) and run
over the committed FASTQ fixtures, the genome fixture's word counts, the layout of dada2hip_filter_params, and what
dada2_amd/api.py decides before it reaches the library (paths, refused arguments)."""
import ctypes as C
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import filter_cases as fc
from dada2_amd import _lib, api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(fc.GOLDEN, "filter.npz"))


def test_genome_fixture_word_counts():
    g = fc.phix()
    assert len(g) == 5386 and not g.strip("ACGT")
    fwd, rev = fc.word_set(g, 16), fc.word_set(fc.rc(g), 16)
    assert len(fwd) == 5386 and len(rev) == 5386 and len(fwd | rev) == 10772
    assert api.read_fasta(fc.PHIX_FA)[1] == [g]


def test_match_ref_equals_the_reference(golden):
    seqs = [str(s) for s in golden["seqs"]]
    g = fc.phix()
    assert len(seqs) >= 200 and "" in seqs
    for w, n in golden["settings"].tolist():
        want = golden["hits_%d_%d" % (w, n)]
        assert fc.match_ref(seqs, g, w, bool(n)) == want[:, 0].tolist(), (w, n)
        assert fc.match_ref(seqs, fc.rc(g), w, bool(n)) == want[:, 1].tolist(), (w, n)
    h = golden["hits_16_1"]
    flagged = (h >= 2).any(axis=1)
    assert 50 < int(flagged.sum()) < len(seqs) - 50                           # both outcomes well represented
    assert int((h.sum(axis=1) >= 2).sum()) > int(flagged.sum())               # a read only the SUM of the counts would flag
    assert (golden["hits_16_0"] >= h).all() and (golden["hits_16_0"] > h).any()


def test_matrix_ee_is_bit_equal_to_the_reference(golden):
    q, ee = golden["quals"], golden["ee"]
    na = np.iinfo(np.int32).min
    for row, want in zip(q, ee):
        vals = row[row != na].tolist()
        assert fc.matrix_ee(vals).hex() == float(want).hex(), vals[:8]
    assert float(ee[200]) == 2.0000000000000004 > 2.0                        # 20 x Q10 in order; a pairwise tree gives 2.0
    assert math.fsum([0.1] * 20) == 2.0


def test_restatement_on_the_fastq_fixtures():
    g = fc.phix()
    kept_240 = {"sam1F": 1087, "sam1R": 509, "sam2F": 1064, "sam2R": 484}
    for name, path in fc.FASTQS.items():
        recs = fc.read_fastq(path)
        seqs = [r[1] for r in recs]
        assert not any(s.strip("ACGT") for s in seqs), name
        assert min(min(r[2].encode()) for r in recs) - 33 > 2, name
        assert not any(a >= 2 or b >= 2 for a, b in zip(fc.match_ref(seqs, g), fc.match_ref(seqs, fc.rc(g)))), name
        kept, counts = fc.restate_fastq(recs, fc.params(rm_phix=True), g)
        assert counts == (len(recs), len(recs)) and kept == recs, name         # the defaults keep these reads as they are
        if name in kept_240:
            kept, counts = fc.restate_fastq(recs, fc.params(trunc_len=240, max_ee=2, rm_phix=True), g)
            assert counts == (1500, kept_240[name]) and {len(r[1]) for r in kept} == {240}, (name, counts)


def test_restated_stage_order_and_edges():
    P = fc.params
    r = lambda s, q, **kw: fc.restate_read(s, q, P(**kw), fc.phix())   # noqa: E731
    s30, q30 = "ACGT" * 7 + "AC", "I" * 30
    assert r(s30, q30)["code"] == 0 and r(s30, q30, max_len=29)["code"] == 1 and r(s30, q30, max_len=30)["code"] == 0
    assert r(s30, q30, trim_left=30)["code"] == 2                              # exactly trimLeft bases: dropped
    assert r(s30, q30, trim_left=29, min_len=0) == {"code": 0, "off": 29, "len": 1, "ee": fc.matrix_ee([40]), "hits": (0, 0)}
    assert r(s30, q30, trim_right=30)["code"] == 3 and r(s30, q30, trim_right=29, min_len=0)["len"] == 1
    assert r(s30, "#" + q30[1:])["code"] == 4 and r(s30, "I#" + q30[2:], min_len=0)["len"] == 1
    assert r(s30, q30, trunc_len=31)["code"] == 5 and r(s30, q30, trunc_len=30)["len"] == 30
    assert r(s30, q30, trim_left=5, trunc_len=4)["len"] == 25                  # truncLen < start: no truncation
    assert r(s30, q30, trim_left=5, trunc_len=25)["len"] == 20 and r(s30, q30, trim_left=5, trunc_len=31)["code"] == 5
    assert r(s30, q30, min_len=31)["code"] == 6
    assert r("N" + s30[1:], q30)["code"] == 7 and r("n" + s30[1:], q30, max_n=1)["code"] == 0
    assert r(s30, "+" + q30[1:], min_q=10)["code"] == 8 and r(s30, "+" + q30[1:], min_q=9)["code"] == 0   # min(q) > minQ, strict
    assert r(s30, "+" + q30[1:], min_q=2)["code"] == 0                         # minQ <= truncQ: not applied
    assert r(s30[:20], "+" * 20, max_ee=2)["code"] == 9 and r(s30[:19], "+" * 19, max_ee=2, min_len=0)["code"] == 0
    g = fc.phix()
    assert r(g[:40], "I" * 40, rm_phix=True)["code"] == 10 and r(g[:40], "I" * 40)["code"] == 0
    assert r("A" * 40, "I" * 40, rm_lowcomplex=1.5)["code"] == 11 and r(s30, q30, rm_lowcomplex=1.5)["code"] == 0
    # the first failed stage is reported: a read that is too long AND full of N
    assert r("N" * 40, "I" * 40, max_len=30)["code"] == 1 and r("N" * 40, "#" * 40)["code"] == 4


def test_case_builders_are_deterministic_and_off_the_thresholds():
    a, b = fc.screen_reads(), fc.screen_reads()
    assert a == b and len(a[0]) == len(a[1])
    seqs = fc.complexity_reads()
    for k in (1, 2, 3, 4):
        for t in fc.lowcomplex_thresholds(seqs, k):                              # asserts: no restated value within 1e-9 of t
            assert any(fc.complexity(s, k) >= t for s in seqs) and any(fc.complexity(s, k) < t for s in seqs)
    assert fc.kmer_counts("ACGTN", 2) == [0, 1, 0, 0] + [0, 0, 1, 0] + [0, 0, 0, 1] + [0, 0, 0, 0]
    assert math.isnan(fc.complexity("NNNN")) and fc.complexity("A" * 10) == 1.0
    assert abs(fc.complexity("ACGT" * 8 + "A", 1) - 4.0) < 0.01
    assert set(fc.LENGTHS) >= {0, 1, 15, 16, 17, 19, 20, 21, 63, 64, 65, 127, 128, 129, 250, 251, 301, 5000}


def test_filter_params_struct_layout(tmp_path):
    P = _lib.CFilterParams
    assert C.sizeof(P) == 72
    offs = {n: getattr(P, n).offset for n, _ in P._fields_}
    assert [offs[n] for n in ("trunc_q", "trunc_len", "trim_left", "trim_right", "max_len", "min_len", "max_n", "min_q")] == list(range(0, 32, 4))
    assert offs["max_ee"] == 32 and offs["rm_lowcomplex"] == 40
    assert [offs[n] for n in ("rm_phix", "min_matches", "non_overlapping", "kmer_size", "qual_offset", "reserved")] == list(range(48, 72, 4))
    p = api.filter_params()
    assert (p.trunc_q, p.trunc_len, p.trim_left, p.trim_right, p.max_len, p.min_len, p.max_n, p.min_q) == (2, 0, 0, 0, 0, 20, 0, 0)
    assert math.isinf(p.max_ee) and p.rm_lowcomplex == 0 and (p.rm_phix, p.min_matches, p.non_overlapping, p.kmer_size, p.qual_offset) == (0, 2, 1, 0, 0)
    q = api.filter_params(1, trunc_len=(240, 160), max_ee=(2, 5), max_len=300.0, trim_left=[3])
    assert (q.trunc_len, q.max_ee, q.max_len, q.trim_left) == (160, 5.0, 300, 3)
    with pytest.raises(ValueError):
        api.filter_params(trunc_len=(1, 2, 3))
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc:                                                                       # the header's own view of the struct
        src = tmp_path / "layout.c"
        names = [n for n, _ in P._fields_]
        src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "dada2hip.h"\nint main(void) { printf("%zu", sizeof(dada2hip_filter_params));\n'
                       + "".join('printf(" %%zu", offsetof(dada2hip_filter_params, %s));\n' % n for n in names) + "return 0; }\n")
        exe = tmp_path / "layout"
        subprocess.check_call([cc, "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
        got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
        assert got == [72] + [offs[n] for n in names]


def test_stats_names_cover_the_header():
    assert len(_lib.FILTER_STATS) == 26 and _lib.FILTER_NSTATS == 32
    assert _lib.FILTER_STATS.index("table_keys") == 13 and _lib.FILTER_STATS.index("total_us") == 24
    assert _lib.FILTER_STATS[2:13] == tuple("dropped_" + s for s in fc.STAGES[1:]) and _lib.FILTER_STAGES == fc.STAGES


def test_arguments_decided_before_the_library(tmp_path):
    src = fc.FASTQS["sam1F"]
    out = str(tmp_path / "o.fastq.gz")
    for kw in ({"orient_fwd": "ACGT"}, {"match_ids": True}, {"id_sep": ":"}, {"id_field": 2}):
        with pytest.raises(NotImplementedError, match="not supported"):
            api.filter_and_trim(src, out, **kw)
    with pytest.raises(TypeError):
        api.filter_and_trim(src, out, no_such_argument=1)
    with pytest.raises(NotImplementedError, match="not supported"):
        api.seq_complexity(["ACGT"], window=25)
    with pytest.raises(ValueError, match="do not exist"):
        api.filter_and_trim(str(tmp_path / "missing.fastq"), out)
    with pytest.raises(ValueError, match="corresponding output file"):
        api.filter_and_trim([src, fc.FASTQS["sam2F"]], [out, out, out])
    with pytest.raises(ValueError, match="must be distinct"):
        api.filter_and_trim([src, fc.FASTQS["sam2F"]], [out, out])
    with pytest.raises(ValueError, match="distinct from the input"):
        api.filter_and_trim(src, src)
    with pytest.raises(ValueError, match="reverse reads are required"):
        api.filter_and_trim(src, out, rev=fc.FASTQS["sam1R"])
    with pytest.raises(ValueError, match="ships no copy"):
        api.filter_and_trim(src, out, rm_phix=True)
    with pytest.raises(FileNotFoundError):
        api.FilterContext(str(tmp_path / "no_genome.fa"))
    assert not os.path.exists(out)


def test_no_cpu_fallback_without_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    with pytest.raises(_lib.Dada2HipError) as ei:
        api.FilterContext(fc.PHIX_FA)
    assert ei.value.code == 2 and "no HIP device" in str(ei.value)
    with pytest.raises(_lib.Dada2HipError) as ei:                                # validation comes before the device
        api.FilterContext(fc.phix(), 33)
    assert ei.value.code == 4
