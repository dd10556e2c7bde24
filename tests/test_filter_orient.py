"""orient.fwd and matchIDs without a device: the restatement of tests/filter_orient_cases.py pinned to hand-worked examples, what
dada2_amd/filtering.py decides before it reaches the library, the bindings, and the promise that without the new arguments
dada2_amd.filtering's functions are dada2_amd.api's."""
import ctypes as C
import os

import pytest

import filter_cases as fc
import filter_orient_cases as oc
from dada2_amd import _lib, api, filtering

P0 = fc.params(min_len=0, quality_type=33)


def rec(i, s, q=None):
    return ("@r%d" % i, s, q or "I" * len(s))


def test_single_end_examples():
    b = "ACG"
    assert oc.orient_of("ACGTT", b) == 0 and oc.orient_of("AACGT", b) == 1 and oc.orient_of("ACGCGT", b) == 0 and oc.orient_of("TTTTT", b) == 2
    v = oc.restate_read_oriented("AACGT", "ABCDE", b, P0)
    assert (v["seq"], v["qual"], v["code"], v["orient"]) == ("ACGTT", "EDCBA", 0, 1)
    assert oc.restate_read_oriented("TTTTT", "IIIII", b, P0)["code"] == 12 and oc.STAGES[12] == "orient" == filtering.STAGES[12]
    recs = [rec(0, "AACGT", "ABCDE"), rec(1, "ACGTT"), rec(2, "TTTTT"), rec(3, "ACGCGT"), rec(4, "TTCGT"), rec(5, "ACGAA")]
    kept, counts = oc.restate_fastq_oriented(recs, b, P0, n=10)
    assert counts == (6, 5)
    assert kept == [rec(1, "ACGTT"), rec(3, "ACGCGT"), rec(5, "ACGAA"), ("@r0", "ACGTT", "EDCBA"), rec(4, "ACGAA")]
    # every as-given read of a chunk, then every flipped one: the order depends on n
    by_n = {n: [r[0] for r in oc.restate_fastq_oriented(recs, b, P0, n=n)[0]] for n in (2, 4, 6)}
    assert by_n[2] == ["@r1", "@r0", "@r3", "@r5", "@r4"] and by_n[4] == ["@r1", "@r3", "@r0", "@r5", "@r4"] and by_n[6] == ["@r1", "@r3", "@r5", "@r0", "@r4"]
    # the stages see the flipped read: the truncQ cut is the first low quality from ITS left end
    v = oc.restate_read_oriented("TTTTTTTCGT", "IIII#IIIII", b, fc.params(min_len=0))
    assert (v["seq"], v["off"], v["len"]) == ("ACGAAAAAAA", 0, 5)
    # IUPAC letters are complemented as the writer does, lower case and N stay
    assert oc.rc_iupac("ACGTMKRYVBHDWSNacgt-") == "-tgcaNSWHDVBRYMKACGT" and oc.rc_iupac("AM") == "KT"
    with pytest.raises(oc.ShortRead, match="record 3 .@r2."):
        oc.restate_fastq_oriented([rec(0, "ACGT"), rec(1, "ACGA"), rec(2, "AC")], b, P0, n=2)
    for bad in ("", "ACN", "acg"):
        with pytest.raises(ValueError):
            oc.restate_fastq_oriented(recs, bad, P0)


def ids(recs):
    return [r[0][1:] for r in recs]


def pairs(names_f, names_r):
    return [("@" + x, "ACGTACGTAC", "IIIIIIIIII") for x in names_f], [("@" + x, "TTGCATTGCA", "IIIIIIIIII") for x in names_r]


def test_match_ids_examples():
    rf, rr = pairs("abcd", "bced")
    kf, kr, counts = oc.restate_paired_ex(rf, rr, P0, n=2, match_ids=True, id_field=1)
    assert ids(kf) == ids(kr) == ["b", "c", "d"] and counts == (4, 3)
    rf, rr = pairs("abcd", "cabd")
    kf, kr, counts = oc.restate_paired_ex(rf, rr, P0, n=2, match_ids=True, id_field=1)
    assert ids(kf) == ids(kr) == ["a", "b", "d"]
    kf, kr, counts = oc.restate_paired_ex(rf, rr, P0, n=4, match_ids=True, id_field=1)   # same membership, another order: mis-paired, as the reference
    assert ids(kf) == ["a", "b", "c", "d"] and ids(kr) == ["c", "a", "b", "d"]
    # one file runs out first; the loop ends when both yield nothing, the remainders are dropped
    rf, rr = pairs("abcdef", "bdf")
    kf, kr, counts = oc.restate_paired_ex(rf, rr, P0, n=2, match_ids=True, id_field=1)
    assert ids(kf) == ids(kr) == ["b", "d", "f"] and counts == (6, 3)
    # without matchIDs: the old error
    with pytest.raises(ValueError, match="Mismatched forward and reverse sequence files: 2, 1."):
        oc.restate_paired_ex(rf, rr, P0, n=2)


def test_id_fields():
    assert oc.detect_id_field("M01:1:A:1:2:3:4 1:N:0:1") == (1, "Current")
    assert oc.detect_id_field("x M01:1:A:1:2:3:4") == (2, "Current")
    assert oc.detect_id_field("X:1:2:3:4#0/1") == (1, "Old")
    for bad in ("plain", "", "a:b:c:d:e:f:g h:i:j:k:l:m:n", "a:b:c:d:e a:b:c:d:e", "a:b:c:d:e:f"):
        with pytest.raises(oc.NoIdField, match="Couldn't automatically detect the sequence identifier field"):
            oc.detect_id_field(bad)
    assert oc.r_strsplit("a  b ") == ["a", "", "b"] and oc.r_strsplit(" a") == ["", "a"] and oc.r_strsplit("") == []
    assert oc.r_strsplit("a\tb\rc") == ["a", "b", "c"] and oc.r_strsplit("a b:c", ":") == ["a b", "c"]
    assert oc.id_field_of("a b", "\\s", 3) is None and oc.id_field_of("a  b", "\\s", 2) == ""
    # the Old format's quirk: '#...' leaves the FORWARD ids only, so the two files of a pair match nothing
    rf, rr = pairs(["X:1:2:3:4#0/1"], ["X:1:2:3:4#0/2"])
    assert oc.restate_paired_ex(rf, rr, P0, match_ids=True)[2] == (1, 0)
    rf, rr = pairs(["X:1:2:3:4#0/1"], ["X:1:2:3:4"])
    assert oc.restate_paired_ex(rf, rr, P0, match_ids=True)[2] == (1, 1)
    # a missing field is NA, and NA matches NA
    rf, rr = pairs(["a x", "b"], ["c", "d y"])
    kf, kr, _ = oc.restate_paired_ex(rf, rr, P0, match_ids=True, id_field=2)
    assert ids(kf) == ["b"] and ids(kr) == ["c"]
    # duplicate ids: kept lists of unequal length are an error
    rf, rr = pairs("aab", "ab")
    with pytest.raises(oc.DuplicateIds):
        oc.restate_paired_ex(rf, rr, P0, match_ids=True, id_field=1)


def test_paired_orientation_examples():
    b = "ACG"
    rf = [("@f0", "ACGTTTTTTT", "I" * 10), ("@f1", "TTTTTTTTTT", "I" * 10), ("@f2", "ACGAAAAAAA", "I" * 10), ("@f3", "GGGGGGGGGG", "I" * 10)]
    rr = [("@r0", "CCCCCCCCCC", "I" * 10), ("@r1", "ACGCCCCCCC", "I" * 10), ("@r2", "ACGGGGGGGG", "I" * 10), ("@r3", "TTTTTTTTTT", "I" * 10)]
    kf, kr, counts = oc.restate_paired_ex(rf, rr, fc.params(min_len=0, trunc_len=(8, 5)), n=10, orient_fwd=b)
    # pair 1 is swapped (no reverse complement), judged by the other direction's truncLen and written behind the others; pair 3 is dropped
    assert kf == [("@f0", "ACGTTTTT", "I" * 8), ("@f2", "ACGAAAAA", "I" * 8), ("@r1", "ACGCCCCC", "I" * 8)]
    assert kr == [("@r0", "CCCCC", "I" * 5), ("@r2", "ACGGG", "I" * 5), ("@f1", "TTTTT", "I" * 5)] and counts == (4, 3)
    with pytest.raises(oc.ShortRead, match="record 2 .@r1."):
        oc.restate_paired_ex(rf, [rr[0], ("@r1", "AC", "II")] + rr[2:], P0, orient_fwd=b)


def test_argument_errors(tmp_path):
    x = str(tmp_path / "x.fastq.gz")
    src = fc.FASTQS["sam1F"]
    for bad, exc in (("", ValueError), ("ACGN", ValueError), ("acgt", ValueError), ("A" * 257, NotImplementedError)):
        for call in (lambda: filtering.fastq_filter(src, x, orient_fwd=bad), lambda: filtering.filter_and_trim(src, x, orient_fwd=bad),
                     lambda: filtering.fastq_paired_filter((src, fc.FASTQS["sam1R"]), (x, x + "2"), orient_fwd=bad),
                     lambda: filtering.filter_reads(["ACGT"], ["IIII"], None, orient_fwd=bad)):
            with pytest.raises(exc):
                call()
    with pytest.raises(ValueError, match="Non-ACGT characters detected in orient.fwd"):
        filtering.check_orient_fwd("ACGU")
    two = ((src, fc.FASTQS["sam1R"]), (x, x + "2"))
    for sep in ("ab", ".", "|", "\\d", "[", ""):
        with pytest.raises(NotImplementedError, match="id_sep"):
            filtering.fastq_paired_filter(*two, match_ids=True, id_sep=sep)
    for field in (0, -1, 1.5):
        with pytest.raises(ValueError, match="id_field"):
            filtering.fastq_paired_filter(*two, match_ids=True, id_field=field)
    assert filtering.check_id_args(None, None) == (b"\\s", 0) and filtering.check_id_args(":", 2) == (b":", 2)
    with pytest.raises(TypeError):
        filtering.fastq_paired_filter(*two, match_ids=True, no_such_argument=1)
    with pytest.raises(ValueError, match="paired needs orient_fwd"):
        filtering.filter_reads(["ACGT"], ["IIII"], None, paired=True)
    assert not os.path.exists(x) and not os.path.exists(x + "2")
    # api still refuses all four, and knows nothing of this module
    assert not hasattr(api, "filtering") and set(("orient_fwd", "match_ids", "id_sep", "id_field")) <= set(api._FILTER_REFUSED)


def test_bindings_and_stats_words():
    assert {"dada2hip_filter_reads_oriented", "dada2hip_filter_fastq_oriented", "dada2hip_filter_fastq_paired_ex"} <= set(_lib.EXPORTS)
    assert filtering.STATS[:26] == _lib.FILTER_STATS and len(_lib.FILTER_STATS) == 26
    assert filtering.STATS[26:] == ("dropped_orient", "flipped", "dropped_ids", "orient_device_us", "id_join_us")
    assert len(filtering.STATS) <= _lib.FILTER_NSTATS and filtering.STAGES[:12] == _lib.FILTER_STAGES == fc.STAGES
    assert C.sizeof(_lib.CFilterParams) == 72
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "dada2hip.h")).read()
    for name in ("dada2hip_filter_reads_oriented", "dada2hip_filter_fastq_oriented", "dada2hip_filter_fastq_paired_ex"):
        assert ("int %s(" % name) in hdr


def test_without_the_new_arguments_the_functions_are_apis(monkeypatch):
    """Without a device: which function of api is reached, and with which arguments."""
    calls = []

    def spy(name):
        def f(*a, **k):
            calls.append((name, a, k))
            return (7, 5)
        return f
    for name in ("filter_reads", "fastq_filter", "fastq_paired_filter"):
        monkeypatch.setattr(api, name, spy(name))
    assert filtering.fastq_filter("a", "b", trunc_len=9, n=3) == (7, 5)
    assert filtering.fastq_filter("a", "b", trunc_len=9, match_ids=True, id_sep="x", id_field=4) == (7, 5)   # single-end: ignored
    assert filtering.fastq_paired_filter(("a", "b"), ("c", "d"), max_ee=(2, 3), match_ids=False, id_field=None) == (7, 5)
    filtering.filter_reads(["ACGT"], ["IIII"], "ctx", kmers=True, max_n=1)
    assert [c[0] for c in calls] == ["fastq_filter", "fastq_filter", "fastq_paired_filter", "filter_reads"]
    assert calls[0][1] == ("a", "b") and calls[0][2]["trunc_len"] == 9 and calls[0][2]["n"] == 3
    assert all(not set(c[2]) & {"orient_fwd", "match_ids", "id_sep", "id_field", "paired"} for c in calls)
    assert calls[2][2]["max_ee"] == (2, 3) and calls[3][1][:3] == (["ACGT"], ["IIII"], "ctx") and calls[3][2]["kmers"] is True
