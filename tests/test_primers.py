"""removePrimers' restatement (tests/primer_cases.py) on the CPU: the reference's example file with its documented call, and each
quirk of the semantics one at a time.  The example's figures were computed by a restatement written from R/filter.R; on that file
no match hangs over a read's end and no read has a second match of a primer (asserted below), so they do not depend on the rule
for the range of match starts, which nobody has checked against Biostrings."""
import pytest

import primer_cases as pc

REV = pc.rc(pc.R1492)


@pytest.fixture(scope="module")
def example():
    return pc.read_fastq(pc.EXAMPLE)


def test_the_documented_call():
    assert REV == "AAGTCGTAACAAGGTARCY" and pc.F27 == "AGRGTTYGATYMTGGCTCAG"


def test_example_file_is_the_reference_s(example):
    lens = [len(s) for _, s, _ in example]
    assert len(example) == 50 and (min(lens), max(lens)) == (1529, 2129)
    assert all(set(s) <= set("ACGT") and len(s) == len(q) for _, s, q in example)


@pytest.mark.parametrize("rev, orient, kept, flipped, shortest, longest", [
    (REV, True, 45, 25, 1458, 1500),
    (None, True, 45, 25, 1493, 1535),
    (REV, False, 20, 0, 1464, 1500),
    (None, False, 20, 0, 1499, 1535),
])
def test_example_file(example, rev, orient, kept, flipped, shortest, longest):
    want = [pc.restate_read(s, pc.F27, rev, max_mismatch=2, orient=orient) for _, s, _ in example]
    nin, out = pc.restate_fastq(example, pc.F27, rev, max_mismatch=2, orient=orient)
    lens = [len(s) for _, s, _ in out]
    assert (nin, len(out), sum(w["flip"] for w in want), min(lens), max(lens)) == (50, kept, flipped, shortest, longest)
    assert all(len(s) == len(q) for _, s, q in out)
    # what makes the figures independent of the unverified rules: no second match, none over an end
    for (_, s, _), w in zip(example, want):
        assert max(w["hits"]) <= 1
        for k, L in enumerate((20, 19, 20, 19)):
            if w["hits"][k]:
                assert 1 <= w["starts"][2 * k] <= len(s) - L + 1


def test_a_flipped_record_is_the_reverse_complement_with_reversed_qualities(example):
    _, out = pc.restate_fastq(example, pc.F27, REV)
    by_id = {h: (s, q) for h, s, q in example}
    n = 0
    for (h, s, q), w in zip(out, [w for w in (pc.restate_read(x, pc.F27, REV) for _, x, _ in example) if w["code"] == 0]):
        src_s, src_q = by_id[h]
        if w["flip"]:
            n += 1
            assert s == pc.rc(src_s)[w["first"] - 1: w["last"]] and q == src_q[::-1][w["first"] - 1: w["last"]]
            assert pc.rc(s) in src_s
        else:
            assert s in src_s
    assert n == 25


FWD, RV = "ACGTTGCAAGGTCCATCA", "GGATTACAGATTACAGCC"


def test_match_range_and_out_of_limits():
    read = "TTTTT" + FWD + "TTTTT"
    assert pc.vmatch(FWD, read, 0, True) == [5] and pc.vmatch(FWD, read, 2, True) == [5]
    assert pc.start_range(28, 18, 2) == (-2, 12) and pc.start_range(28, 18, 0) == (0, 10)
    assert pc.vmatch(FWD, FWD[1:] + "TTTT", 1, True) == [-1] and pc.vmatch(FWD, FWD[1:] + "TTTT", 0, True) == []
    assert pc.vmatch(FWD, FWD[2:] + "TTTT", 2, True) == [-2] and pc.vmatch(FWD, FWD[3:] + "TTTT", 2, True) == []
    assert pc.vmatch(FWD, "TTTT" + FWD[:-2], 2, True) == [4] and pc.vmatch(FWD, "TTTT" + FWD[:-3], 2, True) == []
    assert pc.vmatch(FWD, "", 2, True) == [] and pc.vmatch("AC", "A", 1, True) == [0]


def test_the_two_comparison_rules():
    assert pc.is_acgt(FWD) and not pc.is_acgt(pc.F27) and not pc.is_acgt("ACGN")
    assert pc.vmatch("ACGT", "ACNT", 0, True) == [] and pc.vmatch("ACGT", "ACNT", 0, False) == [0]
    assert pc.vmatch("ACRT", "ACNT", 0, False) == [0] and pc.vmatch("ACRT", "ACYT", 0, False) == [] and pc.vmatch("ACRT", "ACMT", 0, False) == [0]
    assert pc.rc("ACGTMRWSYKVHDBN") == "NVHDBMRSWYKACGT"
    assert pc.restate_read("ACGTTGCAxGGT", FWD)["code"] == 4 and pc.restate_read("ACGTTGCAUGGT", FWD)["code"] == 4


def test_first_of_forward_last_of_reverse():
    read = "TT" + FWD + "AAAA" + FWD + "CCCCCC" + RV + "AAAA" + RV + "TT"
    w = pc.restate_read(read, FWD, RV, max_mismatch=0)
    assert w["hits"][:2] == (2, 2) and w["starts"][:4] == (3, 25, 49, 71)
    assert (w["code"], w["first"], w["last"]) == (0, 21, 70)
    w = pc.restate_read(pc.rc(read), FWD, RV, max_mismatch=0)
    assert (w["code"], w["flip"], w["first"], w["last"]) == (0, 1, 21, 70) and w["starts"][4:] == (3, 25, 49, 71)


def test_flip_only_without_a_forward_match_as_given():
    both = FWD + "AAAAAAAAAA" + pc.rc(FWD) + "CCCCCCCCCC" + RV
    assert pc.restate_read(both, FWD, RV, max_mismatch=0)["flip"] == 0
    split = FWD + "AAAAAAAAAA" + pc.rc(RV)
    w = pc.restate_read(split, FWD, RV, max_mismatch=0)
    assert (w["code"], w["flip"], w["hits"]) == (2, 0, (1, 0, 0, 1))
    assert pc.restate_read(pc.rc(both), FWD, RV, max_mismatch=0, orient=False)["code"] == 2   # (rc(both) holds FWD as given too, but RV on the other strand only)
    assert pc.restate_read(pc.rc(split), FWD, RV, max_mismatch=0, orient=False)["code"] == 1


def test_window_is_strict():
    mk = lambda gap: "TTTTT" + FWD + "A" * gap + RV   # noqa: E731
    assert [pc.restate_read(mk(g), FWD, RV, max_mismatch=0)["code"] for g in (0, 1, 2, 3)] == [3, 3, 0, 0]
    w = pc.restate_read(mk(2), FWD, RV, max_mismatch=0)
    assert (w["first"], w["last"]) == (24, 25)
    w = pc.restate_read(mk(2), FWD, RV, max_mismatch=0, trim_fwd=False, trim_rev=False)
    assert (w["first"], w["last"]) == (1, len(mk(2)))
    assert pc.restate_read(RV + "AAAAAAAAAA" + FWD, FWD, RV, max_mismatch=0)["code"] == 3


def test_whole_file_rule_counts_the_reads_as_given():
    recs = [("@a", pc.rc("TT" + FWD + "ACGTACGTAC" + RV + "TT"), "I" * 50)] * 3
    assert all(pc.restate_read(s, FWD, RV)["code"] == 0 for _, s, _ in recs)
    assert pc.restate_fastq(recs, FWD, RV) == (3, [])
    recs = recs + [("@b", "TT" + FWD + "ACGTACGTAC" + RV + "TT", "I" * 50)]
    assert len(pc.restate_fastq(recs, FWD, RV)[1]) == 4
    assert pc.restate_fastq(recs[:3] + [("@c", "TT" + FWD + "ACGTACGTAC", "I" * 30)], FWD, RV) == (4, [])
