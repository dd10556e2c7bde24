"""The restatements of tests/readqc_cases.py, held to what can be known without a GPU: the per-cycle quality table against an
independent per-character count on the three FASTQ fixtures, the invariants of plotQualityProfile's statistics on them, the
reference's own seqComplexity example, and the refusals that dada2_amd.readqc and the library make before any device work."""
import numpy as np
import pytest

import readqc_cases as rc


@pytest.fixture(scope="module")
def fixtures():
    return {name: rc.read_fastq(path) for name, path in rc.FIXTURES.items()}


@pytest.fixture(scope="module")
def profiles(fixtures):
    return {name: rc.restate_profile([(name + ".fastq.gz", [q for _, _, q in recs])]) for name, recs in fixtures.items()}


def test_fixtures_are_what_the_cases_assume(fixtures):
    f, r, pb = (fixtures[k] for k in ("sam1F", "sam1R", "samPB"))
    assert len(f) == len(r) == 1500 and {len(s) for _, s, _ in f} == {250}
    letters = {ch for _, _, q in f for ch in q}
    assert (min(letters), max(letters)) == ("(", "G")
    assert len(pb) == 500 and (min(len(s) for _, s, _ in pb), max(len(s) for _, s, _ in pb)) == (1456, 1511)
    letters = {ch for _, _, q in pb for ch in q}
    assert (min(letters), max(letters)) == ("%", "~")


@pytest.mark.parametrize("name", tuple(rc.FIXTURES))
def test_restated_table_equals_a_naive_count(fixtures, profiles, name):
    quals = [q for _, _, q in fixtures[name]]
    naive = rc.naive_counts(quals)
    tab = rc.restate_table(quals)
    assert int(tab.sum()) == sum(naive.values()) == sum(len(q) for q in quals)
    cyc, col = np.nonzero(tab)
    assert {(int(c) + 1, int(j) + 33): int(tab[c, j]) for c, j in zip(cyc, col)} == naive
    df = profiles[name]["files"][0]["table"]                        # Count > 0 rows only, by cycle, then by ascending score
    assert (df["count"] > 0).all() and len(df["count"]) == len(naive)
    order = np.lexsort((df["score"], df["cycle"]))
    assert (order == np.arange(len(order))).all()
    assert {(int(c), int(s) + 33): int(n) for c, s, n in zip(df["cycle"], df["score"], df["count"])} == naive


@pytest.mark.parametrize("name", tuple(rc.FIXTURES))
def test_profile_invariants(fixtures, profiles, name):
    lens = np.array([len(q) for _, _, q in fixtures[name]])
    e = profiles[name]["files"][0]
    st, df = e["stats"], e["table"]
    assert e["rc"] == e["profiled"] == len(lens) and e["qual_offset"] == 33
    assert st["Cycle"].tolist() == list(range(1, lens.max() + 1))
    totals = np.bincount(df["cycle"], weights=df["count"])[1:]
    assert totals.tolist() == [int((lens >= c).sum()) for c in st["Cycle"]]   # a cycle's total: the reads at least that long
    assert st["Cum"][0] == 10.0 and (np.diff(st["Cum"]) <= 0).all()
    assert (st["Q25"] <= st["Q50"]).all() and (st["Q50"] <= st["Q75"]).all()
    lo = np.array([df["score"][df["cycle"] == c].min() for c in st["Cycle"]])
    hi = np.array([df["score"][df["cycle"] == c].max() for c in st["Cycle"]])
    assert (lo <= st["Q25"]).all() and (st["Q75"] <= hi).all() and (lo <= st["Mean"]).all() and (st["Mean"] <= hi).all()
    assert profiles[name]["minScore"] == df["score"].min() == e["minScore"]


def test_n_profiles_the_first_records_and_counts_the_file(fixtures):
    quals = [q for _, _, q in fixtures["sam1F"]]
    got = rc.restate_profile([("sam1F.fastq.gz", quals)], n=1000)["files"][0]
    first = rc.restate_profile([("sam1F.fastq.gz", quals[:1000])])["files"][0]
    assert got["rc"] == 1500 and got["profiled"] == 1000 and first["rc"] == 1000
    rc.assert_same_frames(got, first, "n = 1000")                   # (Cum too: 10 * 1000 / min(1500, 1000))
    above = rc.restate_profile([("sam1F.fastq.gz", quals)], n=5000)["files"][0]
    rc.assert_same_frames(above, rc.restate_profile([("sam1F.fastq.gz", quals)])["files"][0], "n above rc")


def test_aggregate_sums_the_tables_and_the_denominators(fixtures):
    qf, qr = ([q for _, _, q in fixtures[k]] for k in ("sam1F", "sam1R"))
    agg = rc.restate_profile([("f", qf), ("r", qr)], n=1000, aggregate=True)["aggregate"]
    both = rc.restate_profile([("fr", qf[:1000] + qr[:1000])])["files"][0]
    for k in ("cycle", "score", "count"):
        assert np.array_equal(agg["table"][k], both["table"][k]), k
    assert agg["rc"] == 3000 and agg["stats"]["Cum"][0] == 10.0     # 10 * 2000 / (min(1500, 1000) + min(1500, 1000))
    for k in ("Mean", "Q25", "Q50", "Q75"):
        assert np.array_equal(agg["stats"][k], both["stats"][k]), k


def test_get_quant_is_the_first_score_at_or_above_the_fraction():
    xx, yy = np.array([2, 10, 30, 40]), np.array([1, 1, 1, 1])
    assert [rc.get_quant(xx, yy, q) for q in (0.25, 0.5, 0.75, 0.76)] == [2, 10, 30, 40]
    assert rc.get_quant(np.array([5, 6]), np.array([1, 3]), 0.25) == 5 and rc.get_quant(np.array([5, 6]), np.array([1, 3]), 0.26) == 6


def test_the_references_complexity_example():
    sqs = [rc.SQ_NORM, rc.SQ_LOWC, rc.SQ_PART]                      # filter.R:1241-1246
    whole = rc.restate_complexity(sqs)
    win = rc.restate_complexity(sqs, kmer_size=3, window=25)
    assert whole[0] > 12 and whole[1] < 5 and whole[2] > 8          # the half-and-half sequence passes as a whole ...
    assert win[0] > 2 * win[2] and abs(win[2] - win[1]) < 1         # ... and is found by the window: as low as the low one
    assert (win <= 64).all() and (whole <= 16).all()
    # by hand: a window of ACGTACGTAC..., k = 1: four letters equally often
    assert abs(rc.restate_complexity(["ACGT" * 6, "A" * 30], kmer_size=1, window=8, by=4)[0] - 4.0) < 1e-12


def test_the_window_loops_quirks_are_the_r_codes():
    body = "ACGTTGCAGTCAAGCTTAGCCATGGATCGATTACGGCTAAGCTAGCTAG"
    low = "T" * 12
    si = rc.restate_complexity([body + low, body[1:] + low, "ACGTACGTAC"], window=12, by=1)
    assert si[0] > 1.0 and si[1] == 1.0 and si[2] == 16.0           # the longest read's last window is never tested; a short read keeps 4^k
    assert np.isnan(rc.restate_complexity(["ACGT" * 5 + "N" * 13 + "ACGT" * 5, "ACGT" * 12], window=12, by=1)[0])
    with pytest.raises(ValueError, match="larger than the kmerSize"):
        rc.restate_complexity([body], kmer_size=3, window=3)
    with pytest.raises(ValueError):
        rc.restate_complexity([body], window=len(body))


def test_module_surface_and_refusals_before_the_device():
    from dada2_amd import _lib, api, readqc
    for name in ("quality_table", "quality_profile", "seq_complexity", "complexity_profile"):
        assert callable(getattr(readqc, name))
    assert not hasattr(api, "plot_complexity") and not hasattr(api, "quality_profile") and not hasattr(api, "plot_quality_profile")
    with pytest.raises(NotImplementedError):
        api.seq_complexity(["ACGT" * 10], window=5)
    with pytest.raises(_lib.Dada2HipError, match="larger than the kmerSize") as ei:
        readqc.seq_complexity([rc.SQ_NORM], kmer_size=3, window=3)
    assert ei.value.code == 1
    with pytest.raises(_lib.Dada2HipError, match="1024") as ei:
        readqc.seq_complexity([rc.SQ_NORM], window=2000)
    assert ei.value.code == 4
    with pytest.raises(ValueError, match="larger than the kmerSize"):
        readqc.seq_complexity([rc.SQ_NORM], window=0)
    with pytest.raises(ValueError, match="directory"):
        readqc.quality_profile(rc.GOLDEN)
    with pytest.raises(_lib.Dada2HipError, match="directory"):
        readqc.quality_table_fastq(rc.GOLDEN)
    cyc = np.array([[0, 3, 0, 1], [2, 0, 0, 0]], dtype=np.int64)    # the module's own statistics on a table by hand
    st = readqc.cycle_stats(cyc, 10, 4)
    assert st["Cycle"].tolist() == [1, 2] and st["Mean"].tolist() == [(3 * 11 + 13) / 4, 10.0]
    assert (st["Q25"].tolist(), st["Q50"].tolist(), st["Q75"].tolist(), st["Cum"].tolist()) == ([11.0, 10.0], [11.0, 10.0], [11.0, 10.0], [10.0, 5.0])
    assert readqc.long_table(cyc, 10) == {"cycle": pytest.approx([1, 1, 2]), "score": pytest.approx([11, 13, 10]), "count": pytest.approx([3, 1, 2])}


def test_without_a_gpu_the_calls_fail_loudly():
    import torch
    if torch.cuda.is_available():
        return                                                      # (tests/test_gpu_readqc.py is this machine's)
    from dada2_amd import _lib, readqc
    for call in (lambda: readqc.quality_table(["IIII"]), lambda: readqc.seq_complexity([rc.SQ_NORM], window=25),
                 lambda: readqc.quality_table_fastq(rc.FIXTURES["sam1F"]), lambda: readqc.complexity_fastq(rc.FIXTURES["sam1F"], window=25)):
        with pytest.raises(_lib.Dada2HipError) as ei:
            call()
        assert ei.value.code == 2 and "no HIP device" in str(ei.value)
