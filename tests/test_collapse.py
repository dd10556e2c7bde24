"""The sequence-table stage without a GPU: the restatement of collapseNoMismatch the device tests compare with
(tests/collapse_cases.py) over the plain-C oracle against itself over the reference compiled in place, the pair-level fixture
(tests/golden/collapse_pairs.npz) and the rule the device's fast path rests on, and the host-only paths of the public interface:
de-duplication, empty and one-column tables, the error messages, make_sequence_table."""
import numpy as np
import pytest

import collapse_cases as cc


@pytest.fixture(scope="module")
def api():
    from dada2_amd import api as a
    return a


# ---- the restatement ------------------------------------------------------------------------------------------------------------------
def test_restatement_over_the_plain_c_oracle_equals_it_over_the_reference(oracle_c, oracle_ref):
    """The generated table (and the low-complexity one, where alignments tie): cport's C_nwalign + eval_pair decides every pair as
    the reference's C_nwvec (vec=TRUE) and C_nwalign (vec=FALSE) do, unbanded and with band 16."""
    for (mat, seqs), mo in ((cc.make_table(), 20), (cc.make_table(), 8), (cc.low_complexity_table(), 4)):
        for band in (-1, 16):
            a = cc.restate(mat, seqs, oracle_c, min_overlap=mo, band=band)
            for vec in (True, False):
                cc.assert_same_table(cc.restate(mat, seqs, oracle_ref, min_overlap=mo, band=band, vec=vec), a, (mo, band, vec))
            assert len(a[1]) < len(seqs)


def test_generated_table_holds_its_regimes(oracle_c):
    counts = cc.table_fact(*cc.make_table(), oracle_c)
    assert counts["columns"] == 320 and counts["kept"] < 200
    tr = {}
    cc.restate(*cc.make_table(), oracle_c, trace=tr)
    view = cc.batch_view(tr, 20, 16)
    assert len(view["own_batch"]) >= 5 and len(view["skipped"]) >= 5          # what the batch test on the device needs
    # (in batches of one the refs are exactly the kept columns: every pair the loop tried, and the ones behind a query's hit)
    assert cc.batch_view(tr, 20, 1)["screened"] >= sum(len(v) for v in tr["tried"].values()) == counts["screened"]


def test_restatement_orders_and_deduplicates_as_the_reference_does(oracle_c):
    # duplicates fold into the first occurrence; queries by total abundance, ties in table order; the output in input order, then
    # orderBy, then (stably) total abundance
    seqs = ["ACGTACGTAC", "TTTTTTTTGG", "ACGTACGTAC", "CGTACGTA", "GGGGGGGGCC"]
    mat = np.array([[3, 1, 2, 9, 1], [0, 4, 0, 0, 4]])
    out, names = cc.restate(mat, seqs, oracle_c, min_overlap=4)
    # CGTACGTA (9) is processed first and kept; ACGTACGTAC (5) contains it: joins it; the two 5s keep table order
    assert names == ["CGTACGTA", "TTTTTTTTGG", "GGGGGGGGCC"] and out.tolist() == [[14, 1, 1], [0, 4, 4]]
    out, names = cc.restate(mat, seqs, oracle_c, min_overlap=4, identical_only=True)
    assert names == ["ACGTACGTAC", "TTTTTTTTGG", "CGTACGTA", "GGGGGGGGCC"] and out.tolist() == [[5, 1, 9, 1], [0, 4, 0, 4]]
    three = ["AAAAAAAA", "CCCCCCCC", "GGGGGGGG"]
    out, names = cc.restate(np.array([[3, 1, 1], [0, 1, 1]]), three, oracle_c, order_by="nsamples")
    assert names == three                                                     # (nsamples 1, 2, 2 - but abundance 3, 2, 2 has the last word)
    out, names = cc.restate(np.array([[2, 1, 1], [0, 1, 1]]), three, oracle_c, order_by="nsamples")
    assert names == ["CCCCCCCC", "GGGGGGGG", "AAAAAAAA"]                      # (abundances tie: the nsamples order stays)


# ---- the pair-level fixture -------------------------------------------------------------------------------------------------------------
def test_pair_fixture_is_the_sweep_and_its_brute_force_scan():
    g = cc.golden()
    qs, rs, mo = cc.sweep_pairs()
    assert [str(x) for x in g["queries"]] == qs and [str(x) for x in g["refs"]] == rs and g["min_overlap"].tolist() == mo
    assert len(qs) == 6000 and {len(s) for s in qs + rs} == set(range(4, 41))
    for i in range(0, 6000, 7):
        assert tuple(int(x) for x in g["scan"][i]) == cc.brute_pair(qs[i], rs[i], mo[i]), i


def test_bound_never_rejects_a_pair_the_reference_collapses():
    """G > match x m_max  =>  nwhamming != 0, for either reference aligner; and the bound does not decide everything: at least
    100 pairs it lets through have a non-zero hamming (the ties only the traceback settles)."""
    g = cc.golden()
    rejects = g["scan"][:, 1] > cc.SCORES[0] * g["scan"][:, 2]
    assert rejects.sum() > 1000 and (~rejects).sum() > 1000
    for ev in (g["ev_vec"], g["ev_plain"]):
        ham = ev[:, 1] + ev[:, 2]
        assert not (rejects & (ham == 0)).any()
        assert (~rejects & (ham != 0)).sum() >= 100 and (~rejects & (ham == 0)).sum() > 1000
    assert np.array_equal(g["ev_vec"][:, 1] + g["ev_vec"][:, 2] == 0, g["ev_plain"][:, 1] + g["ev_plain"][:, 2] == 0)
    assert np.array_equal(g["scan"][:, 3], np.where(g["scan"][:, 0] == 0, 0, np.where(rejects, 1, 2)))
    assert len(set(g["scan"][:, 0].tolist())) == 4                            # no screen bit, either, both


def test_plain_c_oracle_gives_the_fixture_triples(oracle_c):
    g = cc.golden()
    for i in range(0, 6000, 5):
        assert cc.nweval(oracle_c, str(g["queries"][i]), str(g["refs"][i])) == tuple(int(x) for x in g["ev_plain"][i]), i


# ---- host-only paths of the interface ------------------------------------------------------------------------------------------------------
def test_identical_only_folds_duplicate_columns_without_a_device(api, oracle_c):
    mat, seqs = cc.with_duplicates(*cc.make_table())
    st = {}
    got = api.collapse_no_mismatch(mat, seqs, identical_only=True, stats=st)
    cc.assert_same_table(got, cc.restate(mat, seqs, oracle_c, identical_only=True), "identical_only")
    assert got[1] == list(dict.fromkeys(seqs)) and st["columns_dedup"] == len(seqs) - 25 and st["pairs_scanned"] == 0
    first = {s: seqs.index(s) for s in set(seqs)}
    assert st["into"].tolist() == [first[s] for s in seqs]
    assert got[0].dtype == np.int32 and got[0].sum() == mat.sum()
    # letters outside A/C/G/T are names like any other here (the reference returns before it aligns anything)
    m, names = api.collapse_no_mismatch([[1, 2, 3]], ["ANNA", "ACGT", "ANNA"], identical_only=True)
    assert names == ["ANNA", "ACGT"] and m.tolist() == [[4, 2]]


def test_empty_table_and_one_column(api, capsys):
    m, names = api.collapse_no_mismatch(np.zeros((3, 0), dtype=np.int32), [])
    assert m.shape == (3, 0) and names == []
    st = {}
    m, names = api.collapse_no_mismatch([[4], [0]], ["ACGTTGCA"], stats=st, verbose=True)
    assert m.tolist() == [[4], [0]] and names == ["ACGTTGCA"] and st["columns_dedup"] == 1 and st["batches"] == 0
    assert capsys.readouterr().out == "Output 1 collapsed sequences out of 1 input sequences.\n"
    m, names = api.collapse_no_mismatch([[4, 1, 2]], ["ACGTTGCA"] * 3)             # one distinct name
    assert m.tolist() == [[7]] and names == ["ACGTTGCA"]


def test_error_messages(api):
    from dada2_amd._lib import Dada2HipError
    with pytest.raises(Dada2HipError, match="takes A/C/G/T only") as ei:
        api.collapse_no_mismatch([[2, 1]], ["ACGTACGTNA", "ACGTACGT"])
    assert ei.value.code == 4
    with pytest.raises(Dada2HipError, match="takes A/C/G/T only") as ei:
        api.collapse_pairs(["ACGT"], ["ACNT"])
    assert ei.value.code == 4
    big = np.iinfo(np.int32).max
    for mat, seqs in (([[big, 1]], ["ACGT", "ACGT"]),                              # a de-duplicated cell
                      ([[big, 0], [1, 3]], ["ACGTACGT", "TTGGCCAA"])):               # a column total
        with pytest.raises(Dada2HipError, match="exceeds the integer range") as ei:
            api.collapse_no_mismatch(mat, seqs)
        assert ei.value.code == 1
    with pytest.raises(Dada2HipError, match="exceeds the integer range"):
        api.collapse_no_mismatch([[big + 1]], ["ACGT"])
    with pytest.raises(Dada2HipError, match="minOverlap must be at least 1") as ei:
        api.collapse_no_mismatch([[2, 1]], ["ACGTACGT", "ACGTACGA"], min_overlap=0)
    assert ei.value.code == 1
    with pytest.raises(ValueError, match="one column per sequence"):
        api.collapse_no_mismatch([[2, 1]], ["ACGTACGT"])
    with pytest.raises(ValueError, match="order_by"):
        api.collapse_no_mismatch([[2, 1]], ["ACGT", "ACGT"], order_by="size")
    with pytest.raises(Dada2HipError, match="Homopolymer gap penalties are not implemented in the vectorized aligner"):
        api.nweval("ACGT", "ACGA", homo_gap=-1, vec=True)
    with pytest.raises(ValueError, match="equal length"):
        api.nwhamming(["ACGT", "ACGA"], ["ACGT", "ACGA", "AAAA"])
    assert api.nweval([], []).shape == (0, 3) and api.collapse_pairs([], []).shape == (0, 4)


def test_no_cpu_fallback(api):
    """Two distinct columns need the device: without one the call fails loudly (with one it collapses them)."""
    import torch
    from dada2_amd._lib import Dada2HipError
    args = ([[5, 2]], ["ACGTACGTACGTACGTACGTAA", "CGTACGTACGTACGTACGTAA"])
    if torch.cuda.is_available():
        m, names = api.collapse_no_mismatch(*args)
        assert m.tolist() == [[7]] and names == args[1][:1]
        return
    for call in (lambda: api.collapse_no_mismatch(*args), lambda: api.collapse_pairs(args[1][:1], args[1][1:]),
                 lambda: api.nwhamming(*args[1])):
        with pytest.raises(Dada2HipError, match="no HIP device") as ei:
            call()
        assert ei.value.code == 2


def test_make_sequence_table(api):
    from dada2_amd.io import Derep
    from dada2_amd.opts import DadaResult
    s1 = {"GGGG": 3, "AAAA": 5, "CCCC": 5}
    s2 = Derep(["TTTT", "AAAA"], np.array([9, 1], dtype=np.int32), None, np.zeros(0, dtype=np.int32))
    cl = {"sequence": ["CCCC", "ACAC"], "abundance": np.array([2, 4], dtype=np.int32)}
    s3 = DadaResult(cl, {}, None, None, None, None)
    # first appearance: GGGG AAAA CCCC TTTT ACAC
    mat, seqs = api.make_sequence_table([s1, s2, s3], order_by=None)
    assert seqs == ["GGGG", "AAAA", "CCCC", "TTTT", "ACAC"]
    assert mat.tolist() == [[3, 5, 5, 0, 0], [0, 1, 0, 9, 0], [0, 0, 2, 0, 4]] and mat.dtype == np.int32
    # abundance 3 6 7 9 4, stable
    mat, seqs = api.make_sequence_table([s1, s2, s3])
    assert seqs == ["TTTT", "CCCC", "AAAA", "ACAC", "GGGG"] and mat[:, 0].tolist() == [0, 9, 0]
    # samples present 1 2 2 1 1: the ties keep first-appearance order
    mat, seqs = api.make_sequence_table([s1, s2, s3], order_by="nsamples")
    assert seqs == ["AAAA", "CCCC", "GGGG", "TTTT", "ACAC"]
    # merge_pairs rows: the accepted ones; duplicate sequences inside a sample are summed and the sample then goes in byte order
    rows = [dict(sequence="TTGA", abundance=4, accept=True), dict(sequence="", abundance=7, accept=False),
            dict(sequence="ACCA", abundance=2, accept=True), dict(sequence="TTGA", abundance=1, accept=True)]
    mat, seqs = api.make_sequence_table([rows, {"GATC": 1}], order_by=None)
    assert seqs == ["ACCA", "TTGA", "GATC"] and mat.tolist() == [[2, 5, 0], [0, 0, 1]]
    mat, seqs = api.make_sequence_table(rows)                                       # one sample, not in a list
    assert seqs == ["TTGA", "ACCA"] and mat.tolist() == [[5, 2]]
    with pytest.raises(ValueError, match="Unrecognized format"):
        api.make_sequence_table([["ACGT", "ACGA"]])
    with pytest.raises(ValueError, match="order_by"):
        api.make_sequence_table([s1], order_by="size")
