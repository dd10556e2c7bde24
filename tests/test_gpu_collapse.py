"""The sequence-table stage on the MI355X (-m gpu): dada2hip_collapse_pairs (k_collapse_scan) against brute force,
dada2hip_collapse_nomismatch (k_collapse_join + k_collapse_scan + the pair-form lane aligner + the host's replay of the greedy
loop) against the restatement of collapseNoMismatch in tests/collapse_cases.py, dada2hip_nweval against eval_pair of the
oracle's alignments, and the whole path from dada_uniques to is_bimera_denovo_table.  The restatement runs over the reference
compiled in place where oracle/_ref is there (its C_nwvec call, what nwhamming(vec=TRUE) uses), else over the plain-C oracle."""
import numpy as np
import pytest

import collapse_cases as cc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def api():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from dada2_amd import api as a
    return a


@pytest.fixture(scope="module")
def checker(oracle_c):
    from oracle import ref
    return cc.checker_for(oracle_c, ref)


@pytest.fixture(scope="module")
def table():
    return cc.make_table()


_WANT = {}


def want(checker, key, mat, seqs, **kw):
    """The restatement's result (and trace) of a table under one set of arguments, computed once per module."""
    if key not in _WANT:
        tr = {}
        _WANT[key] = (cc.restate(mat, seqs, checker, trace=tr, **kw), tr)
    return _WANT[key]


# ---- the scan kernel ------------------------------------------------------------------------------------------------------------------
def test_collapse_pairs_match_the_fixture(api):
    """All 6 000 pairs of tests/golden/collapse_pairs.npz: both screen bits, G, m_max and the decision."""
    assert cc.check_pairs(api, np.arange(6000)) == 6000


def test_collapse_pairs_past_the_block_cap_of_the_scan(api):
    """32 769 pairs in one call: every block of k_collapse_scan stages a second pair over its first, block 0 a third."""
    assert cc.check_strided_pairs(api) == 32769


def test_collapse_pairs_with_lengths_either_side_of_the_word_boundaries(api):
    """1, 2, 31, 32, 33, 63, 64, 65, 250, 251, 256, 257 and 600 nt, each against each; a copy, a shifted copy, a contained piece, a
    one-mismatch copy; minOverlap 1 to 700 (above 32: longer than the join's key; 700: above every length) - against brute force."""
    qs, rs = cc.boundary_pairs()
    scan = [cc.brute_pair(q, r, 1) for q, r in zip(qs, rs)]          # (G and m_max do not depend on minOverlap)
    assert len(qs) == 4 * len(cc.BOUNDARY_LENGTHS) ** 2
    for mo in cc.BOUNDARY_MIN_OVERLAPS:
        got = api.collapse_pairs(qs, rs, min_overlap=mo)
        for i, (q, r) in enumerate(zip(qs, rs)):
            sc = cc.screen(q, r, mo)
            exp = (sc, scan[i][1], scan[i][2], 0 if sc == 0 else (1 if scan[i][1] > 5 * scan[i][2] else 2))
            assert tuple(int(x) for x in got[i]) == exp, (mo, i, len(q), len(r), got[i].tolist(), exp)
        assert {0, 1, 2, 3} >= set(int(x) for x in got[:, 0]) and len(set(int(x) for x in got[:, 3])) >= 2


# ---- the whole function -----------------------------------------------------------------------------------------------------------------
def test_the_generated_table_holds_the_regimes_it_was_built_for(checker, table):
    counts = cc.table_fact(*table, checker)
    assert counts["columns"] == 320


@pytest.mark.parametrize("band", [-1, 16])
@pytest.mark.parametrize("order_by", ["abundance", "nsamples", None])
@pytest.mark.parametrize("min_overlap", [20, 8, 33])
def test_collapse_equals_the_restatement(api, checker, table, min_overlap, order_by, band):
    """Table, column names and column order."""
    mat, seqs = table
    kw = dict(min_overlap=min_overlap, order_by=order_by, band=band)
    exp, _ = want(checker, ("table", min_overlap, order_by, band), mat, seqs, **kw)
    got = cc.device_collapse(api, mat, seqs, **kw)
    cc.assert_same_table(got, exp, kw)
    assert len(got[1]) < len(seqs) and got[2]["columns_dedup"] == len(seqs)
    if band >= 0:                                                     # (no bound under a band: every screened pair is aligned)
        assert got[2]["pairs_bound_rejected"] == 0 and got[2]["pairs_aligned"] == got[2]["pairs_scanned"] - got[2]["pairs_screened_out"]


@pytest.mark.parametrize("identical_only", [False, True])
def test_collapse_with_duplicate_columns(api, checker, table, identical_only):
    mat, seqs = cc.with_duplicates(*table)
    assert len(set(seqs)) == len(seqs) - 25
    exp, tr = want(checker, ("dups", identical_only), mat, seqs, identical_only=identical_only)
    got = cc.device_collapse(api, mat, seqs, identical_only=identical_only)
    cc.assert_same_table(got, exp, "duplicate columns")
    assert got[2]["columns_dedup"] == tr["ncol"] == len(seqs) - 25
    if identical_only:
        assert got[1] == list(dict.fromkeys(seqs)) and got[2]["pairs_scanned"] == 0


def test_batches_of_1_16_and_1000_agree(api, checker, table):
    """The same `into` whatever the batch; in batches of 16 a query joins a ref of its own batch, and a batch member that has
    itself collapsed is passed over as a ref (both from the restatement's trace)."""
    mat, seqs = table
    exp, tr = want(checker, ("table", 20, "abundance", -1), mat, seqs, min_overlap=20, order_by="abundance", band=-1)
    view = cc.batch_view(tr, 20, 16)
    assert view["own_batch"] and view["skipped"], view
    intos = []
    for b in (1, 16, 1000):
        got = cc.device_collapse(api, mat, seqs, env={"DADA2HIP_COLLAPSE_BATCH": b})
        cc.assert_same_table(got, exp, "batch %d" % b)
        assert got[2]["batches"] == -(-len(seqs) // b)
        assert got[2]["pairs_scanned"] - got[2]["pairs_screened_out"] == cc.batch_view(tr, 20, b)["screened"], b
        intos.append(got[2]["into"])
    assert all(np.array_equal(intos[0], x) for x in intos[1:])
    pos = {s: k for k, s in enumerate(seqs)}
    assert all(intos[1][pos[q]] == pos[r] for q, r in tr["joined"].items())


def test_the_shortcuts_are_invisible(api, checker, table):
    """DADA2HIP_COLLAPSE_SCAN=0 and DADA2HIP_COLLAPSE_JOIN=0, separately and together: the same `into`; the counters say what
    each shortcut saved."""
    mat, seqs = table
    exp, tr = want(checker, ("table", 20, "abundance", -1), mat, seqs, min_overlap=20, order_by="abundance", band=-1)
    runs = {}
    for scan in (1, 0):
        for join in (1, 0):
            got = cc.device_collapse(api, mat, seqs, env={"DADA2HIP_COLLAPSE_SCAN": scan, "DADA2HIP_COLLAPSE_JOIN": join, "DADA2HIP_COLLAPSE_BATCH": 64})
            cc.assert_same_table(got, exp, (scan, join))
            runs[scan, join] = got[2]
    assert all(np.array_equal(runs[1, 1]["into"], st["into"]) for st in runs.values())
    screened = cc.batch_view(tr, 20, 64)["screened"]
    for (scan, join), st in runs.items():
        assert st["pairs_scanned"] - st["pairs_screened_out"] == screened, (scan, join, st)
        assert st["pairs_aligned"] >= st["aligned_ham0"] >= len(tr["joined"])
        assert st["pairs_aligned"] == screened - st["pairs_bound_rejected"]
    for join in (1, 0):
        assert runs[1, join]["pairs_aligned"] < runs[0, join]["pairs_aligned"] == screened and runs[0, join]["pairs_bound_rejected"] == 0
    for scan in (1, 0):
        assert runs[scan, 1]["pairs_scanned"] <= runs[scan, 0]["pairs_scanned"] and runs[scan, 1]["candidate_pairs"] < runs[scan, 0]["candidate_pairs"]


def test_low_complexity_table_where_the_alignments_tie(api, checker):
    """200 columns over {A, C}, 8-40 nt, min_overlap 4."""
    mat, seqs = cc.low_complexity_table()
    tr = {}
    exp = cc.restate(mat, seqs, checker, min_overlap=4, trace=tr)
    ties = sum(1 for v in tr["tried"].values() for _, h in v if h != 0)
    assert ties >= 1000 and len(exp[1]) < len(seqs)
    got = cc.device_collapse(api, mat, seqs, min_overlap=4)
    cc.assert_same_table(got, exp, "low complexity")
    assert got[2]["pairs_aligned"] > got[2]["aligned_ham0"] > 0


def test_more_pairs_than_one_aligner_call_takes(api, oracle_c):
    """More than 65 536 pairs to align (the aligner is called with at most 65 536): `into` against the restatement over the
    plain-C oracle."""
    mat, seqs = cc.many_pairs_table()
    tr = {}
    exp = cc.restate(mat, seqs, oracle_c, trace=tr)
    got = cc.device_collapse(api, mat, seqs)
    cc.assert_same_table(got, exp, "many pairs")
    st = got[2]
    assert st["pairs_aligned"] > 65536 and st["batches"] == 1
    assert st["pairs_aligned"] == st["pairs_scanned"] - st["pairs_screened_out"] - st["pairs_bound_rejected"]
    pos = {s: k for k, s in enumerate(seqs)}
    assert all(st["into"][pos[q]] == pos[r] for q, r in tr["joined"].items()) and len(exp[1]) == len(tr["kept"]) < 20


def test_collapse_wraps_the_aligner_scratch_ring(api, checker):
    """More than 512 pairs in one aligner call under DADA2HIP_NW_RING=4: the table equals the restatement's, the launch was
    sized for three trips and more, and the knob changes nothing."""
    assert cc.ring_run(api, checker) > 512


# ---- nweval / nwhamming ---------------------------------------------------------------------------------------------------------------
def _pair_case(name):
    import pair_cases as P
    case = [c for c in P.vec_cases() if c.name == name][0]
    return P, case, P.build(case)


@pytest.mark.parametrize("name,vec", [("unbanded_n65_default_ef1", True), ("unbanded_n65_default_ef1", False), ("w65_n65_flat_ef1", True),
                                      ("w33_n257_flat_ef0", False)])
def test_nweval_on_the_pairwise_export_cases(api, oracle_c, name, vec):
    """The pairs of tests/pair_cases.py the pairwise-export tests use: nweval = eval_pair of the oracle's alignment of every pair
    (unbanded, banded, and a global call), nwhamming its mismatch + indel; vec true and false."""
    P, case, b = _pair_case(name)
    sc = P.SCORES[case.score]
    exp = np.array([oracle_c.eval_pair(*al) for al in P.expected(oracle_c, case)], dtype=np.int32)
    kw = dict(match=sc[0], mismatch=sc[1], gap=sc[2], band=case.band, endsfree=case.endsfree, vec=vec)
    got = api.nweval(b.s1, b.s2, **kw)
    assert got.shape == (case.n, 3) and np.array_equal(got, exp), np.flatnonzero((got != exp).any(axis=1))[:10]
    assert np.array_equal(api.nwhamming(b.s1, b.s2, **kw), exp[:, 1] + exp[:, 2])
    assert (exp[:, 1] + exp[:, 2] > 0).any() and (exp[:, 2] > 0).any()
    assert api.nwhamming(b.s1[3], b.s2[3], **kw) == int(exp[3, 1] + exp[3, 2])


# ---- the whole path -------------------------------------------------------------------------------------------------------------------
def test_from_dada_uniques_to_the_bimera_flags(api, checker):
    """dada_uniques on sam1F_default and on a second sample made from it (reads trimmed by a few bases, so that something
    collapses), make_sequence_table, collapse_no_mismatch = the restatement on the same table; is_bimera_denovo_table on the
    result runs clean."""
    from helpers import case_inputs
    d, err, pri, opts, exp, meta = case_inputs("sam1F_default")
    r1 = api.dada_uniques(d.seqs, d.abundances, pri, err, d.quals, opts, device=0)
    trimmed = {}
    for s, a, q in zip(d.seqs, d.abundances, d.quals):
        k = 3 + len(trimmed) % 4
        if s[k:] not in trimmed:
            trimmed[s[k:]] = (int(a), np.concatenate([q[k: len(s)], np.full(len(q) - len(s) + k, np.nan)]))
    s2 = list(trimmed)
    q2 = np.array([trimmed[s][1] for s in s2])[:, : max(len(s) for s in s2)]
    r2 = api.dada_uniques(s2, [trimmed[s][0] for s in s2], None, err, q2, opts, device=0)
    mat, seqs = api.make_sequence_table([r1, r2])
    assert mat.shape == (2, len(seqs)) and len(seqs) > r1.nclust
    want_ = cc.restate(mat, seqs, checker)
    got = cc.device_collapse(api, mat, seqs)
    cc.assert_same_table(got, want_, "sam1F + trimmed sam1F")
    assert len(got[1]) < len(seqs)
    flags = api.is_bimera_denovo_table(got[0], got[1])
    assert flags.shape == (len(got[1]),) and flags.dtype == bool
