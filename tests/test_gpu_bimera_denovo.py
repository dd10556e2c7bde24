"""isBimeraDenovo, removeBimeraDenovo and isShiftDenovo on the device (dada2hip_bimera_denovo: k_bimera_worklist, the bimera-mode
aligners, k_bimera_fold) against tests/golden/bimera_denovo.json - the restated R loops over the reference's own C_is_bimera /
C_nwalign / C_eval_pair (tests/bimera_denovo_cases.py; tests/test_bimera_denovo.py re-derives the file on the CPU).  Exact equality
of booleans and tables throughout."""
import numpy as np
import pytest

import bimera_denovo_cases as bc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def api():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from dada2_amd import api
    return api


def _one_row_table(api, name, min_abund, min_fold=2):
    c = bc.cases()[name]
    nflag, _ = api.table_bimera2(np.asarray(c["ab"], dtype=np.int32).reshape(1, -1), c["seqs"], min_fold=min_fold, min_abund=min_abund)
    return (nflag > 0).tolist()


@pytest.mark.parametrize("name", ["n1", "n2", "n3"])
def test_no_query_has_two_parents_to_complete_a_model(api, name):
    st = bc.run_case(api, name)
    assert st["flagged"] == 0 and st["pairs_aligned"] == st["pairs_possible"] == (2 if name == "n3" else 0), st


def test_exactly_two_parents(api):
    st = bc.run_case(api, "two_parents")
    assert st["queries"] == 2 and st["pairs_possible"] == 4 and st["flagged"] == 2 and st["windows"] == 1, st


def test_parent_counts_around_a_chunk_and_the_first_window(api):
    """The ladder holds a query with c parents for every c in 2 .. 138 whose model needs its LAST two parents, and one built from the
    two ranks just behind them: among them per, per + 1 and 2 per parents, and one more and one fewer than the first window (which is
    one chunk of per ranks: per - 1 where that is at least 2)."""
    st = bc.run_case(api, "ladder")
    per = st["per"]
    assert st["aligner_route"] == 1 and 1 <= per and 2 * per <= bc.LADDER_K - 2, st
    _, _, count = bc.ladder()
    assert {max(2, per - 1), max(2, per), per + 1, 2 * per} <= set(count)
    assert st["pairs_possible"] == sum(count) and st["windows"] >= 3, st
    # queries leave the work when their model is complete: the flagged ones need all their parents here, so nothing is saved ...
    assert st["pairs_aligned"] == st["pairs_possible"], st
    # ... and the same vector with a budget of a few chunks: every window in many launches, the same flags
    st2 = bc.run_case(api, "ladder", {"DADA2HIP_BIMERA_SLOTS": 4 * per + 1})
    assert st2["slot_budget"] == 4 * per and st2["launches"] > 20 * st2["windows"] and st2["pairs_aligned"] == st["pairs_aligned"], st2
    assert _one_row_table(api, "ladder", 9) == bc.golden()["cases"]["ladder"]


@pytest.mark.parametrize("name", ["fold_equal", "parent_abundance", "fold_1_5"])
def test_thresholds_are_strict(api, name):
    st = bc.run_case(api, name)
    assert st["queries"] == 2 and st["pairs_possible"] == 4 and st["flagged"] == 1, st     # the equal / the 8 / the 4 is no parent


def test_one_row_table_route_agrees_and_shows_the_strict_comparison(api):
    for name in ("fold_equal", "parent_abundance", "two_parents", "toss", "oo_exact"):
        assert _one_row_table(api, name, 9) == bc.golden()["cases"][name], name
    assert _one_row_table(api, "fold_1_5", 3, 1.5) == bc.golden()["cases"]["fold_1_5"]
    # min_abund = 8 takes the parent of abundance 8 (>=): the query built from it is flagged there and not by isBimeraDenovo (>)
    loose = _one_row_table(api, "parent_abundance", 8)
    assert loose == [False, False, False, True, True] and loose != bc.golden()["cases"]["parent_abundance"]


def test_early_and_late_completion(api):
    early = bc.run_case(api, "early")
    assert early["pairs_possible"] == 4096 and early["pairs_aligned"] < 4096 and early["flagged"] == 1 and early["windows"] == 1, early
    late = bc.run_case(api, "late")
    assert late["pairs_possible"] == 4096 and late["pairs_aligned"] == 4096 and late["flagged"] == 1, late
    assert late["launches"] == late["windows"] > 1, late
    cut = bc.run_case(api, "late", {"DADA2HIP_BIMERA_SLOTS": 300})
    assert cut["launches"] > cut["windows"] == late["windows"] and cut["pairs_aligned"] == 4096 and cut["flagged"] == 1, cut


@pytest.mark.parametrize("name", ["toss", "toss_shift_pair", "oo_exact", "oo_one_off", "oo_one_off_far", "oo_blocked", "oo_unblocked",
                                  "unequal_ms4", "unequal_ms16", "duplicates", "zero"])
def test_named_cases(api, name):
    bc.run_case(api, name)


@pytest.mark.parametrize("name", ["two_parents", "oo_one_off", "unequal_ms16"])
def test_lane_route_forced(api, name):
    st = bc.run_case(api, name, {"DADA2HIP_NW_KERNEL": "lane"})
    assert st["aligner_route"] == 2 and st["per"] == 64, st


def test_reads_past_the_anti_diagonal_kernel_take_the_lane_route(api):
    st = bc.run_case(api, "long")
    assert st["aligner_route"] == 2 and st["per"] == 64 and st["pairs_aligned"] == st["pairs_possible"] == 8, st


def test_other_input_forms(api):
    c = bc.cases()["duplicates"]
    want = bc.golden()["cases"]["duplicates"]
    s, a = api.remove_bimera_denovo((c["seqs"], c["ab"]))
    assert s == [x for x, b in zip(c["seqs"], want) if not b] and a.tolist() == [x for x, b in zip(c["ab"], want) if not b]
    c = bc.cases()["two_parents"]
    assert api.is_bimera_denovo(dict(zip(c["seqs"], c["ab"]))).tolist() == bc.golden()["cases"]["two_parents"]


def test_per_sample(api):
    mat, seqs = bc.per_sample_table()
    g = bc.golden()["per_sample"]
    st = {}
    flags = api.bimera_denovo_rows(mat, seqs, stats=st)
    assert flags.astype(int).tolist() == g["flags"] and st["rows"] == 3 and st["flagged"] == int(np.sum(g["flags"])), st
    one_by_one = np.array([api.is_bimera_denovo((seqs, row)) for row in mat])
    assert np.array_equal(flags, one_by_one)
    st_skip = {}
    skipped = api.bimera_denovo_rows(mat, seqs, skip_zero=True, stats=st_skip)
    assert np.array_equal(skipped, flags & (mat > 0)) and st_skip["pairs_possible"] < st["pairs_possible"], (st, st_skip)
    out, names = api.remove_bimera_denovo((mat, seqs), method="per-sample")
    assert out.tolist() == g["table"] and [seqs.index(s) for s in names] == g["kept"]


def test_table_of_400_through_the_front_end(api):
    mat, seqs = bc.table400()
    g = bc.golden()["table400"]
    pooled, per_sample, consensus = np.array(g["pooled"]), np.array(g["per_sample"], dtype=bool), np.array(g["consensus"])
    assert pooled.any() and per_sample.any() and consensus.any()
    st = {}
    assert api.is_bimera_denovo((mat, seqs), stats=st).tolist() == g["pooled"]
    assert st["pairs_aligned"] < st["pairs_possible"], st                               # bimeras of abundant parents leave early
    out, names = api.remove_bimera_denovo((mat, seqs), method="pooled")
    assert names == [s for s, b in zip(seqs, pooled) if not b] and np.array_equal(out, mat[:, ~pooled])
    out, names = api.remove_bimera_denovo(mat, method="consensus", seqs=seqs)
    assert names == [s for s, b in zip(seqs, consensus) if not b] and np.array_equal(out, mat[:, ~consensus])
    assert np.array_equal(api.bimera_denovo_rows(mat, seqs), per_sample)
    want = mat.copy()
    want[per_sample] = 0
    keep = want.sum(axis=0) != 0
    out, names = api.remove_bimera_denovo((mat, seqs), method="per-sample")
    assert np.array_equal(out, want[:, keep]) and names == [s for s, k in zip(seqs, keep) if k]


@pytest.mark.parametrize("name", sorted(bc.shift_cases()))
def test_is_shift_denovo(api, name):
    s, ab, kw = bc.shift_cases()[name]
    got = api.is_shift_denovo((s, ab), **kw)
    assert got.dtype == bool and got.tolist() == bc.golden()["shift"][name]


def test_refusals(api):
    from dada2_amd import _lib
    c = bc.cases()["two_parents"]
    with pytest.raises(_lib.Dada2HipError, match="A/C/G/T only"):
        api.is_bimera_denovo((c["seqs"][:3] + [c["seqs"][3][:20] + "N" + c["seqs"][3][21:]], c["ab"]))
    with pytest.raises(_lib.Dada2HipError, match="maxShift 0"):
        api.is_bimera_denovo((c["seqs"], c["ab"]), max_shift=0)
    with pytest.raises(ValueError, match="Valid values for method: 'pooled', 'consensus', or 'per-sample'"):
        api.remove_bimera_denovo((np.asarray(c["ab"]).reshape(1, -1), c["seqs"]), method="sample")
