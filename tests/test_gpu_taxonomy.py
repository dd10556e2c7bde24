"""assignTaxonomy on the MI355X (-m gpu): dada2hip_taxonomy_train / _assign against the numpy restatement of tests/taxonomy_cases.py
over the committed fixture tests/golden/taxonomy.npz (the reference's own runs are pinned to the restatement on the CPU, in
tests/test_taxonomy.py).  Per case: the model table bit-equal, ntie exact, untied picks equal and tied picks inside the tie set,
boot recounted from the call's own picks, slab and gather instance identical, two calls with one seed identical, another seed
differing only at tied entries (taxonomy_cases.check_case)."""
import numpy as np
import pytest

import taxonomy_cases as tc

pytestmark = pytest.mark.gpu

_SEEN = {}


@pytest.fixture(scope="module")
def api():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from dada2_amd import api as a
    return a


@pytest.mark.parametrize("name", tc.CASE_NAMES)
def test_case_meets_the_criteria(api, name):
    entries, ties, got, stats = tc.check_case(api, name)
    _SEEN[name] = (entries, ties)
    if name == "twins":
        tc.assert_twins(got, tc.restated(name)[2])
    if name == "lengths":                                        # the 1 500-nt query is past the slab's budget by default
        assert stats[0]["gather_queries"] == 1 and stats[0]["slab_queries"] == 4, stats[0]
        assert (got["tax"][0] == -1) and (got["boot"][0] == 0).all() and (got["boot_tax"][0] == -1).all() and (got["ntie"][0] == 0).all()
    if name == "broken_by_N":                                    # 5 valid k-mers: empty replicates, every genus ties at 0
        assert (got["ntie"][0, 1:] == 20).all() and got["ntie"][0, 0] >= 1
    if name == "try_rc":
        assert tc.restated_flips(name) == [1, 3, 5, 7] and stats[0]["took_reverse_complement"] == 4, stats[0]


@pytest.mark.parametrize("name", tc.CHUNKED)
def test_chunks_of_queries_change_nothing(api, name):
    """DADA2HIP_TAX_CHUNK = 1, 3 and unset: the criteria under each, identical outputs, two launches per extra chunk and instance."""
    tc.check_chunks(api, name)


def test_untied_picks_are_the_reference_runs(api):
    """Where the maximum is untied the device's pick is the reference's recorded pick, in both recorded runs."""
    c = tc.load_case("example")
    tied = tc.restated("example")[2]
    with tc.device_model(api, "example") as m:
        got = api.assign_taxonomy_raw(c["seqs"], m, seed=3, unifs=c["unifs"])
    untied = tied.sum(axis=2) == 1
    assert untied.sum() >= 500
    for run in c["ref_runs"]:
        assert np.array_equal(tc.picks(got)[untied], tc.picks(run)[untied])


def test_tied_share_of_the_compared_cases_is_under_the_cap(api):
    for name in tc.CASE_NAMES:
        if name not in _SEEN:
            _SEEN[name] = tc.check_case(api, name)[:2]
    entries = sum(e for n, (e, t) in _SEEN.items() if n not in tc.TIES_ARE_THE_POINT)
    ties = sum(t for n, (e, t) in _SEEN.items() if n not in tc.TIES_ARE_THE_POINT)
    assert entries >= 6000 and ties <= tc.TIE_CAP * entries, (ties, entries)


def test_slab_budget_boundary(api):
    """DADA2HIP_TAX_SLAB at a query's own k-mer count, one under and one over: the query changes instance, nothing else changes."""
    c = tc.load_case("len57")
    outs = []
    with tc.device_model(api, "len57") as m:
        for slab, want_slab in ((50, 4), (49, 0), (51, 4), (512, 4), (100000, 4)):
            st = {}
            outs.append(tc.with_env({"DADA2HIP_TAX_SLAB": slab}, lambda: api.assign_taxonomy_raw(c["seqs"], m, seed=5, unifs=c["unifs"], stats=st)))
            assert st["slab_queries"] == want_slab and st["gather_queries"] == 4 - want_slab, (slab, st)
    for o in outs[1:]:
        for k in ("tax", "boot", "boot_tax", "ntie"):
            assert np.array_equal(o[k], outs[0][k]), k


def test_the_wrapper_on_the_example_files(api):
    """assign_taxonomy from the FASTA files: the table of names follows the raw call on the same model and seed."""
    seqs = api.read_fasta(tc.EXAMPLE_SEQS)[1]
    with api.TaxonomyModel(tc.EXAMPLE_TRAIN) as m:
        assert m.ngenus == 74 and m.depth == 6 and len(m.refs) == 100
        raw = api.assign_taxonomy_raw(seqs, m, seed=9)
        res = api.assign_taxonomy(seqs, m, min_boot=80, output_bootstraps=True, seed=9)
    assert res["levels"] == ["Kingdom", "Phylum", "Class", "Order", "Family", "Genus"] and np.array_equal(res["boot"], raw["boot"])
    for i, g in enumerate(raw["tax"]):
        names = m.genus_unq[int(g)].rstrip(";").split(";")
        for l in range(6):
            want = names[l] if raw["boot"][i, l] >= 80 and names[l] != "_DADA2_UNSPECIFIED" else None
            assert res["tax"][i, l] == want, (i, l)
    assert res["tax"][0, 0] == "Bacteria"
    assert api.assign_taxonomy(seqs, tc.EXAMPLE_TRAIN, seed=9).shape == (6, 6)


def test_input_errors(api):
    from dada2_amd import _lib
    with pytest.raises(_lib.Dada2HipError) as e:
        api.TaxonomyModel.from_parsed(["ACGTAC"], ["a;"], [0], [[0]])
    assert e.value.code == 1
    with pytest.raises(_lib.Dada2HipError) as e:
        api.TaxonomyModel.from_parsed(["ACGTACGTACGT"], ["a;"], [1], [[0]])
    assert e.value.code == 1
    with tc.device_model(api, "ngenus1") as m:
        with pytest.raises(_lib.Dada2HipError) as e:
            api.assign_taxonomy_raw(["A" * 10000], m)
        assert e.value.code == 1
        with pytest.raises(_lib.Dada2HipError) as e:
            api.assign_taxonomy_raw(["ACGT" * 20], m, unifs=np.full(900, 1.0))
        assert e.value.code == 1
