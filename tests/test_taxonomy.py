"""assignTaxonomy on the CPU: the numpy restatement of tests/taxonomy_cases.py pinned to the reference's recorded runs
(tests/golden/taxonomy.npz, made by tests/golden/make_taxonomy_golden.py from the reference's own src/taxonomy.cpp), and the
Python side of dada2_amd.api that restates R/taxonomy.R:65-160 against hand-written expectations.  The library's own host code
and kernels run in tests/test_emu_taxonomy.py (emulator) and tests/test_gpu_taxonomy.py (device)."""
import gzip
import warnings

import numpy as np
import pytest

import taxonomy_cases as tc
from dada2_amd import api


@pytest.mark.parametrize("name", tc.CASE_NAMES)
def test_restatement_is_pinned_to_both_reference_runs(name):
    """Every reference pick of both runs lies in the restatement's tie set - so every untied case is equal - and the reference's
    boot is the count over its own picks."""
    c = tc.load_case(name)
    table, best, tied = tc.restated(name)
    for k, run in enumerate(c["ref_runs"]):
        tc.assert_picks_in_tie_sets(tc.picks(run), tied, "%s run %d" % (name, k))
        assert np.array_equal(run["boot"], tc.boot_counts(run["tax"], run["boot_tax"], c["genusmat"]))
    untied = tied.sum(axis=2) == 1
    assert np.array_equal(tc.picks(c["ref_runs"][0])[untied], tc.picks(c["ref_runs"][1])[untied])


def test_the_reference_is_not_deterministic_and_the_fixture_shows_it():
    c = tc.load_case("example")
    tied = tc.restated("example")[2]
    differ = tc.picks(c["ref_runs"][0]) != tc.picks(c["ref_runs"][1])
    assert differ.any() and not (differ & (tied.sum(axis=2) <= 1)).any()


def test_tied_share_of_the_fixture_is_under_the_cap():
    entries = ties = 0
    for name in tc.CASE_NAMES:
        tied = tc.restated(name)[2]
        nt = tied.sum(axis=2)
        if name in tc.TIES_ARE_THE_POINT:
            assert (nt > 1).sum() >= 100, name
            continue
        entries += int(tied.any(axis=2).sum())
        ties += int((nt > 1).sum())
    assert entries >= 6000 and 0 < ties <= tc.TIE_CAP * entries, (ties, entries)


def test_numpy_log_is_not_libm_logf_on_the_example_table():
    """Why the restatement (and the library) take the logarithm from libm: numpy's float32 log differs on the example's inputs."""
    c = tc.load_case("example")
    table = tc.restated("example")[0]
    assert table.dtype == np.float32 and table.shape == (74, 65536) and (table < 0).all()
    x = np.unique(np.exp(table.astype(np.float64)).astype(np.float32))[:2000]
    assert np.array_equal(tc.logf(x), np.array([tc._libm.logf(float(v)) for v in x], dtype=np.float32))


def test_unif_buffer_is_the_api_generator():
    assert np.array_equal(tc.unif_buffer(12, 1000), api.taxonomy_unifs(12, 1000))
    u = api.taxonomy_unifs(2 ** 64 - 1, 100000)
    assert u.min() >= 0.0 and u.max() < 1.0 and abs(u.mean() - 0.5) < 0.01


# ---- R/taxonomy.R:76-122 ----------------------------------------------------------------------------------------------------------------
REF = "ACGTTGCAAGGCTTAACCGGTTAACC"      # 26 nt


def test_reference_parsing_ragged_depths_short_references_and_whitespace():
    refs = [REF, "ACGT" * 4, REF + "A", REF + "C", REF + "G"]
    ids = ["  Bacteria;Firmicutes;Bacilli;  ", "Bacteria;Short;", "Bacteria;Firmicutes;", "Bacteria;Firmicutes;Bacilli;", "Archaea;"]
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        kept, genus_unq, r2g, gm = api.taxonomy_reference(refs, ids)
    assert any("too short" in str(x.message) for x in w)
    assert kept == [refs[0], refs[2], refs[3], refs[4]]
    assert genus_unq == ["Bacteria;Firmicutes;Bacilli;", "Bacteria;Firmicutes;_DADA2_UNSPECIFIED;", "Archaea;_DADA2_UNSPECIFIED;_DADA2_UNSPECIFIED;"]
    assert r2g.tolist() == [0, 1, 0, 2] and r2g.dtype == np.int32
    assert gm.shape == (3, 3) and gm.dtype == np.int32
    assert gm[0, 0] == gm[1, 0] != gm[2, 0] and gm[0, 1] == gm[1, 1] != gm[2, 1] and gm[0, 2] != gm[1, 2] and gm[1, 2] == gm[2, 2]


def test_reference_parsing_unite_ids():
    ids = ["Fungus_sp|KX1|SH1.07FU|reps|k__Fungi;p__Ascomycota;c__unidentified;o__unidentified;f__unidentified;g__unidentified;s__Fungus_sp",
           "Saccharomyces_cerevisiae|AB2|SH2.07FU|refs|k__Fungi;p__Ascomycota;c__Sacc;o__Sacch;f__Saccha;g__Saccharomyces;s__Saccharomyces_cerevisiae"]
    ids = ids * 5
    refs = [REF + "ACGT"[i % 4] * (i // 4 + 1) for i in range(10)]
    kept, genus_unq, r2g, gm = api.taxonomy_reference(refs, ids)
    assert genus_unq == ["k__Fungi;p__Ascomycota;_DADA2_UNSPECIFIED;_DADA2_UNSPECIFIED;_DADA2_UNSPECIFIED;_DADA2_UNSPECIFIED;_DADA2_UNSPECIFIED;",
                         "k__Fungi;p__Ascomycota;c__Sacc;o__Sacch;f__Saccha;g__Saccharomyces;s__cerevisiae;"] or genus_unq == [
        "k__Fungi;p__Ascomycota;_DADA2_UNSPECIFIED;_DADA2_UNSPECIFIED;_DADA2_UNSPECIFIED;_DADA2_UNSPECIFIED;_DADA2_UNSPECIFIED",
        "k__Fungi;p__Ascomycota;c__Sacc;o__Sacch;f__Saccha;g__Saccharomyces;s__cerevisiae"]
    assert r2g.tolist() == [0, 1] * 5 and gm.shape == (2, 7)
    # nine ids, or a first id that does not match: not UNITE, the id is taken whole
    with pytest.raises(ValueError, match="Incorrect reference file format"):
        api.taxonomy_reference(refs[:9], [x.replace(";", ",") for x in ids[:9]])


def test_reference_parsing_format_check():
    with pytest.raises(ValueError, match="assignSpecies"):
        api.taxonomy_reference([REF], ["AB123 Escherichia coli"])
    with pytest.raises(ValueError, match="Incorrect reference file format for assignTaxonomy.$"):
        api.taxonomy_reference([REF], ["Bacteria"])


def test_read_fasta_plain_and_gzip(tmp_path):
    text = ">a;b; \nacgt\nNNAC\n>c;\nGG\n\n"
    p1, p2 = tmp_path / "x.fa", tmp_path / "x.fa.gz"
    p1.write_text(text)
    with gzip.open(p2, "wt") as fh:
        fh.write(text)
    for p in (p1, p2):
        assert api.read_fasta(str(p)) == (["a;b; ", "c;"], ["ACGTNNAC", "GG"])
    ids, seqs = api.read_fasta(tc.EXAMPLE_TRAIN)
    assert len(ids) == 100 and all(i.endswith(";") for i in ids)
    kept, genus_unq, r2g, gm = api.taxonomy_reference(seqs, ids)
    c = tc.load_case("example")
    assert kept == c["refs"] and np.array_equal(r2g, c["ref_to_genus"]) and gm.shape == (74, 6) and len(genus_unq) == 74


def test_min_boot_cut_and_unspecified_levels():
    genus_unq = ["K;P;_DADA2_UNSPECIFIED;G;", "K;Q;C;H;"]
    tax = np.array([0, 1, -1, 1])
    boot = np.array([[100, 80, 60, 50], [100, 49, 49, 10], [0, 0, 0, 0], [100, 100, 100, 100]])
    out = api.taxonomy_table_out(genus_unq, tax, boot, min_boot=50)
    assert out.tolist() == [["K", "P", None, "G"], ["K", None, None, None], [None] * 4, ["K", "Q", "C", "H"]]
    assert api.taxonomy_table_out(genus_unq, tax, boot, min_boot=80).tolist()[0] == ["K", "P", None, None]
