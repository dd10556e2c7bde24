"""assignSpecies / addSpecies without a device: the restatement of tests/species_cases.py pinned to the reference's own example
data (inst/extdata/example_species_assignment.fa.gz, example_seqs.fa: 14 references, two of them with one non-ACGT letter, six
queries of 201 nt), and the pure host functions of dada2_amd/api.py - the id parsing and its two format errors, species_table_out
(mapHits), match_genera, the query checks - held to the R lines and to the restatement."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import species_cases as sc
from dada2_amd import _lib, api


def test_restatement_on_the_example_data():
    refs, ids, seqs = sc.example()
    assert len(refs) == 14 and [len(s) for s in seqs] == [201] * 6
    assert [sum(1 for c in r if c not in "ACGT") for r in refs] == [0] * 12 + [1, 1]
    hits = sc.restate_hits(seqs, refs)
    assert [len(h) for h in hits] == [8, 0, 1, 0, 2, 0]
    assert sc.restate_hits(seqs, refs, try_rc=True) == hits
    one = sc.restate_assign(seqs, refs, ids)
    assert one == [("Lactobacillus", None), (None, None), ("Virgibacillus", "kekensis"), (None, None),
                   ("Clostridium", "hydrogeniformans"), (None, None)]
    many = sc.restate_assign(seqs, refs, ids, allow_multiple=True)
    assert many[0] == ("Lactobacillus", "mixtipabuli/odoratitofui/similis") and many[1:] == one[1:]
    assert sc.restate_assign(seqs, refs, ids, try_rc=True) == one


def test_read_fasta_and_id_parsing_on_the_example_reference():
    refs, ids, _ = sc.example()
    got_ids, got_refs = api.read_fasta(sc.EXAMPLE_SPECIES)
    assert got_ids == ids and got_refs == refs
    assert api.species_reference(ids) == sc.genus_species(ids)
    g, s = api.species_reference(["x Ab cd", "y  Ab", "z Ab\tcd ef", "w"])          # one separator per whitespace character
    assert g == ["Ab", "", "Ab", None] and s == ["cd", "Ab", "cd", None]


def test_the_two_format_errors():
    with pytest.raises(ValueError, match="this looks like a file formatted for assignTaxonomy"):
        api.species_reference(["Bacteria;Firmicutes;Bacilli;Lactobacillales;"])
    with pytest.raises(ValueError, match=r"^Incorrect reference file format for assignSpecies\.$"):
        api.species_reference(["id1 Lactobacillus"])
    with pytest.raises(ValueError, match=r"^Incorrect reference file format for assignSpecies\.$"):
        api.SpeciesModel((["ACGT"], ["a;b;c"]))                                     # (before anything is opened)
    assert api.species_reference(["a b c", "Bacteria;x;y;z;"]) == (["b", None], ["c", None])   # only the FIRST id is checked


def test_species_table_out_is_map_hits():
    genus = ["Escherichia", "Shigella", "Bacillus", "Bacillus", None, "bacillus", "Zeta"]
    species = ["coli", "flexneri", "subtilis", "cereus", "anthracis", None, "alpha"]
    hits = [[0, 1], [2, 3], [2, 3, 6], [], [2, 4], [5], [3, 5], [6, 2]]
    for keep in (1, 2, 3, math.inf):
        got = api.species_table_out([np.array(h, dtype=np.int32) for h in hits], genus, species, keep)
        assert got.shape == (8, 2)
        for i, h in enumerate(hits):
            assert got[i, 0] == sc.map_hits(h, genus, 1) and got[i, 1] == sc.map_hits(h, species, keep), (keep, i)
    got = api.species_table_out(hits, genus, species, 2)
    assert tuple(got[0]) == ("Escherichia/Shigella", "coli/flexneri")               # the rule renames whole names
    assert tuple(got[1]) == ("Bacillus", "cereus/subtilis")
    assert tuple(got[2]) == (None, None)                                            # two genera; three species > keep
    assert tuple(got[3]) == (None, None)                                            # no hits
    assert got[4, 0] is None and got[4, 1] == "anthracis/subtilis"                  # a None genus counts as a name
    assert tuple(got[5]) == ("bacillus", None)                                      # only a None species: nothing to join
    assert got[6, 0] is None and got[6, 1] == "cereus"                              # None counts (2 <= keep) and is left out
    assert got[7, 0] is None and got[7, 1] == "alpha/subtilis"
    assert api.species_table_out(hits, genus, species, 1)[6, 1] is None
    assert api.species_table_out([[0, 1]], ["Escherichia coli group", "Shigella"], ["a", "a"], 1).tolist() == [["Escherichia/Shigella", "a"]]
    assert api.species_table_out([[1, 0]], ["b", "B"], ["b", "a"], 2).tolist() == [[None, "a/b"]]   # code-point order


def test_match_genera():
    for f in (api.match_genera, sc.match_genera):
        assert f("Bacillus", "Bacillus")
        assert f("Clostridium sensu stricto", "Clostridium") and f("Clostridium_XI", "Clostridium") and f("Escherichia/Shigella", "Escherichia")
        assert f("Escherichia/Shigella", "Shigella")
        assert not f("Clostridiumx", "Clostridium") and not f("Paraclostridium", "Clostridium") and not f("Shigella/Escherichia x", "Escherichia")
        assert not f(None, "Bacillus") and not f("Bacillus", None) and not f("", "Bacillus") and not f("Bacillus", "")
        assert f("Ba-cillus group", "Ba.cillus") and f("X/Ba-cillus", "Ba.cillus")                                       # the binomial's genus is a regular expression, unescaped
    assert api.match_genera("X-Y", "Y", split_glyph="-") and not api.match_genera("X-Y", "Y")


def test_query_checks_need_no_device():
    L = _lib.lib()
    for seqs, msg in ((["ACGT", "ACGN"], "Non-ACGT characters present in the query sequences."), (["ACGT", "acgt"], "Non-ACGT"),
                      (["ACGT", ""], "empty query")):
        with pytest.raises(ValueError, match=msg):
            api.assign_species(seqs, (["ACGTACGT"], ["a b c"]))
        h = C.c_void_p()
        eb = C.create_string_buffer(512)
        arr = (C.c_char_p * len(seqs))(*[s.encode() for s in seqs])
        rc_ = L.dada2hip_species_match(None, len(seqs), arr, 0, C.byref(h), None, eb, 512)   # (checked before the handle is looked at)
        assert rc_ == 1 and msg in eb.value.decode() and not h.value
    h = C.c_void_p()
    eb = C.create_string_buffer(512)
    assert L.dada2hip_species_open(0, (C.c_char_p * 1)(), 0, C.byref(h), None, eb, 512) == 1 and not h.value


def test_add_species_needs_one_row_per_sequence():
    with pytest.raises(ValueError):
        api.add_species([["a", "b"]], ["ACGT", "ACGT"], (["ACGT"], ["a b c"]))
    assert os.path.getsize(sc.EXAMPLE_SPECIES) < 4096
