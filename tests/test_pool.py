"""The host side of pooled dada() on the CPU (no GPU): dada2hip_derep_combine against the restatement of combineDereps2 in
tests/pool_cases.py - golden samples with their maps, synthetic samples that cover the edges, the error cases, and a guard that the
cases can tell a contracted (fused multiply-add) build from the right one - and the restated split of a pooled result against
hand-worked expectations, with the library's split_pooled beside it.  Bit for bit throughout."""
import numpy as np
import pytest

import pool_cases as pc
from dada2_amd import _lib, api
from dada2_amd.io import Derep
from dada2_amd.opts import DadaResult, NA_INTEGER
from helpers import _same_float

NA = NA_INTEGER


@pytest.fixture(scope="module")
def goldens():
    return {n: pc.golden_derep(api, n) for n in ("sam1F", "sam2F", "sam1R", "sam2R")}


def test_two_golden_samples_combine_as_the_restatement_says(goldens):
    got, u2p = pc.check_combine(api, [goldens["sam1F"], goldens["sam2F"]])
    assert got.nraw < goldens["sam1F"].nraw + goldens["sam2F"].nraw          # the samples share uniques
    assert got.map.size == goldens["sam1F"].map.size + goldens["sam2F"].map.size and int(got.abundances.sum()) == 3000
    assert np.all(np.diff(got.abundances.astype(np.int64)) <= 0)
    assert [got.seqs[int(k)] for k in u2p[1]] == goldens["sam2F"].seqs


def test_three_samples_one_a_reordered_part_of_another(goldens):
    d = goldens["sam1R"]
    rows = np.random.default_rng(3).permutation(d.nraw)[: d.nraw - 7]         # a few rows dropped, the rest reordered
    third = pc.subset_derep(d, rows)
    assert (third.map < 0).any()
    got, u2p = pc.check_combine(api, [d, goldens["sam2R"], third])
    assert np.array_equal(u2p[2], u2p[0][rows])                               # the repeated sequence set lands on the same pooled rows


def test_synthetic_samples_cover_the_edges():
    sy = pc.synthetic_dereps()
    assert [d.quals.shape[1] for d in sy] == [60, 48, 60] and all(len({len(s) for s in d.seqs}) > 5 for d in sy)
    sets = [set(d.seqs) for d in sy]
    assert sets[0] & sets[1] & sets[2] and (sets[0] & sets[2]) - sets[1] and sets[0] - sets[1] - sets[2]
    assert all((d.map < 0).sum() == 4 for d in sy)
    got, u2p = pc.check_combine(api, sy)
    assert got.quals.shape[1] == 60
    # ties in the pooled abundances, settled by first appearance: the restatement's stable order is what was compared; make sure
    # the case has ties between uniques first seen in different samples
    first_seen = np.array([min(i for i, s in enumerate(sets) if x in s) for x in got.seqs])
    ties = [k for k in range(got.nraw - 1) if got.abundances[k] == got.abundances[k + 1] and first_seen[k] != first_seen[k + 1]]
    assert ties and all(first_seen[k] < first_seen[k + 1] for k in ties)
    # a unique of the narrow sample that is longer elsewhere does not exist (equal sequences, equal lengths); the NA padding shows
    # where the narrow sample's uniques stop short of the pooled width
    k = got.seqs.index(sy[1].seqs[-1])
    assert np.isnan(got.quals[k, len(got.seqs[k]):]).all() and not np.isnan(got.quals[k, : len(got.seqs[k])]).any()


def test_native_and_numpy_dereps_mix(goldens, tmp_path):
    import os
    nd = api.NativeDerep(os.path.join(pc.GOLDEN, "sam1F.fastq.gz"))
    try:
        pc.check_combine(api, [goldens["sam1F"], goldens["sam2F"]], inputs=[nd, goldens["sam2F"]])
        pc.check_combine(api, [goldens["sam2F"], goldens["sam1F"]], inputs=[goldens["sam2F"], nd])
    finally:
        nd.close()
    # the library's NA map entries and the numpy Derep's -1 both mean NA: a FASTQ file with a zero-length read
    fq = tmp_path / "z.fastq"
    fq.write_text("@a\nACGTACGT\n+\nIIIIIIII\n@b\n\n+\n\n@c\nACGTACGT\n+\nIIIIHHHH\n@d\nTTTTACGT\n+\nIIIIIIII\n")
    nz = api.NativeDerep(str(fq))
    try:
        dz = nz.to_derep()
        assert dz.map.tolist() == [0, -1, 0, 1]
        got, _ = pc.check_combine(api, [dz, dz_other()], inputs=[nz, dz_other()])
        assert got.map.tolist()[:4] == [0, -1, 0, int(got.seqs.index("TTTTACGT"))]
    finally:
        nz.close()


def dz_other():
    return Derep(["GGGGACGT", "ACGTACGT"], np.array([2, 1], dtype=np.int32), np.array([[30.5] * 8, [20.25] * 8]), np.array([0, 1, -1, 0], dtype=np.int32))


def test_one_sample_and_an_empty_map():
    d = Derep(["ACGTAC", "ACG"], np.array([1, 4], dtype=np.int32), np.array([[30.0] * 6, [31.0] * 3 + [np.nan] * 3]), np.zeros(0, dtype=np.int32))
    got, u2p = pc.check_combine(api, [d])
    assert got.seqs == ["ACG", "ACGTAC"] and u2p[0].tolist() == [1, 0] and got.map.size == 0


def test_a_duplicate_inside_a_sample_and_an_overflowing_sum_are_input_errors():
    q = np.full((2, 4), 30.0)
    dup = Derep(["ACGT", "ACGT"], np.array([2, 1], dtype=np.int32), q, np.zeros(0, dtype=np.int32))
    ok = Derep(["ACGT", "AAAA"], np.array([2, 1], dtype=np.int32), q, np.zeros(0, dtype=np.int32))
    with pytest.raises(_lib.Dada2HipError) as e:
        api.combine_dereps([ok, dup])
    assert e.value.code == 1 and "twice" in str(e.value)
    big = Derep(["ACGT", "CCCC"], np.array([2**31 - 2, 1], dtype=np.int32), q, np.zeros(0, dtype=np.int32))
    with pytest.raises(_lib.Dada2HipError) as e:
        api.combine_dereps([ok, big])
    assert e.value.code == 1 and "integer" in str(e.value)
    edge = Derep(["ACGT", "CCCC"], np.array([2**31 - 3, 1], dtype=np.int32), q, np.zeros(0, dtype=np.int32))
    got, _ = pc.check_combine(api, [ok, edge])                                # exactly INT32_MAX is a sum R can hold
    assert int(got.abundances[0]) == 2**31 - 1
    bad_map = Derep(["ACGT", "AAAA"], np.array([2, 1], dtype=np.int32), q, np.array([0, 2], dtype=np.int32))
    with pytest.raises(_lib.Dada2HipError) as e:
        api.combine_dereps([ok, bad_map])
    assert e.value.code == 1
    with pytest.raises(ValueError):
        api.combine_dereps([])


def test_the_cases_can_see_a_fused_multiply_add():
    """A build whose acc + q * c were contracted into one rounding would differ from the restatement at these positions - so the
    equality above shows the library's loop is not contracted."""
    sy = pc.synthetic_dereps()
    want, _ = pc.restate_combine(sy)
    fused = pc.fused_quals(sy)
    ok = ~np.isnan(want.quals)
    assert np.array_equal(ok, ~np.isnan(fused))
    differ = ok & (fused != want.quals)
    assert differ.sum() >= 1
    got, _ = api.combine_dereps(sy)
    _same_float(got.quals, want.quals, 0)
    assert (got.quals[differ] != fused[differ]).all()
    # ... by one unit in the last place
    assert np.all(np.abs(fused[differ] - want.quals[differ]) <= np.spacing(np.abs(want.quals[differ])))


def _toy_pooled():
    """A pooled result of 4 clusters over 7 pooled uniques; unique 5 is not corrected (NA)."""
    cl = {"sequence": ["AAAA", "CCCC", "GGGG", "TTTT"], "abundance": np.array([50, 30, 12, 8], dtype=np.int32),
          "n0": np.array([40, 20, 10, 8], dtype=np.int32), "n1": np.array([5, 4, 1, 0], dtype=np.int32), "nunq": np.array([3, 2, 1, 1], dtype=np.int32),
          "pval": np.array([np.nan, 1e-30, 1e-50, 1e-12]), "birth_from": np.array([NA, 1, 1, 2], dtype=np.int32),
          "birth_pval": np.array([np.nan, 1e-40, 1e-60, 1e-20]), "birth_fold": np.array([np.nan, 10.0, 20.0, 30.0]),
          "birth_ham": np.array([NA, 2, 3, 1], dtype=np.int32), "birth_qave": np.array([np.nan, 35.0, 36.5, 30.0])}
    bs = {"pos": np.array([1, 3, 0, 1, 2, 3], dtype=np.int32), "ref": list("AAAAAC"), "sub": list("CCGGGT"),
          "qual": np.array([30.0, 31.0, 32.0, 33.0, 34.0, 35.0]), "clust": np.array([2, 2, 3, 3, 3, 4], dtype=np.int32)}
    return DadaResult(cl, bs, np.arange(16 * 3, dtype=np.int32).reshape(16, 3), np.arange(16.0).reshape(4, 4),
                      np.array([1, 2, 1, 3, 2, NA, 4], dtype=np.int32), np.linspace(0.1, 0.7, 7))


def test_the_split_against_hand_worked_expectations():
    res = _toy_pooled()
    # sample A holds pooled uniques 0, 3, 5 (NA) and 2: clusters 1 and 3; cluster 2 and 4 are dropped
    u2p, ab = np.array([0, 3, 5, 2]), np.array([7, 4, 1, 2], dtype=np.int32)
    for split in (pc.restate_split, api.split_pooled):
        s = split(res, ab, u2p)
        assert s.clustering["sequence"] == ["AAAA", "GGGG"]
        assert s.map.tolist() == [1, 2, NA, 1]                                # newBi = 1 1 2 2; NA kept
        assert s.clustering["abundance"].tolist() == [9, 4]                   # this sample's reads: 7 + 2, 4
        assert s.clustering["n0"].tolist() == [40, 10] and s.clustering["nunq"].tolist() == [3, 1]   # the pooled run's
        assert s.clustering["birth_from"].tolist() == [NA, 1] and s.clustering["birth_ham"].tolist() == [NA, 3]
        _same_float(s.clustering["pval"], [np.nan, 1e-50], 0)
        assert s.birth_subs["clust"].tolist() == [2, 2, 2] and s.birth_subs["pos"].tolist() == [0, 1, 2]   # cluster 3's rows, now cluster 2
        assert s.birth_subs["ref"] == list("AAA") and s.birth_subs["sub"] == list("GGG") and s.birth_subs["qual"].tolist() == [32.0, 33.0, 34.0]
        assert np.array_equal(s.clusterquals, res.clusterquals[:, [0, 2]])
        assert np.array_equal(s.subqual, res.subqual) and np.array_equal(s.pval, res.pval)   # still the pooled run's
    # sample B holds 1, 4 and 6: clusters 2 and 4; birth_from still counts POOLED clusters
    u2p, ab = np.array([6, 1, 4]), np.array([8, 20, 10], dtype=np.int32)
    for split in (pc.restate_split, api.split_pooled):
        s = split(res, ab, u2p)
        assert s.clustering["sequence"] == ["CCCC", "TTTT"] and s.map.tolist() == [2, 1, 1]
        assert s.clustering["abundance"].tolist() == [30, 8] and s.clustering["birth_from"].tolist() == [1, 2]
        assert s.birth_subs["clust"].tolist() == [1, 1, 2] and s.birth_subs["sub"] == list("CCT")
    # a sample whose every unique is NA keeps nothing
    s = api.split_pooled(res, np.array([3], dtype=np.int32), np.array([5]))
    assert s.nclust == 0 and s.map.tolist() == [NA] and s.birth_subs["clust"].size == 0 and s.clusterquals.shape == (4, 0)


def test_dada_refuses_what_a_pooled_run_cannot_mean():
    d = [pc.synthetic_dereps()[0], pc.synthetic_dereps()[2]]
    with pytest.raises(ValueError, match="Invalid pool argument."):
        api.dada(d, np.ones((16, 41)), pool="all")
    with pytest.raises(ValueError, match="Invalid pool argument."):
        api.dada(d, np.ones((16, 41)), pool=None)
    with pytest.raises(ValueError):
        api.dada(d, np.ones((16, 41)), pool=True, priors=[None, None])
    with pytest.raises(ValueError):
        api.dada(d, np.ones((16, 41)), pool=True, samples=[None, None])
    with pytest.raises(ValueError):
        api.dada(d, np.ones((16, 41)), pool="pseudo", err_fun=None)
