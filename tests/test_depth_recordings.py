"""The recordings of the reference at bench.py's depth (tests/golden/depth_*.expected.npz) and the comparator the GPU tests
hold them against (helpers.assert_matches_recording), checked without a GPU:

  - each recording is what its workload is: the options bench.py uses, the error matrix it draws configs[4] with, and for the
    selfConsist loop every pass's err is the refit of the pass before it (accumulate_trans -> noqual_errfun -> the
    R/dada.R:385-388 diagonal fix after pass 0 -> extend_err), with the loop's stopping rule;
  - the files stay within the size budget of committed files;
  - the comparator is sensitive: one changed p-value (1e-9 relative), map entry, birth_subs position or subqual count of a
    recorded result is rejected.

The input hashes are checked against the generator by the GPU tests, which draw the samples anyway (200 000 x 1.5 kb and
10^6 x 250 nt take minutes and several GB here: too much for the CPU suite)."""
import copy
import os
import sys

import numpy as np
import pytest

from helpers import DEPTH_RECORDINGS, GOLDEN, assert_matches_recording, canon_sha256, load_recording, tperr1
from dada2_amd.api import accumulate_trans, noqual_errfun
from dada2_amd.io import extend_err
from dada2_amd.opts import DadaOpts, DadaResult

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def bench():
    sys.path.insert(0, ROOT)
    import bench as b
    return b


@pytest.fixture(scope="module", params=sorted(DEPTH_RECORDINGS))
def rec(request):
    return load_recording(request.param)


def test_recordings_fit_the_size_budget():
    sizes = [os.path.getsize(os.path.join(GOLDEN, f)) for f in DEPTH_RECORDINGS.values()]
    assert all(s < 1_000_000 for s in sizes) and sum(sizes) < 2_000_000, sizes


def test_long_read_recording_is_bench_config5(bench):
    r = load_recording("cfg5")
    c = bench.CONFIGS[5]
    assert DadaOpts(**r["meta"]["opts"]) == DadaOpts(BAND_SIZE=c["band"])          # bench.py sub_config5 / --config 5
    assert r["meta"]["nuniques"] == c["uniques"] and r["meta"]["npasses"] == 1 and r["err_out"] is None
    p = r["passes"][0]
    assert np.array_equal(p["err"], extend_err(tperr1(), c["q_max"]))                # bench.make_inputs
    assert p["max_clust"] is None and p["nclust"] == c["variants"] == 128             # no MAX_CLUST: every partition
    assert p["result"].map is not None and p["result"].pval is not None              # small enough to keep


def test_selfconsist_recording_is_the_refit_loop(bench):
    r = load_recording("sc1M")
    o = DadaOpts(**r["meta"]["opts"])
    assert o == DadaOpts(BAND_SIZE=bench.CONFIGS[3]["band"])                         # bench.py --selfconsist
    assert r["meta"]["nuniques"] == bench.CONFIGS[3]["uniques"]
    ps = r["passes"]
    q = ps[0]["err"].shape[1] - 1
    assert np.all(ps[0]["err"] == 1.0) and ps[0]["max_clust"] == 1 and ps[0]["nclust"] == 1   # R/dada.R:298 start
    assert all(p["max_clust"] is None for p in ps[1:]) and max(p["nclust"] for p in ps) > 100
    errs = []                                                                         # the loop's list, as api.dada keeps it
    for k, p in enumerate(ps):
        new = noqual_errfun(accumulate_trans([p["result"].subqual]))
        if k == 0:
            new[[0, 5, 10, 15], :] = 1.0                                              # R/dada.R:385-388
        if k + 1 < len(ps):
            assert np.array_equal(extend_err(new, q), ps[k + 1]["err"]), f"err of pass {k + 1} is not the refit of pass {k}"
            errs.append(new)
        else:
            assert np.array_equal(new, r["err_out"]), "err_out is not the refit of the last pass"
    converged = any(np.array_equal(e, r["err_out"]) for e in errs)
    assert converged == r["meta"]["converged"]
    assert converged or len(ps) == o.MAX_CONSIST + 1


def _long_read_pass():
    """The recorded configs[4] pass, and a whole result that matches it (p-values of the rows not recorded are 1.0).  The
    recording keeps clusterquals as a sha256 only: the pass gets a stand-in array and its hash."""
    r = load_recording("cfg5")["passes"][0]
    want = r["result"]
    cq = want.clusterquals
    if cq is None:
        cq = np.round(np.random.default_rng(5).uniform(20, 90, size=(1510, r["nclust"])), 2)
        cq[1480:, :7] = np.nan
        r = dict(r, clusterquals_sha256=canon_sha256(cq))
    return r, cq


def _whole(r, cq):
    want = r["result"]
    pval = np.ones(int(r["pval_rows"].max()) + 1)
    pval[r["pval_rows"]] = want.pval
    return DadaResult(copy.deepcopy(want.clustering), copy.deepcopy(want.birth_subs), want.subqual.copy(), cq.copy(),
                      want.map.copy(), pval)


def _first_finite(a):
    return np.unravel_index(np.flatnonzero(np.isfinite(a))[0], a.shape)


def _perturbations(r):
    """(what, function that changes a copy of the result in one place)."""
    want = r["result"]
    rows = np.flatnonzero((want.pval > 0) & (want.pval < 1))
    assert rows.size, "no p-value strictly between 0 and 1 recorded"
    i = int(r["pval_rows"][rows[0]])
    cp = int(np.flatnonzero(np.isfinite(want.clustering["birth_fold"]))[-1])
    b = len(want.birth_subs["pos"]) // 2
    sq = tuple(np.argwhere(want.subqual > 0)[0])

    def pval(g): g.pval[i] *= 1 + 1e-9
    def fold(g): g.clustering["birth_fold"][cp] = np.nextafter(g.clustering["birth_fold"][cp], np.inf)
    def map_(g): m = np.flatnonzero(g.map > 0)[len(g.map) // 3]; g.map[m] = g.map[m] % r["nclust"] + 1
    def bs_pos(g): g.birth_subs["pos"][b] += 1
    def subqual(g): g.subqual[sq] += 1
    def cquals(g): g.clusterquals[_first_finite(g.clusterquals)] += 1.0
    def seq(g): g.clustering["sequence"][-1] = g.clustering["sequence"][-1][::-1]
    return [("pval", pval), ("birth_fold by one ulp", fold), ("map", map_), ("birth_subs pos", bs_pos), ("subqual", subqual),
            ("clusterquals", cquals), ("sequence", seq)]


def test_comparator_accepts_the_recording_and_rejects_one_change():
    r, cq = _long_read_pass()
    assert_matches_recording(_whole(r, cq), r)
    for what, change in _perturbations(r):
        g = _whole(r, cq)
        change(g)
        try:
            assert_matches_recording(g, r)
        except AssertionError:
            continue
        pytest.fail(f"a changed {what} went through")


def test_comparator_checks_what_a_recording_keeps_only_as_a_hash():
    # (passes of the 10^6 loop whose map / clusterquals did not fit: the sha256 alone must catch a change)
    r, cq = _long_read_pass()
    g = _whole(r, cq)
    slim = dict(r, result=DadaResult(r["result"].clustering, r["result"].birth_subs, r["result"].subqual, None, None,
                                     r["result"].pval))
    assert_matches_recording(g, slim)
    g.map[-1] = g.map[-1] % r["nclust"] + 1
    with pytest.raises(AssertionError, match="map sha256"):
        assert_matches_recording(g, slim)
    g = _whole(r, cq)
    k = _first_finite(g.clusterquals)
    g.clusterquals[k] = np.nextafter(g.clusterquals[k], np.inf)
    with pytest.raises(AssertionError, match="clusterquals sha256"):
        assert_matches_recording(g, slim)


def test_every_recorded_pass_is_complete(rec):
    for p in rec["passes"]:
        res = p["result"]
        n = p["nclust"]
        assert len(res.clustering["sequence"]) == n and all(len(res.clustering[c]) == n for c in res.clustering)
        assert np.all(np.diff(p["pval_rows"]) > 0) and p["pval_rows"][-1] < rec["meta"]["nuniques"]
        if res.pval is not None:
            assert res.pval.shape == p["pval_rows"].shape
        assert res.subqual.shape == (16, p["err"].shape[1])
        if res.map is not None:
            assert res.map.shape == (rec["meta"]["nuniques"],) and res.map.min() >= 1 and res.map.max() <= n


def test_input_cache_is_never_seen_half_written(bench, tmp_path, monkeypatch):
    """The GPU tests draw their samples through bench.py's input cache, possibly while an at-size worker draws the same one:
    a cache file appears under its final name only once it is whole (written aside, then renamed)."""
    from dada2_amd.io import Derep
    monkeypatch.setenv("DADA2HIP_BENCH_CACHE", str(tmp_path))
    d = Derep(["ACGT", "ACGA"], np.array([3, 1], dtype=np.int32), np.full((2, 4), 30.0), np.array([1, 2], dtype=np.int32))
    real_savez, writes = np.savez, []

    def savez(path, **kw):
        writes.append(path)
        assert not [f for f in os.listdir(tmp_path) if f.endswith(".npz") and ".tmp" not in f], "final name taken before the write"
        real_savez(path, **kw)

    monkeypatch.setattr(bench.np, "savez", savez)
    got = bench._cached(lambda err, n, **kw: d)(np.ones((16, 41)), 2, seed=1)
    assert len(writes) == 1 and ".tmp" in os.path.basename(writes[0])
    (final,) = [f for f in os.listdir(tmp_path)]
    assert ".tmp" not in final
    again = bench._cached(lambda err, n, **kw: pytest.fail("drawn twice"))(np.ones((16, 41)), 2, seed=1)
    assert again.seqs == got.seqs and np.array_equal(again.quals, d.quals) and np.array_equal(again.abundances, d.abundances)
