"""isBimeraDenovo / removeBimeraDenovo / isShiftDenovo on the CPU (tests/bimera_denovo_cases.py): the recorded expectations of
tests/golden/bimera_denovo.json re-derived from the reference's own C++ and from its C restatement; the ranking and the parent
prefixes of dada2_amd/csrc/bimera_plain.h through a stand-alone program built with the address and undefined-behaviour
sanitizers (tools/bimera_plain_check.cpp: plain host C++, nothing loaded into Python) against the parent sets of R/chimeras.R:127
themselves; get_uniques, the table bookkeeping of remove_bimera_denovo with the device call replaced by the restatement, and its
error message."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import bimera_denovo_cases as bc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def test_goldens_from_the_reference(oracle_ref):
    oracle_ref.set_threads(16)
    assert bc.derive(oracle_ref) == bc.golden()


def test_goldens_from_the_c_restatement(oracle_c):
    assert bc.derive(oracle_c) == bc.golden()


def test_the_cases_decide_something():
    """Every threshold case has its TRUE and its FALSE where the issue puts them; the ladder flags no query built from non-parents."""
    g = bc.golden()["cases"]
    for name in ("fold_equal", "parent_abundance", "fold_1_5"):
        assert g[name] == [False, False, False, False, True], name
    assert g["early"][-1] and g["late"][-1] and not any(g["early"][:-1]) and not any(g["late"][:-1])
    assert g["toss"] == [False] * 3 and g["toss_shift_pair"] == [False] * 3
    assert g["oo_exact"] == [False, False, False, False, True] and g["oo_one_off"] == [False, False, True, True, True]
    assert g["oo_one_off_far"] == g["oo_exact"] and g["oo_blocked"] == [False] * 3 and g["oo_unblocked"] == [False, False, True]
    assert g["unequal_ms4"] != g["unequal_ms16"]
    assert g["long"] == [False, False, False, False, True, False]
    assert g["duplicates"] == [False, False, True, False, True, False] and g["zero"] == [False, False, True, True, False]
    lad = g["ladder"]
    ins, outs = lad[bc.LADDER_K::2], lad[bc.LADDER_K + 1::2]
    assert sum(ins) >= 100 and not any(outs) and not any(lad[:bc.LADDER_K])
    sh = bc.golden()["shift"]
    assert sh["pure_shift"] == [False, True, False] and sh["shift_below_overlap"] == [False, False]
    assert sh["shift_above_overlap"] == [False, True] and sh["subsequence_flag0"] == sh["subsequence_flag1"] == [False, False]
    assert 5 <= sum(sh["sixty"]) < len(sh["sixty"])
    ps = np.array(bc.golden()["per_sample"]["flags"])
    assert ps.any(axis=1).all() and len({tuple(r) for r in ps.tolist()}) == 3


# ---- bimera_plain.h ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def plain_check(tmp_path_factory):
    if not (os.path.exists(HIPCC) or shutil.which(HIPCC)):
        pytest.skip("no hipcc for the host build")
    exe = str(tmp_path_factory.mktemp("bimera_plain") / "bimera_plain_check")
    subprocess.check_call([HIPCC, "-O1", "-g", "-std=c++17", "-Wall", "-Xarch_host", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-x", "c++", os.path.join(ROOT, "tools", "bimera_plain_check.cpp"), "-o", exe])
    return exe


def _windows(per, upto):
    ends, r0, w = [], 0, per
    while r0 < upto:
        r0 = min(upto, r0 + w)
        ends.append(r0)
        w = 3 * r0
    return ends


def test_ranking_and_parent_prefixes(plain_check):
    rng = np.random.default_rng(9)
    cases = [([], 2.0, 8.0, 0, 1), ([5], 2.0, 8.0, 0, 1), ([9, 9, 1], 2.0, 8.0, 0, 1), ([8, 9, 100, 1, 1], 2.0, 8.0, 0, 1),
             ([20, 21, 500, 10, 10], 2.0, 8.0, 0, 1), ([4, 5, 100, 3, 3], 1.5, 2.0, 0, 1), ([100, 90, 0, 1, 0], 2.0, 8.0, 0, 1),
             ([100, 90, 0, 1, 0], 2.0, 8.0, 1, 1), ([7] * 9, 0.5, 0.0, 0, 1), ([2 ** 31 - 1, 2 ** 30, 2 ** 30 - 1, 1, 0], 2.0, 8.0, 0, 1),
             ([3, 3, 3, 100, 100, 7, 7], 2.3, 2.5, 0, 1)]
    for _ in range(60):
        n = int(rng.integers(1, 90))
        hi = int(rng.choice([4, 30, 5000]))
        cases.append((rng.integers(0, hi, size=n).tolist(), float(rng.choice([1.0, 1.5, 2.0, 3.7])), float(rng.choice([0, 2, 8, 8.5])),
                      int(rng.integers(0, 2)), int(rng.choice([1, 3]))))
    text = []
    for ab, mf, mp, sz, stride in cases:
        row = []
        for a in ab:
            row += [a] + [int(x) for x in rng.integers(0, 99, size=stride - 1)]    # the other rows of a column-major table
        text.append("%d %r %r %d %d %s" % (len(ab), mf, mp, sz, stride, " ".join(map(str, row))))
    out = subprocess.run([plain_check], input="\n".join(text) + "\n", capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "bimera_plain_check: %d cases" % len(cases) in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]
    lines = out.stdout.splitlines()
    for k, (ab, mf, mp, sz, _) in enumerate(cases):
        rank, P = bc.restate_ranking(ab, mf, mp, bool(sz))
        blk = lines[6 * k: 6 * k + 6]
        assert [int(x) for x in blk[0].split()[1:]] == rank, (k, ab)
        assert [int(x) for x in blk[1].split()[1:]] == P, (k, ab, mf, mp)
        assert blk[2] == "sum %d nquery %d max %d" % (sum(P), sum(p > 0 for p in P), max(P, default=0))
        for line, per in zip(blk[3:], (1, 3, 64)):
            assert [int(x) for x in line.split(":")[1].split()] == _windows(per, max(P, default=0)), (k, per)


# ---- the Python layer, the device call replaced by the restatement ---------------------------------------------------------------------
@pytest.fixture()
def restated_device(monkeypatch, oracle_c):
    from dada2_amd import api

    def rows(mat, seqs, min_fold_parent_over_abundance=2, min_parent_abundance=8, allow_one_off=False, min_one_off_parent_distance=4,
             max_shift=16, match=5, mismatch=-4, gap_p=-8, skip_zero=False, device=0, stats=None):
        return np.array([bc.restate_is_bimera_denovo(oracle_c, list(seqs), r, min_fold_parent_over_abundance, min_parent_abundance,
                                                     allow_one_off, min_one_off_parent_distance, max_shift) for r in np.asarray(mat)], dtype=bool)
    monkeypatch.setattr(api, "bimera_denovo_rows", rows)
    monkeypatch.setattr(api, "is_bimera_denovo_table", lambda mat, seqs, **kw: np.array(bc.restate_consensus(oracle_c, mat, seqs, **kw)))
    return api


def test_get_uniques_forms():
    from dada2_amd import api
    from dada2_amd.io import Derep
    from dada2_amd.opts import DadaResult
    s, a = ["GG", "AC", "TT"], [3, 5, 1]
    for obj in (dict(zip(s, a)), (s, a), (s, np.array(a)), Derep(s, np.array(a, dtype=np.int32), np.zeros((3, 2)), np.zeros(0, dtype=np.int32))):
        gs, ga = api.get_uniques(obj)
        assert gs == s and ga.tolist() == a and ga.dtype == np.int32
    res = DadaResult({"sequence": s, "abundance": np.array(a, dtype=np.int32)}, {}, None, None, None, None)
    assert api.get_uniques(res)[0] == s and api.get_uniques(res)[1].tolist() == a
    mat = np.array([[1, 2, 0], [4, 0, 6]])
    for got in (api.get_uniques((mat, s)), api.get_uniques(mat, seqs=s)):
        assert got[0] == s and got[1].tolist() == [5, 2, 6]
    gs, ga = api.get_uniques((["GG", "AC", "GG", "AA"], [3, 5, 4, 1]))                # tapply(..., sum): merged, then in order of the names
    assert gs == ["AA", "AC", "GG"] and ga.tolist() == [1, 5, 7]
    assert (gs, ga.tolist()) == tuple(bc.restate_get_uniques(["GG", "AC", "GG", "AA"], [3, 5, 4, 1]))
    with pytest.raises(ValueError, match="Unrecognized format"):
        api.get_uniques(7)


def test_remove_bimera_denovo_bookkeeping(restated_device, oracle_c):
    api = restated_device
    g = bc.golden()
    mat, seqs = bc.per_sample_table()
    out, names = api.remove_bimera_denovo((mat, seqs), method="per-sample")
    assert out.tolist() == g["per_sample"]["table"] and [seqs.index(s) for s in names] == g["per_sample"]["kept"]
    assert out.shape[1] < mat.shape[1] and (out.sum(axis=0) > 0).all()
    pooled = np.array(bc.restate_is_bimera_denovo(oracle_c, seqs, mat.sum(axis=0)))
    out, names = api.remove_bimera_denovo(mat, method="pooled", seqs=seqs)
    assert names == [s for s, b in zip(seqs, pooled) if not b] and np.array_equal(out, mat[:, ~pooled])
    cons = np.array(bc.restate_consensus(oracle_c, mat, seqs))
    out, names = api.remove_bimera_denovo((mat, seqs))
    assert names == [s for s, b in zip(seqs, cons) if not b] and np.array_equal(out, mat[:, ~cons])
    # every other input goes through is_bimera_denovo whatever the method says, and keeps its form and order
    c = bc.cases()["duplicates"]
    want = g["cases"]["duplicates"]
    for method in ("consensus", "pooled", "no such method"):
        s, a = api.remove_bimera_denovo((c["seqs"], c["ab"]), method=method)
        assert s == [x for x, b in zip(c["seqs"], want) if not b] and a.tolist() == [x for x, b in zip(c["ab"], want) if not b]
    assert api.is_bimera_denovo((c["seqs"], c["ab"])).tolist() == want
    c = bc.cases()["fold_1_5"]
    assert api.is_bimera_denovo(dict(zip(c["seqs"], c["ab"])), **bc.api_kw(c["kw"])).tolist() == g["cases"]["fold_1_5"]


def test_remove_bimera_denovo_refuses_an_unknown_method():
    from dada2_amd import api
    mat, seqs = bc.per_sample_table()
    with pytest.raises(ValueError, match="Valid values for method: 'pooled', 'consensus', or 'per-sample'"):
        api.remove_bimera_denovo((mat, seqs), method="per_sample")
