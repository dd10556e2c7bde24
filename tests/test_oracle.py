"""CPU tests (-m "not gpu"): pin the oracle.

1. oracle/dada_oracle.c (plain-C restatement) against the committed goldens that the
   REFERENCE ITSELF produced (tests/golden/make_golden.py via oracle/_ref) — bit-exact,
   p-values included, since both sides share oracle/rmath_ppois.c.
2. where oracle/_ref is present, restatement vs reference live on fresh seeded inputs.
3. the ppois restatement against 60-digit truth (golden) and scipy.
"""
import os

import numpy as np
import pytest

from helpers import (BASE_OPTION_CASES, GOLDEN, SCORE_OPTION_CASES, WHOLE_PATH_CASES, assert_results_equal, case_inputs,
                     long_read_sample, seeded_option_sample, tperr1)
from dada2_amd.opts import DadaOpts


@pytest.mark.parametrize("name", WHOLE_PATH_CASES)
def test_restatement_matches_reference_goldens(oracle_c, name):
    d, err, pri, opts, exp, meta = case_inputs(name)
    got = oracle_c.dada_uniques(d.seqs, d.abundances, pri, err, d.quals, opts)
    assert got.nclust == meta["nclust"]
    assert_results_equal(got, exp, exact_float=True, check_birth_from="priors" not in meta)


def test_known_outcomes_from_survey(oracle_c):
    """SURVEY.md §4 probe: sam1F + tperr1 -> 10 partitions, 8655 comparisons / 3032 shrouded."""
    d, err, pri, opts, exp, meta = case_inputs("sam1F_default")
    got = oracle_c.dada_uniques(d.seqs, d.abundances, None, err, d.quals, opts)
    assert got.clustering["abundance"].tolist() == [543, 376, 160, 61, 47, 69, 9, 13, 82, 68]
    assert (got.stats["nalign"], got.stats["nshroud"]) == (8655, 3032)
    d, err, pri, opts, exp, meta = case_inputs("samPB_band32")
    got = oracle_c.dada_uniques(d.seqs, d.abundances, None, err, d.quals, opts)
    assert got.clustering["abundance"].tolist() == [59, 107, 53, 68, 53, 27, 34, 18, 8, 13, 18, 12]


def test_nwalign_goldens(oracle_c):
    z = np.load(os.path.join(GOLDEN, "nwalign_pairs.npz"))
    for s1, s2, band, a0, a1 in zip(z["s1"], z["s2"], z["band"], z["al0"], z["al1"]):
        assert oracle_c.nwalign(str(s1), str(s2), 5, -4, -8, int(band)) == (str(a0), str(a1))


@pytest.mark.parametrize("fq,band", [("sam1F", 16), ("samPB", 32)])
def test_compare_goldens(oracle_c, fq, band):
    from helpers import load_input
    from dada2_amd.io import extend_err
    d = load_input(fq)
    err = extend_err(tperr1(), int(np.ceil(np.nanmax(d.quals))))
    rows = np.load(os.path.join(GOLDEN, f"compare_{fq}.npy"))
    o = DadaOpts(BAND_SIZE=band)
    for c, r, lam, ham, kd, ko in rows[:: (1 if fq == "sam1F" else 2)]:
        c, r = int(c), int(r)
        got = oracle_c.compare(d.seqs[c], d.quals[c, :len(d.seqs[c])], d.seqs[r], d.quals[r, :len(d.seqs[r])], err, o,
                               kdist_cutoff=0.42)
        assert got == (lam, int(ham), kd, ko)


def test_input_validation(oracle_c):
    err = tperr1()
    with pytest.raises(RuntimeError, match="Zero input"):
        oracle_c.dada_uniques([], [], None, err, None)
    with pytest.raises(RuntimeError, match="kmer-size"):
        oracle_c.dada_uniques(["ACGT"], [1], None, err, None)


def test_ppois_against_truth_and_scipy(oracle_c):
    from scipy.special import pdtrc
    rows = np.load(os.path.join(GOLDEN, "ppois_grid.npy"))
    x, lam, truth, ref_p = rows[:, 0], rows[:, 1], rows[:, 2], rows[:, 3]
    got = np.array([oracle_c.ppois_upper(a, b) for a, b in zip(x, lam)])
    assert np.array_equal(got, ref_p)                      # same bits as when the goldens were made
    normal = truth > 2.3e-308
    rel = np.abs(got[normal] - truth[normal]) / truth[normal]
    # R's algorithm redoes results < 1e-292 in log space (pgamma.c), losing ~|log p|*eps there
    main = truth[normal] > 1e-290
    # dpois_raw = exp(-stirlerr - bd0)/sqrt(2 pi x): conditioning ~ |log p| * eps, so deep tails carry ~1e-12
    assert rel[main].max() < 2e-12, rel[main].max()
    shallow = truth[normal] > 1e-20
    assert rel[shallow].max() < 1e-13, rel[shallow].max()
    assert rel[~main].max() < 2e-11, rel[~main].max()
    assert (got[truth == 0.0] == 0.0).all()
    sp = pdtrc(x[normal][main], lam[normal][main])
    ok = sp > 1e-300
    assert (np.abs(sp[ok] - got[normal][main][ok]) / got[normal][main][ok]).max() < 1e-11
    # calc_pA columns (conditional / unconditional), reference pval.cpp:44-64
    for (a, b, pc, pu) in rows[::7, [0, 1, 4, 5]]:
        assert oracle_c.calc_pA(int(a) + 1, b, False) == pc or (np.isnan(pc) and np.isnan(oracle_c.calc_pA(int(a) + 1, b, False)))
        assert oracle_c.calc_pA(int(a) + 1, b, True) == pu


# ---------------------------------------------------------------------------------------------
# live cross-checks against the reference (only where oracle/_ref has been built)
def _random_sample(seed, n=600, L=120, G=8, Lmin=None, indel=0.0):
    from dada2_amd.synth import make_sample
    return make_sample(tperr1(), n, L=L, G=G, seed=seed, Lmin=Lmin, indel_rate=indel, chunk=2000)


@pytest.mark.parametrize("seed,kw", BASE_OPTION_CASES + SCORE_OPTION_CASES, ids=lambda v: str(v) if isinstance(v, int) else "-".join(f"{k}={x}" for k, x in v.items()) or "default")
def test_restatement_vs_reference_live(oracle_c, oracle_ref, seed, kw):
    """The seeded option sweep (tests/helpers.py): restatement == reference, serial and multithreaded - among them the user
    alignment scores and SSE = 1 that select code paths of their own on both sides."""
    d, pri = seeded_option_sample(seed, n=600, chunk=2000)
    o = DadaOpts(**kw)
    for mt in (False, True):
        a = oracle_ref.dada_uniques(d.seqs, d.abundances, pri, tperr1(), d.quals, o, multithread=mt)
        b = oracle_c.dada_uniques(d.seqs, d.abundances, pri, tperr1(), d.quals, o, multithread=mt)
        assert_results_equal(a, b, exact_float=True, check_birth_from=pri is None)


def _regime_case_names():
    import regime_cases as R
    return list(R.CASES)


@pytest.mark.parametrize("name", _regime_case_names())
def test_restatement_vs_reference_live_on_the_regime_cases(oracle_c, oracle_ref, name):
    """tests/regime_cases.py - more than 1 024 partitions, tie lists of thousands of candidates (the scan-order rule with
    bi_pop_raw's swap-with-last), abundances up to the top of R's integer range (where $subqual and the 32-bit q * reads of
    $clusterquals wrap) - restatement == reference, serial and multithreaded: what licenses the restatement as the checker of the
    emulated and the -m gpu runs in these regimes.  The case's facts are asserted on the way."""
    import regime_cases as R
    d, pri, opts, facts = R.build(name)
    b = R.check_facts(name)
    for mt in (False, True):
        a = oracle_ref.dada_uniques(d.seqs, d.abundances, pri, tperr1(), d.quals, opts, multithread=mt)
        if mt and name not in R.GPU_ONLY:    # (the restatement's flag only changes its work counters: not run twice on the largest case)
            b = oracle_c.dada_uniques(d.seqs, d.abundances, pri, tperr1(), d.quals, opts, multithread=True)
        assert_results_equal(a, b, exact_float=True, check_birth_from=pri is None)
    if "subqual_and_the_q_times_reads_product_wrap" in facts:
        assert (a.subqual < 0).any() and np.array_equal(a.clusterquals, b.clusterquals, equal_nan=True)


def test_restatement_vs_reference_reads_longer_than_2047(oracle_c, oracle_ref):
    """2.1-2.3 kb reads (PacBio-style qualities, band 32): the checker of the -m gpu long-read case, pinned to the reference."""
    d, err = long_read_sample()
    o = DadaOpts(BAND_SIZE=32)
    a = oracle_ref.dada_uniques(d.seqs, d.abundances, None, err, d.quals, o)
    b = oracle_c.dada_uniques(d.seqs, d.abundances, None, err, d.quals, o)
    assert a.nclust > 8 and max(map(len, d.seqs)) > 2047
    assert_results_equal(a, b, exact_float=True)


# NOTE: there is no "no quality matrix" case to pin: with a 0-row quals matrix the reference
# itself crashes (error.cpp:158 reads raw->qual[pos1] unconditionally), and R always passes
# quals (R/dada.R:337) — the product therefore rejects quals == NULL up front.


def test_nwalign_vs_both_reference_aligners(oracle_c, oracle_ref):
    rng = np.random.default_rng(99)
    for k in range(1500):
        L1 = int(rng.integers(6, 200))
        a = rng.integers(0, 4, L1)
        b = a.copy() if k % 4 else rng.integers(0, 4, int(rng.integers(6, 200)))
        for _ in range(int(rng.integers(0, 6))):
            p = int(rng.integers(0, len(b)))
            r = rng.random()
            b = np.delete(b, p) if (r < 0.3 and len(b) > 8) else (np.insert(b, p, rng.integers(0, 4)) if r < 0.6 else b)
            if r >= 0.6:
                b[p] = rng.integers(0, 4)
        s1 = "".join("ACGT"[i] for i in a)
        s2 = "".join("ACGT"[i] for i in b)
        band = int(rng.choice([1, 2, 3, 8, 15, 16, 17, 32, -1]))
        g = int(rng.choice([-8, -2, -12]))
        want = oracle_ref.nwalign(s1, s2, 5, -4, g, band, "vectorized")
        assert want == oracle_ref.nwalign(s1, s2, 5, -4, g, band, "endsfree")
        assert oracle_c.nwalign(s1, s2, 5, -4, g, band) == want


def test_homopolymer_gap_restatement_matches_the_reference_on_homopolymer_rich_reads(oracle_c, oracle_ref):
    """nwalign_endsfree_homo inside the whole path (HOMOPOLYMER_GAP_PENALTY, the 454 / Ion Torrent setting): reads whose errors are
    run-length changes of homopolymers, where the option changes the result - restatement vs the reference itself."""
    from helpers import HOMO_OPTION_CASES, homopolymer_sample
    from dada2_amd.io import extend_err
    changed = 0
    for seed, kw in HOMO_OPTION_CASES:
        d = homopolymer_sample(seed)
        err = extend_err(tperr1(), 40)
        want = oracle_ref.dada_uniques(d.seqs, d.abundances, None, err, d.quals, DadaOpts(**kw))
        got = oracle_c.dada_uniques(d.seqs, d.abundances, None, err, d.quals, DadaOpts(**kw))
        assert_results_equal(got, want)
        plain = dict(kw); plain.pop("HOMOPOLYMER_GAP_PENALTY")
        other = oracle_c.dada_uniques(d.seqs, d.abundances, None, err, d.quals, DadaOpts(**plain))
        changed += not np.array_equal(other.subqual, got.subqual)
    assert changed == len(HOMO_OPTION_CASES)          # (the sample is one on which the homopolymer penalty matters)


def test_bimera_pair_quantities_restatement_matches_the_reference(oracle_c, oracle_ref):
    """get_lr / get_ham_endsfree per alignment (chimera.cpp:211-293): the restatement against the reference's own functions on
    its own alignments - shared halves, shifts, truncations, indels, unrelated pairs; one-off on and off, four bands, two score sets."""
    from helpers import BIMERA_PAIR_OPTIONS, bimera_pair_cases
    for seed, n, L in ((1, 150, 60), (2, 150, 130), (3, 120, 251)):
        qs, ps = bimera_pair_cases(seed, n, L)
        for oo, ms, sc in BIMERA_PAIR_OPTIONS:
            want = oracle_ref.bimera_pairs(qs, ps, oo, *sc, ms)
            got = oracle_c.bimera_pairs(qs, ps, oo, *sc, ms)
            assert np.array_equal(got, want), (seed, oo, ms, sc, np.nonzero((got != want).any(axis=1))[0][:5])
        assert (want[:, 0] + want[:, 1] > 0).any() and (want[:, 4] > 0).any()
    from helpers import bimera_short_pair_cases
    qs, ps = bimera_short_pair_cases(5, 400)
    for oo, ms in ((True, 16), (False, 16), (True, 4), (True, 1), (True, 40)):
        assert np.array_equal(oracle_c.bimera_pairs(qs, ps, oo, max_shift=ms), oracle_ref.bimera_pairs(qs, ps, oo, max_shift=ms)), (oo, ms)


def test_bimera_restatement_matches_reference_goldens(oracle_c):
    """Bimera identification (src/chimera.cpp): the C restatement against the vectors the reference itself produced
    (tests/golden/make_bimera_golden.py) - the checker of the GPU path's dada2hip_table_bimera2 / dada2hip_is_bimera."""
    z = np.load(os.path.join(GOLDEN, "bimera_table.npz"))
    mat, seqs = z["mat"], [str(s) for s in z["seqs"]]
    for oo in (0, 1):
        for ms in (16, 4):
            nflag, nsam = oracle_c.table_bimera2(mat, seqs, allow_one_off=bool(oo), max_shift=ms)
            assert np.array_equal(nflag, z[f"nflag_oo{oo}_ms{ms}"]) and np.array_equal(nsam, z[f"nsam_oo{oo}_ms{ms}"])
        tot = mat.sum(axis=0)
        for j, s in enumerate(seqs):
            pars = [seqs[k] for k in range(len(seqs)) if tot[k] > 2 * tot[j] and tot[k] > 8]
            assert oracle_c.is_bimera(s, pars, allow_one_off=bool(oo)) == bool(z[f"isbim_oo{oo}"][j]), (j, oo)
    assert z["nflag_oo0_ms16"].max() == 2 and z["nflag_oo1_ms16"].sum() > z["nflag_oo0_ms16"].sum()


def test_restated_aligner_variants_match_the_reference_goldens(oracle_c):
    """nw_general() of the C restatement - nwalign_endsfree, nwalign_endsfree_homo, global nwalign - on the 300 pairs whose
    alignments came out of the reference's own C_nwalign (tests/golden/make_homo_golden.py)."""
    z = np.load(os.path.join(GOLDEN, "nwalign_variants.npz"))
    kinds = set()
    for i in range(len(z["s1"])):
        got = oracle_c.C_nwalign(str(z["s1"][i]), str(z["s2"][i]), 5, -4, -8, int(z["homo_gap"][i]), int(z["band"][i]), bool(z["endsfree"][i]))
        assert got == (str(z["al0"][i]), str(z["al1"][i])), i
        kinds.add((bool(z["endsfree"][i]), int(z["homo_gap"][i]) != -8))
    assert kinds == {(True, False), (True, True), (False, False), (False, True)}


def test_restated_homopolymer_path_matches_the_reference_live(oracle_c, oracle_ref):
    """dada_uniques with HOMOPOLYMER_GAP_PENALTY (raw_align -> nwalign_endsfree_homo) : restatement vs the reference, live."""
    from dada2_amd.opts import DadaOpts
    from dada2_amd.synth import make_sample
    d = make_sample(tperr1(), 700, L=110, G=8, seed=77, Lmin=90, indel_rate=3e-3, chunk=4000)
    for kw in (dict(HOMOPOLYMER_GAP_PENALTY=-1), dict(HOMOPOLYMER_GAP_PENALTY=-2, BAND_SIZE=-1), dict(HOMOPOLYMER_GAP_PENALTY=0, BAND_SIZE=8)):
        o = DadaOpts(**kw)
        a = oracle_c.dada_uniques(d.seqs, d.abundances, None, tperr1(), d.quals, o)
        b = oracle_ref.dada_uniques(d.seqs, d.abundances, None, tperr1(), d.quals, o)
        assert_results_equal(a, b, exact_float=True)



def test_restated_compare_matches_the_reference_on_the_aligner_case_table(oracle_c, oracle_ref):
    """tests/aligner_cases.py (the short-read cases, thinned): the restatement's compare against the reference's own sub_new +
    compute_lambda_ts, bit for bit - so the restatement and the kernels cannot share one misreading of these shapes."""
    import aligner_cases as A
    npairs = 0
    for c in A.small_cases():
        b = A.build(c, lean=True)
        for ci in b.centres:
            cq = b.quals[ci, : len(b.seqs[ci])]
            for i, s in enumerate(b.seqs):
                rq = b.quals[i, : len(s)]
                got = oracle_c.compare(b.seqs[ci], cq, s, rq, b.err, b.opts, kdist_cutoff=1.0)
                want = oracle_ref.compare(b.seqs[ci], cq, s, rq, b.err, b.opts, kdist_cutoff=1.0)
                assert got[:2] == want[:2], (c.name, b.kinds[ci], b.kinds[i], got, want)
                npairs += 1
    assert npairs > 20000


def test_restated_bimera_pairs_match_the_reference_on_the_aligner_case_table(oracle_c, oracle_ref):
    import aligner_cases as A
    for ms, diff, _, _ in A.LR_ROWS:
        qs, ps = A.bimera_pair_set(ms, diff, seed=ms * 100 + diff)
        for sc in A.LR_SCORES:
            for oo in (False, True):
                assert np.array_equal(oracle_c.bimera_pairs(qs, ps, oo, *sc, ms), oracle_ref.bimera_pairs(qs, ps, oo, *sc, ms)), (ms, diff, sc, oo)


def _nwvec_excluded(a, c, sc):
    """The two stated differences between C_nwvec and C_nwalign: a second sequence of one base (nwalign_vectorized2 against
    nwalign_endsfree), and C_nwvec's 16-bit scores ((len1 + len2) max|score| >= 32 767)."""
    return len(c) == 1 or (len(a) + len(c)) * max(abs(x) for x in sc) >= 32767


def test_restated_aligners_match_the_reference_on_the_pair_case_table(oracle_c, oracle_ref):
    """tests/pair_cases.py, every case: the restatement's C_nwalign (what the GPU tests of the pairwise exports compare with)
    against the reference's own C_nwalign, and for the nwvec cases against the reference's C_nwvec call too, less the two
    stated exclusions - which may take at most 5 % of a case's pairs and never all pairs of a pair class.  Each batch's facts
    (interior gaps in either string, a pair that depends on the tie order) are asserted on the way."""
    import pair_cases as P
    npairs = nvec = 0
    for c in P.vec_cases():
        b = P.build(c)
        sc = P.SCORES[c.score]
        want = P.expected(oracle_c, c, oracle_ref)
        P.check_facts(oracle_c, c, want)
        left = {}
        nexcl = 0
        for i, (a, s, al) in enumerate(zip(b.s1, b.s2, want)):
            P.check_alignment(c.name, i, a, s, al)
            left.setdefault(b.kinds[i], 0)
            if not c.letters:
                assert tuple(al) == tuple(oracle_ref.C_nwalign(a, s, sc[0], sc[1], sc[2], None, c.band, c.endsfree)), (c.name, i, b.kinds[i], a, s)
                npairs += 1
                if _nwvec_excluded(a, s, sc):
                    nexcl += 1
                    continue
                assert tuple(al) == tuple(oracle_ref.nwvec_raw(a, s, sc[0], sc[1], sc[2], c.band, c.endsfree)), (c.name, i, b.kinds[i], a, s)
                nvec += 1
            left[b.kinds[i]] += 1
        assert nexcl * 20 <= c.n, (c.name, "excluded from the C_nwvec comparison:", nexcl, "of", c.n)
        assert all(v > 0 for v in left.values()), (c.name, "pair classes with no pair left:", [k for k, v in left.items() if not v])
    for c in P.align_cases():
        for a, s in c.pairs:
            assert oracle_c.C_nwalign(a, s, 5, -4, -8, c.homo_gap, c.band, True) == oracle_ref.C_nwalign(a, s, 5, -4, -8, c.homo_gap, c.band, True), (c.name, a, s)
            npairs += 1
    assert npairs > 4000 and nvec > 4000, (npairs, nvec)


def test_reference_global_aligners_part_below_the_band_sentinel(oracle_c, oracle_ref):
    """the reference's global alignment of C_nwalign (band edge -9999) and of C_nwvec (band edge INT16_MIN + 64)
    give different strings once in-band scores fall below -9999 - 1/-64/-64, 233 nt against 40 nt, band 32.  The restatement (and
    the device) follow C_nwalign there; tests/pair_cases.py keeps its global 1/-64/-64 batches at reads of at most 105 nt."""
    import pair_cases as P
    rng = np.random.default_rng(258)
    a = P._rnd(rng, 233)
    b = a[96:136]
    assert not _nwvec_excluded(a, b, (1, -64, -64))
    want = oracle_ref.C_nwalign(a, b, 1, -64, -64, None, 32, False)
    assert oracle_c.C_nwalign(a, b, 1, -64, -64, None, 32, False) == want
    assert tuple(oracle_ref.nwvec_raw(a, b, 1, -64, -64, 32, False)) != tuple(want)
    for ef, sc in ((True, (1, -64, -64)), (False, (1, -8, -8))):         # (ends free, or global with scores above -9999: one answer)
        assert tuple(oracle_ref.nwvec_raw(a, b, *sc, 32, ef)) == tuple(oracle_ref.C_nwalign(a, b, *sc, None, 32, ef))
