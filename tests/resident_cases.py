"""One resident sample (dada2hip_sample_create once, then runs, set_priors, set_prior_seqs and compares in any order) across changing
options, error matrices, prior flags, aborts and errors: the cases the library is held to.  tests/test_gpu_resident.py runs them on
the device, tests/test_emu_resident.py a cut of them (emu_run) under the emulator.

What a run leaves on the handle - the Run object with its partition state, the round-engine buffers that are not cleared, the
aligner rings sized by band and class, the uploaded error matrix, buffers that never shrink, freed memory that the allocation
cache hands to the next sample - is DESIGN.md §9a.  Every expected result is the oracle's on a FRESH computation
(oracle.cport.dada_uniques, which tests/test_oracle.py pins to the reference; pool_cases.reference_run for the match sample),
compared with helpers.assert_results_equal at P_RTOL, the work counters with it (ncompare - nskipped = the reference's nalign;
nshroud), and computed once per process and set of inputs (_ORACLE).

Facts before trust (the habit of tests/regime_cases.py): a walk proves nothing where two consecutive steps give the same result, so
that they differ is asserted from the oracle alone before the library is asked (assert_steps_differ); likewise that a prior flag
changes the reference's result, and that the constructed inputs of the device-raised error fail, or succeed, in the oracle where
they must."""
from collections import namedtuple
from dataclasses import replace

import numpy as np

from dada2_amd.io import Derep, extend_err, inflate_err
from dada2_amd.opts import DadaOpts
from helpers import P_RTOL, assert_results_equal, case_inputs, seeded_option_sample, tperr1
from species_cases import with_env

ERR_RUNTIME, ERR_ABORTED = 3, 5                                      # include/dada2hip.h
ENGINE_ENVS = [{}, {"DADA2HIP_V3_GRID": "3"}, {"DADA2HIP_V2_TAIL": "chain"}, {"DADA2HIP_ENGINE": "classic"}]   # test_gpu_scale_and_edges.py
ENGINE_IDS = ["persistent-tail", "persistent-tail-grid3", "chains", "classic-engine"]
COUNTERS = ("ncompare", "nskipped", "nshroud", "nnw", "ngapless")


# ---- the samples ------------------------------------------------------------------------------------------------------------------------
def _rand(rng, n):
    return "".join("ACGT"[int(x)] for x in rng.integers(0, 4, size=n))


def _shifted(rng, s, shift, lo, hi):
    """s with ``shift`` bases taken out at lo and as many random ones put in at hi: the same length (the band is not widened by a
    length difference, nwalign_endsfree.cpp), and s[lo + shift:hi] sits ``shift`` cells off the main diagonal - an alignment finds
    it only with BAND_SIZE >= shift (or -1); a narrower band pairs unrelated bases there and the unique is born as a partition."""
    return s[:lo] + s[lo + shift:hi] + _rand(rng, shift) + s[hi:]


_SAMPLES = {}


def option_sample(small=False):
    """helpers.seeded_option_sample(14) (800 uniques of 100-120 nt, ragged, single-base deletions) - or, ``small``, the emulator's
    150 uniques of 66-80 nt - plus a few copies of its most abundant unique with a stretch shifted by 6, by 20 and by 40 cells,
    three reads each, and one by 40 with a single read.  Without them every band from 4 to -1 gives one result on this sample (the
    oracle says so) and a walk over BAND_SIZE would compare nothing; with them band 4, 16, 32 and -1 give four, and
    DETECT_SINGLETONS has a singleton to detect."""
    key = "small" if small else "option"
    if key not in _SAMPLES:
        if small:
            from dada2_amd.synth import make_sample
            d = make_sample(tperr1(), 150, L=80, G=8, seed=33, Lmin=66, indel_rate=4e-3, chunk=600)
            shifts = ((6, 12, 60, 3), (20, 8, 70, 3), (20, 6, 72, 1))
        else:
            d, _ = seeded_option_sample(14)
            shifts = ((6, 20, 90, 3), (20, 15, 95, 3), (40, 10, 100, 3), (40, 8, 102, 1))
        rng = np.random.default_rng(140)
        s0 = d.seqs[0]
        assert all(hi <= len(s0) for _, _, hi, _ in shifts), len(s0)
        seqs, ab, q = list(d.seqs), list(d.abundances), [row for row in np.asarray(d.quals)]
        for shift, lo, hi, reads in shifts:
            s = _shifted(rng, s0, shift, lo, hi)
            assert s not in seqs and len(s) == len(s0)
            seqs.append(s); ab.append(reads); q.append(q[0].copy())
        order = np.argsort(-np.asarray(ab), kind="stable")
        first20 = len(d.seqs) + [s[0] for s in shifts].index(20)     # (the first unique shifted by 20 cells: a centre for compare())
        _SAMPLES[key + ":shift20"] = int(np.flatnonzero(order == first20)[0])
        _SAMPLES[key] = Derep([seqs[int(k)] for k in order], np.asarray(ab, dtype=np.int32)[order], np.asarray(q)[order], np.zeros(0, dtype=np.int32))
    return _SAMPLES[key]


def other_sample():
    """A smaller, different sample (the second tenant of case 7): 300 uniques of 90 nt."""
    if "other" not in _SAMPLES:
        from dada2_amd.synth import make_sample
        _SAMPLES["other"] = make_sample(tperr1(), 300, L=90, G=8, seed=71, chunk=1500)
    return _SAMPLES["other"]


# ---- the oracle, once per set of inputs -------------------------------------------------------------------------------------------------
Step = namedtuple("Step", "name kw use_quals emu")


def S(name, emu=False, use_quals=1, **kw):
    return Step(name, kw, use_quals, emu)


def copts_of(step, max_clust=None):
    """dada2hip_opts of a step: DadaOpts.to_c, and use_quals, which R/dada.R hard-wires and only the C ABI can switch off."""
    co = DadaOpts(**step.kw).to_c(max_clust=max_clust)
    co.use_quals = int(step.use_quals)
    return co


DEFAULTS = S("defaults", emu=True)
_ORACLE = {}


def oracle_run(d, err, step=DEFAULTS, priors=None, max_clust=None):
    """oracle.cport.dada_uniques on a fresh computation, given the same dada2hip_opts the library gets."""
    from oracle import cport
    co = copts_of(step, max_clust)
    pr = None if priors is None else np.ascontiguousarray(priors, dtype=np.uint8)
    key = (id(d), bytes(co), np.ascontiguousarray(err).tobytes(), err.shape, None if pr is None else pr.tobytes())
    if key not in _ORACLE:
        _ORACLE[key] = cport.dada_uniques(d.seqs, d.abundances, pr, err, d.quals, copts=co)
    return _ORACLE[key]


def results_differ(a, b):
    """In clustering, map or pval - by far more than the comparison's tolerance, or it could not tell them apart."""
    if a.clustering["sequence"] != b.clustering["sequence"] or not np.array_equal(a.map, b.map):
        return True
    if any(not np.array_equal(a.clustering[c], b.clustering[c]) for c in ("abundance", "n0", "n1", "nunq", "birth_ham", "birth_from")):
        return True
    x, y = np.nan_to_num(a.pval, nan=-1.0), np.nan_to_num(b.pval, nan=-1.0)
    return not np.allclose(x, y, rtol=1e4 * P_RTOL, atol=0)


def check_run(got, want, check_birth_from=True):
    assert_results_equal(got, want, p_rtol=P_RTOL, check_birth_from=check_birth_from)
    st = got.stats
    assert st["ncompare"] - st["nskipped"] == want.stats["nalign"], ("nalign", st["ncompare"], st["nskipped"], want.stats["nalign"])
    assert st["nshroud"] == want.stats["nshroud"], ("nshroud", st["nshroud"], want.stats["nshroud"])


def assert_same_run(a, b):
    """Two runs of one sample with the same inputs: every bit and every work counter."""
    assert_results_equal(a, b, exact_float=True)
    assert [a.stats[c] for c in COUNTERS] == [b.stats[c] for c in COUNTERS], [(c, a.stats[c], b.stats[c]) for c in COUNTERS]


# ---- case 1: the option walk ------------------------------------------------------------------------------------------------------------
USER_SCORES = dict(MATCH=4, MISMATCH=-5, GAP_PENALTY=-7)
WALK = [
    DEFAULTS,
    S("band32", emu=True, BAND_SIZE=32), S("band4", emu=True, BAND_SIZE=4), S("band-1", BAND_SIZE=-1), S("band0", emu=True, BAND_SIZE=0),
    S("band19_user_scores", BAND_SIZE=19, **USER_SCORES),
    DEFAULTS,
    S("no_kmers", emu=True, USE_KMERS=False), S("no_greedy_no_gapless", GREEDY=False, GAPLESS=False),
    # SSE = 1 and SSE = 2 are ONE path in the library (ScreenParams::sse is only ever asked `>= 1`), so no stats word can tell that
    # SSE = 1 arrived; SSE = 0 follows it, which takes the gapless pairing away from pairs of unequal length: ngapless shows it
    S("sse1", SSE=1), S("sse0", SSE=0),
    S("not_vectorized_kdist03", VECTORIZED_ALIGNMENT=False, KDIST_CUTOFF=0.3),
    S("homopolymer_gap", emu=True, HOMOPOLYMER_GAP_PENALTY=-1),
    S("small_scores_band8", MATCH=1, MISMATCH=-2, GAP_PENALTY=-3, BAND_SIZE=8),
    S("max_clust1", emu=True, MAX_CLUST=1), S("max_clust3", emu=True, MAX_CLUST=3), S("max_clust0", MAX_CLUST=0),
    S("detect_singletons", DETECT_SINGLETONS=True),
    S("min_fold_hamming_abundance", MIN_FOLD=2, MIN_HAMMING=2, MIN_ABUNDANCE=2),
    S("omegas", OMEGA_A=1e-4, OMEGA_C=1e-2),
    S("no_quals", emu=True, use_quals=0),
    DEFAULTS,
]


def walk_order(how, small=False):
    """forward; reversed (growing a buffer gets fresh memory, shrinking one keeps a stale tail); one fixed seeded shuffle of the
    steps between the first and the last default run."""
    steps = [s for s in WALK if s.emu] if small else list(WALK)
    if how == "reversed":
        steps = steps[::-1]
    elif how == "shuffled":
        mid = steps[1:-1]
        steps = [steps[0]] + [mid[int(k)] for k in np.random.default_rng(7).permutation(len(mid))] + [steps[-1]]
    else:
        assert how == "forward", how
    return steps


def assert_steps_differ(d, err, steps):
    """From the oracle alone: each step's result differs from the result of the step before it."""
    for a, b in zip(steps, steps[1:]):
        assert results_differ(oracle_run(d, err, a), oracle_run(d, err, b)), ("the oracle gives one result for", a.name, "and", b.name)


def _reached(step, got, default_run):
    """The options that are result-neutral by design, seen arriving in the run's own counters."""
    if step.kw.get("GAPLESS") is False:
        assert got.stats["ngapless"] == 0 < default_run.stats["ngapless"], (step.name, got.stats["ngapless"])
    if step.kw.get("SSE") == 0:
        assert got.stats["ngapless"] < default_run.stats["ngapless"], (step.name, got.stats["ngapless"], default_run.stats["ngapless"])
    if step.kw.get("USE_KMERS") is False:
        assert got.stats["nshroud"] == 0 < default_run.stats["nshroud"], step.name


_FIRST_DEFAULT = {}


def case_option_walk(api, how, small=False):
    d, err = option_sample(small), tperr1()
    steps = walk_order(how, small)
    assert steps[0] is DEFAULTS and steps[-1] is DEFAULTS
    assert_steps_differ(d, err, steps)
    smp = api.Sample.from_derep(d)
    try:
        got = None
        for k, step in enumerate(steps):
            got = smp.run(err, copts=copts_of(step))
            try:
                check_run(got, oracle_run(d, err, step))
            except AssertionError as e:
                raise AssertionError("%s walk, step %d (%s) after %s: %s" % (how, k, step.name, steps[k - 1].name if k else "nothing", e)) from e
            if step is DEFAULTS:
                _FIRST_DEFAULT.setdefault(small, got)
            _reached(step, got, _FIRST_DEFAULT[small])
        assert_same_run(got, _FIRST_DEFAULT[small])
    finally:
        smp.close()
    return len(steps)


# ---- case 1b: the band steps on the aligners that keep a scratch ring --------------------------------------------------------------------
# The rounds of a default run align on k_nw_ad, which keeps nothing between runs; the lane kernels (ensure_scratch: a ring by register
# class and band) and the wide anti-diagonal kernel (ensure_adw_scratch: a ring by band) serve it only for BAND_SIZE = -1 and for
# reads past 2 047 nt.  DADA2HIP_NW_KERNEL sends every round to them, so that the rings are resized between the runs of one handle:
# classes 65, 129, 33, generic, (gapless), generic with a wider band, 65 with other bands, 65.  The launch ledger says that the
# rounds did go there.
BAND_WALK = [DEFAULTS, WALK[1], WALK[2], S("band-1", emu=True, BAND_SIZE=-1), WALK[4],
             # (band 0 pairs gaplessly and leaves the ring alone: the generic lane kernel's ring goes from band -1 to a band that is
             #  wider than it - 2 * 200 + 1 columns against 2 * maxlen + 1 -, the one change of band that no change of class announces)
             S("band200", emu=True, BAND_SIZE=200), WALK[5], S("small_scores_band8", emu=True, MATCH=1, MISMATCH=-2, GAP_PENALTY=-3, BAND_SIZE=8),
             S("band24", emu=True, BAND_SIZE=24), S("band19", BAND_SIZE=19), DEFAULTS]


def case_band_walk(api, kernel, how, small=False):
    d, err = option_sample(small), tperr1()
    steps = [s for s in BAND_WALK if s.emu or not small][:: -1 if how == "reversed" else 1]
    assert_steps_differ(d, err, steps)

    def body():
        import aligner_cases as A
        smp = api.Sample.from_derep(d)
        try:
            runs = []
            A.read_ledger()
            for k, step in enumerate(steps):
                runs.append(smp.run(err, copts=copts_of(step)))
                try:
                    check_run(runs[-1], oracle_run(d, err, step))
                except AssertionError as e:
                    raise AssertionError("%s band walk on %s, step %d (%s) after %s: %s" % (how, kernel, k, step.name, steps[k - 1].name if k else "nothing", e)) from e
            assert_same_run(runs[-1], runs[0])
            ran = A.read_ledger()
            lane_bits, wide_bits = ((1 << 18) - 1) << 72, ((1 << 8) - 1) << 64      # k_nw<WMAX> / k_nw_gen; k_nw_adw (engine.h)
            assert ran & (wide_bits if kernel == "wide" else lane_bits), (kernel, A.describe(ran))
            if kernel == "lane":
                assert ran & A.bit_gen() and sum(1 for w in A.NW_CLASSES if ran & (7 << (72 + 3 * A.NW_CLASSES.index(w)))) >= 3, A.describe(ran)
        finally:
            smp.close()
    with_env({"DADA2HIP_NW_KERNEL": kernel}, body)


# ---- case 2: the err walk ---------------------------------------------------------------------------------------------------------------
def case_err_walk(api, small=False):
    from dada2_amd import _lib
    d, e41 = option_sample(small), tperr1()
    assert e41.shape == (16, 41) and np.nanmax(d.quals) <= 40
    smp = api.Sample.from_derep(d)
    try:
        first = smp.run(e41)
        check_run(first, oracle_run(d, e41))
        e94 = extend_err(e41, 93)                                   # 94 columns: another row stride of the device's copy
        e94[:, 41:] = 1.0                                           # (... whose new columns would show if a stride were mixed up)
        assert e94.shape == (16, 94)
        check_run(smp.run(e94), oracle_run(d, e94))
        e3 = inflate_err(e41, 3)
        assert results_differ(oracle_run(d, e3), oracle_run(d, e41))
        check_run(smp.run(e3), oracle_run(d, e3))
        ones = np.ones((16, 41))                                    # the first pass of selfConsist (R/dada.R:256-405)
        p0 = smp.run(ones, max_clust=1)
        check_run(p0, oracle_run(d, ones, max_clust=1))
        learned = api.noqual_errfun(api.accumulate_trans([p0.subqual]))
        assert learned.shape[1] >= 41 and results_differ(oracle_run(d, learned), oracle_run(d, e41))
        check_run(smp.run(learned), oracle_run(d, learned))
        assert_same_run(smp.run(e41), first)
        # the refusal of test_use_quals_off_still_checks_the_err_range, then a run straight after it
        with_narrow = e41[:, :20]
        assert np.nanmax(d.quals) > 19
        try:
            smp.run(with_narrow)
            raise SystemExit("a 20-column err was accepted")
        except _lib.Dada2HipError as e:
            assert e.code == ERR_RUNTIME and "exceeded range of err lookup table" in str(e), (e.code, str(e))
        check_run(smp.run(e41), oracle_run(d, e41))
    finally:
        smp.close()


# ---- case 3: the priors walk ------------------------------------------------------------------------------------------------------------
def priors_walk(smp, n, run, reference, flags_a, seq_list, or_flags, want_list_flags, flags_b):
    """set_priors, set_priors(zeros), set_prior_seqs, set_priors again on one handle, each followed by a run against the reference
    with the same flags.  ``run()`` is the library's run, ``reference(flags)`` the fresh computation.  Facts, from the reference
    alone: every set of flags changes its result, and the last set gives another result than the sequence list did - so a
    set_priors call that left the list's flags standing would show."""
    zeros = np.zeros(n, dtype=np.uint8)
    plain = reference(zeros)
    for f in (flags_a, want_list_flags, flags_b):
        assert f.any() and results_differ(reference(f), plain)
    assert results_differ(reference(flags_b), reference(want_list_flags)) and results_differ(reference(flags_a), reference(flags_b))
    assert results_differ(reference(flags_b | want_list_flags), reference(flags_b))
    first = run()
    check_run(first, plain)
    smp.set_priors(flags_a)
    check_run(run(), reference(flags_a), check_birth_from=False)
    smp.set_priors(zeros)
    assert_same_run(run(), first)
    nset = smp.set_prior_seqs(seq_list, or_flags=or_flags)
    assert nset == int(want_list_flags.sum()), (nset, int(want_list_flags.sum()))
    check_run(run(), reference(want_list_flags), check_birth_from=False)
    smp.set_priors(flags_b)
    check_run(run(), reference(flags_b), check_birth_from=False)
    smp.set_priors(zeros)
    assert_same_run(run(), first)


def case_priors_walk(api):
    """On pool_cases.match_sample() with MATCH_RUN_OPTS against pool_cases.reference_run (the reference's own dada_uniques)."""
    import pool_cases as pc
    m = pc.match_sample()
    n = len(m["seqs"])
    priors, orf = pc.prior_lists()["mixed_or"]
    want = np.array([s in set(priors) for s in m["seqs"]]) | (orf != 0)
    flags_a = (np.arange(n) % 97 == 5).astype(np.uint8)
    flags_b = (np.arange(n) % 89 == 11).astype(np.uint8)
    dm = Derep(m["seqs"], m["ab"], m["quals"], np.zeros(0, dtype=np.int32))
    loosened = S("match_run_opts", **pc.MATCH_RUN_OPTS)

    def reference(f):
        # the reference's own run; its work counters are not exported (dada.h:113-114), so those are the restatement's
        r = pc.reference_run(np.asarray(f, dtype=np.uint8))
        c = oracle_run(dm, tperr1(), loosened, priors=f)
        return replace(r, stats={k: c.stats[k] for k in ("nalign", "nshroud")})
    smp = api.Sample(m["seqs"], m["ab"], None, m["quals"])
    try:
        priors_walk(smp, n, lambda: smp.run(tperr1(), copts=copts_of(loosened)), reference, flags_a, priors, orf, want.astype(np.uint8), flags_b)
    finally:
        smp.close()


PRIOR_STEP = S("omega_p_loosened", OMEGA_P=0.2)


def case_priors_walk_small(api):
    """The emulator's: the small option sample, a handful of flags, against the oracle."""
    d, err = option_sample(small=True), tperr1()
    n = d.nraw
    flags_a, flags_b, orf = (np.zeros(n, dtype=np.uint8) for _ in range(3))
    flags_a[[20, 47, 77]] = 1
    flags_b[[33, 58, 121]] = 1
    orf[[28]] = 1
    listed = [d.seqs[63], "ACGTN", d.seqs[102], d.seqs[63], d.seqs[3][:-1]]
    want = orf.copy()
    want[[63, 102]] = 1
    smp = api.Sample.from_derep(d)
    try:
        priors_walk(smp, n, lambda: smp.run(err, copts=copts_of(PRIOR_STEP)), lambda f: oracle_run(d, err, PRIOR_STEP, priors=f),
                    flags_a, listed, orf, want, flags_b)
    finally:
        smp.close()


# ---- case 4: compare() between runs -----------------------------------------------------------------------------------------------------
def check_compare(smp, d, centre, err, opts):
    """One b_compare round against the oracle's, unique by unique: class, lambda bits and hamming (tests/aligner_cases.py)."""
    from oracle import cport
    o = opts.normalised()
    lam, ham, cls, st = smp.compare(centre, err, opts)
    L1 = len(d.seqs[centre])
    classes = set()
    for i in range(d.nraw):
        wl, wh, kd, ko = cport.compare(d.seqs[centre], d.quals[centre, :L1], d.seqs[i], d.quals[i, : len(d.seqs[i])], err, opts)
        if kd > o.KDIST_CUTOFF:
            assert wh < 0
            want = (1, 0.0, 0xFFFFFFFF)
        else:
            want = (2 if (o.BAND_SIZE == 0 or (o.GAPLESS and ko == kd)) else 3, wl, wh)
        got = (int(cls[i]), float(lam[i]), int(ham[i]))
        assert got == want, ("centre", centre, "band", o.BAND_SIZE, "unique", i, got, want)
        classes.add(want[0])
    assert classes == {1, 2, 3}, classes                             # shrouded, gapless and aligned pairs: all three were there
    return lam


def case_compare_between_runs(api, small=False):
    d, err = option_sample(small), tperr1()
    k = _SAMPLES[("small" if small else "option") + ":shift20"]       # a centre other than partition 0's: band 16 and band 32 differ on it
    assert k > 0
    b16, b32, b4 = S("band16", BAND_SIZE=16), S("band32", BAND_SIZE=32), S("band4", BAND_SIZE=4)
    assert_steps_differ(d, err, [b16, b4, DEFAULTS])
    smp = api.Sample.from_derep(d)
    try:
        check_run(smp.run(err, copts=copts_of(b16)), oracle_run(d, err, b16))
        l32 = check_compare(smp, d, k, err, DadaOpts(BAND_SIZE=32))
        check_run(smp.run(err, copts=copts_of(b4)), oracle_run(d, err, b4))
        l16 = check_compare(smp, d, k, err, DadaOpts(BAND_SIZE=16))
        assert not np.array_equal(l16, l32)                          # (the two compares were two different questions)
        check_run(smp.run(err), oracle_run(d, err))
    finally:
        smp.close()


# ---- case 5: abort, then a run on the same handle ---------------------------------------------------------------------------------------
def _sam1F():
    if "sam1F" not in _SAMPLES:
        d, err, pri, o, exp, meta = case_inputs("sam1F_default")
        assert pri is None and o == DadaOpts()
        _SAMPLES["sam1F"] = (d, err, exp)
    return _SAMPLES["sam1F"]


def case_abort_then_run(api, env, polls_at=(1, 3, 8)):
    from dada2_amd import _lib
    d, err, golden = _sam1F()
    b32 = S("band32", BAND_SIZE=32)

    def body():
        smp = api.Sample.from_derep(d)
        try:
            for k in polls_at:
                polls = []

                def stop():
                    polls.append(1)
                    return len(polls) >= k
                try:
                    smp.run(err, should_abort=stop)
                    raise SystemExit("the run was not aborted")
                except _lib.Dada2HipError as e:
                    assert e.code == ERR_ABORTED and "aborted" in str(e), (e.code, str(e))
                assert len(polls) == k, (len(polls), k)
                check_run(smp.run(err, copts=copts_of(b32)), oracle_run(d, err, b32))      # the aborted handle, other options
                got = smp.run(err)
                assert_results_equal(got, golden)
                check_run(got, oracle_run(d, err))
        finally:
            smp.close()
    with_env(env, body)


# ---- case 6: the device-raised error, then a run on the same handle -----------------------------------------------------------------------
BAD_LAMBDA = "Bad lambda."                                          # pval.cpp:138, :194
Q_ALL, Q_STAR, P_STAR = 30, 3, 31
A2A, C2C = 0, 5                                                     # rows of err: 4 * from + to


def error_sample():
    """Two true variants of 60 nt and their one-substitution families.  V0 (400 reads) has A at P_STAR, V1 (150 reads; five more
    substitutions elsewhere) has C there; every quality is Q_ALL, but the V1 family carries Q_STAR at P_STAR - and nobody else
    carries Q_STAR anywhere.  So err[C2C, Q_STAR] is read only when a V1-family read meets a centre with C at P_STAR: V1 itself,
    never V0 (against V0 that position looks up A2C)."""
    if "error" not in _SAMPLES:
        rng = np.random.default_rng(60)
        v0 = list(_rand(rng, 60))
        v0[P_STAR] = "A"
        v1 = list(v0)
        v1[P_STAR] = "C"
        for p in (3, 14, 27, 44, 55):
            v1[p] = "ACGT"[("ACGT".index(v1[p]) + 1 + int(rng.integers(0, 3))) & 3]
        v0, v1 = "".join(v0), "".join(v1)

        def family(v, m):
            out = []
            while len(out) < m:
                p = int(rng.integers(0, 60))
                if p == P_STAR or p in (3, 14, 27, 44, 55):
                    continue
                s = v[:p] + "ACGT"[("ACGT".index(v[p]) + 1 + int(rng.integers(0, 3))) & 3] + v[p + 1:]
                if s not in out:
                    out.append(s)
            return out
        f0, f1 = family(v0, 14), family(v1, 9)
        seqs = [v0, v1] + f0 + f1
        ab = [400, 150] + [int(x) for x in rng.integers(1, 4, size=len(f0) + len(f1))]
        q = np.full((len(seqs), 60), float(Q_ALL))
        for i in [1] + list(range(2 + len(f0), len(seqs))):
            q[i, P_STAR] = float(Q_STAR)
        order = np.argsort(-np.asarray(ab), kind="stable")
        _SAMPLES["error"] = (Derep([seqs[int(k)] for k in order], np.asarray(ab, dtype=np.int32)[order], q[order], np.zeros(0, dtype=np.int32)), v1)
    return _SAMPLES["error"]


def error_inputs():
    """name -> err: 'round0' fails in the first compare (a self-transition above 1 at the quality every base has), 'later_round' only
    once V1 is a centre.  The facts, from the oracle alone."""
    d, v1 = error_sample()
    good = tperr1()
    r0, later = good.copy(), good.copy()
    r0[A2A, Q_ALL] = 1.5
    later[C2C, Q_STAR] = 4.0
    assert d.seqs[0].count("A") >= 5 and 0 < good[1, Q_STAR] < 1
    for e in (r0, later):
        try:
            oracle_run(d, e)
            raise SystemExit("the oracle accepted an err entry above 1")
        except RuntimeError as ex:
            assert str(ex) == BAD_LAMBDA, str(ex)
    try:
        oracle_run(d, r0, max_clust=1)
        raise SystemExit("the oracle's round 0 accepted a self-transition above 1")
    except RuntimeError as ex:
        assert str(ex) == BAD_LAMBDA, str(ex)
    assert oracle_run(d, later, max_clust=1).nclust == 1            # round 0 is in range: the failure is a later round's
    want = oracle_run(d, good)
    assert want.nclust == 2 and want.clustering["sequence"][1] == v1   # V1 is born as partition 2
    return {"round0": r0, "later_round": later}


def case_device_error_then_run(api, env, which=("round0", "later_round")):
    from dada2_amd import _lib
    d, _ = error_sample()
    errs = error_inputs()
    good = tperr1()

    def body():
        smp = api.Sample.from_derep(d)
        try:
            for name in which:
                try:
                    smp.run(errs[name])
                    raise SystemExit("no error from " + name)
                except _lib.Dada2HipError as e:
                    assert e.code == ERR_RUNTIME and str(e) == BAD_LAMBDA, (name, e.code, str(e))
                got = smp.run(good)                                  # the handle that failed
                check_run(got, oracle_run(d, good))
                if name == "later_round" and "DADA2HIP_ENGINE" not in env:
                    assert got.stats["batch_compares"] > 0           # (the engine whose batch-compare site had fired)
        finally:
            smp.close()
    with_env(env, body)


# ---- case 7: neighbours in the process ----------------------------------------------------------------------------------------------------
def case_two_samples_interleaved(api):
    da, err = option_sample(), tperr1()
    db, eb, _ = _sam1F()
    sa, sb = api.Sample.from_derep(da), api.Sample.from_derep(db)
    a_steps = [S("band32", BAND_SIZE=32), S("no_kmers", USE_KMERS=False), S("band4", BAND_SIZE=4)]
    b_steps = [S("homopolymer_gap", HOMOPOLYMER_GAP_PENALTY=-1), S("band-1", BAND_SIZE=-1), DEFAULTS]
    try:
        for x, y in zip(a_steps, b_steps):
            check_run(sa.run(err, copts=copts_of(x)), oracle_run(da, err, x))
            check_run(sb.run(eb, copts=copts_of(y)), oracle_run(db, eb, y))
    finally:
        sa.close()
        sb.close()


def case_memory_handed_on(api, trim):
    """A sample run with BAND_SIZE = -1 (the largest buffers it can ask for) is closed; what it frees goes to the allocation cache
    (or, ``trim``, back to the device through dada2hip_trim_cache) and the next, smaller sample is built from it."""
    from dada2_amd import _lib
    big, small, err = option_sample(), other_sample(), tperr1()
    full = S("band-1", BAND_SIZE=-1)
    smp = api.Sample.from_derep(big)
    try:
        check_run(smp.run(err, copts=copts_of(full)), oracle_run(big, err, full))
    finally:
        smp.close()
    if trim:
        _lib.lib().dada2hip_trim_cache()
    smp = api.Sample.from_derep(small)
    try:
        check_run(smp.run(err), oracle_run(small, err))
    finally:
        smp.close()


# ---- the emulator's job (tests/test_emu_resident.py) ------------------------------------------------------------------------------------
def emu_run():
    import time
    from dada2_amd import api
    t0 = time.time()
    laps = []

    def lap(name):
        laps.append("%s %.0fs" % (name, time.time() - t0))
    n = case_option_walk(api, "forward", small=True)
    case_option_walk(api, "reversed", small=True)
    lap("walks(%d steps)" % n)
    for kernel in ("lane", "wide"):
        for how in ("forward", "reversed"):
            case_band_walk(api, kernel, how, small=True)
    lap("band walks")
    case_err_walk(api, small=True)
    lap("err")
    case_priors_walk_small(api)
    lap("priors")
    case_compare_between_runs(api, small=True)
    lap("compare")
    case_abort_then_run(api, {}, polls_at=(3,))
    lap("abort")
    for env in ({}, {"DADA2HIP_V2_TAIL": "chain"}):
        case_device_error_then_run(api, env)
    lap("device error")
    return "ok " + ", ".join(laps)
