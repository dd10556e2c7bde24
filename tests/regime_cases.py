"""Seeded samples for three regimes the generator of the other sweeps (dada2_amd.synth.make_sample) never reaches, each with
branches of its own in the round kernels:

crowd  more than 1 024 partitions: the per-partition LDS tables of the round tail (DELTA_TAB / PUPD_TAB = 1 024 entries,
       rounds_common.h) overflow into their global-memory arms, and the per-cluster device arrays grow 1 024 -> 2 048.
tied   long lists of EXACTLY tied bud candidates (p = 0, equal reads): past the 64 records published inline (BUD_TIES), past
       the 4 096 full records the device keeps (TIES_FULL: the host then rebuilds the records from the index list).
deep   abundances of real magnitude (top unique 2^16 + 1 ... 3e8 reads, total <= 2^31 - 1): E = lambda * reads leaves the
       small-x arm of pgamma_lower (csrc/ppois.h) inside a whole run, candidates sit right at OMEGA_A, and at the top of R's
       integer range $subqual and the 32-bit q * reads product of $clusterquals wrap as the reference's do.

Pure Python on numpy; reads nothing outside tests/.  Every builder returns (Derep, priors, DadaOpts, facts): `facts` is a dict
of named checks - callables taking (oracle module, oracle result) - that hold for the sample by construction and
are computed from the sample or from the ORACLE alone, never from the library under test.  A test asserts them (check_facts)
before it trusts a comparison: if a sample stops reaching its branch, the test fails instead of passing vacuously."""
import numpy as np

from helpers import tperr1
from dada2_amd.io import Derep
from dada2_amd.opts import DadaOpts

TAB = 1024            # DELTA_TAB = PUPD_TAB (dada2_amd/csrc/rounds_common.h)
BUD_TIES = 64         # dada2_amd/csrc/engine.h
TIES_FULL = 4096
INT_MAX = 2 ** 31 - 1


def _rnd(rng, L):
    return "".join("ACGT"[int(x)] for x in rng.integers(0, 4, size=L))


def _mut(rng, s, nsub):
    s = list(s)
    for p in rng.choice(len(s), size=nsub, replace=False):
        s[p] = "ACGT"[("ACGT".index(s[p]) + int(rng.integers(1, 4))) & 3]
    return "".join(s)


def _derep(seqs, ab, quals, first_seen=None):
    """Abundance order the way derepFastq leaves it (R/sequenceIO.R:98: decreasing reads, ties in order of first appearance)."""
    first_seen = np.arange(len(seqs)) if first_seen is None else first_seen
    order = np.lexsort((first_seen, -np.asarray(ab, dtype=np.int64)))
    return Derep([seqs[i] for i in order], np.asarray(ab, dtype=np.int32)[order], np.asarray(quals, dtype=np.float64)[order],
                 np.zeros(0, dtype=np.int32)), order


# ---- crowd ---------------------------------------------------------------------------------------------------------------
def crowd(seed, G, L, nerr, greedy=True, priors=False, nsubvar=8):
    """G unrelated true variants with DISTINCT read counts (300 ... 300 + 3 G, so the births come in decreasing-reads order:
    each is shrouded against every centre before its own, lambda = 0, p = 0), each with `nerr` single-substitution neighbours of
    1-3 reads that sit in partition 0 until their variant is born and then move to it - for the variants born after the
    1 024th into a partition past the LDS tables.  `nsubvar` of the variants born last (the fewest reads) also have a
    sub-variant three substitutions away (40 ... reads, two neighbours of its own): it and its neighbours first move INTO their
    variant's partition, past the tables, and OUT of it again when the sub-variant is born from there at the end of the run -
    reads subtracted from a partition past the tables, a birth out of one."""
    assert G > 1100
    rng = np.random.default_rng(seed)
    seqs, ab, seen = [], [], set()
    reads = 300 + 3 * rng.permutation(G) + rng.integers(0, 3, size=G)      # distinct: 3 k + {0, 1, 2}
    for g in range(G):
        v = _rnd(rng, L)
        while v in seen:
            v = _rnd(rng, L)
        seen.add(v); seqs.append(v); ab.append(int(reads[g]))
        for _ in range(nerr):
            e = _mut(rng, v, 1)
            if e not in seen:
                seen.add(e); seqs.append(e); ab.append(int(rng.integers(1, 4)))
    last = np.argsort(reads)[:nsubvar]               # (born last: at index G - 1, G - 2, ...)
    vseq = [s for s, a in zip(seqs, ab) if a >= 300]
    for j, g in enumerate(last):
        sv = _mut(rng, vseq[g], 3)
        seen.add(sv); seqs.append(sv); ab.append(40 + j)
        for _ in range(2):
            e = _mut(rng, sv, 1)
            if e not in seen:
                seen.add(e); seqs.append(e); ab.append(int(rng.integers(1, 3)))
    quals = rng.integers(25, 41, size=(len(seqs), L)).astype(np.float64)
    d, _ = _derep(seqs, ab, quals, first_seen=rng.permutation(len(seqs)))
    pri = (np.arange(d.nraw) % 17 == 3).astype(np.uint8) if priors else None
    opts = DadaOpts(GREEDY=greedy)

    def more_than_1024_partitions(oracle, res):
        return res.nclust > TAB

    def a_mover_joined_a_table_overflow_partition(oracle, res):
        return bool((res.clustering["nunq"][TAB + 1:] > 1).any())         # (0-based index > 1 024 = 1-based index > 1 025)

    def a_unique_left_partition_0_for_an_overflow_partition(oracle, res):
        cen = set(res.stats["center"].tolist())
        moved = [i for i in np.nonzero(res.map - 1 >= TAB)[0] if i not in cen]
        return len(moved) > 0 and int(res.clustering["abundance"][0]) < int(d.abundances.sum())

    def a_partition_was_born_out_of_an_overflow_partition_and_took_members_along(oracle, res):
        frm, nunq = res.clustering["birth_from"], res.clustering["nunq"]           # (birth_from is 1-based)
        return any(frm[c] - 1 >= TAB and nunq[c] > 1 for c in range(TAB, res.nclust)) and (nsubvar == 0 or res.nclust >= G + nsubvar)

    facts = dict(more_than_1024_partitions=more_than_1024_partitions,
                 a_partition_was_born_out_of_an_overflow_partition_and_took_members_along=a_partition_was_born_out_of_an_overflow_partition_and_took_members_along,
                 a_mover_joined_a_table_overflow_partition=a_mover_joined_a_table_overflow_partition,
                 a_unique_left_partition_0_for_an_overflow_partition=a_unique_left_partition_0_for_an_overflow_partition)
    return d, pri, opts, facts


# ---- tied ----------------------------------------------------------------------------------------------------------------
def tied(seed, K, L=200, max_clust=24, K3=0, movers=False, permuted=False):
    """One true variant with a family of point errors (3-6 reads each, five singletons) plus K unrelated random reads of 2 reads
    each (and K3 more of 3 reads: a second tie group that is exhausted first).  The first centre is compared with every unique
    WITHOUT the k-mer screen (Rmain.cpp:309-310 passes a cutoff of 1), so a junk read does get a lambda - of some sixty
    mismatches at quality 38-40, below 1e-170: E = lambda * reads is so small that calc_pA (about E^2 / 2) underflows to EXACTLY 0; against every
    later centre it is shrouded and keeps that comparison.  So b_bud sees K3 (then K) candidates of one key, (p = 0, reads), and
    keeps the first in (partition, slot) scan order (cluster.cpp:284-308) - and bi_pop_raw fills the vacated slot with the
    partition's LAST member (containers.cpp:187),
    so that order is not the index order: once the five singletons at the end have been used up, the junk read at the end of the
    list is born next.  movers: the first junk reads get a singleton neighbour each, which moves behind them when they are
    born (the scan order then depends on the shuffle's pops as well, and the exact birth order is left to the oracle).
    permuted: the uniques in REVERSE order - slot 0 of partition 0 is not its centre, which puts the run in plain mode."""
    rng = np.random.default_rng(seed)
    centre = _rnd(rng, L)
    seqs, ab, seen = [centre], [3000], {centre}
    for k in range(45):
        e = _mut(rng, centre, int(rng.integers(1, 3)))
        if e not in seen:
            seen.add(e); seqs.append(e); ab.append(1 if k < 5 else int(rng.integers(3, 7)))
    junk = []
    for k in range(K3 + K):
        j = _rnd(rng, L)
        while j in seen:
            j = _rnd(rng, L)
        seen.add(j); junk.append(j); seqs.append(j); ab.append(3 if k < K3 else 2)
    if movers:
        for j in junk[:12]:
            e = _mut(rng, j, 1)
            if e not in seen:
                seen.add(e); seqs.append(e); ab.append(1)
    quals = rng.integers(25, 41, size=(len(seqs), L)).astype(np.float64)
    j0 = seqs.index(junk[0])
    quals[j0:j0 + K3 + K] = rng.integers(38, 41, size=(K3 + K, L))
    if K3:                                           # (family members of 3 reads would sit between the groups: keep the groups clean)
        ab = [4 if (a == 3 and s not in set(junk)) else a for s, a in zip(seqs, ab)]
    d, _ = _derep(seqs, ab, quals)
    if permuted:
        d = Derep(d.seqs[::-1], d.abundances[::-1].copy(), d.quals[::-1].copy(), np.zeros(0, dtype=np.int32))
    opts = DadaOpts(MAX_CLUST=max_clust)
    isjunk = np.array([s in set(junk) for s in d.seqs])
    c0 = int(np.argmax(d.abundances))                # bi_assign_center: the first of the most abundant

    def every_junk_read_has_p_exactly_0_against_centre_0(oracle, res):
        """... from the oracle's compare without the screen and its calc_pA with what partition 0 holds in round 1; with the
        screen (every later centre) the same pair is shrouded."""
        err, tot = tperr1(), int(d.abundances.sum())
        for i in np.nonzero(isjunk)[0]:
            lam, ham, kd, ko = oracle.compare(d.seqs[c0], d.quals[c0], d.seqs[i], d.quals[i], err, opts, kdist_cutoff=1.0)
            # (get_pA, pval.cpp:67-89: a lambda that has itself underflowed to 0 gives p = 0 without calc_pA)
            if not (0.0 <= lam < 1e-170 and ham > 40 and (lam == 0.0 or oracle.calc_pA(int(d.abundances[i]), lam * tot, False) == 0.0)):
                return False
            if i % 64 == 0 and oracle.compare(d.seqs[c0], d.quals[c0], d.seqs[i], d.quals[i], err, opts)[:2] != (0.0, -1):
                return False
        return int(isjunk.sum()) == K + K3

    def births_follow_the_scan_order_with_swap_with_last(oracle, res):
        """b_bud + bi_pop_raw replayed on partition 0's member list (nothing ever moves in these samples: a junk read is
        shrouded against everything).  Group by group (3 reads before 2), the first listed junk read wins."""
        lst = list(range(d.nraw))
        want = []
        while len(want) < max_clust - 1:
            best = None
            for r in range(1, len(lst)):             # (slot 0 is skipped as "the centre", cluster.cpp:285)
                if isjunk[lst[r]] and (best is None or d.abundances[lst[r]] > d.abundances[lst[best]]):
                    best = r
            if best is None:
                break
            want.append(lst[best])
            lst[best] = lst[-1]
            lst.pop()
        return res.stats["center"].tolist()[1:] == want and len(want) == min(max_clust - 1, K + K3)

    def births_are_junk_reads_with_p_0(oracle, res):
        cen = res.stats["center"].tolist()[1:]
        return (len(cen) == max_clust - 1 and all(isjunk[c] for c in cen) and (res.clustering["birth_pval"][1:] == 0.0).all()
                and sorted((-d.abundances[c] for c in cen)) == [-d.abundances[c] for c in cen]
                and int((d.abundances[cen] == 3).sum()) == min(K3, max_clust - 1))

    def tie_list_lengths(oracle, res):
        """The lengths of the tie list over the run's rounds reach the tier the case is for."""
        n3 = min(K3, max_clust - 1)
        lens = [K3 - k for k in range(n3)] + [K - k for k in range(max_clust - 1 - n3)]
        facts["tie_lens"] = lens
        return max(lens) == max(K, K3) and sum(n >= 2 for n in lens) >= len(lens) - 1

    facts = dict(every_junk_read_has_p_exactly_0_against_centre_0=every_junk_read_has_p_exactly_0_against_centre_0,
                 births_are_junk_reads_with_p_0=births_are_junk_reads_with_p_0, tie_list_lengths=tie_list_lengths)
    if not movers:
        facts["births_follow_the_scan_order_with_swap_with_last"] = births_follow_the_scan_order_with_swap_with_last
    return d, None, opts, facts


# ---- deep ----------------------------------------------------------------------------------------------------------------
def pgamma_arm(E, reads):
    """Which arm of pgamma_lower(x = E, alph = reads) (dada2_amd/csrc/ppois.h) a candidate takes: 1 pgamma_smallx_lower,
    2 pd_upper_series, 3 pd_lower_series, 4 ppois_asymp; 0 = none (x <= 0)."""
    x, alph = float(E), float(reads)
    if x <= 0.0:
        return 0
    if x < 1:
        return 1
    if x <= alph - 1 and x < 0.8 * (alph + 50):
        return 2
    if alph - 1 < x and alph < 0.8 * (x + 50):
        return 3
    return 4


def _threshold_reads(oracle, E, n, omega, prior=False):
    """Smallest reads with calc_pA(reads, E) * n < omega (calc_pA falls with reads)."""
    lo, hi = 1, 2
    while oracle.calc_pA(hi, E, prior) * n >= omega:
        lo, hi = hi, hi * 2
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if oracle.calc_pA(mid, E, prior) * n < omega:
            hi = mid
        else:
            lo = mid
    return hi


DEEP_TOPS = {"2p16": 2 ** 16 + 1, "2p24": 2 ** 24 + 1, "3e8": 320_000_000}


def deep(seed, top, L=80, nfam=6, nnb=36, priors=False, **optkw):
    """`nfam` unrelated true variants of top, 0.85 top, 0.7 top ... reads, each with neighbours (`nnb` for the first, a third of
    that for the others) at one to three substitutions whose qualities at the substituted positions range from 22 to 40 (lambda
    from 1e-2 down to 1e-13).  A neighbour's reads are NOT a fixed fraction of its parent's: they are E * m with m drawn from
    0.3 ... 3 (or 0.9 ... 1.1) around E = lambda * parent reads - for the first variant's neighbours the reads of the whole
    sample, which is what partition 0 holds in round 1 -, or the count at which calc_pA * N crosses OMEGA_A, give or take a few
    reads: candidates fall on both sides of the expectation and of the threshold, and with E from < 1 to > 1e6 into every arm of
    pgamma_lower.  lambda comes from the oracle's own compare."""
    from oracle import cport as oracle
    rng = np.random.default_rng(seed)
    err = tperr1()
    opts = DadaOpts(**optkw)
    fam = [_rnd(rng, L) for _ in range(nfam)]
    fq = rng.integers(30, 41, size=(nfam, L)).astype(np.float64)
    fam_reads = [int(top * (1 - 0.15 * g)) - g for g in range(nfam)]
    seqs, quals, parent, kind, mult, seen = list(fam), [q for q in fq], [-1] * nfam, [None] * nfam, [0.0] * nfam, set(fam)
    for g in range(nfam):
        for k in range(nnb if g == 0 else nnb // 3):
            nsub = (1, 1, 1, 2, 2, 3)[k % 6]
            e = _mut(rng, fam[g], nsub)
            if e in seen:
                continue
            seen.add(e)
            q = rng.integers(30, 41, size=L).astype(np.float64)
            for p in [p for p in range(L) if e[p] != fam[g][p]]:
                q[p] = float(rng.choice([22, 27, 31, 34, 37, 40]))
            seqs.append(e); quals.append(q); parent.append(g)
            kind.append(("around_E", "threshold", "close_to_E", "threshold")[k % 4])
            mult.append(float(np.exp(rng.uniform(np.log(0.3), np.log(3.0)))) if k % 4 == 0 else float(rng.uniform(0.9, 1.1)))
    off = rng.integers(-3, 4, size=len(seqs))
    lam = [0.0] * len(seqs)
    for i in range(nfam, len(seqs)):
        g = parent[i]
        lam[i] = oracle.compare(fam[g], fq[g], seqs[i], quals[i], err, opts)[0]
        assert lam[i] > 0, (i, g)
    N = len(seqs)
    total = sum(fam_reads) * 1.05
    for _ in range(6):                               # E depends on the total, the total on the neighbours' reads: a few turns settle it
        ab = list(fam_reads) + [0] * (N - nfam)
        for i in range(nfam, N):
            E = lam[i] * (total if parent[i] == 0 else fam_reads[parent[i]])   # (round 1: everything is still in partition 0)
            if kind[i] != "threshold":
                ab[i] = max(1, int(round(E * mult[i])))
            else:
                ab[i] = max(1, _threshold_reads(oracle, E, N, opts.OMEGA_A) + int(off[i]))
        total = float(sum(ab))
    assert sum(ab) <= INT_MAX, sum(ab)
    d, _ = _derep(seqs, ab, np.array(quals))
    pri = None
    if priors:
        pri = (np.arange(d.nraw) % 5 == 2).astype(np.uint8)
    c0 = 0
    tot = int(d.abundances.astype(np.int64).sum())

    def _round1():
        """(reads, E = lambda * reads of partition 0) of every unique the first centre's compare gave a lambda > 0."""
        if "round1" not in facts:
            rows = []
            for i in range(1, d.nraw):
                lm = oracle.compare(d.seqs[c0], d.quals[c0], d.seqs[i], d.quals[i], err, opts)[0]
                if lm > 0:
                    rows.append((int(d.abundances[i]), lm * tot))
            facts["round1"] = rows
        return facts["round1"]

    def round_1_reaches_every_arm_of_pgamma_lower(orc, res):
        arms = {pgamma_arm(E, r) for r, E in _round1()}
        facts["arms"] = sorted(arms)
        return arms >= {1, 2, 3, 4}

    def candidates_within_a_factor_10_of_omega_a_on_each_side(orc, res):
        pa = np.array([orc.calc_pA(r, E, False) * d.nraw for r, E in _round1()])
        below = ((pa < opts.OMEGA_A) & (pa >= opts.OMEGA_A / 10)).sum()
        above = ((pa >= opts.OMEGA_A) & (pa <= opts.OMEGA_A * 10)).sum()
        facts["near_omega_a"] = (int(below), int(above))
        return below >= 1 and above >= 1

    def reads_on_both_sides_of_the_expectation(orc, res):
        r1 = _round1()
        return sum(r > E for r, E in r1) >= 3 and sum(r < E for r, E in r1) >= 3

    def total_reads_fit_an_r_integer(orc, res):
        return tot <= INT_MAX and int(d.abundances.max()) >= top * 0.99

    def subqual_and_the_q_times_reads_product_wrap(orc, res):
        qmax = int(np.rint(np.nanmax(d.quals[0])))
        return bool((res.subqual < 0).any()) and qmax * int(d.abundances[0]) > 2 ** 32

    facts = dict(round_1_reaches_every_arm_of_pgamma_lower=round_1_reaches_every_arm_of_pgamma_lower,
                 candidates_within_a_factor_10_of_omega_a_on_each_side=candidates_within_a_factor_10_of_omega_a_on_each_side,
                 reads_on_both_sides_of_the_expectation=reads_on_both_sides_of_the_expectation,
                 total_reads_fit_an_r_integer=total_reads_fit_an_r_integer)
    if top >= 2 ** 28:
        facts["subqual_and_the_q_times_reads_product_wrap"] = subqual_and_the_q_times_reads_product_wrap
    return d, pri, opts, facts


# ---- the table -----------------------------------------------------------------------------------------------------------
# name -> (builder, keywords).  GPU_ONLY cases are too slow for the emulator; EMU_CASES are the ones tests/test_emu.py must keep.
CASES = {
    "crowd_small": (crowd, dict(seed=11, G=1104, L=60, nerr=1)),
    "crowd_small_nogreedy": (crowd, dict(seed=12, G=1104, L=60, nerr=1, greedy=False)),
    "crowd_small_priors": (crowd, dict(seed=13, G=1104, L=60, nerr=1, priors=True)),
    "crowd_large": (crowd, dict(seed=14, G=1300, L=100, nerr=6)),
    "tied_65": (tied, dict(seed=21, K=65)),
    "tied_300": (tied, dict(seed=22, K=300, max_clust=40)),
    "tied_4096": (tied, dict(seed=23, K=4096)),
    "tied_4100": (tied, dict(seed=24, K=4100)),
    "tied_4200": (tied, dict(seed=25, K=4200)),
    # (in what order the device lists tied candidates is up to its atomics; under the emulator, whose order is fixed, this is the
    #  size at which the first-born candidate is listed past the 4 096th place: a list cut short there loses it)
    "tied_5000": (tied, dict(seed=25, K=5000, max_clust=8)),
    "tied_two_groups_movers": (tied, dict(seed=26, K=300, K3=10, max_clust=30, movers=True)),
    "tied_4200_permuted": (tied, dict(seed=27, K=4200, permuted=True)),
    "tied_300_permuted": (tied, dict(seed=28, K=300, max_clust=40, permuted=True)),
    "deep_2p16": (deep, dict(seed=31, top=DEEP_TOPS["2p16"])),
    "deep_2p24": (deep, dict(seed=32, top=DEEP_TOPS["2p24"])),
    "deep_3e8": (deep, dict(seed=33, top=DEEP_TOPS["3e8"])),
    "deep_2p24_minfold_minabund": (deep, dict(seed=34, top=DEEP_TOPS["2p24"], MIN_FOLD=2, MIN_ABUNDANCE=40)),
    "deep_2p16_singletons": (deep, dict(seed=35, top=DEEP_TOPS["2p16"], DETECT_SINGLETONS=True)),
    "deep_3e8_priors_omega_p": (deep, dict(seed=36, top=DEEP_TOPS["3e8"], priors=True, OMEGA_P=1e-20)),
}
GPU_ONLY = ("crowd_large",)
EMU_CASES = ("crowd_small", "tied_65", "tied_300", "tied_4200", "tied_5000", "deep_3e8")

_BUILT, _ORACLE = {}, {}


def build(name):
    """(Derep, priors, DadaOpts, facts) of a case, built once per process."""
    if name not in _BUILT:
        fn, kw = CASES[name]
        _BUILT[name] = fn(**kw)
    return _BUILT[name]


def oracle_result(name, oracle=None, multithread=False):
    """The oracle's result of a case, computed once per process and checker (it does not depend on the engine under test, and
    on these samples the oracle is the slow side)."""
    if oracle is None:
        from oracle import cport as oracle
    key = (name, oracle.__name__, multithread)
    if key not in _ORACLE:
        d, pri, opts, _ = build(name)
        _ORACLE[key] = oracle.dada_uniques(d.seqs, d.abundances, pri, tperr1(), d.quals, opts, multithread=multithread)
    return _ORACLE[key]


def check_facts(name, res=None):
    """Assert every fact of a case on the oracle's result; returns that result."""
    from oracle import cport
    d, pri, opts, facts = build(name)
    res = oracle_result(name) if res is None else res
    for key, fn in list(facts.items()):
        if callable(fn):
            assert fn(cport, res), (name, key, {k: v for k, v in facts.items() if not callable(v) and k != "round1"})
    return res
