"""Pooled and pseudo-pooled dada() (R/dada.R:185-196, :391-404, :443-475; combineDereps2, R/multiSample.R:165-203): restatements in
plain numpy, written from the R semantics, and the cases the library is held to.  tests/test_pool.py runs the host parts on the
CPU; tests/test_emu_pool.py and tests/test_gpu_pool.py run the device parts, identically, under the emulator and on the device.

Everything is compared bit for bit (helpers.assert_results_equal, helpers._same_float(..., 0)); the p-value columns get
helpers.P_RTOL.  The denoising core of every restated run is oracle.ref.dada_uniques, the reference's own C++.  One column is left
out where priors are in play, as everywhere in this suite (helpers.assert_results_equal, check_birth_from): the reference never
sets ``birth_from`` for a prior-driven birth ("Reference quirks to preserve": cluster.cpp:331-345), so what it returns
there is whatever the memory held."""
import os
from fractions import Fraction

import numpy as np

from dada2_amd.io import Derep, extend_err
from dada2_amd.opts import DadaOpts, DadaResult, NA_INTEGER
from helpers import GOLDEN, _same_float, assert_results_equal, load_input, tperr1
from species_cases import with_env


# ---- combineDereps2 -------------------------------------------------------------------------------------------------------------------
def restate_combine(dereps):
    """(Derep, [unique_to_pool per sample]) as combineDereps2 builds them.  Maps: -1 = NA."""
    maxlen = max(d.quals.shape[1] for d in dereps)
    pos = {}
    for d in dereps:                                              # unique(do.call(c, lapply(dereps, getSequences)))
        assert len(set(d.seqs)) == len(d.seqs)
        for s in d.seqs:
            pos.setdefault(s, len(pos))
    counts = np.zeros(len(pos), dtype=np.int64)
    acc = np.zeros((len(pos), maxlen), dtype=np.float64)
    maps, u2p = [], []
    for d in dereps:
        q = np.asarray(d.quals, dtype=np.float64)
        if q.shape[1] < maxlen:                                   # cbind(derep$quals, matrix(NA, ...)), :184
            q = np.concatenate([q, np.full((q.shape[0], maxlen - q.shape[1]), np.nan)], axis=1)
        idx = np.array([pos[s] for s in d.seqs], dtype=np.int64)
        counts[idx] += np.asarray(d.abundances, dtype=np.int64)
        prod = q * np.asarray(d.abundances, dtype=np.float64)[:, None]   # sweep(derep$quals, 1, derep$uniques, "*")
        acc[idx] = acc[idx] + prod                                # two roundings: a product, then a sum
        m = np.asarray(d.map, dtype=np.int64)
        maps.append(np.where(m < 0, -1, idx[np.where(m < 0, 0, m)]) if m.size else np.zeros(0, dtype=np.int64))
        u2p.append(idx)
    assert counts.max() <= np.iinfo(np.int32).max
    acc = acc / counts.astype(np.float64)[:, None]                # sweep(derepQuals, 1, derepCounts, "/")
    order = np.argsort(-counts, kind="stable")                    # order(derepCounts, decreasing = TRUE)
    rank = np.empty(len(order), dtype=np.int64)
    rank[order] = np.arange(len(order))
    seqs = list(pos)
    allmap = np.concatenate(maps) if maps else np.zeros(0, dtype=np.int64)
    allmap = np.where(allmap < 0, -1, rank[np.where(allmap < 0, 0, allmap)]).astype(np.int32)
    return (Derep([seqs[int(k)] for k in order], counts[order].astype(np.int32), acc[order], allmap),
            [rank[u].astype(np.int32) for u in u2p])


def fused_quals(dereps):
    """restate_combine's qualities with every acc + q * c rounded ONCE (a fused multiply-add, through exact rationals), in the
    restatement's row order: what a contracted build of the library's loop would give."""
    pooled, u2p = restate_combine(dereps)
    out = np.full(pooled.quals.shape, np.nan)
    for k, s in enumerate(pooled.seqs):
        for p in range(len(s)):
            acc = 0.0
            for d, u in zip(dereps, u2p):
                j = np.flatnonzero(u == k)
                if j.size:
                    acc = float(Fraction(float(d.quals[j[0], p])) * int(d.abundances[j[0]]) + Fraction(acc))
            out[k, p] = acc / float(pooled.abundances[k])
    return out


def assert_derep_equal(got: Derep, want: Derep):
    assert got.seqs == want.seqs
    assert np.array_equal(got.abundances, want.abundances)
    _same_float(got.quals, want.quals, 0)
    assert np.array_equal(np.asarray(got.map), np.asarray(want.map))


def check_combine(api, dereps, inputs=None):
    """The library's combine of ``inputs`` (default: ``dereps``, which are numpy Dereps holding the same content) equals the restatement."""
    got, gu = api.combine_dereps(dereps if inputs is None else inputs)
    want, wu = restate_combine(dereps)
    assert_derep_equal(got, want)
    assert len(gu) == len(wu) and all(np.array_equal(a, b) for a, b in zip(gu, wu))
    return got, gu


def golden_derep(api, name):
    """A golden sample dereplicated by the library from its FASTQ file: a Derep with its map."""
    return api.derep_fastq(os.path.join(GOLDEN, name + ".fastq.gz"))


def subset_derep(d: Derep, rows):
    """The uniques ``rows`` of d, in that order; reads of the others are NA in the map."""
    rows = np.asarray(rows, dtype=np.int64)
    to = np.full(d.nraw, -1, dtype=np.int64)
    to[rows] = np.arange(rows.size)
    m = np.asarray(d.map, dtype=np.int64)
    return Derep([d.seqs[int(r)] for r in rows], np.asarray(d.abundances)[rows].copy(), np.asarray(d.quals)[rows].copy(),
                 np.where(m < 0, -1, to[np.where(m < 0, 0, m)]).astype(np.int32))


def _rand(rng, n):
    return "".join("ACGT"[int(x)] for x in rng.integers(0, 4, size=n))


def synthetic_dereps(seed=5):
    """Three samples of a few dozen uniques: unequal maxlen (60, 48, 60), variable lengths inside a sample, uniques present in all,
    in one, and in the first and last only, abundance ties across first-appearance order, NA map entries, and mean qualities with
    full mantissas (sums over 3 or 7 reads)."""
    rng = np.random.default_rng(seed)
    shared_all = [_rand(rng, n) for n in (48, 40, 33, 48)]
    first_last = [_rand(rng, n) for n in (60, 55, 41)]
    own = [[_rand(rng, int(rng.integers(20, 61 if s != 1 else 49))) for _ in range(25)] for s in range(3)]
    samples = []
    for s in range(3):
        seqs = list(shared_all) + (first_last if s != 1 else []) + own[s]
        order = rng.permutation(len(seqs))
        seqs = [seqs[int(k)] for k in order]
        ab = rng.integers(1, 5, size=len(seqs)).astype(np.int32)   # small counts: many ties
        ab[:3] = (40, 40, 7)
        o2 = np.argsort(-ab, kind="stable")
        seqs, ab = [seqs[int(k)] for k in o2], ab[o2]
        maxlen = 48 if s == 1 else 60
        q = np.full((len(seqs), maxlen), np.nan)
        for i, x in enumerate(seqs):
            q[i, : len(x)] = rng.integers(60, 280, size=len(x)) / float(rng.choice([3.0, 7.0]))
        m = np.repeat(np.arange(len(seqs)), ab).astype(np.int32)
        rng.shuffle(m)
        m = np.concatenate([m, np.full(4, -1, dtype=np.int32)])  # zero-length reads
        m = m[rng.permutation(m.size)]
        samples.append(Derep(seqs, ab, q, m))
    return samples


# ---- the split of a pooled result (R/dada.R:451-472) ----------------------------------------------------------------------------------
def restate_split(res: DadaResult, abundances, u2p) -> DadaResult:
    m = [int(res.map[int(u)]) for u in u2p]                       # map[names(derep.in[[i]]$uniques)], 1-based, NA_INTEGER
    kept = sorted({x for x in m if x != NA_INTEGER})              # unique(map[...]), NA ignored by %in% below
    keep = [c + 1 in kept for c in range(res.nclust)]
    new_bi = np.cumsum(keep)
    rows = [c for c in range(res.nclust) if keep[c]]
    cl = {c: ([v[r] for r in rows] if c == "sequence" else np.asarray(v)[rows]) for c, v in res.clustering.items()}
    new_map = np.array([NA_INTEGER if x == NA_INTEGER else new_bi[x - 1] for x in m], dtype=np.int32)
    sums = {}
    for x, a in zip(new_map, abundances):                         # tapply(derep.in[[i]]$uniques, map, sum)
        if x != NA_INTEGER:
            sums[int(x)] = sums.get(int(x), 0) + int(a)
    cl["abundance"] = np.array([sums[k] for k in sorted(sums)], dtype=np.int32)
    brow = [r for r, c in enumerate(res.birth_subs["clust"]) if keep[int(c) - 1]]
    bs = {c: ([v[r] for r in brow] if c in ("ref", "sub") else np.asarray(v)[brow]) for c, v in res.birth_subs.items()}
    bs["clust"] = np.array([new_bi[int(res.birth_subs["clust"][r]) - 1] for r in brow], dtype=np.int32)
    return DadaResult(cl, bs, res.subqual, np.asarray(res.clusterquals)[:, rows], new_map, res.pval)


# ---- the pass loop (R/dada.R:256-405) over the reference's dada_uniques -----------------------------------------------------------------
def restate_dada(dereps, err, self_consist, err_fun, opts, pool=False, prior_seqs=(), flags=None):
    """(results per INPUT sample, err_out, errs) as R's dada() gives them, the core being oracle.ref.dada_uniques."""
    from dada2_amd import api
    from oracle import ref
    o = (opts or DadaOpts()).normalised()
    inputs = list(dereps)
    pseudo = pool == "pseudo"
    pooled = pool is True and len(inputs) > 1
    if pooled:
        comb, u2p = restate_combine(inputs)
        dereps = [comb]
    else:
        dereps = inputs
    priors, pseudo_priors = list(prior_seqs or ()), []
    initialize = self_consist and err is None
    nconsist = 0 if initialize else 1
    errs = []
    while True:
        if nconsist > 0:
            errs.append(np.array(err, copy=True))
        results = []
        want = set(priors) | set(pseudo_priors)
        for i, d in enumerate(dereps):
            qmax = int(np.ceil(np.nanmax(d.quals)))
            erri = np.ones((16, max(41, qmax + 1))) if initialize else extend_err(err, qmax)
            pri = np.array([s in want for s in d.seqs], dtype=np.uint8)
            if flags is not None and flags[i] is not None:
                pri |= np.asarray(flags[i], dtype=np.uint8)
            results.append(ref.dada_uniques(d.seqs, d.abundances, pri, erri, d.quals, o, max_clust=1 if initialize else None))
        cur = api.accumulate_trans([r.subqual for r in results])
        err = err_fun(cur) if err_fun is not None else None
        if initialize:
            initialize = False
            err[[0, 5, 10, 15], :] = 1.0
        if (not self_consist) or any(np.array_equal(e, err) for e in errs) or nconsist >= o.MAX_CONSIST:
            if not pseudo or nconsist >= 2:
                break
        if pseudo and nconsist >= 1:
            mat, names = api.make_sequence_table(results)
            hit = ((mat > 0).sum(axis=0) >= o.PSEUDO_PREVALENCE) | (mat.sum(axis=0) >= o.PSEUDO_ABUNDANCE)
            pseudo_priors = [s for s, h in zip(names, hit) if h]
        nconsist += 1
    if pooled:
        results = [restate_split(results[0], d.abundances, u) for d, u in zip(inputs, u2p)]
    return results, err, errs


def check_dada(api, dereps, err, self_consist, opts, pool, prior_seqs=None, flags=None):
    """api.dada against restate_dada, every input sample's result and the error matrices."""
    got, gerr, gerrs = api.dada(dereps, err, self_consist=self_consist, opts=opts, pool=pool, prior_seqs=prior_seqs, priors=flags)
    want, werr, werrs = restate_dada(dereps, err, self_consist, api.noqual_errfun, opts, pool, prior_seqs, flags)
    assert len(got) == len(want) == len(dereps)
    no_priors = pool != "pseudo" and not prior_seqs and flags is None
    for g, w in zip(got, want):
        assert_results_equal(g, w, check_birth_from=no_priors)
    _same_float(gerr, werr, 0)
    assert len(gerrs) == len(werrs)
    for a, b in zip(gerrs, werrs):
        _same_float(a, b, 0)
    return got, want


_PAIR = {}


def golden_pair():
    """sam1F and sam2F (tests/golden), with tperr1."""
    if not _PAIR:
        _PAIR.update(dereps=[load_input("sam1F"), load_input("sam2F")], err=tperr1())
    return _PAIR["dereps"], _PAIR["err"]


def pseudo_differs(dereps, err, self_consist, opts):
    """From the reference alone: the pseudo-pooled result differs from the independent one in at least one sample."""
    from dada2_amd import api
    a, _, _ = restate_dada(dereps, err, self_consist, api.noqual_errfun, opts, "pseudo")
    b, _, _ = restate_dada(dereps, err, self_consist, api.noqual_errfun, opts, False)
    return any(x.clustering["sequence"] != y.clustering["sequence"] or not np.array_equal(x.map, y.map) for x, y in zip(a, b))


# ---- the match kernel -----------------------------------------------------------------------------------------------------------------
_MATCH = {}


def match_sample():
    """About 700 uniques (not a multiple of 64 or 256) of lengths 15, 16, 17, 31, 32, 33, 63, 64, 65 and 250, among them pairs that share
    their first 32 bases and differ only in the last base, pairs that differ only in the last base of a full word, and one sequence
    that is a proper prefix of another.  (seqs, abundances, quals), built once per process."""
    if not _MATCH:
        rng = np.random.default_rng(21)

        def other(c):
            return "ACGT"[("ACGT".index(c) + 1) % 4]
        seqs = []
        for L in (15, 16, 17, 31, 32, 33, 63, 64, 65, 250):
            for _ in range(60):
                seqs.append(_rand(rng, L))
        base = _rand(rng, 250)
        for L in (33, 63, 64, 65, 250):                           # equal first 32 bases (one key), different in the last base only
            seqs += [base[: L - 1] + "A", base[: L - 1] + "C", base[: L - 1] + "G"]
        for L in (16, 32, 48, 64, 240):                           # ... in the last base of a full word
            b2 = _rand(rng, L)
            seqs += [b2, b2[:-1] + other(b2[-1])]
        pre = _rand(rng, 100)
        seqs += [pre, pre[:64], pre[:40], pre[:17]]               # proper prefixes of one another
        for _ in range(40):                                       # many sequences under one key
            seqs.append(base[:32] + _rand(rng, int(rng.integers(1, 60))))
        seqs = list(dict.fromkeys(seqs))
        while len(seqs) % 64 == 0 or len(seqs) % 256 == 0:
            seqs.append(_rand(rng, 70))
        n = len(seqs)
        assert 650 <= n <= 760, n
        ab = np.sort(rng.integers(1, 30, size=n).astype(np.int32))[::-1].copy()
        q = np.full((n, 250), np.nan)
        for i, s in enumerate(seqs):
            q[i, : len(s)] = rng.integers(20, 41, size=len(s))
        _MATCH.update(seqs=seqs, ab=ab, quals=q, base=base, pre=pre)
    return _MATCH


def prior_lists():
    """name -> (prior sequences, or_flags or None)."""
    d = match_sample()
    seqs, base, pre = d["seqs"], d["base"], d["pre"]
    rng = np.random.default_rng(22)
    n = len(seqs)
    mixed = [seqs[5], seqs[n - 1], _rand(rng, 40), seqs[5], seqs[300], seqs[61][:-1] + "N", "ACGTN", _rand(rng, 300), seqs[0] + "A",
             base[:62] + "A", base[:62] + "C", base[:249] + "G", base[:249] + "T", pre[:64], pre[:63], pre, seqs[300], "", "acgt" * 8]
    mixed += [base[:32] + _rand(rng, int(rng.integers(1, 60))) for _ in range(30)]    # many entries under one key, none a unique
    mixed += [s for s in seqs if s.startswith(base[:32])][::2]                            # ... and every second unique under it
    last_word = [s for s in seqs if len(s) in (16, 32, 48, 64, 240)][::3]
    orf = np.zeros(n, dtype=np.uint8)
    orf[[1, 7, n - 2]] = 1                                         # uniques that match nothing in `mixed`
    assert not any(seqs[i] in mixed for i in (1, 7, n - 2))
    every = list(seqs[::-1]) + [seqs[3]]
    return {"mixed": (mixed, None), "mixed_or": (mixed, orf), "empty": ([], None), "empty_or": ([], orf), "one": ([seqs[305]], None),
            "one_miss": ([_rand(rng, 64)], None), "last_word": (last_word, None), "every": (every, None)}


_REF_RUNS = {}
MATCH_RUN_OPTS = dict(OMEGA_P=0.2, OMEGA_A=1e-40)


def reference_run(flags):
    """The reference's dada_uniques on the match sample with these prior flags and OMEGA_P loosened: computed once per set of flags."""
    from oracle import ref
    d = match_sample()
    key = np.asarray(flags, dtype=np.uint8).tobytes()
    if key not in _REF_RUNS:
        _REF_RUNS[key] = ref.dada_uniques(d["seqs"], d["ab"], np.asarray(flags, dtype=np.uint8), tperr1(), d["quals"], DadaOpts(**MATCH_RUN_OPTS))
    return _REF_RUNS[key]


def check_match(api, smp, name, env=None, run=True):
    """One set_prior_seqs call against list.index / in; with ``run`` also one Sample.run with OMEGA_P loosened, against the reference
    run with the same flags: every unique's flag shows there (h_prior, which the host's replay reads, and the device array agree
    with what the call reported).  That the flags show is asserted from the reference alone: with any flag set its result differs
    from its result without flags."""
    d = match_sample()
    priors, orf = prior_lists()[name]
    first = {}
    for j, s in enumerate(priors):
        first.setdefault(s, j)
    want_match = np.array([first.get(s, -1) for s in d["seqs"]], dtype=np.int32)
    want_flags = (want_match >= 0) | (orf != 0 if orf is not None else False)
    nset, got = with_env(env, lambda: smp.set_prior_seqs(priors, or_flags=orf, want_match=True))
    assert np.array_equal(got, want_match), (name, env, np.flatnonzero(got != want_match)[:8])
    assert nset == int(np.sum(want_flags)), (name, env, nset, int(np.sum(want_flags)))
    st = smp.prior_seqs_stats()
    assert st["given"] == len(priors) and st["flags_set"] == nset, st
    if run:
        want = reference_run(want_flags)
        if want_flags.any():
            plain = reference_run(np.zeros(len(d["seqs"]), dtype=np.uint8))
            assert want.clustering["sequence"] != plain.clustering["sequence"] or not np.array_equal(want.map, plain.map), name
        res = smp.run(tperr1(), DadaOpts(**MATCH_RUN_OPTS))
        assert_results_equal(res, want, check_birth_from=not want_flags.any())
    return st


def case_match(api, env=None, run=True):
    """Every prior list on one resident sample, one call after the other (each call replaces the flags of the one before), each
    followed by the run that shows the flags."""
    d = match_sample()
    out = {}
    smp = api.Sample(d["seqs"], d["ab"], None, d["quals"])
    try:
        for name in prior_lists():
            out[name] = check_match(api, smp, name, env=env, run=run)
    finally:
        smp.close()
    return out


MATCH_PATHS = {"lds": None, "global": {"DADA2HIP_PRIORS_LDS_KEYS": 4}, "strided": {"DADA2HIP_PRIORS_GRID": 1},
               "strided_global": {"DADA2HIP_PRIORS_GRID": 2, "DADA2HIP_PRIORS_LDS_KEYS": 0}}


def case_match_path(api, path, run=True):
    """Every prior list through one path of k_prior_match: the keys in LDS, the keys in global memory (a budget of 4 keys), one block
    that strides over the 667 uniques, and two blocks that stride with the keys in global memory."""
    st = case_match(api, env=MATCH_PATHS[path], run=run)
    lds = {n: s["keys_in_lds"] for n, s in st.items()}
    blocks = {s["blocks"] for s in st.values()}
    if path == "lds":
        assert blocks == {3} and lds == dict(lds, mixed=1, every=1, one=1, empty=0), st
    elif path == "global":
        assert blocks == {3} and lds == dict(lds, mixed=0, last_word=0, every=0, one=1), st
    elif path == "strided":
        assert blocks == {1} and lds["mixed_or"] == 1, st
    else:
        assert blocks == {2} and not any(lds.values()), st


def case_match_paths(api, run=True):
    for path in MATCH_PATHS:
        case_match_path(api, path, run=run)


def small_pair():
    """Two synthetic samples of 150 uniques x 80 nt that share their true variants (the emulator's pooled runs)."""
    from dada2_amd.synth import make_sample, true_variants
    err = tperr1()
    tv = true_variants(np.random.default_rng(30), 8, 80)
    return [make_sample(err, 150, L=80, seed=s, chunk=600, variants=tv) for s in (31, 32)], err


def emu_run():
    """The emulator's job (tests/test_emu_pool.py): the match kernel's cases without the runs, one small pooled and one small
    pseudo-pooled run."""
    from dada2_amd import api
    case_match_paths(api, run=False)
    dereps, err = small_pair()
    check_dada(api, dereps, err, False, DadaOpts(), True, prior_seqs=[dereps[1].seqs[-1], dereps[0].seqs[3]])
    check_dada(api, dereps, err, False, DadaOpts(), "pseudo")
    return "ok"
