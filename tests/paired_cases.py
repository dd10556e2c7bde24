"""The cases of the run-level mergePairs (dada2_amd.paired.merge_pairs, dada2hip_merge_run), shared by tests/test_paired.py (no
GPU), tests/test_gpu_paired.py (the MI355X) and tests/test_emu_paired.py (the emulated library, the lighter forms).

The specification: oracle/merge.py per sample with oracle.cport - which tests/test_merge.py pins to the reference's own C_nwalign,
C_eval_pair and C_pair_consensus - and, around it, ``spec_merge_pairs`` below: the list handling, the names, propagateCol and the
messages, written from R/paired.R with its lines cited.  Every comparison is row for row on every key, rejects included; every
case asserts a ``fact`` on the ORACLE's rows - that it reaches what it was built for - before anything is compared."""
import contextlib
import io
import os

import numpy as np

import merge_cases as mc
from oracle import cport, merge as omerge

KEYS = ("sequence", "abundance", "forward", "reverse", "nmatch", "nmismatch", "nindel", "prefer", "accept")
NO_MATCH = "Non-corresponding derep-class and dada-class objects."
NA = np.iinfo(np.int32).min


class SpecError(Exception):
    pass


# ---- the objects ----------------------------------------------------------------------------------------------------------------------------

def dada_of(seqs, n0, umap, **cols):
    """A DadaResult of which mergePairs reads the clustering table and the map (1-based, NA_INTEGER for NA)."""
    from dada2_amd.opts import DadaResult
    n = len(seqs)
    clustering = {"sequence": list(seqs), "abundance": np.arange(n, 0, -1, dtype=np.int32), "n0": np.asarray(n0, dtype=np.int32),
                  "birth_ham": np.arange(n, dtype=np.int32) % 5, "birth_fold": np.linspace(1.0, 2.0, n) if n else np.zeros(0)}
    clustering.update(cols)
    return DadaResult(clustering, {}, np.zeros((16, 1), np.int32), np.zeros((1, n)), np.asarray(umap, dtype=np.int32), np.zeros(len(umap)))


def derep_of(rmap, nuniq):
    from dada2_amd.io import Derep
    return Derep(["A"] * nuniq, np.ones(nuniq, np.int32), np.zeros((nuniq, 1)), np.asarray(rmap, dtype=np.int32))


def sample_of(c, na_by="both"):
    """(dadaF, derepF, dadaR, derepR) of a merge_cases case: read i names unique fwd[i] - 1, which the dada map sends to sequence
    fwd[i]; an NA read is NA in the derep map (every second one, or all with na_by="derep") or names a unique that was not
    corrected.  A dada map is as long as the largest entry of its derep map asks for (:117-118)."""
    out = []
    for key, seqs, n0 in (("fwd", c["seqsF"], c["n0F"]), ("rev", c["seqsR"], c["n0R"])):
        n = len(seqs)
        idx = np.asarray(c[key], dtype=np.int64)
        rmap = np.where(idx > 0, idx - 1, -1)
        nas = np.flatnonzero(idx <= 0)
        if na_by != "derep":
            rmap[nas if na_by == "dada" else nas[1::2]] = n        # the unique behind the sequences: not corrected
        umap = np.concatenate([np.arange(1, n + 1), [NA]])[: int(rmap.max()) + 1] if rmap.size and rmap.max() >= 0 else np.zeros(0, np.int64)
        out += [dada_of(seqs, n0, umap), derep_of(rmap, len(umap))]
    return tuple(out)


def denoised(dada, derep):
    """dada$map[derep$map] (:121-122): 1-based, <= 0 for NA."""
    rmap = np.asarray(derep.map, dtype=np.int64)
    umap = np.asarray(dada.map, dtype=np.int64)
    out = np.full(rmap.size, -1, dtype=np.int64)
    ok = rmap >= 0
    out[ok] = umap[rmap[ok]]
    return np.where(out > 0, out, -1)


# ---- the specification ----------------------------------------------------------------------------------------------------------------------

def spec_sample(dF, eF, dR, eR, min_overlap=12, max_mismatch=0, return_rejects=False, propagate_col=(), just_concatenate=False,
                trim_overhang=False, verbose=False, messages=None):
    mF, mR = np.asarray(eF.map), np.asarray(eR.map)
    okF, okR = mF[mF >= 0], mR[mR >= 0]
    if not (mF.size == mR.size and okF.size and okR.size and okF.max() + 1 == len(dF.map) and okR.max() + 1 == len(dR.map)):   # :116-120
        raise SpecError(NO_MATCH)
    fwd, rev = denoised(dF, eF), denoised(dR, eR)
    if (fwd > dF.nclust).any() or (rev > dR.nclust).any():          # (R would index past the clustering table: NA rows, then an error in rc())
        raise SpecError(NO_MATCH)
    rows = omerge.merge_pairs(fwd, rev, list(dF.clustering["sequence"]), dF.clustering["n0"], list(dR.clustering["sequence"]),
                              dR.clustering["n0"], cport, min_overlap=min_overlap, max_mismatch=max_mismatch, trim_overhang=trim_overhang,
                              just_concatenate=just_concatenate, return_rejects=True)
    messages = messages if messages is not None else []
    if not rows:                                                    # :128-137
        if verbose:
            messages.append("No paired-reads (in ZERO unique pairings) successfully merged out of %d pairings) input." % mF.size)
        return []
    for col in [c for c in propagate_col if c in dF.clustering]:    # :179-183
        for r in rows:
            f, b = dF.clustering[col][r["forward"] - 1], dR.clustering[col][r["reverse"] - 1]
            r["F." + col], r["R." + col] = (f.item() if hasattr(f, "item") else f), (b.item() if hasattr(b, "item") else b)
    if verbose:                                                     # :187-189
        messages.append("%d paired-reads (in %d unique pairings) successfully merged out of %d (in %d pairings) input."
                        % (sum(r["abundance"] for r in rows if r["accept"]), sum(r["accept"] for r in rows), sum(r["abundance"] for r in rows), len(rows)))
    if not return_rejects:                                          # :190
        rows = [r for r in rows if r["accept"]]
    seqs = [r["sequence"] for r in rows]
    if len(set(seqs)) < len(seqs):                                  # :192-194
        messages.append("Duplicate sequences in merged output.")
    return rows


def spec_merge_pairs(dadaF, derepF, dadaR, derepR, **kw):
    """(result, messages): dadaF / dadaR lists or dicts of DadaResult, derepF / derepR lists of Derep (:94-111, :198-201)."""
    names = list(dadaF) if isinstance(dadaF, dict) else None
    dF = list(dadaF.values()) if isinstance(dadaF, dict) else list(dadaF)
    dR = list(dadaR.values()) if isinstance(dadaR, dict) else list(dadaR)
    if len({len(dF), len(derepF), len(dR), len(derepR)}) > 1:
        raise SpecError("The dadaF/derepF/dadaR/derepR arguments must be the same length.")
    messages = []
    out = [spec_sample(dF[i], derepF[i], dR[i], derepR[i], messages=messages, **kw) for i in range(len(dF))]
    if len(out) == 1:
        return out[0], messages
    return (dict(zip(names, out)) if names is not None else out), messages


def same_rows(got, want, what=""):
    assert len(got) == len(want), (what, len(got), len(want))
    for i, (g, w) in enumerate(zip(got, want)):
        assert set(g) == set(w), (what, i, sorted(g), sorted(w))
        for k in w:
            assert g[k] == w[k] and (g[k] is None) == (w[k] is None), (what, i, k, g, w)


def with_env(env, fn):
    old = {k: os.environ.get(k) for k in (env or {})}
    os.environ.update({k: str(v) for k, v in (env or {}).items()})
    try:
        return fn()
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def run(P, samples, names=None, env=None, stats=None, **kw):
    """paired.merge_pairs on [(dadaF, derepF, dadaR, derepR)]: always a list of the samples' rows, and what it printed."""
    dF, eF, dR, eR = ([s[i] for s in samples] for i in range(4))
    if names:
        dF, dR = dict(zip(names, dF)), dict(zip(names, dR))
    text = io.StringIO()
    with contextlib.redirect_stdout(text):
        got = with_env(env, lambda: P.merge_pairs(dF, eF, dR, eR, stats=stats, **kw))
    if len(samples) == 1:
        got = [got]
    elif names:
        assert list(got) == list(names)
        got = list(got.values())
    return got, text.getvalue().splitlines()


def check(P, samples, what="", fact=None, **kw):
    """The run against the specification, sample by sample, rejects included; ``fact`` is asserted on the oracle's rows first."""
    opts = {k: v for k, v in kw.items() if k not in ("env", "stats", "names")}
    messages = []
    want = [spec_sample(*s, return_rejects=True, messages=messages, **opts) for s in samples]
    if fact:
        fact(want)
    got, printed = run(P, samples, return_rejects=True, **kw)
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        same_rows(g, w, (what, "sample", i, opts))
    assert printed == messages, (what, printed, messages)
    return got


def refused(P, samples, text, **kw):
    from dada2_amd import _lib
    try:
        run(P, samples, **kw)
    except _lib.Dada2HipError as e:
        assert e.code == 1 and str(e).find(NO_MATCH) >= 0 and text in str(e), (str(e), text)
        return str(e)
    raise AssertionError("not refused: " + text)


# ---- tally ----------------------------------------------------------------------------------------------------------------------------------

def _short_tables(rng, nF, nR, L=34):
    """Short denoised sequences cut from three templates: cheap to align, some pairs merge and some do not."""
    tpl = [mc._rnd(rng, 64) for _ in range(3)]
    seqsF = [tpl[i % 3][(i * 5) % 12:(i * 5) % 12 + L - i % 7] for i in range(nF)]
    seqsR = [mc.rc(tpl[j % 3][64 - (L - j % 5) - (j * 3) % 10:64 - (j * 3) % 10]) for j in range(nR)]
    assert len(set(seqsF)) == nF and len(set(seqsR)) == nR
    return seqsF, seqsR


def _case(rng, fwd, rev, nF, nR):
    seqsF, seqsR = _short_tables(rng, nF, nR)
    return dict(seqsF=seqsF, seqsR=seqsR, fwd=np.asarray(fwd), rev=np.asarray(rev), n0F=rng.integers(1, 50, nF), n0R=rng.integers(1, 50, nR))


def case_tally_sizes(P, light=False):
    """1, 63, 64, 65 and 257 read pairs - a wave less one, a wave, a wave and one, a block and one - as five samples of one run;
    no reads at all is the reference's refusal (max() of an empty map is -Inf, :117)."""
    rng = np.random.default_rng(11)
    samples = []
    for n in (1, 63, 64, 65, 257):
        fwd, rev = rng.integers(1, 4, n), rng.integers(1, 4, n)
        fwd[-1], rev[-1] = 3, 3                                     # (the last unique of either map is named)
        samples.append(sample_of(_case(rng, fwd, rev, 3, 3)))

    def fact(want):
        assert [sum(r["abundance"] for r in w) for w in want] == [1, 63, 64, 65, 257] and all(len(w) > 3 for w in want[1:])
    st = {}
    got = check(P, samples, "sizes", fact, stats=st)
    assert st["samples"] == 5 and st["read_pairs_in"] == 450 and st["pairs_na"] == 0 and st["unique_pairs"] == sum(len(g) for g in got)
    empty = (dada_of(["ACGT" * 10], [1], []), derep_of([], 0), dada_of(["ACGT" * 10], [1], []), derep_of([], 0))
    refused(P, [empty], "sample 1")
    refused(P, [samples[0], empty], "sample 2")


def case_tally_waves(P, light=False):
    """One key in all 64 lanes of a wave; a key whose first appearance is read 0 and whose others lie in another block (reads
    >= 4 096) against a key of equal abundance that starts at read 1; keys that differ only in f, only in r."""
    rng = np.random.default_rng(12)
    one = _case(rng, [1] * 64 + [2], [2] * 64 + [2], 2, 2)
    n = 4200
    fwd, rev = np.full(n, 3), np.full(n, 3)
    fwd[0], rev[0] = 1, 2
    fwd[4096:4100], rev[4096:4100] = 1, 2                          # key A: read 0 and four reads of the second block of 4 096
    fwd[1:6], rev[1:6] = 2, 1                                      # key B: reads 1..5 - as abundant as A, and later
    far = _case(rng, fwd, rev, 3, 3)
    differ = _case(rng, [1, 2, 1, 2, 2, 2], [1, 1, 2, 2, 1, 2], 2, 2)

    def fact(want):
        assert [(r["forward"], r["reverse"], r["abundance"]) for r in want[0]] == [(1, 2, 64), (2, 2, 1)]
        assert [(r["forward"], r["reverse"], r["abundance"]) for r in want[1]] == [(3, 3, n - 10), (1, 2, 5), (2, 1, 5)]
        assert [(r["forward"], r["reverse"], r["abundance"]) for r in want[2]] == [(2, 1, 2), (2, 2, 2), (1, 1, 1), (1, 2, 1)]
    check(P, [sample_of(one), sample_of(far), sample_of(differ)], "waves", fact)


def case_tally_na(P, light=False):
    """NA on either side at either step - the derep map, the dada map -, and a sample whose every pair has one."""
    rng = np.random.default_rng(13)
    fwd = [1, -1, 2, 2, -1, 1, 2, -1, 2, 1, -1, 2]
    rev = [2, 1, -1, 2, -1, 1, -1, 2, 2, -1, 1, 2]
    c = _case(rng, fwd, rev, 2, 2)
    gone = _case(rng, [1, -1, 2, -1, -1, -1], [-1, 2, -1, 1, -1, -1], 2, 2)
    samples = [sample_of(c, "both"), sample_of(c, "derep"), sample_of(c, "dada"), sample_of(gone, "both")]
    for s in samples[:3]:
        assert (np.asarray(s[1].map) < 0).any() or NA in s[0].map
    assert (np.asarray(samples[0][1].map) < 0).any() and NA in samples[0][0].map and NA in samples[0][2].map

    def fact(want):
        assert [sum(r["abundance"] for r in w) for w in want] == [5, 5, 5, 0] and want[3] == []
    st = {}
    check(P, samples, "na", fact, stats=st, verbose=True)
    assert st["pairs_na"] == 3 * 7 + 6 and st["read_pairs_in"] == 42
    assert check(P, [samples[3]], "all na alone", verbose=True) == [[]]


def case_tally_collisions(P, light=False):
    """A few hundred keys under a hash of 0 and of 4 bits: rows unchanged, the walk counted."""
    rng = np.random.default_rng(14)
    nF, nR = (12, 10) if light else (20, 15)
    fwd = np.concatenate([np.repeat(np.arange(1, nF + 1), nR), rng.integers(1, nF + 1, 500)])
    rev = np.concatenate([np.tile(np.arange(1, nR + 1), nF), rng.integers(1, nR + 1, 500)])
    sample = sample_of(_case(rng, fwd, rev, nF, nR))

    def fact(want):
        assert len(want[0]) == nF * nR and sum(r["accept"] for r in want[0]) >= 5 and sum(not r["accept"] for r in want[0]) >= 50
    plain = {}
    base = check(P, [sample], "hash unmasked", fact, stats=plain, max_mismatch=1)
    assert plain["table_capacity"] == (256 if light else 1024)      # the next power of two at or above 2 min(reads, nF nR)
    for bits in (0, 4):
        st = {}
        got = check(P, [sample], "hash of %d bits" % bits, stats=st, env={"DADA2HIP_MERGE_HASH_BITS": bits}, max_mismatch=1)
        assert got == base and st["collisions"] > max(plain["collisions"], nF * nR // 2), (bits, st["collisions"], plain["collisions"])


def case_tally_two_samples(P, light=False):
    """The same (f, r) in two samples of one call with different counts: the samples do not see each other."""
    rng = np.random.default_rng(15)
    a = _case(rng, [1, 1, 1, 2, 2], [1, 1, 1, 2, 2], 2, 2)
    b = dict(a, fwd=np.array([2, 1, 2, 2, 2, 2, 2]), rev=np.array([2, 1, 2, 2, 2, 2, 2]))

    def fact(want):
        assert [(r["forward"], r["abundance"]) for r in want[0]] == [(1, 3), (2, 2)] and [(r["forward"], r["abundance"]) for r in want[1]] == [(2, 6), (1, 1)]
    check(P, [sample_of(a), sample_of(b)], "two samples", fact, names=["first", "second"])


def case_tally_index(P, light=False):
    """An index one past either table, first at read 70 and again at read 3: read 3 is named, with the sample."""
    rng = np.random.default_rng(16)
    n = 100
    fwd, rev = rng.integers(1, 4, n), rng.integers(1, 4, n)
    fwd[-1] = rev[-1] = 3
    good = sample_of(_case(rng, fwd, rev, 3, 3))
    for side in (0, 2):
        dada, derep = good[side], good[side + 1]
        rmap = np.array(derep.map)
        rmap[[70, 3]] = len(dada.map)                              # one past the dada-class object's uniques
        bad = list(good)
        bad[side + 1] = derep_of(rmap, len(dada.map))
        msg = refused(P, [good, tuple(bad)], "sample 2, read 3 ")
        assert ("forward" if side == 0 else "reverse") in msg and "unique 4 of 3" in msg, msg
        umap = np.array(dada.map)
        rmap = np.array(derep.map)
        rmap[[70, 3]] = 1
        umap[1] = dada.nclust + 1                                  # one past the clustering table, reached from reads 3 and 70
        rmap[[0, 1, 2]] = [0, 2, 2]
        bad = list(good)
        bad[side], bad[side + 1] = dada_of(dada.clustering["sequence"], dada.clustering["n0"], umap), derep_of(rmap, len(umap))
        first = int(np.flatnonzero(rmap == 1)[0])
        msg = refused(P, [tuple(bad)], "sample 1, read %d " % first)
        assert "sequence 4 of 3" in msg, msg
    check(P, [good], "the good sample runs")


# ---- eval and consensus -------------------------------------------------------------------------------------------------------------------

def _pairs_case(pairs, n0F=None, n0R=None):
    c = mc._case("built", pairs, [dict()], None, n0F=n0F, n0R=n0R)
    return sample_of(c)


def case_eval_constructed(P, light=False):
    """Every constructed case of merge_cases.py - overlap at min_overlap and one below, max_mismatch 0 / 1 / 2 / 3, read-through,
    containment either way, prefer, no overlap, repeats, 2 x 300 nt, no pair left - as ONE run of nine samples under every option
    set any of them names, each case's own fact asserted on the oracle's rows under its own options."""
    cases = mc.constructed_cases()
    assert len(cases) == 9
    samples = [sample_of(c) for c in cases]
    option_sets = []
    for o in [o for c in cases for o in c["options"]] + list(mc.OPTION_SETS.values()):
        if o not in option_sets:
            option_sets.append(o)
    if light:
        option_sets = [dict(), dict(max_mismatch=1), dict(trim_overhang=True)]
    by_option = {}

    for o in option_sets:
        def fact(want, o=o):
            by_option[repr(o)] = want
        check(P, samples, "constructed", fact, **o)
    if not light:
        for i, c in enumerate(cases):                               # (the spec's rows are the oracle's rows: the facts hold for them)
            c["fact"]({k: by_option[repr(o)][i] for k, o in enumerate(c["options"])})


def case_eval_tiles(P, light=False):
    """Alignments of 63, 64, 65, 128 and 129 columns; overhangs of 64 and 70 columns on each side, so that a gap run crosses a
    tile, kept and trimmed; an indel and a mismatch at columns 63 and 64, the mismatch with prefer 1 and 2."""
    rng = np.random.default_rng(21)
    lengths = []
    for a, b, ov in ((40, 40, 17), (40, 40, 16), (40, 40, 15), (70, 70, 12), (70, 71, 12)):
        amp = mc._rnd(rng, a + b - ov)
        lengths.append(((amp[:a], mc.rc(amp[a - ov:])), amp))

    def fact_len(want):
        assert [len(r["sequence"]) for r in mc._by_pair(want[0])] == [63, 64, 65, 128, 129] and all(r["accept"] for r in want[0])
        assert [r["sequence"] for r in mc._by_pair(want[0])] == [amp for _, amp in lengths]
    check(P, [_pairs_case([p for p, _ in lengths])], "columns", fact_len)

    over = []
    for k in (64, 70):
        amp, xf, xr = mc._rnd(rng, 90), mc._rnd(rng, k), mc._rnd(rng, k)
        over.append(((amp + xf, mc.rc(xr + amp)), xr + amp + xf, amp))
    for trim in (False, True):
        def fact_over(want, trim=trim):
            assert [r["sequence"] for r in mc._by_pair(want[0])] == [o[2 if trim else 1] for o in over] and all(r["nmatch"] == 90 for r in want[0])
        check(P, [_pairs_case([o[0] for o in over])], "overhangs", fact_over, trim_overhang=trim)

    amp = mc._rnd(rng, 160)
    f = amp[:100]                                                   # the reverse read starts at column 40: columns 63 and 64 lie in the overlap
    pairs, n0F, n0R = [], [], []
    for col in (63, 64):
        for n0 in ((9, 3), (3, 9)):
            pairs.append((f, mc.rc(mc._flip(amp[40:], col - 40))))
            n0F.append(n0[0]); n0R.append(n0[1])
        pairs.append((f, mc.rc(amp[40:col] + amp[col + 1:])))
        n0F.append(5); n0R.append(5)

    def fact_mid(want):
        rr = mc._by_pair(want[0])
        assert [r["prefer"] for r in rr] == [1, 2, 1, 1, 2, 1] and all(r["accept"] for r in rr)
        assert [(r["nmismatch"], r["nindel"]) for r in rr] == [(1, 0), (1, 0), (0, 1)] * 2
        assert rr[0]["sequence"] == amp == rr[3]["sequence"] and rr[1]["sequence"] == mc._flip(amp, 63) and rr[4]["sequence"] == mc._flip(amp, 64)
        assert rr[2]["sequence"] == amp == rr[5]["sequence"]
    check(P, [_pairs_case(pairs, n0F, n0R)], "columns 63 and 64", fact_mid, max_mismatch=1)


# ---- chunking -------------------------------------------------------------------------------------------------------------------------------

def chunk_samples(light=False):
    rng = np.random.default_rng(31)
    samples = []
    for nF, nR in ((10, 10), (15, 12), (20, 15), (11, 10), (13, 19)) if not light else ((7, 6), (8, 8), (5, 9)):
        fwd = np.concatenate([np.repeat(np.arange(1, nF + 1), nR), rng.integers(1, nF + 1, 200)])
        rev = np.concatenate([np.tile(np.arange(1, nR + 1), nF), rng.integers(1, nR + 1, 200)])
        samples.append(sample_of(_case(rng, fwd, rev, nF, nR)))
    return samples


def case_chunks(P, light=False):
    """Five samples of 100 to 300 unique pairs under DADA2HIP_MERGE_CHUNK=128: chunk borders inside samples and between them; the
    launch ledger shows k_nw_gen<pair> and nothing else of the aligner; the same call with the knob unset gives equal rows."""
    import aligner_cases as A
    samples = chunk_samples(light)
    chunk = 32 if light else 128

    def fact(want):
        sizes = [len(w) for w in want]
        assert sizes == ([42, 64, 45] if light else [100, 180, 300, 110, 247]), sizes
        ends = np.cumsum(sizes)
        assert any(e % chunk for e in ends[:-1]) and sum(r["accept"] for w in want for r in w) >= 10
    st, whole = {}, {}
    A.read_ledger()
    cut = check(P, samples, "chunks", fact, stats=st, env={"DADA2HIP_MERGE_CHUNK": chunk}, max_mismatch=1)
    ran = A.read_ledger() & ~A.GAPLESS_BITS
    assert ran == (0 if getattr(P, "SERVED_BY_SPEC", False) else A.bit_gen(True)), A.describe(ran)
    assert st["chunks"] == -(-st["unique_pairs"] // chunk) > len(samples)
    assert check(P, samples, "one chunk", stats=whole, max_mismatch=1) == cut and whole["chunks"] == 1
    assert whole["accepted"] == st["accepted"] == sum(r["accept"] for w in cut for r in w)


def case_concat(P, light=False):
    """just_concatenate: the tally is the device's, nothing is aligned; the three committed cases against the golden rows."""
    import json

    from helpers import GOLDEN
    z = np.load(os.path.join(GOLDEN, "merge_pairs.npz"))
    samples = [sample_of(mc.make_case(seed)) for seed in (1, 2, 3)]
    got = check(P, samples, "concat", just_concatenate=True)
    for seed, g in zip((1, 2, 3), got):
        same_rows(g, [dict(r, accept=bool(r["accept"])) for r in json.loads(str(z["c%d_concat" % seed]))], ("golden concat", seed))


# ---- the interface where it needs the tally ---------------------------------------------------------------------------------------------

def fixture_samples():
    """The FASTQ fixtures sam1F / sam1R and sam2F / sam2R with made-up dada-class objects over short sequences: mergePairs reads
    the maps and the clustering tables, not the reads.  [(dadaF, path F, dadaR, path R)] and the same with Dereps."""
    from dada2_amd import api
    from helpers import GOLDEN
    rng = np.random.default_rng(41)
    files, dereps = [], []
    for k, sam in enumerate(("sam1", "sam2")):
        amps = [mc._rnd(rng, 60) for _ in range(6 + k)]             # forward i and reverse i overlap by 20 and merge
        seqsF, seqsR = [a[:40] for a in amps], [mc.rc(a[20:]) for a in amps[: 5 + k]]
        row_f, row_d = [], []
        for side, seqs in (("F", seqsF), ("R", seqsR)):
            path = os.path.join(GOLDEN, sam + side + ".fastq.gz")
            d = api.derep_fastq(path)
            umap = (np.arange(d.nraw) * 5 + k) % (len(seqs) + 1)   # 0: not corrected
            dada = dada_of(seqs, rng.integers(1, 50, len(seqs)), np.where(umap > 0, umap, NA))
            row_f += [dada, path]
            row_d += [dada, d]
        files.append(tuple(row_f))
        dereps.append(tuple(row_d))
    return files, dereps


def case_interface(P, light=False):
    """Every input form that reaches the tally: single objects, lists and dicts with names; Derep, NativeDerep, file names, a
    directory, mixed - all against the specification on the Derep form; propagate_col with a real column, an unknown one and
    several; return_rejects off; the verbose text; the result through api.make_sequence_table."""
    import shutil
    import tempfile

    from dada2_amd import api
    files, dereps = fixture_samples()
    kw = dict(max_mismatch=1, verbose=True)
    want, messages = spec_merge_pairs([s[0] for s in dereps], [s[1] for s in dereps], [s[2] for s in dereps], [s[3] for s in dereps], **kw)
    assert all(len(w) >= 5 for w in want) and len(messages) == 2 and all("successfully merged" in m for m in messages), messages

    def call(dF, eF, dR, eR, **more):
        text = io.StringIO()
        with contextlib.redirect_stdout(text):
            got = P.merge_pairs(dF, eF, dR, eR, **dict(kw, **more))
        return got, text.getvalue().splitlines()

    def same_run(got, printed, what):
        assert printed == messages, (what, printed, messages)
        for g, w in zip(got, want):
            same_rows(g, w, what)
    native = [(s[0], api.NativeDerep(s[1]), s[2], api.NativeDerep(s[3])) for s in files]
    forms = {"dereps": dereps, "file names": files, "native dereps": native, "mixed": [dereps[0][:3] + (files[0][3],), (native[1][0], files[1][1]) + native[1][2:]]}
    for what, ss in forms.items():
        got, printed = call([s[0] for s in ss], [s[1] for s in ss], [s[2] for s in ss], [s[3] for s in ss])
        assert isinstance(got, list) and len(got) == 2
        same_run(got, printed, what)
    got, printed = call({"a": dereps[0][0], "b": dereps[1][0]}, [s[1] for s in dereps], {"a": dereps[0][2], "b": dereps[1][2]}, [s[3] for s in dereps])
    assert isinstance(got, dict) and list(got) == ["a", "b"]
    same_run(list(got.values()), printed, "names")
    got, printed = call(*dereps[0])                                  # one sample: its rows alone (:200)
    same_rows(got, want[0], "single objects")
    assert printed == messages[:1]
    tmp = tempfile.mkdtemp()
    try:
        for side in (1, 3):
            os.mkdir(os.path.join(tmp, str(side)))
            for s in files:
                shutil.copy(s[side], os.path.join(tmp, str(side)))
        got, printed = call([s[0] for s in files], os.path.join(tmp, "1"), [s[2] for s in files], os.path.join(tmp, "3"))
        same_run(got, printed, "directories")
    finally:
        shutil.rmtree(tmp)
    # propagate_col (:179-183), return_rejects (:190)
    dF, eF, dR, eR = ([s[i] for s in dereps] for i in range(4))
    for cols in (("n0",), ("nope",), ("birth_ham", "nope", "birth_fold", "sequence")):
        for rejects in (False, True):
            w, m = spec_merge_pairs(dF, eF, dR, eR, max_mismatch=1, propagate_col=cols, return_rejects=rejects)
            text = io.StringIO()
            with contextlib.redirect_stdout(text):
                got = P.merge_pairs(dF, eF, dR, eR, max_mismatch=1, propagate_col=cols, return_rejects=rejects)
            assert text.getvalue().splitlines() == m
            for g, x in zip(got, w):
                same_rows(g, x, (cols, rejects))
            if cols[0] != "nope":
                assert "F." + cols[0] in w[0][0] and "R." + cols[0] in w[0][0] and not any("nope" in k for k in w[0][0])
            assert rejects or all(r["accept"] for x in w for r in x)
    mat, seqs = api.make_sequence_table(got)
    wmat, wseqs = api.make_sequence_table(w)
    assert seqs == wseqs and np.array_equal(mat, wmat) and mat.shape[0] == 2 and mat.sum() > 0


CASES = {"tally_sizes": case_tally_sizes, "tally_waves": case_tally_waves, "tally_na": case_tally_na, "tally_collisions": case_tally_collisions,
         "tally_two_samples": case_tally_two_samples, "tally_index": case_tally_index, "eval_constructed": case_eval_constructed,
         "eval_tiles": case_eval_tiles, "chunks": case_chunks, "concat": case_concat, "interface": case_interface}
CASE_NAMES = tuple(CASES)
# what needs no alignment: the tally, the order, the refusals, the concatenation - and so runs wherever the library loads
EMU_NAMES = CASE_NAMES


def emu_run(names=None):
    """The emulator's job (tests/test_emu_paired.py): every case in its lighter form."""
    from dada2_amd import paired
    names = names or EMU_NAMES
    for name in names:
        CASES[name](paired, light=True)
    return "ok %d cases" % len(names)
