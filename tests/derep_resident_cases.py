"""The resident form of the device dereplicator (dada2_amd.dereplicate: derep_reads_resident, filter_and_sample, dada), run by
the emulator and GPU tests.

The oracle is the route the library already has and already pins to the reference: dereplicate.derep_reads / filter_and_derep ->
Sample.from_native.  Every case makes the same reads resident both ways (``both``) and requires
  (a) the two derep objects to agree on sequences, abundances, map, maxlen, nreads and qmax();
  (b) dada2hip_sample_rows of the two samples to be equal byte for byte - seq2, len, reads, qual, padding included - and the
      geometry words with them;
  (c) run(err) with tests/golden/tperr1.npy to be equal field for field (floats bit for bit);
and, wherever the resident route's stats are taken, the traffic condition: the bytes it copied down are at most
U (28 + 4 W2) + A + 4 096 for U uniques of A letters in all - no 8-bytes-per-base term.

A case takes the module dada2_amd.dereplicate and raises AssertionError; ``light`` is the emulator's form (the 3 000 reads of one
unique are 300 there, the sample of the table's growth is narrower; the properties are the same).  CASES are the issue's cases 1-6
(reads in memory); FUSED_CASES, the files through the filter, are the card's alone."""
import os
import random
import tempfile
import warnings

import numpy as np

from derep_dev_cases import SAM1F, SAM1R, pool_reads, qbytes, rand_qual, rand_seq, with_quals
from primer_cases import _raises, with_env

NO_MATRIX = "no quality matrix"


# ---- the comparison ---------------------------------------------------------------------------------------------------------------------

def fields(nd):
    """What a derep object of either kind shows without its matrix."""
    from dada2_amd import _lib
    L = _lib.lib()
    sp = L.dada2hip_derep_seqs(nd._h)
    seqs = [sp[i].decode("latin-1") for i in range(nd.nuniques)]
    ab = np.ctypeslib.as_array(L.dada2hip_derep_abundances(nd._h), (nd.nuniques,)).copy()
    mp = np.ctypeslib.as_array(L.dada2hip_derep_map(nd._h), (nd.nreads,)).copy() if nd.nreads else np.zeros(0, np.int32)
    return dict(seqs=seqs, abundances=ab, map=mp, maxlen=nd.maxlen, nreads=nd.nreads, nuniques=nd.nuniques, qmax=nd.qmax())


def same_derep(rd, nd, what=""):
    g, w = fields(rd), fields(nd)
    assert g["seqs"] == w["seqs"], (what, "sequences", g["seqs"][:3], w["seqs"][:3])
    assert np.array_equal(g["abundances"], w["abundances"]), (what, "abundances")
    assert g["map"].shape == w["map"].shape and np.array_equal(g["map"], w["map"]), (what, "map")
    for k in ("maxlen", "nreads", "nuniques", "qmax"):
        assert g[k] == w[k], (what, k, g[k], w[k])
    return w


def same_rows(got, want, what=""):
    """dada2hip_sample_rows of two samples, byte for byte."""
    a, b = got.rows(), want.rows()
    for k in ("n", "W2", "LQ", "maxlen", "minlen", "qmax"):
        assert a[k] == b[k], (what, k, a[k], b[k])
    for k in ("len", "reads", "seq2", "qual"):
        assert a[k].shape == b[k].shape and a[k].dtype == b[k].dtype, (what, k, a[k].shape, b[k].shape)
        bad = np.argwhere(a[k] != b[k])
        assert bad.size == 0, (what, k, "first difference at", bad[0].tolist(), a[k][tuple(bad[0])], b[k][tuple(bad[0])], len(bad))
    return b


def same_run(got, want, qmax, what=""):
    from dada2_amd.io import extend_err
    from helpers import assert_results_equal, tperr1
    err = extend_err(tperr1(), qmax)
    a, b = got.run(err), want.run(err)
    assert_results_equal(a, b, exact_float=True)
    return b


def traffic(st, w, rows, what=""):
    U, A = w["nuniques"], sum(len(s) for s in w["seqs"])
    bound = U * (28 + 4 * rows["W2"]) + A + 4096
    assert 0 < st["resident_download_bytes"] <= bound, (what, "bytes down", st["resident_download_bytes"], bound)
    assert st["resident_upload_bytes"] <= 4 * U + 64 and st["resident_uniques"] == U, (what, st)


def both(dd, seqs, quals, n=10 ** 6, qual_offset=0, env=None, what="", stats=None, run=True):
    """The same reads resident both ways, held to (a), (b), (c) and the traffic condition.  Returns the host route's fields, its
    rows and (with ``run``) its result."""
    from dada2_amd import api
    quals = qbytes(quals)
    st = {} if stats is None else stats
    nd = dd.derep_reads(seqs, quals, n=n, qual_offset=qual_offset)
    smp = rd = None
    try:
        smp = api.Sample.from_native(nd)
        rd = with_env(env, lambda: dd.derep_reads_resident(seqs, quals, n=n, qual_offset=qual_offset, stats=st))
        assert isinstance(rd, api.NativeDerep) and isinstance(rd.sample, api.Sample) and rd.sample.nraw == rd.nuniques, what
        w = same_derep(rd, nd, what)
        rows = same_rows(rd.sample, smp, what)
        traffic(st, w, rows, what)
        res = same_run(rd.sample, smp, w["qmax"], what) if run else None
        return w, rows, res
    finally:
        for o in (rd, smp, nd):
            if o is not None:
                o.close()


def near(rng, s, k=1):
    """s with k substitutions."""
    t = list(s)
    for p in rng.sample(range(len(t)), k):
        t[p] = rng.choice([c for c in "ACGT" if c != t[p]])
    return "".join(t)


# ---- case 1: word and row borders ---------------------------------------------------------------------------------------------------------

BORDER_LENGTHS = (6, 15, 16, 17, 31, 32, 33, 63, 64, 65, 250)


def case_borders(dd, light=False):
    rng = random.Random(1201)
    seqs = []
    for l in BORDER_LENGTHS:
        for copies in (1, 2, 3):
            seqs += [rand_seq(rng, l)] * copies
    long = seqs[-1]
    seqs += [near(rng, long)] * 2 + [long] * 20                    # (something for the run to decide: a neighbour of the commonest)
    rng.shuffle(seqs)
    w, rows, _ = both(dd, seqs, with_quals(rng, seqs), what="lengths 6 .. 250 in one sample")
    assert rows["W2"] == 16 and rows["LQ"] == 256 and rows["minlen"] == 6 and rows["maxlen"] == 250, rows["W2"]
    assert sorted(set(rows["len"].tolist())) == list(BORDER_LENGTHS)
    # the zero tails of the short rows are there to be seen: every word behind a read, every byte from len on
    for r, l in enumerate(rows["len"].tolist()):
        assert not rows["seq2"][r, (l + 15) // 16:].any() and not rows["qual"][r, l:].any(), (r, l)
    # a sample whose longest read ends on a word border, and one a base past it: W2 rounds to four words either way
    for top in (64, 65):
        seqs = [rand_seq(rng, l) for l in (7, 16, 33, top) for _ in range(2)]
        seqs += [seqs[-1]] * 3
        w, rows, _ = both(dd, seqs, with_quals(rng, seqs), what="longest read %d" % top)
        assert rows["W2"] == (4 if top == 64 else 8) and rows["LQ"] == (64 if top == 64 else 80), (top, rows["W2"], rows["LQ"])


# ---- case 2: ties of the rounding -----------------------------------------------------------------------------------------------------------

def tie_reads(rng, lo, hi, big, L=60):
    """Uniques whose means are k + 1/2 (2 reads), k + 1/3, 2/3 (3 reads), k + 1/4, 1/2, 3/4 (4 reads) at every position, one unique
    of ``big`` reads, its neighbour, and a singleton; quality characters in lo .. hi."""
    seqs, quals = [], []

    def add(s, ups, total):
        base = bytes(rng.randint(lo, hi - 1) for _ in range(len(s)))
        for i in range(total):
            seqs.append(s)
            quals.append(bytes(c + 1 for c in base) if i < ups else base)
    for ups, total in ((1, 2), (1, 3), (2, 3), (1, 4), (2, 4), (3, 4)):
        add(rand_seq(rng, L), ups, total)
    common = rand_seq(rng, L)
    for _ in range(big):
        seqs.append(common)
        quals.append(rand_qual(rng, L, lo, hi))
    for _ in range(3):
        seqs.append(near(rng, common))
        quals.append(rand_qual(rng, L, lo, hi))
    seqs.append(rand_seq(rng, L))
    quals.append(rand_qual(rng, L, lo, hi))
    order = list(range(len(seqs)))
    rng.shuffle(order)
    return [seqs[i] for i in order], [quals[i] for i in order]


def case_ties(dd, light=False):
    rng = random.Random(1202)
    big = 300 if light else 3000
    for what, lo, hi, off in (("Auto resolving to 33", 35, 73, 0), ("Auto resolving to 64", 66, 104, 0), ("offset 33 given", 35, 73, 33),
                              ("offset 64 given", 66, 104, 64)):
        seqs, quals = tie_reads(rng, lo, hi, big)
        w, rows, _ = both(dd, seqs, quals, qual_offset=off, what=what)
        assert w["abundances"][0] == big and sorted(w["abundances"].tolist())[:1] == [1], what
        assert 2 <= rows["qual"][rows["qual"] > 0].min() and rows["qmax"] <= 41 and w["qmax"] <= 41, (what, rows["qmax"], w["qmax"])
        # the ties went up: a unique of two reads that differ by one everywhere has the larger character's quality
        for r in np.flatnonzero(rows["reads"] == 2):
            i = [k for k, s in enumerate(seqs) if s == w["seqs"][r]]
            hi_q = np.maximum(np.frombuffer(quals[i[0]], np.uint8), np.frombuffer(quals[i[1]], np.uint8)).astype(int) - (33 if lo < 59 else 64)
            assert rows["qual"][r, :len(hi_q)].tolist() == hi_q.tolist(), (what, "k + 1/2 rounds away from zero")


# ---- case 3: the order ------------------------------------------------------------------------------------------------------------------------

def case_order(dd, light=False):
    rng = random.Random(1203)
    A, B, Cc = "AAGTCC" * 5, "CAGTCC" * 5, "GAGTCC" * 5
    seqs = [Cc, A, B, A, Cc, B]
    for n, order in ((1, [Cc, A, B]), (2, [A, Cc, B]), (6, [A, B, Cc])):
        w, _, _ = both(dd, seqs, with_quals(rng, seqs), n=n, what="C A B A C B, n = %d" % n)
        assert w["seqs"] == order, (n, w["seqs"])
    # equal abundances whose first occurrences lie in different chunks; several pieces; a table that is rebuilt and an arena that
    # doubles before the finish (it starts at 64 KiB of letters)
    nd_, L = (290, 250) if not light else (150, 460)
    seqs = pool_reads(rng, nd_, nd_ + nd_ // 8, length=L)
    assert sum(len(s) for s in set(seqs)) > 65536
    quals = with_quals(rng, seqs)
    base, rows0, res0 = both(dd, seqs, quals, n=50, what="equal abundances over chunks of 50", run=not light)
    assert sorted(base["seqs"]) != base["seqs"] and len({int(a) for a in base["abundances"]}) < 8
    for env in ({"DADA2HIP_DEREP_PIECE": 16}, {"DADA2HIP_DEREP_PIECE": 64, "DADA2HIP_DEREP_TABLE": 8}):
        st = {}
        w, rows, _ = both(dd, seqs, quals, n=50, env=env, what="... with %s" % env, stats=st, run=False)
        assert w["seqs"] == base["seqs"] and np.array_equal(rows["qual"], rows0["qual"]), env
        assert st["pieces"] == (len(seqs) + env["DADA2HIP_DEREP_PIECE"] - 1) // env["DADA2HIP_DEREP_PIECE"], (env, st)
        assert ("DADA2HIP_DEREP_TABLE" not in env) or (st["rebuilds"] >= 1 and st["table_capacity"] >= 2 * nd_), (env, st)


# ---- case 4: the stride loop --------------------------------------------------------------------------------------------------------------------

def case_stride(dd, light=False):
    rng = random.Random(1204)
    seqs = pool_reads(rng, 300, 420, length=lambda: rng.randint(30, 50))
    quals = with_quals(rng, seqs)
    st = {}
    w, _, _ = both(dd, seqs, quals, env={"DADA2HIP_DD_SAMPLE_BLOCKS": 2}, what="300 uniques on two blocks", stats=st, run=not light)
    assert w["nuniques"] == 300 and st["resident_blocks"] == 2, st          # eight waves, 38 rows each: the knob held
    st = {}
    both(dd, seqs, quals, what="... and on its own grid", stats=st, run=False)
    assert st["resident_blocks"] == 75, st


# ---- case 5: input errors -----------------------------------------------------------------------------------------------------------------------

def case_errors(dd, light=False):
    from dada2_amd import api
    E = dd._lib.Dada2HipError
    rng = random.Random(1205)
    good = pool_reads(rng, 12, 30, length=40)
    for what, seqs, lo, hi, off, text in (
            ("an N in a read", good + [good[0][:20] + "N" + good[0][21:]], 35, 73, 0, "Sequences must be made up only of A/C/G/T."),
            ("a 5-nt read", good + ["ACGTA"], 35, 73, 0, "longer than the kmer-size (5)"),
            ("a 5-nt read with an N: the length comes first", good + ["ACNTA"], 35, 73, 0, "longer than the kmer-size (5)"),
            ("offset 64 forced on Phred+33 characters", good, 35, 60, 64, "Quality values must be positive integers.")):
        quals = with_quals(rng, seqs, lo=lo, hi=hi)
        seen = []
        nd = dd.derep_reads(seqs, quals, qual_offset=off)
        try:
            api.Sample.from_native(nd)
        except E as e:
            seen.append(e)
        finally:
            nd.close()
        try:
            got = dd.derep_reads_resident(seqs, quals, qual_offset=off)
            got.close()
        except E as e:
            seen.append(e)
        assert len(seen) == 2, (what, "both routes must refuse", [str(e) for e in seen])
        assert type(seen[0]) is type(seen[1]) and seen[0].code == seen[1].code == 1 and str(seen[0]) == str(seen[1]), (what, [str(e) for e in seen])
        assert text in str(seen[1]), (what, str(seen[1]))
    # the dereplicator's own refusals are derep_reads'
    _raises(E, lambda: dd.derep_reads_resident(["", ""], [b"", b""]), "Only zero-length sequences", code=1)
    _raises(E, lambda: dd.derep_reads_resident(["ACGTACGT"], [b"IIIIIIII"], qual_offset=50), "offset", code=1)
    _raises(ValueError, lambda: dd.derep_reads_resident(["ACGT"], [b"III"]), "as many quality characters")
    # means a little below zero round to zero on both routes: offset 64 on characters 64, 64, 64 and 63 is a mean of -1/4
    z = rand_seq(rng, 40)
    seqs = [z] * 4 + good
    quals = [bytes([64] * 40)] * 3 + [bytes([63] * 40)] + with_quals(rng, good, lo=66, hi=100)
    w, rows, _ = both(dd, seqs, quals, qual_offset=64, what="a mean of -1/4 is the byte 0", run=False)
    r = w["seqs"].index(z)
    assert not rows["qual"][r].any() and rows["reads"][r] == 4


# ---- case 6: what a ResidentDerep refuses -----------------------------------------------------------------------------------------------------

def case_refusals(dd, light=False):
    from dada2_amd import api
    from helpers import assert_results_equal, tperr1
    E = dd._lib.Dada2HipError
    rng = random.Random(1206)
    seqs = pool_reads(rng, 10, 40, length=40)
    seqs += [near(rng, seqs[0])] * 2
    quals = with_quals(rng, seqs)
    rds = [dd.derep_reads_resident(seqs, quals), dd.derep_reads_resident(seqs[5:], quals[5:])]
    nd, nd2 = dd.derep_reads(seqs, quals), dd.derep_reads(seqs[5:], quals[5:])
    try:
        L = dd._lib.lib()
        assert L.dada2hip_derep_has_quals(rds[0]._h) == 0 and not L.dada2hip_derep_quals(rds[0]._h)
        assert L.dada2hip_derep_has_quals(nd._h) == 1 and L.dada2hip_derep_qmax(nd._h) == nd.qmax()
        _raises(ValueError, lambda: rds[0].to_derep(), "filter_and_derep")
        _raises(ValueError, lambda: rds[0].to_derep(), NO_MATRIX)
        _raises(E, lambda: api.Sample.from_native(rds[0]), NO_MATRIX, code=1)
        _raises(E, lambda: api.combine_dereps(rds), NO_MATRIX, code=1)
        _raises(E, lambda: api.combine_dereps([nd, rds[1]]), NO_MATRIX, code=1)
        _raises(E, lambda: dd.dada(rds, tperr1(), pool=True), NO_MATRIX, code=1)
        _raises(E, lambda: api.dada(rds, tperr1(), pool=True), NO_MATRIX, code=1)
        _raises(ValueError, lambda: dd.dada([nd], tperr1()), "ResidentDerep")
        _raises(TypeError, lambda: dd.ResidentDerep("reads.fastq"), "derep_reads_resident")
        # what it does NOT refuse: dada(), on a list and on one object, running the samples the dereps came with
        res, _, _ = dd.dada(rds, tperr1())
        want, _, _ = api.dada([nd, nd2], tperr1())
        assert len(res) == 2
        for g, w in zip(res, want):
            assert_results_equal(g, w, exact_float=True)
        one, _, _ = dd.dada(rds[0], tperr1())
        assert_results_equal(one, want[0], exact_float=True)
        assert rds[0].sample._h and rds[1].sample._h, "dada() closes no sample it did not make"
    finally:
        for d in [nd, nd2] + rds:
            d.close()
        assert rds[0]._h is None and rds[0].sample._h is None, "close() closes both"


def case_pseudo(dd, light=False):
    """pool="pseudo" on ResidentDereps equals api.dada's on full objects of the same reads."""
    from dada2_amd import api
    from helpers import assert_results_equal, tperr1
    rng = random.Random(1207)
    samples = []
    common = rand_seq(rng, 60)
    variant = near(rng, common)
    for k in range(2):
        seqs = [common] * 60 + [variant] * (8 if k == 0 else 1) + pool_reads(rng, 6, 12, length=60)
        rng.shuffle(seqs)
        samples.append((seqs, with_quals(rng, seqs)))
    rds = [dd.derep_reads_resident(s, q) for s, q in samples]
    nds = [dd.derep_reads(s, q) for s, q in samples]
    try:
        def err_fun(trans):
            return tperr1()
        got, _, _ = dd.dada(rds, tperr1(), pool="pseudo", err_fun=err_fun)
        want, _, _ = api.dada(nds, tperr1(), pool="pseudo", err_fun=err_fun)
        for g, w in zip(got, want):
            assert_results_equal(g, w, exact_float=True)
    finally:
        for d in rds + nds:
            d.close()


CASES = {"borders": case_borders, "ties": case_ties, "order": case_order, "stride": case_stride, "errors": case_errors,
         "refusals": case_refusals, "pseudo": case_pseudo}
CASE_NAMES = tuple(CASES)
POISON_NAMES = ("borders", "ties", "order")                        # the issue's cases 1-3, once more on dirty memory


def run_poisoned(dd, byte, names=POISON_NAMES, light=False):
    """Cases 1-3 with the allocation cache handing out memory filled with ``byte``, as tests/poison_cases.py sets the knob: every
    pad word and byte of the resident rows must be WRITTEN by the new code (the host route's are, and the rows are compared)."""
    import poison_cases as P
    s0 = P.poison_stats()
    P._with_knob(byte, lambda: [CASES[n](dd, light=light) for n in names])
    s1 = P.poison_stats()
    assert s1[0] > s0[0] and s1[1] - s0[1] >= 256 * (s1[0] - s0[0]), ("no device block was filled: %s ignored?" % P.KNOB, s0, s1)
    P._with_knob(None, lambda: [CASES[n](dd, light=light) for n in names[:1]])   # ... and on what that run left in the cache
    assert P.poison_stats() == s1


# ---- case 7: fused, single and paired (the card's alone) -----------------------------------------------------------------------------------------

FILTER = dict(trunc_len=240, max_ee=2)


def same_resident(rd, nd, what):
    """A ResidentDerep and its sample against the NativeDerep of the host route and Sample.from_native of it: (a), (b), (c)."""
    from dada2_amd import api
    smp = api.Sample.from_native(nd)
    try:
        w = same_derep(rd, nd, what)
        rows = same_rows(rd.sample, smp, what)
        same_run(rd.sample, smp, w["qmax"], what)
        return w, rows
    finally:
        smp.close()


def case_fused_single(dd):
    with tempfile.TemporaryDirectory() as tmp:
        for filt in (None, os.path.join(tmp, "kept.fastq.gz")):
            st = {}
            counts, rd = dd.filter_and_sample(SAM1F, filt, n_derep=400, stats=st, **FILTER)
            want_counts, nd = dd.filter_and_derep(SAM1F, None, n_derep=400, **FILTER)
            try:
                assert counts == want_counts and 0 < counts[1] < counts[0] == 1500 and rd.nreads == counts[1]
                w, rows = same_resident(rd, nd, ("fused single", filt is not None))
                traffic(st, w, rows, "fused single")
                assert st["derep_uniques"] == w["nuniques"] and st["reads_kept"] == counts[1], st
            finally:
                rd.close()
                nd.close()
        ref = os.path.join(tmp, "ref.fastq.gz")
        from dada2_amd import api
        api.filter_and_trim(SAM1F, ref, **FILTER)
        with open(filt, "rb") as a, open(ref, "rb") as b:
            assert a.read() == b.read(), "the file is filter_and_trim's byte for byte"


def case_fused_paired(dd):
    from dada2_amd import api, paired
    from helpers import tperr1
    args = dict(trunc_len=(240, 200), max_ee=2)
    st = {}
    counts, rds = dd.filter_and_sample(SAM1F, None, SAM1R, None, n_derep=400, stats=st, **args)
    want_counts, nds = dd.filter_and_derep(SAM1F, None, SAM1R, None, n_derep=400, **args)
    try:
        assert counts == want_counts and 0 < counts[1] < 1500 and rds[0].nreads == rds[1].nreads == counts[1]
        for rd, nd, d, pre in zip(rds, nds, "FR", ("resident_", "resident_rev_")):
            w, rows = same_resident(rd, nd, ("fused pair", d))
            traffic({"resident_" + k: st[pre + k] for k in dd.RESIDENT_STATS}, w, rows, ("fused pair", d))
        err = tperr1()
        got = [dd.dada(rd, err)[0] for rd in rds]
        want = [api.dada(nd, err)[0] for nd in nds]
        a = paired.merge_pairs(got[0], rds[0], got[1], rds[1], return_rejects=True)
        b = paired.merge_pairs(want[0], nds[0], want[1], nds[1], return_rejects=True)
        assert a == b and sum(r["abundance"] for r in a if r["accept"]) > 0, "merge_pairs fed the ResidentDereps"
    finally:
        for d in tuple(rds) + tuple(nds):
            d.close()


def case_fused_keeps_nothing(dd):
    for rev in (None, SAM1R):
        with warnings.catch_warnings(record=True) as seen:
            warnings.simplefilter("always")
            counts, rd = dd.filter_and_sample(SAM1F, None, rev, None, trunc_len=1000 if rev is None else (240, 1000))
        assert counts == (1500, 0) and rd is None and any("No reads passed the filter" in str(w.message) for w in seen), (counts, rd)
    _raises(NotImplementedError, lambda: dd.filter_and_sample(SAM1F, None, orient_fwd="ACGT"), "orient_fwd is not supported by filter_and_sample")
    _raises(ValueError, lambda: dd.filter_and_sample([SAM1F, SAM1R], None), "one sample")
    _raises(TypeError, lambda: dd.filter_and_sample(SAM1F, None, no_such_argument=1), "no_such_argument")


def case_fused_n_passes(dd):
    """A filter with max_n > 0 lets an N through: the sample refuses it, on both routes alike, and the new route leaves no object."""
    from dada2_amd import api
    E = dd._lib.Dada2HipError
    rng = random.Random(1208)
    reads = pool_reads(rng, 10, 30, length=50)
    reads[4] = reads[4][:10] + "N" + reads[4][11:]
    with tempfile.TemporaryDirectory() as tmp:
        path, out = os.path.join(tmp, "with_n.fastq"), os.path.join(tmp, "kept.fastq.gz")
        from derep_dev_cases import write_fastq
        write_fastq(path, reads, with_quals(rng, reads, lo=45))       # (above truncQ's 2: no read is cut)
        counts, nd = dd.filter_and_derep(path, None, max_n=1)
        seen = []
        try:
            assert counts == (30, 30)
            api.Sample.from_native(nd)
        except E as e:
            seen.append(e)
        finally:
            nd.close()
        try:
            dd.filter_and_sample(path, out, max_n=1)
        except E as e:
            seen.append(e)
        assert len(seen) == 2 and str(seen[0]) == str(seen[1]) and seen[1].code == 1 and "only of A/C/G/T" in str(seen[1]), [str(e) for e in seen]
        assert not os.path.exists(out), "a failed call leaves no file"


FUSED_CASES = {"fused_single": case_fused_single, "fused_paired": case_fused_paired, "fused_keeps_nothing": case_fused_keeps_nothing,
               "fused_n_passes": case_fused_n_passes}
FUSED_NAMES = tuple(FUSED_CASES)


def emu_run(names=None, poison=None):
    """The emulator's job (tests/test_emu_derep_resident.py): the cases in their light form; with ``poison`` a byte, cases 1-3 on
    dirty memory instead."""
    from dada2_amd import dereplicate
    if poison is not None:
        run_poisoned(dereplicate, poison, light=True)
        return "ok poisoned 0x%02X" % poison
    names = names or CASE_NAMES
    for name in names:
        CASES[name](dereplicate, light=True)
    return "ok %d cases" % len(names)
