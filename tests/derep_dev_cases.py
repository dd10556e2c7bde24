"""The device dereplicator's cases (dada2_amd.dereplicate: dada2hip_derep_reads, dada2hip_filter_derep_fastq, _paired), run by the
CPU, emulator and GPU tests.

Checkers, both exact - sequences, abundances, map, maxlen, and the quality matrix bit for bit with NA where NA:
  * oracle.derep.derep_from_reads, the line-by-line restatement of R/sequenceIO.R:45-183;
  * the host's dada2hip_derep_fastq (api.derep_fastq) on a file of the same reads, itself pinned by tests/test_derep.py.
Auto is resolved for the oracle by the rule the issue states: a character below ';' anywhere in the FIRST chunk of n reads means
+33, else +64 (no quality character at all: 33).

A case takes the module dada2_amd.dereplicate and raises AssertionError; ``light`` is the emulator's form (smaller counts, the same
properties).  CASES are cases 1-9 of the issue (reads in memory); FUSED_CASES are 11-14 (files through the filter), the card's
alone, as is check_two_default_pieces (case 10)."""
import gzip
import os
import random
import tempfile
import warnings

import numpy as np

from primer_cases import _raises, with_env

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
SAM1F, SAM1R = (os.path.join(GOLDEN, n + ".fastq.gz") for n in ("sam1F", "sam1R"))
ONLY_EMPTY = "Only zero-length sequences detected during dereplication."


# ---- the comparison -------------------------------------------------------------------------------------------------------------------

def auto_offset(quals, n):
    m = min((c for q in quals[:n] for c in q), default=255)
    return 33 if m >= 255 or m < 59 else 64


def qbytes(quals):
    return [q if isinstance(q, bytes) else q.encode("latin-1") for q in quals]


def same(got, want, what=""):
    """Two Derep objects equal in every field; the quality matrices bit for bit (float.hex), NA where NA."""
    assert list(got.seqs) == list(want.seqs), (what, "sequences", list(got.seqs)[:4], list(want.seqs)[:4])
    assert np.array_equal(np.asarray(got.abundances), np.asarray(want.abundances)), (what, "abundances")
    gm, wm = np.asarray(got.map), np.asarray(want.map)
    assert gm.shape == wm.shape and np.array_equal(gm, wm), (what, "map", gm[:12], wm[:12])
    gq, wq = np.ascontiguousarray(got.quals, dtype=np.float64), np.ascontiguousarray(want.quals, dtype=np.float64)
    assert gq.shape == wq.shape, (what, "maxlen", gq.shape, wq.shape)
    gn, wn = np.isnan(gq), np.isnan(wq)
    assert np.array_equal(gn, wn), (what, "NA positions", np.argwhere(gn != wn)[:4])
    bad = np.argwhere((gq.view(np.uint64) != wq.view(np.uint64)) & ~wn)
    assert bad.size == 0, (what, "quality", bad[0].tolist(), float(gq[tuple(bad[0])]).hex(), float(wq[tuple(bad[0])]).hex())


def write_fastq(path, seqs, quals, gz=False):
    text = b"".join(b"@r%d\n%s\n+\n%s\n" % (i, s.encode("latin-1"), q) for i, (s, q) in enumerate(zip(seqs, qbytes(quals))))
    with open(path, "wb") as fh:
        fh.write(gzip.compress(text) if gz else text)


def check(dd, seqs, quals, n=10 ** 6, qual_offset=0, what="", stats=None, env=None, host=True):
    """derep_reads against the oracle and, with ``host``, against the host dereplicator on a file of the reads."""
    from oracle.derep import derep_from_reads
    from dada2_amd import api
    quals = qbytes(quals)
    nd = with_env(env, lambda: dd.derep_reads(seqs, quals, n=n, qual_offset=qual_offset, stats=stats))
    try:
        got = nd.to_derep()
        assert (nd.nuniques, nd.nreads, nd.maxlen) == (len(got.seqs), len(seqs), got.quals.shape[1]), what
    finally:
        nd.close()
    off = qual_offset or auto_offset(quals, n)
    same(got, derep_from_reads(seqs, quals, n, off), (what, "oracle"))
    if host:
        with tempfile.TemporaryDirectory() as tmp:
            path = os.path.join(tmp, "reads.fastq")
            write_fastq(path, seqs, quals)
            same(got, api.derep_fastq(path, n, qual_offset), (what, "host derep_fastq"))
    return got


def rand_seq(rng, n, letters="ACGT"):
    return "".join(rng.choice(letters) for _ in range(n))


def rand_qual(rng, n, lo=35, hi=73):
    return bytes(rng.randint(lo, hi) for _ in range(n))


def with_quals(rng, seqs, **kw):
    return [rand_qual(rng, len(s), **kw) for s in seqs]


def pool_reads(rng, ndistinct, nreads, length=60):
    """nreads reads over ndistinct sequences, every one at least once, some often."""
    pool = []
    while len(pool) < ndistinct:
        s = rand_seq(rng, length if not callable(length) else length())
        if s not in pool:
            pool.append(s)
    seqs = pool + [pool[min(int(rng.expovariate(3.0 / ndistinct)), ndistinct - 1)] for _ in range(nreads - ndistinct)]
    rng.shuffle(seqs)
    return seqs


# ---- cases 1-9: reads in memory ---------------------------------------------------------------------------------------------------------

def case_prefixes_and_ends(dd, light=False):
    rng = random.Random(901)
    a, b = rand_seq(rng, 250), rand_seq(rng, 250)
    seqs = ["ACGTACG", "ACGTACGT", "ACGTACGTA", "ACGTACGT", a[:-1] + "A", a[:-1] + "C", "A" + b[1:], "C" + b[1:], a[:-1] + "A"]
    got = check(dd, seqs, with_quals(rng, seqs), what="prefixes, first and last base")
    assert len(got.seqs) == 7 and got.quals.shape[1] == 250 and np.isnan(got.quals[got.seqs.index("ACGTACG"), 7:]).all()
    seqs = [rand_seq(rng, n) for n in (1, 63, 64, 65, 256, 257, 4500, 64, 1)]
    seqs[7], seqs[8] = seqs[2], seqs[0]
    got = check(dd, seqs, with_quals(rng, seqs), what="lengths 1 .. 4 500")
    assert got.quals.shape == (7, 4500) and not np.isnan(got.quals[got.seqs.index(seqs[6])]).any()


def case_letters(dd, light=False):
    rng = random.Random(902)
    seqs = ["ACGN", "acgt", "ACGT", "ACGT", "acgt", "ACGN", "RYKM", "ACGT"]
    got = check(dd, seqs, with_quals(rng, seqs), what="N, IUPAC and lower case are letters")
    assert sorted(got.seqs) == sorted({"ACGN", "acgt", "ACGT", "RYKM"}) and got.seqs[0] == "ACGT"


def case_zero_length(dd, light=False):
    rng = random.Random(903)
    seqs = ["", "ACGTAC", "", "TTGCA", "ACGTAC", "", ""]
    for n in (10 ** 6, 2):
        got = check(dd, seqs, with_quals(rng, seqs), n=n, what="zero-length reads, n = %d" % n)
        assert got.map.tolist() == [-1, 0, -1, 1, 0, -1, -1]
    E = dd._lib.Dada2HipError
    _raises(E, lambda: dd.derep_reads(["", "", ""], [b"", b"", b""]), ONLY_EMPTY, code=1)
    _raises(E, lambda: dd.derep_reads([], []), ONLY_EMPTY, code=1)
    _raises(E, lambda: dd.derep_reads(["ACGT"], [b"IIII"], qual_offset=50), "offset", code=1)
    _raises(ValueError, lambda: dd.derep_reads(["ACGT"], [b"III"]), "as many quality characters")


def case_order(dd, light=False):
    rng = random.Random(904)
    A, B, Cc = "AAGT" * 5, "CAGT" * 5, "GAGT" * 5
    seqs = [Cc, A, B, A, Cc, B]
    for n, order in ((1, [Cc, A, B]), (2, [A, Cc, B]), (6, [A, B, Cc])):
        got = check(dd, seqs, with_quals(rng, seqs), n=n, what="C A B A C B, n = %d" % n)
        assert got.seqs == order and got.abundances.tolist() == [2, 2, 2], (n, got.seqs)
    seqs = pool_reads(rng, 40, 150, length=lambda: rng.randint(20, 70))
    quals = with_quals(rng, seqs)
    for n in (3, 7):
        check(dd, seqs, quals, n=n, what="40 distinct reads, n = %d" % n)


def case_auto(dd, light=False):
    rng = random.Random(905)
    seqs = pool_reads(rng, 12, 40, length=30)
    hi = with_quals(rng, seqs, lo=64, hi=104)
    low_first = list(hi)
    low_first[3] = low_first[3][:10] + b"5" + low_first[3][11:]
    low_second = list(hi)
    low_second[17] = low_second[17][:10] + b"5" + low_second[17][11:]
    a = check(dd, seqs, low_first, n=8, what="a character below ';' in the first chunk")
    b = check(dd, seqs, low_second, n=8, what="... in the second chunk only")
    assert np.nanmin(a.quals) >= 20 and np.nanmax(b.quals) <= 40   # judged +33 and +64: the letters are '5' and '@'..'h'
    check(dd, seqs, low_second, n=20, what="... which a larger n makes the first")
    check(dd, seqs, hi, n=8, qual_offset=33, what="offset 33 given")
    check(dd, seqs, low_first, n=8, qual_offset=64, what="offset 64 given")


def case_contention(dd, light=False):
    rng = random.Random(906)
    s = rand_seq(rng, 250)
    n = 300 if light else 5000
    st = {}
    got = check(dd, [s] * n, [rand_qual(rng, 250, 33, 74) for _ in range(n)], what="one unique, every sum hit by every read", stats=st)
    assert got.abundances.tolist() == [n] and st["uniques"] == 1 and st["reads_in"] == n, st


def case_growth(dd, light=False):
    rng = random.Random(907)
    n = 300 if light else 3000
    seqs = pool_reads(rng, n, n + n // 3, length=lambda: rng.randint(30, 50))
    quals = with_quals(rng, seqs)
    st = {}
    check(dd, seqs, quals, what="from a table of 8 slots", stats=st, env={"DADA2HIP_DEREP_TABLE": 8}, host=not light)
    assert st["rebuilds"] > 0 and st["uniques"] == n and st["table_capacity"] >= 2 * n, st
    st = {}                                                         # pieces of 64: the rebuilds move uniques that are already in
    check(dd, seqs, quals, what="... in pieces of 64", stats=st, env={"DADA2HIP_DEREP_TABLE": 8, "DADA2HIP_DEREP_PIECE": 64}, host=False)
    assert st["rebuilds"] >= (1 if light else 3) and st["pieces"] == (len(seqs) + 63) // 64 and st["table_capacity"] >= 2 * n, st


def case_collisions(dd, light=False):
    rng = random.Random(908)
    seqs = pool_reads(rng, 40, 130, length=lambda: rng.randint(20, 70))
    quals = with_quals(rng, seqs)
    base = check(dd, seqs, quals, n=50, what="40 distinct reads")
    for bits in (0, 2):
        for extra in ({}, {"DADA2HIP_DEREP_PIECE": 7, "DADA2HIP_DEREP_TABLE": 8}):
            st = {}
            got = check(dd, seqs, quals, n=50, what="hash of %d bits %s" % (bits, extra), stats=st,
                        env=dict(extra, DADA2HIP_DEREP_HASH_BITS=bits), host=False)
            same(got, base, "collisions change nothing")
            assert st["collision_rounds"] > 0 and st["uniques"] == 40, st
    st = {}
    check(dd, seqs, quals, n=50, what="the whole hash", stats=st, host=False)
    assert st["collision_rounds"] == 0, st


def case_pieces(dd, light=False):
    rng = random.Random(909)
    for total in (65, 257):
        first = rand_seq(rng, 40)
        seqs = pool_reads(rng, total // 5, total - 1, length=lambda: rng.randint(30, 60))
        seqs = [first] + [s for s in seqs]                         # read 1's unique comes again in every later stretch of the call
        for at in range(9, total, 9):
            seqs[at] = first
        quals = with_quals(rng, seqs)
        base = check(dd, seqs, quals, n=100, what="%d reads, one piece" % total)
        for env in ({"DADA2HIP_DEREP_PIECE": 1}, {"DADA2HIP_DEREP_PIECE": 3}, {"DADA2HIP_DEREP_PIECE": 64},
                    {"DADA2HIP_DEREP_PIECE_BYTES": 200}):
            if light and total == 257 and env.get("DADA2HIP_DEREP_PIECE") == 1:
                continue
            st = {}
            got = check(dd, seqs, quals, n=100, what="%d reads, %s" % (total, env), stats=st, env=env, host=False)
            same(got, base, "pieces change nothing")
            want = {1: total, 3: (total + 2) // 3, 64: (total + 63) // 64}.get(env.get("DADA2HIP_DEREP_PIECE"))
            assert st["pieces"] == want if want else st["pieces"] > total // 6, (env, st)


CASES = {"prefixes_and_ends": case_prefixes_and_ends, "letters": case_letters, "zero_length": case_zero_length, "order": case_order,
         "auto": case_auto, "contention": case_contention, "growth": case_growth, "collisions": case_collisions, "pieces": case_pieces}
CASE_NAMES = tuple(CASES)


# ---- case 10: more than one default piece (the card's alone) ------------------------------------------------------------------------------

def check_two_default_pieces(dd):
    """70 000 reads x 100 nt over 2 000 uniques from dada2_amd.synth: two pieces of 65 536 reads at the most."""
    from dada2_amd import synth
    rng = np.random.default_rng(910)
    codes, _ = synth.true_variants(rng, 2000, 100)
    pool = ["".join("ACGT"[c] for c in row) for row in np.asarray(codes)]
    assert len(set(pool)) > 1900
    idx = np.minimum(rng.zipf(1.3, size=70000) - 1, len(pool) - 1)
    seqs = [pool[i] for i in idx]
    quals = [bytes(row) for row in rng.integers(35, 74, size=(70000, 100), dtype=np.uint8)]
    st = {}
    check(dd, seqs, quals, n=30000, what="70 000 reads", stats=st)
    assert st["pieces"] == 2 and st["reads_in"] == 70000 and st["uniques"] == len(set(seqs)), st
    return st


# ---- cases 11-14: through the filter (the card's alone) -----------------------------------------------------------------------------------

FILTER = dict(trunc_len=240, max_ee=2)


def native(nd):
    try:
        return nd.to_derep()
    finally:
        nd.close()


def case_fused_single(dd):
    from dada2_amd import api
    with tempfile.TemporaryDirectory() as tmp:
        two = os.path.join(tmp, "two_step.fastq.gz")
        counts, _ = api.filter_and_trim(SAM1F, two, **FILTER)
        assert 0 < counts[0, 1] < counts[0, 0] == 1500
        for n_derep in (10 ** 6, 400):
            want = api.derep_fastq(two, n_derep)
            for env in ({}, {"DADA2HIP_FILTER_PIECE": 300}):
                st = {}
                got_counts, nd = with_env(env, lambda: dd.filter_and_derep(SAM1F, None, n_derep=n_derep, stats=st, **FILTER))
                assert got_counts == (int(counts[0, 0]), int(counts[0, 1])) and nd.nreads == counts[0, 1], (got_counts, counts)
                same(native(nd), want, ("no file", n_derep, env))
                assert st["derep_reads_in"] == counts[0, 1] and st["derep_uniques"] == len(want.seqs) and st["reads_kept"] == counts[0, 1], st
                assert st["derep_pieces"] == (1 if not env else 5) and st["write_us"] == 0 and st["deflate_us"] == 0, st
                for compress in (True, False):
                    out = os.path.join(tmp, "fused_%d_%d.fastq" % (n_derep, compress) + (".gz" if compress else ""))
                    got_counts, nd = with_env(env, lambda: dd.filter_and_derep(SAM1F, out, n_derep=n_derep, compress=compress, **FILTER))
                    assert got_counts == (int(counts[0, 0]), int(counts[0, 1]))
                    same(native(nd), want, ("with a file", n_derep, compress, env))
                    same(api.derep_fastq(out, n_derep), want, "the file written beside the derep")
                    ref = os.path.join(tmp, "ref" + os.path.basename(out))
                    api.filter_and_trim(SAM1F, ref, compress=compress, **FILTER)
                    with open(out, "rb") as a, open(ref, "rb") as b:
                        assert a.read() == b.read(), ("the file is filter_and_trim's byte for byte", compress)
        # the filter's chunks smaller than the derep's, and the complexity rule, whose verdict is the host's
        counts, _ = api.filter_and_trim(SAM1F, two, n=256, rm_lowcomplex=10, **FILTER)
        got_counts, nd = dd.filter_and_derep(SAM1F, None, n=256, n_derep=400, rm_lowcomplex=10, **FILTER)
        assert got_counts == (1500, int(counts[0, 1])) and 0 < got_counts[1] < 1500
        same(native(nd), api.derep_fastq(two, 400), "chunks of 256, rm_lowcomplex")


def case_fused_paired(dd):
    from dada2_amd import api
    from helpers import tperr1
    args = dict(trunc_len=(240, 200), max_ee=2)
    with tempfile.TemporaryDirectory() as tmp:
        two = [os.path.join(tmp, "two_%s.fastq.gz" % d) for d in "FR"]
        counts, _ = api.filter_and_trim(SAM1F, two[0], SAM1R, two[1], **args)
        want = [api.derep_fastq(p, 400) for p in two]
        outs = [os.path.join(tmp, "fused_%s.fastq.gz" % d) for d in "FR"]
        for filt in (None, outs):
            got_counts, nds = dd.filter_and_derep(SAM1F, filt and filt[0], SAM1R, filt and filt[1], n_derep=400, **args)
            assert got_counts == (int(counts[0, 0]), int(counts[0, 1])) and 0 < got_counts[1] < 1500
            got = [native(nd) for nd in nds]
            assert len(got[0].map) == len(got[1].map) == got_counts[1]
            for g, w, d in zip(got, want, "FR"):
                same(g, w, ("paired", d, filt is not None))
        for o, t in zip(outs, two):
            with open(o, "rb") as a, open(t, "rb") as b:
                assert a.read() == b.read(), "the paired files are filter_and_trim's byte for byte"
        err = tperr1()
        rows = []
        for pair in (got, want):
            res = [api.dada(d, err)[0] for d in pair]
            rows.append(api.merge_pairs(res[0], pair[0], res[1], pair[1], return_rejects=True))
        assert rows[0] == rows[1] and sum(r["abundance"] for r in rows[0] if r["accept"]) > 0, (len(rows[0]), len(rows[1]))


def case_fused_keeps_nothing(dd):
    with tempfile.TemporaryDirectory() as tmp:
        for filt in (None, os.path.join(tmp, "none.fastq.gz")):
            with warnings.catch_warnings(record=True) as seen:
                warnings.simplefilter("always")
                counts, nd = dd.filter_and_derep(SAM1F, filt, trunc_len=1000)
            assert counts == (1500, 0) and nd is None and any("No reads passed the filter" in str(w.message) for w in seen), (counts, nd)
            assert filt is None or not os.path.exists(filt)
        with warnings.catch_warnings(record=True) as seen:
            warnings.simplefilter("always")
            counts, nd = dd.filter_and_derep(SAM1F, None, SAM1R, None, trunc_len=(240, 1000))
        assert counts == (1500, 0) and nd is None and len(seen) >= 1


def case_fused_refusals(dd):
    _raises(NotImplementedError, lambda: dd.filter_and_derep(SAM1F, None, orient_fwd="ACGT"), "orient_fwd is not supported by filter_and_derep")
    _raises(NotImplementedError, lambda: dd.filter_and_derep(SAM1F, None, SAM1R, None, match_ids=True), "match_ids is not supported")
    _raises(ValueError, lambda: dd.filter_and_derep([SAM1F, SAM1R], None), "one sample")
    _raises(ValueError, lambda: dd.filter_and_derep(os.path.join(GOLDEN, "missing.fastq")), "do not exist")
    _raises(TypeError, lambda: dd.filter_and_derep(SAM1F, None, no_such_argument=1), "no_such_argument")


FUSED_CASES = {"fused_single": case_fused_single, "fused_paired": case_fused_paired, "fused_keeps_nothing": case_fused_keeps_nothing,
               "fused_refusals": case_fused_refusals}
FUSED_NAMES = tuple(FUSED_CASES)


def emu_run(names=None):
    """The emulator's job (tests/test_emu_derep_dev.py): cases 1-9 in their lighter form."""
    from dada2_amd import dereplicate
    names = names or CASE_NAMES
    for name in names:
        CASES[name](dereplicate, light=True)
    return "ok %d cases" % len(names)
