"""mergeSequenceTables: the specification, twice, and the cases the CPU, emulator and GPU tests share.

``spec_merge`` restates R/multiSample.R:290-364 (validation :206-238, the in-table collapse :106-115) line for line in plain
Python, with the stated deviations: a table that holds a column or a row name twice, or that is empty, is refused; a merged cell
above INT32_MAX is refused; with tryRC every letter must be one of ACGTMRWSYKVHDBN.  It keeps the quadratic prefix test of :334 as
written.  ``spec_merge_fast`` is the same with dicts, for the larger cases.  Both return ``(mat, seqs, sample_names, col_map)`` -
col_map[c] the 0-based column of the result that input column c (table after table) went to - or raise SpecError(code).

A case takes the module dada2_amd.seqtables and raises AssertionError; ``light`` is the emulator's form (smaller counts, the same
properties).  Every comparison is exact: the matrix with its dtype and layout, the sequences, the sample names, the column map."""
import random

import numpy as np

from primer_cases import with_env

INT32_MAX = 2 ** 31 - 1
_COMP = str.maketrans("ACGTMRWSYKVHDBN", "TGCAKYWSRMBDHVN")   # Biostrings' complement of the IUPAC codes
_LETTERS = set("ACGTMRWSYKVHDBN")
STAT_WORDS = ("tables", "input_columns", "distinct_sequences", "flagged_sequences", "output_rows", "output_columns", "table_capacity",
              "rebuilds", "collision_rounds", "rc_failed_compares", "pieces", "upload_bytes", "download_bytes", "upload_us", "identity_us",
              "rc_lookup_us", "accumulate_us", "download_us", "total_us")


def rc(s):
    return s.translate(_COMP)[::-1]


class SpecError(Exception):
    def __init__(self, code, msg):
        super().__init__(msg)
        self.code = code


def _unique(xs):
    return list(dict.fromkeys(xs))


# ---- the specification ----------------------------------------------------------------------------------------------------------------

def _validated(tables, order_by):
    if order_by not in (None, "abundance", "nsamples"):
        raise SpecError(1, 'order_by must be "abundance", "nsamples" or None')
    if not isinstance(tables, (list, tuple)) or len(tables) < 2:                       # :310
        raise SpecError(1, "At least two sequence tables are expected")
    tabs = []
    for i, (mat, seqs, names) in enumerate(tables):                                    # is.sequence.table, :206-238
        m = np.asarray(mat)
        if m.ndim != 2:
            raise SpecError(1, "Not a matrix (sequence table %d)." % (i + 1))
        if m.shape != (len(names), len(seqs)):
            raise SpecError(1, "Sequence table %d: the cells do not fit the names." % (i + 1))
        tabs.append((m.astype(np.int64), [str(s) for s in seqs], [str(n) for n in names]))
    for i, (m, seqs, names) in enumerate(tabs):
        if m.shape[0] == 0 or m.shape[1] == 0:
            raise SpecError(1, "sequence table %d is empty" % (i + 1))
    for what, k in (("column (sequence)", 1), ("row (sample)", 2)):
        for i, t in enumerate(tabs):
            if not all(len(s) > 0 for s in t[k]):
                raise SpecError(1, "Some %s names are blank (sequence table %d)." % (what, i + 1))
    for i, (m, seqs, names) in enumerate(tabs):
        if not (m >= 0).all():
            raise SpecError(1, "Negative entries (sequence table %d)." % (i + 1))
    for i, (m, seqs, names) in enumerate(tabs):
        if len(set(names)) != len(names):                                              # (the reference warns, :234)
            raise SpecError(1, "Duplicated row (sample) names in sequence table %d" % (i + 1))
    return tabs


def _check_letters(tabs):
    for i, (m, seqs, names) in enumerate(tabs):
        for j, s in enumerate(seqs):
            if not set(s) <= _LETTERS:
                raise SpecError(4, "tryRC takes the upper-case letters ACGTMRWSYKVHDBN only: table %d, column %d (%s)." % (i + 1, j + 1, s[:60]))


def _finish(tabs, sample_names, seqs, renamed, order_by):
    """:349-362 on tables whose flagged columns have been renamed; ``renamed``: {flagged sequence: its reverse complement}."""
    row = {n: i for i, n in enumerate(sample_names)}
    col = {s: i for i, s in enumerate(seqs)}
    rval = np.zeros((len(sample_names), len(seqs)), dtype=np.int64)
    for m, cols, names in tabs:
        ri = np.array([row[n] for n in names])
        ci = np.array([col[s] for s in cols])
        np.add.at(rval, (ri[:, None], ci[None, :]), m)                                # rval[rownames(tab), colnames(tab)] += tab
    if rval.size and rval.max() > INT32_MAX:
        raise SpecError(1, "a merged cell of the sequence tables exceeds the integer range (NA in the reference)")
    if order_by == "abundance":
        o = np.argsort(-rval.sum(axis=0), kind="stable")
    elif order_by == "nsamples":
        o = np.argsort(-(rval > 0).sum(axis=0), kind="stable")
    else:
        o = np.arange(len(seqs))
    place = {seqs[int(k)]: p for p, k in enumerate(o)}
    return np.ascontiguousarray(rval[:, o].astype(np.int32)), [seqs[int(k)] for k in o], list(sample_names), place


def _dup_columns(tabs):
    for i, (m, seqs, names) in enumerate(tabs):
        if len(set(seqs)) != len(seqs):                                                # (the reference warns, :231)
            raise SpecError(1, "Duplicated column (sequences) names in sequence table %d" % (i + 1))


def spec_merge(tables, repeats="error", order_by="abundance", try_rc=False):
    tabs = _validated(tables, order_by)
    sample_names = [n for t in tabs for n in t[2]]                                     # :321
    dup = [n for i, n in enumerate(sample_names) if n in sample_names[:i]]            # duplicated()
    if dup:
        if repeats == "error":
            raise SpecError(1, "Duplicated sample names detected in the sequence table row names: " + ", ".join(_unique(dup)))
        sample_names = _unique(sample_names)
    _dup_columns(tabs)
    original = [s for t in tabs for s in t[1]]
    seqs = _unique(original)                                                           # :332
    renamed = {}
    if try_rc and len(seqs) > 1:                                                       # :333
        _check_letters(tabs)
        earlier_rc = [False] + [rc(seqs[i]) in seqs[:i] for i in range(1, len(seqs))]  # :334, the growing prefix as written
        rc_seqs = [s for s, f in zip(seqs, earlier_rc) if f]
        if rc_seqs:
            for k, (m, cols, names) in enumerate(tabs):
                do_rc = [c in rc_seqs for c in cols]
                if any(do_rc):
                    cols = [rc(c) if f else c for c, f in zip(cols, do_rc)]            # :341
                    dupes = [c in cols[:j] for j, c in enumerate(cols)]               # collapseNoMismatch(identicalOnly=TRUE), :106-115
                    keep = [j for j, d in enumerate(dupes) if not d]
                    st = m[:, keep].copy()
                    kept_cols = [cols[j] for j in keep]
                    for j, d in enumerate(dupes):
                        if d:
                            st[:, kept_cols.index(cols[j])] += m[:, j]
                    tabs[k] = (st, kept_cols, names)
            renamed = {s: rc(s) for s in rc_seqs}
            seqs = [s for s in seqs if s not in rc_seqs]                               # :345
    mat, out_seqs, out_names, place = _finish(tabs, sample_names, seqs, renamed, order_by)
    col_map = np.array([place[renamed.get(s, s)] for s in original], dtype=np.int32)
    return mat, out_seqs, out_names, col_map


def spec_merge_fast(tables, repeats="error", order_by="abundance", try_rc=False):
    tabs = _validated(tables, order_by)
    sample_names = [n for t in tabs for n in t[2]]
    seen, dup = set(), []
    for n in sample_names:
        if n in seen:
            dup.append(n)
        seen.add(n)
    if dup:
        if repeats == "error":
            raise SpecError(1, "Duplicated sample names detected in the sequence table row names: " + ", ".join(_unique(dup)))
        sample_names = _unique(sample_names)
    _dup_columns(tabs)
    original = [s for t in tabs for s in t[1]]
    seqs = _unique(original)
    renamed = {}
    if try_rc and len(seqs) > 1:
        _check_letters(tabs)
        at = {s: i for i, s in enumerate(seqs)}
        for i, s in enumerate(seqs):
            r = rc(s)
            if at.get(r, i) < i:
                renamed[s] = r
        if renamed:
            for k, (m, cols, names) in enumerate(tabs):
                if any(c in renamed for c in cols):
                    cols = [renamed.get(c, c) for c in cols]
                    first = {}
                    for j, c in enumerate(cols):
                        first.setdefault(c, len(first))
                    st = np.zeros((m.shape[0], len(first)), dtype=np.int64)
                    np.add.at(st, (slice(None), np.array([first[c] for c in cols])), m)
                    tabs[k] = (st, list(first), names)
            seqs = [s for s in seqs if s not in renamed]
    mat, out_seqs, out_names, place = _finish(tabs, sample_names, seqs, renamed, order_by)
    col_map = np.array([place[renamed.get(s, s)] for s in original], dtype=np.int32)
    return mat, out_seqs, out_names, col_map


# ---- the comparison ---------------------------------------------------------------------------------------------------------------------

def same(got, want, what=""):
    gm, gs, gn, gc = got
    wm, ws, wn, wc = want
    assert list(gn) == list(wn), (what, "sample names", gn[:6], wn[:6])
    assert list(gs) == list(ws), (what, "sequences", len(gs), len(ws), [s[:12] for s in gs[:6]], [s[:12] for s in ws[:6]])
    gm = np.asarray(gm)
    assert gm.dtype == np.int32 and gm.flags["C_CONTIGUOUS"] and gm.shape == wm.shape, (what, gm.dtype, gm.shape, wm.shape)
    assert np.array_equal(gm, wm), (what, "cells", np.argwhere(gm != wm)[:4].tolist())
    assert np.array_equal(np.asarray(gc), wc), (what, "column map", np.flatnonzero(np.asarray(gc) != wc)[:6].tolist())


def merged(st, tables, env=None, stats=None, **kw):
    s = {} if stats is None else stats
    mat, seqs, names = with_env(env, lambda: st.merge_sequence_tables(tables, stats=s, **kw))
    return mat, seqs, names, s["col_map"]


def check(st, tables, what="", spec=spec_merge, env=None, stats=None, **kw):
    got = merged(st, tables, env=env, stats=stats, **kw)
    same(got, spec(tables, **kw), (what, kw))
    return got


def check_all(st, tables, what="", spec=spec_merge, repeats="error"):
    """both values of try_rc, every order_by"""
    for try_rc in (False, True):
        for order_by in ("abundance", "nsamples", None):
            check(st, tables, what, spec=spec, try_rc=try_rc, order_by=order_by, repeats=repeats)


def refused(st, tables, code, text, spec=spec_merge, **kw):
    """the module and the specification both refuse, with this code (a ValueError of the module counts as an input error)"""
    try:
        spec(tables, **kw)
    except SpecError as e:
        assert e.code == code and text in str(e), ("specification", e.code, str(e))
    else:
        raise AssertionError("the specification did not refuse: " + text)
    try:
        st.merge_sequence_tables(tables, **kw)
    except ValueError as e:
        assert code == 1 and text in str(e), str(e)
    except st._lib.Dada2HipError as e:
        assert e.code == code and text in str(e), (e.code, str(e))
    else:
        raise AssertionError("not refused: " + text)


def rand_seq(rng, n, letters="ACGT"):
    return "".join(rng.choice(letters) for _ in range(n))


def table(rows, cols, cells):
    return np.array(cells, dtype=np.int32).reshape(len(rows), len(cols)), list(cols), list(rows)


def rand_table(rng, rows, cols, hi=50, zero=0.5):
    cells = [[0 if rng.random() < zero else rng.randint(1, hi) for _ in cols] for _ in rows]
    return table(rows, cols, cells)


WORKED = (table(["a", "b"], ["AAC", "GGT"], [[5, 1], [0, 2]]), table(["c"], ["GTT", "ACC", "AAC"], [[3, 4, 7]]))


# ---- the cases ----------------------------------------------------------------------------------------------------------------------------

def case_worked_example(st, light=False):
    mat, seqs, names, cmap = merged(st, WORKED, try_rc=False)
    assert seqs == ["AAC", "ACC", "GGT", "GTT"] and names == ["a", "b", "c"], (seqs, names)
    assert mat.tolist() == [[5, 0, 1, 0], [0, 0, 2, 0], [7, 4, 0, 3]] and cmap.tolist() == [0, 2, 3, 1, 0], (mat, cmap)
    mat, seqs, names, cmap = merged(st, WORKED, try_rc=True)
    assert seqs == ["AAC", "GGT"] and names == ["a", "b", "c"] and mat.tolist() == [[5, 1], [0, 2], [10, 4]], (seqs, names, mat)
    assert cmap.tolist() == [0, 1, 0, 1, 0] and mat.dtype == np.int32 and mat.flags["C_CONTIGUOUS"], cmap
    check_all(st, WORKED, "the worked example")


def case_lengths(st, light=False):
    rng = random.Random(1101)
    fwd = ["A", "AC"] + [rand_seq(rng, n) for n in (63, 64, 65, 127, 128, 129, 250, 1500)]
    assert all(rc(s) != s for s in fwd)
    half = rand_seq(rng, 32)
    pal4, pal64 = "ACGT", half + rc(half)
    assert rc(pal4) == pal4 and rc(pal64) == pal64
    a, c = rand_seq(rng, 250), rand_seq(rng, 250)
    flip = {"A": "C", "C": "G", "G": "T", "T": "A"}
    b = flip[rc(a)[0]] + rc(a)[1:]                                 # b is a's reverse complement but for its first base
    d = rc(c)[:-1] + flip[rc(c)[-1]]                               # d is c's but for its last base
    t1 = rand_table(rng, ["s1", "s2", "s3"], fwd + [pal4, pal64, a, c], zero=0.2)
    t2 = rand_table(rng, ["s4", "s5"], [rc(s) for s in reversed(fwd)] + [pal64, b, d, pal4], zero=0.2)
    check_all(st, (t1, t2), "lengths 1 .. 1 500, palindromes, first and last base")
    stt = {}
    mat, seqs, names, cmap = check(st, (t1, t2), "flags", stats=stt, try_rc=True, order_by=None)
    assert seqs == t1[1] + [b, d], seqs
    if "tables" in stt:                                            # (the library's counters: not where the case is served otherwise)
        assert stt["flagged_sequences"] == len(fwd) and stt["distinct_sequences"] == 2 * len(fwd) + 6, stt
    assert cmap[len(t1[1]):len(t1[1]) + len(fwd)].tolist() == list(range(len(fwd) - 1, -1, -1))


def case_in_table_collapse(st, light=False):
    rng = random.Random(1102)
    s, x, y = rand_seq(rng, 70), rand_seq(rng, 70), rand_seq(rng, 33)
    t1 = table(["a", "b"], [x, s], [[3, 5], [0, 7]])
    t2 = table(["c", "d"], [s, y, rc(s)], [[1, 2, 4], [8, 0, 16]])
    t3 = table(["e"], [rc(s), rc(x), s, rc(y)], [[32, 1, 64, 9]])
    check_all(st, (t1, t2, t3), "s and rc(s) in one table, in both orders")
    mat, seqs, names, cmap = merged(st, (t1, t2, t3), try_rc=True, order_by=None)
    assert seqs == [x, s, y] and mat[:, 1].tolist() == [5, 7, 5, 24, 96] and cmap.tolist() == [0, 1, 1, 2, 1, 1, 0, 1, 2], (mat, cmap)
    # the order of the tables decides which orientation survives
    mat, seqs, names, cmap = check(st, (t3, t1), "rc(s) first", try_rc=True, order_by=None)
    assert seqs == [rc(s), rc(x)] + [rc(y)], seqs


def case_contention(st, light=False):
    rng = random.Random(1103)
    s = rand_seq(rng, 120)
    tabs = [table(["x"], [s, rc(s)] if k % 2 == 0 else [rc(s), s], [[10 ** k, 3 * 10 ** k]]) for k in range(4)]
    mat, seqs, names, cmap = check(st, tabs, "eight adds into one cell", repeats="sum", try_rc=True)
    assert mat.tolist() == [[4 * 1111]] and seqs == [s] and names == ["x"] and cmap.tolist() == [0] * 8
    check_all(st, tabs, "one sample name in four tables", repeats="sum")
    refused(st, tabs, 1, "row names: x", repeats="error")


def case_order(st, light=False):
    s = ["ACGTA", "CCGTA", "GCGTA", "TCGTA", "AAGTA", "CAGTA"]
    # sums 6 6 9 6 1 9, positive cells 2 1 1 3 1 1: ties in both keys
    t1 = table(["a", "b"], s[:4], [[3, 6, 0, 2], [0, 0, 9, 2]])
    t2 = table(["c"], [s[4], s[0], s[3], s[5]], [[1, 3, 2, 9]])
    for ob, want in (("abundance", [2, 5, 0, 1, 3, 4]), ("nsamples", [3, 0, 1, 2, 4, 5]), (None, [0, 1, 2, 3, 4, 5])):
        mat, seqs, names, cmap = check(st, (t1, t2), "ties", order_by=ob)
        assert seqs == [s[k] for k in want], (ob, seqs)
    refused(st, (t1, t2), 1, "order_by", order_by="samples")


def case_iupac(st, light=False):
    q = ["ACNRVT", "GGKMHD", "WSWSAC"]
    t1 = table(["a"], q, [[1, 2, 3]])
    t2 = table(["b", "c"], [rc(q[1]), "NNNN", rc(q[0]), rc(q[2])], [[4, 5, 6, 7], [0, 1, 0, 1]])
    assert rc(q[0]) == "ABYNGT" and rc("NNNN") == "NNNN"
    check_all(st, (t1, t2), "N, R/Y, V/B, K/M, H/D, W, S")
    mat, seqs, names, cmap = merged(st, (t1, t2), try_rc=True, order_by=None)
    assert seqs == q + ["NNNN"] and cmap.tolist() == [0, 1, 2, 1, 3, 0, 2], (seqs, cmap)
    for bad in ("ACgT", "AC-GT", "AC+GT", "AC.GT"):
        t3 = table(["d"], ["ACGT", bad, "GGGA"], [[1, 1, 1]])
        refused(st, (t1, t2, t3), 4, "table 3, column 2", try_rc=True)
        check(st, (t1, t2, t3), "bytes without tryRC", try_rc=False)
    one = table(["a"], ["acgt"], [[1]]), table(["b"], ["acgt"], [[2]])
    check(st, one, "one distinct sequence: tryRC does nothing", try_rc=True)


def case_overflow(st, light=False):
    s, x = "ACGTTGCAAC", "CCGTTGCAAC"
    t1 = table(["a", "b"], [s, x], [[INT32_MAX, 1], [1, 1]])
    t2 = table(["a"], [x, s], [[1, 1]])
    refused(st, (t1, t2), 1, "integer range", repeats="sum")
    t2 = table(["a"], [rc(s), x], [[1, 1]])
    check(st, (t1, t2), "no overflow without tryRC", repeats="sum", try_rc=False)
    refused(st, (t1, t2), 1, "integer range", repeats="sum", try_rc=True)
    # every cell in range, the column sum past 2^31: ordered by the 64-bit sum
    t1 = table(["a", "b"], [s, x], [[1, INT32_MAX - 5], [INT32_MAX, 3]])
    t2 = table(["c", "d"], [x, s], [[INT32_MAX, INT32_MAX], [INT32_MAX, 7]])
    mat, seqs, names, cmap = check(st, (t1, t2), "column sums of 64 bits", order_by="abundance")
    assert seqs == [x, s] and int(mat[:, 0].astype(np.int64).sum()) == 3 * INT32_MAX - 2


def case_validation(st, light=False):
    ok = table(["a", "b"], ["ACG", "CCG"], [[1, 2], [3, 4]])
    ok2 = table(["c"], ["ACG", "TTG"], [[5, 6]])
    refused(st, [ok], 1, "At least two sequence tables")
    refused(st, [], 1, "At least two sequence tables")
    refused(st, [ok, (np.array([1, 2], dtype=np.int32), ["ACG", "TTG"], ["c"])], 1, "Not a matrix")
    refused(st, [ok, (np.zeros((1, 3), dtype=np.int32), ["ACG", "TTG"], ["c"])], 1, "Sequence table 2")
    refused(st, [ok, (np.zeros((2, 2), dtype=np.int32), ["ACG", "TTG"], ["c"])], 1, "Sequence table 2")
    refused(st, [ok, table(["c"], ["ACG", "TTG"], [[5, -1]])], 1, "Negative entries")
    refused(st, [ok, table(["c"], ["ACG", ""], [[5, 1]])], 1, "column (sequence) names are blank")
    refused(st, [table(["a", ""], ["ACG", "CCG"], [[1, 2], [3, 4]]), ok2], 1, "row (sample) names are blank")
    refused(st, [ok, table(["c"], ["ACG", "TTG", "ACG"], [[5, 1, 1]])], 1, "Duplicated column (sequences) names in sequence table 2")
    refused(st, [table(["a", "a"], ["ACG", "CCG"], [[1, 2], [3, 4]]), ok2], 1, "Duplicated row (sample) names in sequence table 1")
    refused(st, [ok, (np.zeros((0, 2), dtype=np.int32), ["ACG", "TTG"], [])], 1, "sequence table 2 is empty")
    refused(st, [ok, (np.zeros((1, 0), dtype=np.int32), [], ["c"])], 1, "sequence table 2 is empty")
    t3 = table(["b", "d", "a"], ["GGG"], [[1], [2], [3]])
    refused(st, [ok, ok2, t3], 1, "Duplicated sample names detected in the sequence table row names: b, a", repeats="error")
    t4 = table(["d", "c", "a"], ["ACG", "GGG"], [[1, 1], [2, 2], [3, 3]])
    mat, seqs, names, cmap = check(st, [ok, ok2, t3, t4], "repeats = sum over three and four tables", repeats="sum", order_by=None)
    assert names == ["a", "b", "c", "d"] and mat[0].tolist() == [1 + 3, 2, 0, 3 + 3], (names, mat)
    check_all(st, [ok, ok2, t3, t4], "repeated sample names", repeats="sum")
    try:
        st.merge_sequence_tables([ok, ok2], repeats="mean")
    except ValueError as e:
        assert "repeats" in str(e)
    else:
        raise AssertionError("repeats = mean was taken")


def _collision_tables(rng, n=40, length=48):
    pool = []
    while len(pool) < n:
        s = rand_seq(rng, length)
        if s not in pool and rc(s) not in pool and rc(s) != s:
            pool.append(s)
    t1 = rand_table(rng, ["a", "b"], pool[:n // 2], zero=0.2)
    t2 = rand_table(rng, ["c", "d"], [rc(s) for s in pool[5:n // 2]] + pool[n // 2:], zero=0.2)
    t3 = rand_table(rng, ["e"], pool[::3] + [rc(s) for s in pool[1::3]], zero=0.2)
    return (t1, t2, t3)


def case_collisions(st, light=False):
    rng = random.Random(1109)
    tabs = _collision_tables(rng)
    s0 = {}
    base = check(st, tabs, "the whole hash", stats=s0, try_rc=True)
    assert s0["collision_rounds"] == 0 and s0["rc_failed_compares"] == 0 and s0["flagged_sequences"] > 10, s0
    for bits in (0, 4):
        for extra in ({}, {"DADA2HIP_DEREP_PIECE": 7, "DADA2HIP_DEREP_TABLE": 8}):
            s1 = {}
            got = check(st, tabs, "hash of %d bits %s" % (bits, extra), stats=s1, env=dict(extra, DADA2HIP_DEREP_HASH_BITS=bits), try_rc=True)
            same(got, base, "collisions change nothing")
            assert s1["collision_rounds"] > 0 and s1["rc_failed_compares"] > 0 and s1["distinct_sequences"] == s0["distinct_sequences"], s1


def case_growth(st, light=False):
    rng = random.Random(1110)
    n = 120 if light else 900
    pool = [rand_seq(rng, rng.randint(30, 50)) for _ in range(n)]
    assert len(set(pool) | {rc(s) for s in pool}) == 2 * n
    tabs = []
    for k in range(6):
        cols = [s if rng.random() < 0.5 else rc(s) for s in rng.sample(pool, n // 2)]
        tabs.append(rand_table(rng, ["r%d_%d" % (k, i) for i in range(3)], cols))
    for try_rc in (False, True):
        base = check(st, tabs, "the default table", spec=spec_merge_fast, try_rc=try_rc)
        s1 = {}
        env = {"DADA2HIP_DEREP_TABLE": 8, "DADA2HIP_DEREP_PIECE": n // 4}
        got = check(st, tabs, "from a table of 8 slots, in pieces", spec=spec_merge_fast, stats=s1, env=env, try_rc=try_rc)
        same(got, base, "growth and pieces change nothing")
        assert s1["rebuilds"] > 0 and s1["pieces"] >= 3 and s1["table_capacity"] >= 2 * s1["distinct_sequences"], s1
        assert s1["input_columns"] == 6 * (n // 2) and s1["tables"] == 6 and s1["output_rows"] == 18, s1


def random_tables(seed, ntab=12, nrow=8, maxcol=300, npool=600, lo=200, hi=260, flip_whole=0.5, both=0.1, repeat_names=True):
    """``ntab`` tables of ``nrow`` rows and up to ``maxcol`` columns drawn from ``npool`` sequences of lo..hi nt; a share
    ``flip_whole`` of the tables is reverse-complemented as a whole, a share ``both`` of the pool occurs in both orientations, and
    with ``repeat_names`` sample names partly repeat between (never within) tables."""
    rng = np.random.default_rng(seed)
    letters = np.frombuffer(b"ACGT", dtype=np.uint8)
    lens = rng.integers(lo, hi + 1, size=npool)
    text = letters[rng.integers(0, 4, size=int(lens.sum()))].tobytes().decode("ascii")
    ends = np.cumsum(lens).tolist()
    pool = list(dict.fromkeys(text[e - n:e] for e, n in zip(ends, lens.tolist())))
    pool = [q for q in pool if rc(q) != q]
    two = set(rng.choice(len(pool), size=int(len(pool) * both), replace=False).tolist())
    flipped = set(rng.choice(ntab, size=int(ntab * flip_whole), replace=False).tolist())
    tabs = []
    for t in range(ntab):
        picks = rng.choice(len(pool), size=min(maxcol, len(pool)), replace=False).tolist()
        cols = []
        for i in picks:
            cols.append(pool[i])
            if i in two and (i + t) % 3:
                cols.append(rc(pool[i]))
        cols = cols[:maxcol]
        if t in flipped:
            cols = [rc(q) for q in cols]
        if repeat_names:
            names = ["S%d" % i for i in rng.choice(nrow * ntab // 2, size=nrow, replace=False).tolist()]
        else:
            names = ["S%d_%d" % (t, i) for i in range(nrow)]
        cells = rng.integers(1, 2001, size=(nrow, len(cols)), dtype=np.int32) * (rng.random((nrow, len(cols))) >= 0.6)
        tabs.append((np.ascontiguousarray(cells, dtype=np.int32), cols, names))
    return tabs


def case_random(st, light=False):
    tabs = random_tables(1111, ntab=4, maxcol=40, npool=80, lo=60, hi=90) if light else random_tables(1111)
    for try_rc in (False, True):
        check(st, tabs, "random tables", spec=spec_merge_fast, try_rc=try_rc, repeats="sum")
    refused(st, tabs, 1, "Duplicated sample names detected", spec=spec_merge_fast, repeats="error")
    tabs = random_tables(1112, ntab=4, maxcol=40, npool=80, lo=60, hi=90, repeat_names=False) if light else random_tables(1112, repeat_names=False)
    for try_rc in (False, True):
        check(st, tabs, "random tables, no repeated names", spec=spec_merge_fast, try_rc=try_rc, repeats="error")


def case_surface(st, light=False):
    from dada2_amd import api
    for name in ("merge_sequence_tables", "get_sequences", "uniques_to_fasta"):
        assert hasattr(st, name) and not hasattr(api, name), name
    s = {}
    merged(st, WORKED, stats=s, try_rc=True)
    assert set(STAT_WORDS) <= set(s) and tuple(st.STATS) == STAT_WORDS, sorted(s)
    assert (s["tables"], s["input_columns"], s["distinct_sequences"], s["flagged_sequences"], s["output_rows"], s["output_columns"]) == (2, 5, 4, 2, 3, 2), s
    assert s["pieces"] >= 1 and s["upload_bytes"] > 0 and s["download_bytes"] > 0 and s["total_us"] > 0, s


CASES = {"worked_example": case_worked_example, "lengths": case_lengths, "in_table_collapse": case_in_table_collapse,
         "contention": case_contention, "order": case_order, "iupac": case_iupac, "overflow": case_overflow, "validation": case_validation,
         "collisions": case_collisions, "growth": case_growth, "random": case_random, "surface": case_surface}
CASE_NAMES = tuple(CASES)


def check_large(st):
    """40 tables x 5 000 columns x 4 rows against spec_merge_fast (the card's alone): one call."""
    tabs = random_tables(1113, ntab=40, nrow=4, maxcol=5000, npool=30000, lo=200, hi=260)
    assert sum(len(t[1]) for t in tabs) > 120000
    s = {}
    check(st, tabs, "40 tables of up to 5 000 columns", spec=spec_merge_fast, stats=s, try_rc=True, repeats="sum")
    assert s["flagged_sequences"] > 1000 and s["pieces"] >= 2, s
    return s


def emu_run(names=None):
    """The emulator's job (tests/test_emu_seqtables.py): every case in its lighter form."""
    from dada2_amd import seqtables
    names = names or CASE_NAMES
    for name in names:
        CASES[name](seqtables, light=True)
    return "ok %d cases" % len(names)
