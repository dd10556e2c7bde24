"""isBimeraDenovo, removeBimeraDenovo and isShiftDenovo (R/chimeras.R:105-154, :294-346, :380-417): line-by-line restatements of the R
loops over an oracle's C_is_bimera / C_nwalign / C_eval_pair (oracle.ref: the reference's own C++; oracle.cport: its C restatement),
and the named cases the library is held to.  The expected flags of every case are recorded in tests/golden/bimera_denovo.json
(``python tests/bimera_denovo_cases.py`` rewrites it from oracle.ref): tests/test_bimera_denovo.py re-derives them on the CPU,
tests/test_gpu_bimera_denovo.py needs only the file.  Everything is compared for equality; there are no tolerances."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN_JSON = os.path.join(ROOT, "tests", "golden", "bimera_denovo.json")


# ---- restatements ---------------------------------------------------------------------------------------------------------------------
def restate_get_uniques(seqs, abunds):
    """getUniques (R/misc.R:33-62) of a named integer vector: duplicates merged by tapply(unqs, names(unqs), sum) - summed, and then
    in ascending order of the names."""
    seqs, abunds = list(seqs), [int(a) for a in abunds]
    if len(set(seqs)) == len(seqs):
        return seqs, abunds
    tot = {}
    for s, a in zip(seqs, abunds):
        tot[s] = tot.get(s, 0) + a
    keys = sorted(tot, key=lambda x: x.encode("ascii"))
    return keys, [tot[k] for k in keys]


def restate_is_bimera_denovo(oracle, seqs_in, abunds_in, min_fold=2, min_parent_abundance=8, allow_one_off=False,
                             min_one_off_parent_distance=4, max_shift=16):
    """isBimeraDenovo (:105-154), single-threaded branch (:144): one bool per INPUT sequence."""
    seqs, abunds = restate_get_uniques(seqs_in, abunds_in)                # unqs.int (:107)
    bims = []
    for i in range(len(seqs)):                                            # loopFun (:124-133)
        abund = abunds[i]
        pars = [seqs[k] for k in range(len(seqs)) if abunds[k] > (min_fold * abund) and abunds[k] > min_parent_abundance]
        if len(pars) < 2:
            bims.append(False)
        else:
            bims.append(bool(oracle.is_bimera(seqs[i], pars, allow_one_off, min_one_off_parent_distance, 5, -4, -8, max_shift)))
    flagged = {s for s, b in zip(seqs, bims) if b}
    return [s in flagged for s in seqs_in]                                # seqs.input %in% seqs[bims] (:150)


def restate_per_sample(oracle, mat, seqs, **kw):
    """removeBimeraDenovo(method = "per-sample") (:321-333): (bim [rows, cols], the table that is left, its sequences)."""
    mat = np.asarray(mat)
    bim = np.array([restate_is_bimera_denovo(oracle, seqs, row, **kw) for row in mat], dtype=bool)   # t(apply(unqs, 1, isBimeraDenovo))
    out = mat.copy()
    out[bim] = 0
    keep = out.sum(axis=0) != 0
    return bim, out[:, keep], [s for s, k in zip(seqs, keep) if k]


def restate_consensus(oracle, mat, seqs, min_sample_fraction=0.9, ignore_n_negatives=1):
    """isBimeraDenovoTable (:220-247) with its own defaults (1.5, 2)."""
    nflag, nsam = oracle.table_bimera2(mat, seqs)
    return [bool(f >= n or (f > 0 and f >= (n - ignore_n_negatives) * min_sample_fraction)) for f, n in zip(nflag, nsam)]


def _oracle_endsfree(oracle, s1, s2):
    """nwalign(sq1, sq2, band = -1) of R/misc.R:179: C_nwalign, ends-free, default scores."""
    if oracle.__name__.endswith("ref"):
        return oracle.nwalign(s1, s2, 5, -4, -8, -1, which="endsfree")
    return oracle.nwalign(s1, s2, 5, -4, -8, -1)


def restate_is_shift_denovo(oracle, seqs_in, abunds_in, min_overlap=20, flag_subseqs=False):
    """isShiftDenovo (:380-399) over isShift / isShiftedPair (:412-424).  flagSubseqs is NOT passed on (:391)."""
    del flag_subseqs
    seqs, abunds = restate_get_uniques(seqs_in, abunds_in)

    def shifted_pair(sq1, sq2, flag=False):                               # :412-417
        al = _oracle_endsfree(oracle, sq1, sq2)
        m, mm, indel = oracle.eval_pair(al[0], al[1])
        return (m < len(sq1) or flag) and (m < len(sq2) or flag) and m >= min_overlap and mm == 0 and indel == 0

    shifts = []
    for sq, abund in zip(seqs, abunds):                                   # loopFun (:385-393)
        pars = [seqs[k] for k in range(len(seqs)) if abunds[k] > abund]
        shifts.append(any(shifted_pair(sq, p) for p in pars))             # isShift: any(sapply(pars, isShiftedPair, ...))
    flagged = {s for s, b in zip(seqs, shifts) if b}
    return [s in flagged for s in seqs_in]


def restate_ranking(abunds, min_fold, min_parent_abundance, skip_zero=False):
    """(rank, P) as bimera_plain.h defines them, from the parent sets of :127 themselves: the ranking is abundance descending, index
    ascending; P[j] = the number of parents of j (their set must be the ranking's first P[j] entries), 0 where there are fewer than 2."""
    a = [int(x) for x in abunds]
    rank = sorted(range(len(a)), key=lambda k: (-a[k], k))
    P = []
    for j in range(len(a)):
        pars = {k for k in range(len(a)) if a[k] > (min_fold * a[j]) and a[k] > min_parent_abundance}
        assert pars == set(rank[: len(pars)])
        P.append(0 if len(pars) < 2 or (skip_zero and a[j] == 0) else len(pars))
    return rank, P


def fold_records(L, recs, allow_one_off, min_one_off_par_dist, maxima=None):
    """chimera.cpp:29-50 on the records (left, right, left_oo, right_oo, ham) of one query of length L, all of them visited:
    (the six maxima, the flag)."""
    m = list(maxima) if maxima is not None else [0] * 6
    for left, right, left_oo, right_oo, ham in recs:
        if left + right >= L:
            continue
        m[0], m[1] = max(m[0], left), max(m[1], right)
        if allow_one_off and ham >= min_one_off_par_dist:
            m[2], m[3], m[4], m[5] = max(m[2], left), max(m[3], right), max(m[4], left_oo), max(m[5], right_oo)
    flag = m[0] + m[1] >= L or bool(allow_one_off and (m[2] + m[5] >= L or m[4] + m[3] >= L))
    return m, flag


# ---- the cases ------------------------------------------------------------------------------------------------------------------------
def _rnd(rng, n):
    return "".join("ACGT"[int(x)] for x in rng.integers(0, 4, size=n))


def _sub(s, p):
    return s[:p] + "ACGT"[("ACGT".index(s[p]) + 1) & 3] + s[p + 1:]


LADDER_K = 140


def ladder():
    """140 unrelated parents of 120 nt with abundances 2 (3000 - r), r their rank, and for every c in 2 .. 138 two queries of abundance
    3000 - c: their parents are exactly the ranks [0, c) - rank c is exactly twice as abundant and is none.  One is the bimera of
    ranks c - 2 and c - 1, the last two parents; the other the bimera of ranks c and c + 1, which are not its parents."""
    rng = np.random.default_rng(101)
    par = [_rnd(rng, 120) for _ in range(LADDER_K)]
    seqs, ab, count = list(par), [2 * (3000 - r) for r in range(LADDER_K)], [0] * LADDER_K
    for c in range(2, LADDER_K - 1):
        cut = 30 + (c * 7) % 60
        seqs += [par[c - 2][:cut] + par[c - 1][cut:], par[c][:cut] + par[c + 1][cut:]]
        ab += [3000 - c, 3000 - c]
        count += [c, c]
    return seqs, ab, count


def big_equal(late):
    """4 096 sequences of 64 nt and abundance 100, none a parent of another, and one exact bimera of abundance 1: of ranks 0 and 1, or
    (late) of the last two ranks."""
    rng = np.random.default_rng(202)
    seqs = list(dict.fromkeys(_rnd(rng, 64) for _ in range(4200)))[:4096]
    a, b = (seqs[4094], seqs[4095]) if late else (seqs[0], seqs[1])
    return seqs + [a[:30] + b[30:]], [100] * 4096 + [1]


def _cases():
    rng = np.random.default_rng(303)
    C = {}
    A, B, Cc, D = (_rnd(rng, 150) for _ in range(4))
    bim = lambda x, y, cut=70: x[:cut] + y[cut:]   # noqa: E731
    C["n1"] = dict(seqs=[A], ab=[50])
    C["n2"] = dict(seqs=[A, bim(A, B)], ab=[50, 1])
    C["n3"] = dict(seqs=[A, B, _rnd(rng, 150)], ab=[50, 9, 1])             # the third has two parents and is no bimera; the second has one
    C["two_parents"] = dict(seqs=[A, B, bim(A, B), bim(B, A, 40)], ab=[50, 40, 2, 1])
    s, ab, _ = ladder()
    C["ladder"] = dict(seqs=s, ab=ab)
    # a_k == 2 a_j is no parent, 2 a_j + 1 is (a_j = 10)
    C["fold_equal"] = dict(seqs=[A, B, Cc, bim(A, Cc), bim(B, Cc)], ab=[20, 21, 500, 10, 10])
    # abundance 8 is no parent at the default, 9 is (a_j = 1); a one-row table_bimera2 with min_abund = 8 takes the 8 as well
    C["parent_abundance"] = dict(seqs=[A, B, Cc, bim(A, Cc), bim(B, Cc)], ab=[8, 9, 100, 1, 1])
    # min_fold = 1.5, a_j = 3: 4 is no parent (4 > 4.5 fails), 5 is
    C["fold_1_5"] = dict(seqs=[A, B, Cc, bim(A, Cc), bim(B, Cc)], ab=[4, 5, 100, 3, 3], kw=dict(min_fold=1.5, min_parent_abundance=2))
    for late in (False, True):
        s, ab = big_equal(late)
        C["late" if late else "early"] = dict(seqs=s, ab=ab)
    # the toss rule: a parent equal to the query up to a shift, one with an internal indel: neither completes a model
    Q = _rnd(rng, 150)
    C["toss"] = dict(seqs=[Q[5:] + "ACGTA", Q[:80] + Q[81:], Q], ab=[100, 90, 3])
    C["toss_shift_pair"] = dict(seqs=[Q[5:] + "ACGTA", "TTGCA" + Q[:-5], Q], ab=[100, 90, 3])
    # one-off models: the mismatch right of the breakpoint (left + right_oo) and left of it (left_oo + right)
    oo_r, oo_l = _sub(bim(A, B), 95), _sub(bim(A, B), 40)
    for name, kw in (("exact", {}), ("one_off", dict(allow_one_off=True)),
                     ("one_off_far", dict(allow_one_off=True, min_one_off_parent_distance=200))):
        C["oo_" + name] = dict(seqs=[A, B, oo_r, oo_l, bim(A, B)], ab=[100, 90, 2, 2, 1], kw=kw)
    # ... blocked by minOneOffParentDistance: the parents are within 3 of the query
    A2 = _sub(_sub(A, 140), 145)
    q_close = _sub(A[:100] + A2[100:], 20)
    for name, kw in (("blocked", dict(allow_one_off=True)), ("unblocked", dict(allow_one_off=True, min_one_off_parent_distance=1))):
        C["oo_" + name] = dict(seqs=[A, A2, q_close], ab=[100, 90, 2], kw=kw)
    # unequal lengths: the left parent starts 6 bases before the query does - inside maxShift 16, outside maxShift 4
    E, F = _rnd(rng, 100), _rnd(rng, 110)
    uq = [E, F, E[6:50] + F[50:], E[:50] + F[50:104], F[2:60] + E[52:]]
    for ms in (4, 16):
        C["unequal_ms%d" % ms] = dict(seqs=uq, ab=[100, 80, 3, 2, 1], kw=dict(max_shift=ms))
    # 2 100 nt: past what the anti-diagonal kernel takes, the lane route
    Ls = [_rnd(rng, 2100) for _ in range(4)]
    C["long"] = dict(seqs=Ls + [Ls[0][:900] + Ls[1][900:], Ls[2][:1000] + _rnd(rng, 1100)], ab=[100, 50, 40, 30, 2, 3])
    # duplicated input sequences (the bimera twice; a parent that is abundant enough only once merged), a zero abundance
    C["duplicates"] = dict(seqs=[A, B, bim(A, B), B, bim(A, B), Cc], ab=[100, 4, 1, 5, 2, 30])
    C["zero"] = dict(seqs=[A, B, bim(A, B), bim(B, A), Cc], ab=[100, 90, 0, 1, 0])
    return C


_CASES = {}


def cases():
    if not _CASES:
        _CASES.update(_cases())
    return _CASES


def per_sample_table():
    """A 3 x 40 table: 10 unrelated sequences of 100 nt and 30 two-parent mosaics of them; every row has its own abundances - so its own
    ranking - and zero cells, among the parents and among the mosaics."""
    rng = np.random.default_rng(404)
    true = [_rnd(rng, 100) for _ in range(10)]
    seqs = list(true)
    while len(seqs) < 40:
        a, b = rng.choice(10, 2, replace=False)
        ch = true[a][: int(rng.integers(20, 80))]
        ch = ch + true[b][len(ch):]
        if ch not in seqs:
            seqs.append(ch)
    mat = np.zeros((3, 40), dtype=np.int32)
    for i in range(3):
        mat[i, :10] = rng.permutation(10) * 37 + 20
        mat[i, 10:] = rng.integers(1, 12, size=30)
        mat[i, rng.choice(40, 9, replace=False)] = 0
    return mat, seqs


def table400():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from bench_bimera import make_table
    return make_table(400, 4)


def shift_cases():
    """name -> (seqs, abundances, kwargs) for isShiftDenovo."""
    rng = np.random.default_rng(505)
    X = _rnd(rng, 120)
    Y = _rnd(rng, 120)
    S = {}
    S["pure_shift"] = ([X, X[10:] + "ACGTTGCATG", Y], [50, 5, 7], {})                   # overlap 110
    S["shift_below_overlap"] = ([X, X[95:] + _rnd(rng, 95)], [50, 5], dict(min_overlap=30))   # overlap 25 < 30
    S["shift_above_overlap"] = ([X, X[95:] + _rnd(rng, 95)], [50, 5], dict(min_overlap=25))
    for fs in (False, True):
        S["subsequence_flag%d" % fs] = ([X, X[10:100]], [50, 5], dict(flag_subseqs=fs))
    sh = X[10:] + "ACGTTGCATG"
    S["shift_mismatch"] = ([X, _sub(sh, 50)], [50, 5], {})
    S["shift_indel"] = ([X, sh[:60] + sh[61:]], [50, 5], {})
    S["no_parent"] = ([X[10:] + "ACGTTGCATG", X], [5, 5], {})
    seqs, ab = [], []
    base = [_rnd(rng, int(rng.integers(80, 121))) for _ in range(12)]
    for k in range(60):
        b = base[int(rng.integers(0, 12))]
        kind = int(rng.integers(0, 5))
        if kind == 0:
            s = b
        elif kind == 1:
            d = int(rng.integers(1, 30)); s = b[d:] + _rnd(rng, d)
        elif kind == 2:
            d = int(rng.integers(1, 30)); s = _rnd(rng, d) + b[:-d]
        elif kind == 3:
            s = _sub(b[5:] + "ACGTA", int(rng.integers(0, len(b) - 1)))
        else:
            s = b[int(rng.integers(1, 10)): -int(rng.integers(1, 10))]
        if s not in seqs:
            seqs.append(s); ab.append(int(rng.integers(1, 40)))
    S["sixty"] = (seqs, ab, {})
    return S


def _kw(kw):
    kw = dict(kw or {})
    if "min_fold" in kw:
        kw["min_fold_parent_over_abundance"] = kw.pop("min_fold")
    return kw


def api_kw(kw):
    """A case's keywords under the names of api.is_bimera_denovo."""
    return _kw(kw)


def derive(oracle):
    """Every expected value of the golden file from ``oracle`` (oracle.ref or oracle.cport)."""
    out = {"cases": {}, "shift": {}}
    for name, c in cases().items():
        out["cases"][name] = [bool(x) for x in restate_is_bimera_denovo(oracle, c["seqs"], c["ab"], **(c.get("kw") or {}))]
    mat, seqs = per_sample_table()
    bim, left, names = restate_per_sample(oracle, mat, seqs)
    out["per_sample"] = {"flags": bim.astype(int).tolist(), "table": left.tolist(), "kept": [seqs.index(s) for s in names]}
    mat, seqs = table400()
    out["table400"] = {"pooled": [bool(x) for x in restate_is_bimera_denovo(oracle, seqs, mat.sum(axis=0))],
                       "per_sample": restate_per_sample(oracle, mat, seqs)[0].astype(int).tolist(),
                       "consensus": restate_consensus(oracle, mat, seqs)}
    for name, (s, ab, kw) in shift_cases().items():
        out["shift"][name] = [bool(x) for x in restate_is_shift_denovo(oracle, s, ab, **kw)]
    return out


# ---- the two kernels on made-up arrays (dada2hip_bimera_worklist_probe, dada2hip_bimera_fold_probe) -----------------------------------
def worklist_probe(rank, P, flags, live, r0, wr, per, device=0):
    import ctypes as C
    from dada2_amd import _lib
    i32 = lambda x: np.ascontiguousarray(x, dtype=np.int32)   # noqa: E731
    rank, P, live, flags = i32(rank), i32(P), i32(live), np.ascontiguousarray(flags, dtype=np.uint8)
    nq = live.size
    cc, work = np.full(nq * wr // per, -7, dtype=np.int32), np.full(nq * wr, -7, dtype=np.int32)
    eb = C.create_string_buffer(2048)
    _lib.check(_lib.lib().dada2hip_bimera_worklist_probe(rank.size, rank.ctypes.data, P.ctypes.data, flags.ctypes.data, nq, live.ctypes.data,
                                                         r0, wr, per, device, cc.ctypes.data, work.ctypes.data, eb, 2048), eb)
    return cc, work


def fold_probe(lens, P, live, r0, wr, work, rec, allow_one_off, min_dist, last, maxima, flags, device=0):
    import ctypes as C
    from dada2_amd import _lib
    i32 = lambda x: np.ascontiguousarray(x, dtype=np.int32)   # noqa: E731
    lens, P, live, work, rec = i32(lens), i32(P), i32(live), i32(work), i32(rec)
    maxima, flags = i32(maxima).copy(), np.ascontiguousarray(flags, dtype=np.uint8).copy()
    nq = live.size
    nxt, nn, al = np.zeros(nq, dtype=np.int32), np.zeros(1, dtype=np.int32), np.zeros(1, dtype=np.int64)
    eb = C.create_string_buffer(2048)
    _lib.check(_lib.lib().dada2hip_bimera_fold_probe(lens.size, lens.ctypes.data, P.ctypes.data, nq, live.ctypes.data, r0, wr, work.ctypes.data,
                                                     rec.ctypes.data, int(allow_one_off), int(min_dist), int(last), device, maxima.ctypes.data,
                                                     flags.ctypes.data, nxt.ctypes.data, nn.ctypes.data, al.ctypes.data, eb, 2048), eb)
    return maxima.reshape(-1, 6), flags, nxt, int(nn[0]), int(al[0])


def check_worklist(seed, n, nq, r0, wr, per):
    rng = np.random.default_rng(seed)
    rank = rng.permutation(n)
    P = rng.integers(0, n + 1, size=n)
    flags = (rng.random(n) < 0.2).astype(np.uint8)
    live = rng.choice(n, nq, replace=False)
    cc, work = worklist_probe(rank, P, flags, live, r0, wr, per)
    want = [[int(rank[r]) if (r < P[q] and not flags[q]) else -1 for r in range(r0, r0 + wr)] for q in live]
    assert work.reshape(nq, wr).tolist() == want, (seed, n, nq, r0, wr, per)
    assert cc.reshape(nq, wr // per).tolist() == [[int(q)] * (wr // per) for q in live]


def check_fold(seed, n, nq, r0, wr, allow_one_off, min_dist, last):
    """Records written by hand - lengths 40 .. 60, coverages around half a length so that models complete, fail by one, and are tossed
    (left + right >= len), hamming distances on both sides of min_dist -, some slots empty, maxima and flags from earlier windows."""
    rng = np.random.default_rng(seed)
    lens = rng.integers(40, 61, size=n)
    P = rng.integers(0, 3 * (r0 + wr), size=n)
    live = rng.choice(n, nq, replace=False)
    work = np.where(rng.random((nq, wr)) < 0.8, rng.integers(0, n, size=(nq, wr)), -1)
    work[0, :] = -1                                               # a query whose slots are all empty
    rec = np.zeros((nq, wr, 5), dtype=np.int32)
    cap = (lens[live] // 2 + rng.integers(-6, 2, size=nq))[:, None]   # per query: the most a side covers, around half its length
    rec[..., 0] = rng.integers(0, 1 << 20, size=(nq, wr)) % (cap + 1); rec[..., 1] = rng.integers(0, 1 << 20, size=(nq, wr)) % (cap + 1)
    rec[..., 2] = rec[..., 0] + rng.integers(0, 4, size=(nq, wr)); rec[..., 3] = rec[..., 1] + rng.integers(0, 4, size=(nq, wr))
    rec[..., 4] = rng.integers(0, 9, size=(nq, wr))
    rec[1:, 0, :2] = lens[live][1:, None] // 2 + 1                # tossed: left + right >= len, whatever else the record says
    rec[work < 0] = 12345                                         # what an empty slot holds is never read
    maxima0 = np.zeros((n, 6), dtype=np.int32)
    maxima0[live[::2]] = rng.integers(0, 18, size=(len(live[::2]), 6))
    flags0 = np.zeros(n, dtype=np.uint8)
    flags0[live[1::5]] = 1                                        # flagged by an earlier launch of the window: stays flagged
    maxima, flags, nxt, nn, al = fold_probe(lens, P, live, r0, wr, work, rec, allow_one_off, min_dist, last, maxima0, flags0)
    want_next, nflag = [], 0
    for k, q in enumerate(live):
        recs = [tuple(int(x) for x in rec[k, o]) for o in range(wr) if work[k, o] >= 0]
        m, f = fold_records(int(lens[q]), recs, allow_one_off, min_dist, maxima0[q])
        f = f or bool(flags0[q])
        assert maxima[q].tolist() == m and bool(flags[q]) == f, (seed, k, int(q), maxima[q].tolist(), m, f)
        nflag += f
        if last and not f and P[q] > r0 + wr:
            want_next.append(int(q))
    untouched = np.setdiff1d(np.arange(n), live)
    assert np.array_equal(maxima[untouched], maxima0[untouched]) and not flags[untouched].any()
    assert al == int((work >= 0).sum())
    assert nn == len(want_next) and sorted(nxt[:nn].tolist()) == sorted(want_next) and (nxt[nn:] == -1).all(), (seed, nn, want_next)
    return nflag, len(want_next)


def case_kernels():
    """Both kernels over shapes that cross a block (256 slots, 4 queries), leave a wave a partial last stride (wr no multiple of 64),
    and give a query fewer slots than a wave has lanes."""
    for seed, (n, nq, r0, wr, per) in enumerate([(50, 1, 0, 3, 3), (50, 7, 3, 9, 3), (300, 130, 12, 36, 3), (300, 5, 0, 128, 64),
                                                 (90, 33, 64, 192, 64), (40, 40, 5, 7, 1)]):
        check_worklist(seed, n, nq, r0, wr, per)
    flagged = live_on = 0
    for seed, (n, nq, r0, wr, oo, md, last) in enumerate([(50, 2, 0, 3, 0, 4, 1), (50, 9, 3, 9, 1, 4, 1), (300, 130, 12, 36, 1, 4, 1),
                                                          (300, 130, 12, 36, 0, 4, 0), (90, 33, 64, 192, 1, 2, 1), (60, 41, 0, 100, 1, 9, 1),
                                                          (60, 41, 0, 65, 0, 4, 1)]):
        f, l = check_fold(100 + seed, n, nq, r0, wr, oo, md, last)
        flagged += f
        live_on += l
    assert flagged > 20 and live_on > 20, (flagged, live_on)


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


def run_case(api, name, env=None):
    """One named case through api.is_bimera_denovo against the golden file: (flags as expected, the call's stats)."""
    c = cases()[name]
    st = {}
    got = with_env(env, lambda: api.is_bimera_denovo((c["seqs"], c["ab"]), stats=st, **api_kw(c.get("kw"))))
    assert got.dtype == bool and got.tolist() == golden()["cases"][name], (name, env, np.flatnonzero(got != np.array(golden()["cases"][name]))[:8])
    return st


def emu_run():
    """The emulator's job (tests/test_emu_bimera_denovo.py): the two kernels on made-up arrays, then small cases end to end - through
    both aligner routes, one with a slot budget that cuts its windows into many launches - and the per-sample table."""
    from dada2_amd import api
    case_kernels()
    for name in ("n3", "two_parents", "parent_abundance", "fold_1_5", "toss", "oo_one_off", "oo_blocked", "unequal_ms16", "duplicates", "zero"):
        run_case(api, name)
    st = run_case(api, "oo_one_off", {"DADA2HIP_NW_KERNEL": "lane"})
    assert st["aligner_route"] == 2 and st["per"] == 64, st
    st = run_case(api, "two_parents", {"DADA2HIP_BIMERA_SLOTS": 1})
    assert st["launches"] > st["windows"] and st["slot_budget"] == st["per"], st
    mat, seqs = per_sample_table()
    out, names = api.remove_bimera_denovo((mat[:, :24], seqs[:24]), method="per-sample")
    rows = [api.is_bimera_denovo((seqs[:24], r)) for r in mat[:, :24]]
    want = mat[:, :24].copy()
    want[np.array(rows)] = 0
    keep = want.sum(axis=0) != 0
    assert np.array_equal(out, want[:, keep]) and names == [s for s, k in zip(seqs[:24], keep) if k]
    for name in ("pure_shift", "shift_below_overlap", "subsequence_flag1", "shift_mismatch"):
        s, ab, kw = shift_cases()[name]
        assert api.is_shift_denovo((s, ab), **kw).tolist() == golden()["shift"][name], name
    return "ok"


def golden():
    with open(GOLDEN_JSON) as f:
        return json.load(f)


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    from oracle import ref
    ref.set_threads(16)
    with open(GOLDEN_JSON, "w") as f:
        json.dump(derive(ref), f, separators=(",", ":"))
        f.write("\n")
    print("wrote", GOLDEN_JSON)
