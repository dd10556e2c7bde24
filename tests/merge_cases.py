"""Synthetic mergePairs inputs shared by the golden generator and the tests: denoised forward / reverse sequence sets of
one sample cut from a few amplicons, and the per-read-pair indices into them (1-based, <= 0 for NA)."""
import numpy as np

_COMP = str.maketrans("ACGT", "TGCA")

OPTION_SETS = {
    "default": dict(),
    "mismatch1": dict(max_mismatch=1),
    "overlap40_trim": dict(min_overlap=40, trim_overhang=True),
    "concat": dict(just_concatenate=True),
}


def rc(s):
    return s.translate(_COMP)[::-1]


def make_case(seed, namp=14, npairs=900):
    rng = np.random.default_rng(seed)
    seqsF, seqsR = [], []
    truth = []                                             # (forward index, reverse index) that belong together
    for a in range(namp):
        L = int(rng.integers(150, 330))                    # amplicon length: overlaps from long to none, and overhangs
        amp = "".join(rng.choice(list("ACGT"), size=L))
        lf, lr = int(rng.integers(110, 160)), int(rng.integers(110, 160))
        f = amp[:lf] if lf <= L else amp + "".join(rng.choice(list("ACGT"), size=lf - L))    # read-through past the amplicon
        r_fw = amp[max(0, L - lr):]
        if lr > L:
            r_fw = "".join(rng.choice(list("ACGT"), size=lr - L)) + amp
        if a % 5 == 1:                                     # a substitution inside the reverse read: mismatch in the overlap
            p = 8 if lf + lr - L >= 30 else int(rng.integers(5, len(r_fw) - 5))      # (inside the overlap when there is one)
            r_fw = r_fw[:p] + "ACGT"[("ACGT".index(r_fw[p]) + 1) % 4] + r_fw[p + 1:]
        if a % 7 == 2:                                     # a deletion: indel in the overlap
            p = 14 if lf + lr - L >= 30 else int(rng.integers(10, len(r_fw) - 10))
            r_fw = r_fw[:p] + r_fw[p + 1:]
        seqsF.append(f)
        seqsR.append(rc(r_fw))
        truth.append((a + 1, a + 1))
    permF, permR = rng.permutation(namp), rng.permutation(namp)   # the two denoised tables are ordered independently
    seqsF = [seqsF[i] for i in permF]
    seqsR = [seqsR[i] for i in permR]
    posF = {int(old) + 1: new + 1 for new, old in enumerate(permF)}
    posR = {int(old) + 1: new + 1 for new, old in enumerate(permR)}
    w = rng.dirichlet(np.full(namp, 0.5))
    fwd, rev = [], []
    for _ in range(npairs):
        a = int(rng.choice(namp, p=w)) + 1
        f, r = posF[a], posR[a]
        u = rng.random()
        if u < 0.06:
            r = int(rng.integers(1, namp + 1))             # chimeric / mispaired read pair
        elif u < 0.09:
            f = -1                                         # NA: the forward read was not assigned
        elif u < 0.12:
            r = -1
        fwd.append(f)
        rev.append(r)
    n0F = rng.integers(1, 200, size=namp).astype(np.int32)
    n0R = rng.integers(1, 200, size=namp).astype(np.int32)
    return dict(seqsF=seqsF, seqsR=seqsR, fwd=np.array(fwd, dtype=np.int32), rev=np.array(rev, dtype=np.int32), n0F=n0F, n0R=n0R)


# ---- constructed cases: one regime of mergePairs each --------------------------------------------------------------------------------
# make_case above stays as it is (the committed goldens were made from it).  A constructed case is the same dict plus `name`,
# `options` (the option sets it runs under) and `fact`: a function of {option index: the oracle's rows, rejects included, in
# the order of the case's pairs} that asserts the case reaches what it was built for - called before anything is compared.
def _rnd(rng, n):
    return "".join("ACGT"[int(x)] for x in rng.integers(0, 4, size=n))


def _flip(s, p):
    return s[:p] + "ACGT"[("ACGT".index(s[p]) + 1) % 4] + s[p + 1:]


def _reads(amp, lf, lr):
    """(forward read, reverse read as sequenced) of an amplicon: its first lf and the reverse complement of its last lr bases."""
    return amp[:lf], rc(amp[len(amp) - lr:])


def _case(name, pairs, options, fact, n0F=None, n0R=None, fwd=None, rev=None):
    """pairs: [(forward sequence, reverse sequence as sequenced)]: read pair k names forward k and reverse k, k + 1 times over
    (so the rows come back in the reverse of the pairs' order, by abundance)."""
    n = len(pairs)
    if fwd is None:
        fwd = [k + 1 for k in range(n) for _ in range(k + 1)]
        rev = list(fwd)
    return dict(name=name, seqsF=[p[0] for p in pairs], seqsR=[p[1] for p in pairs], fwd=np.array(fwd, dtype=np.int32),
                rev=np.array(rev, dtype=np.int32), n0F=np.array(n0F if n0F is not None else [10] * n, dtype=np.int32),
                n0R=np.array(n0R if n0R is not None else [10] * n, dtype=np.int32), options=options, fact=fact)


def _by_pair(rows):
    return sorted(rows, key=lambda r: r["forward"])


def _c_overlap(rng):
    """Overlaps of exactly min_overlap and one less, for the default 12 and for 20."""
    pairs = [_reads(_rnd(rng, 200), 100 + ov // 2, 100 + ov - ov // 2) for ov in (12, 11, 20, 19)]

    def fact(rows):
        r12, r20 = _by_pair(rows[0]), _by_pair(rows[1])
        assert [r["nmatch"] for r in r12] == [12, 11, 20, 19] and [r["nmismatch"] + r["nindel"] for r in r12] == [0] * 4, r12
        assert [r["accept"] for r in r12] == [True, False, True, True] and [r["accept"] for r in r20] == [False, False, True, False]
    return _case("overlap_at_min_overlap", pairs, [dict(), dict(min_overlap=20)], fact)


def _c_mismatches(rng):
    """k = 0..3 differences in an overlap of 60 (substitutions 15 apart; the second one is a deleted base instead) under
    max_mismatch 0, 1 and 2: exactly max_mismatch is accepted, one more is not."""
    pairs = []
    for k in range(4):
        amp = _rnd(rng, 240)
        f, r_fw = amp[:150], amp[90:]
        for q in range(k):
            p = 10 + 15 * q                               # (position in the overlap = in r_fw)
            r_fw = r_fw[:p] + r_fw[p + 1:] if (q == 1) else _flip(r_fw, p)
        pairs.append((f, rc(r_fw)))

    def fact(rows):
        for m in (0, 1, 2):
            rr = _by_pair(rows[m])
            assert [r["accept"] for r in rr] == [k <= m for k in range(4)], (m, rr)
            if m:                                         # (with -64 / -64 an alignment slides apart rather than hold a mismatch)
                assert [r["nmismatch"] + r["nindel"] for r in rr[: m + 2]] == list(range(m + 2)), (m, rr)
                assert rr[2]["nindel"] == 1, rr[2]
    return _case("mismatches_at_max_mismatch", pairs, [dict(), dict(max_mismatch=1), dict(max_mismatch=2)], fact)


def _c_read_through(rng):
    """Both reads run through the amplicon into what follows it: overhangs on both sides, kept or trimmed."""
    amp, xf, xr = _rnd(rng, 90), _rnd(rng, 25), _rnd(rng, 30)
    pairs = [(amp + xf, rc(xr + amp)), (amp[:70] + xf[:5], rc(xr[:7] + amp[:70]))]

    def fact(rows):
        keep, trim = _by_pair(rows[0]), _by_pair(rows[1])
        assert all(r["accept"] for r in keep + trim)
        assert keep[0]["sequence"] == xr + amp + xf and trim[0]["sequence"] == amp, (keep[0], trim[0])
        assert keep[1]["sequence"] != trim[1]["sequence"] == amp[:70]
    return _case("read_through_both_sides", pairs, [dict(), dict(trim_overhang=True)], fact)


def _c_contained(rng):
    """The forward read inside rc(reverse), and the reverse."""
    amp = _rnd(rng, 120)
    pairs = [(amp[30:80], rc(amp)), (amp, rc(amp[25:85]))]

    def fact(rows):
        rr = _by_pair(rows[0])
        assert [(r["nmatch"], r["accept"]) for r in rr] == [(50, True), (60, True)], rr
        assert rr[0]["sequence"] == amp and rr[1]["sequence"] == amp
        # (trim_overhang cuts what lies before the forward read's start and behind the reverse read's start, evaluate.cpp:160-171)
        assert [r["sequence"] for r in _by_pair(rows[1])] == [amp[30:], amp[:85]]
    return _case("contained_either_way", pairs, [dict(), dict(trim_overhang=True)], fact)


def _c_prefer(rng):
    """prefer: n0F == n0R and n0F > n0R take the forward base of a mismatch, n0R > n0F the reverse one."""
    amp = _rnd(rng, 200)
    f, r_fw = amp[:130], _flip(amp[70:], 30)
    pairs = [(f, rc(r_fw)), (f, rc(r_fw)), (f, rc(r_fw))]

    def fact(rows):
        rr = _by_pair(rows[0])
        assert [r["prefer"] for r in rr] == [1, 2, 1] and all(r["accept"] and r["nmismatch"] == 1 for r in rr), rr
        assert rr[0]["sequence"] == amp == rr[2]["sequence"] and rr[1]["sequence"] == _flip(amp, 100), rr
    return _case("prefer_by_n0", pairs, [dict(max_mismatch=1)], fact, n0F=[7, 7, 9], n0R=[7, 8, 3])


def _c_no_overlap(rng):
    pairs = [(_rnd(rng, 120), _rnd(rng, 130)), (_rnd(rng, 60), _rnd(rng, 45))]

    def fact(rows):
        for rr in rows.values():
            assert all(not r["accept"] and r["sequence"] == "" and r["nmatch"] < 12 for r in rr), rr
    return _case("no_overlap", pairs, [dict(), dict(max_mismatch=1)], fact)


def _c_repeats(rng):
    """Repeat-rich overlaps: the overlap is a tandem repeat or a homopolymer (placements a unit apart score alike but for the
    flanks), and two with a unit missing inside a flanked repeat - the gap may sit at any unit."""
    u, v = _rnd(rng, 60), _rnd(rng, 60)
    pairs = [(u + "AC" * 12, rc("AC" * 12 + v)), (u + "ACG" * 9 + v[:20], rc(u[-20:] + "ACG" * 8 + v)), (u + "T" * 14, rc("T" * 14 + v)),
             (u + "GA" * 10 + v[:25], rc(u[-20:] + "GA" * 9 + v))]

    def fact(rows):
        rr = _by_pair(rows[0])
        assert [r["accept"] for r in rr] == [True, False, True, False], rr
        assert rr[0]["sequence"] == u + "AC" * 12 + v and rr[2]["sequence"] == u + "T" * 14 + v
        r1 = _by_pair(rows[1])
        assert all(r["accept"] for r in r1) and r1[1]["nindel"] == 3 and r1[3]["nindel"] == 2, r1
        assert r1[1]["sequence"] == u + "ACG" * 9 + v and r1[3]["sequence"] == u + "GA" * 10 + v
    return _case("repeat_rich_overlap", pairs, [dict(), dict(max_mismatch=3)], fact)


def _c_reads_of_300(rng):
    """2 x 300 nt: the unbanded window is 601 wide."""
    a1, a2 = _rnd(rng, 450), _rnd(rng, 580)
    pairs = [_reads(a1, 300, 300), (a1[:300], rc(_flip(a1[150:], 75))), _reads(a2, 300, 300)]

    def fact(rows):
        rr = _by_pair(rows[0])
        assert [len(s) for p in pairs for s in p] == [300] * 6
        assert [(r["nmatch"], r["accept"]) for r in rr] == [(150, True), (rr[1]["nmatch"], False), (20, True)], rr
        assert rr[0]["sequence"] == a1 and rr[2]["sequence"] == a2
        r1 = _by_pair(rows[1])
        assert (r1[1]["nmatch"], r1[1]["nmismatch"], r1[1]["accept"]) == (149, 1, True) and r1[1]["sequence"] == a1, r1[1]
    return _case("reads_of_300", pairs, [dict(), dict(max_mismatch=1)], fact)


def _c_all_na(rng):
    """Every read pair has a side that was not assigned."""
    pairs = [_reads(_rnd(rng, 150), 100, 100), _reads(_rnd(rng, 150), 100, 100)]

    def fact(rows):
        assert all(rr == [] for rr in rows.values())
    return _case("all_pairs_na", pairs, [dict(), dict(max_mismatch=1)], fact, fwd=[1, -1, 2, -1, -1], rev=[-1, 2, -1, 1, -1])


def constructed_cases():
    rng = np.random.default_rng(20240)
    out = [f(rng) for f in (_c_overlap, _c_mismatches, _c_read_through, _c_contained, _c_prefer, _c_no_overlap, _c_repeats,
                            _c_reads_of_300, _c_all_na)]
    names = [c["name"] for c in out]
    assert len(set(names)) == len(names)
    return out


def large_case():
    """300 forward x 220 reverse sequences of 30-40 nt cut from three templates, every combination a read pair: 66 000 unique
    pairs, more than the 65 536 dada2hip_merge_pairs aligns per call.  Every fifth pair occurs twice, so the abundance order
    takes rows from both sides of the chunk boundary apart and puts them side by side."""
    rng = np.random.default_rng(66000)
    tpl = [_rnd(rng, 64) for _ in range(3)]
    seqsF, seqsR = [], []
    for i in range(300):
        t = tpl[i % 3]
        n = 30 + i % 11
        a = int(rng.integers(0, 12))
        seqsF.append(t[a: a + n] if i % 4 else _flip(t[a: a + n], int(rng.integers(0, n))))
    for j in range(220):
        t = tpl[j % 3]
        n = 30 + (j * 7) % 11
        a = int(rng.integers(64 - n - 12, 64 - n + 1))
        seqsR.append(rc(t[a: a + n]))
    fwd = np.repeat(np.arange(1, 301, dtype=np.int32), 220)
    rev = np.tile(np.arange(1, 221, dtype=np.int32), 300)
    again = np.arange(0, fwd.size, 5)
    fwd, rev = np.concatenate([fwd, fwd[again]]), np.concatenate([rev, rev[again]])

    def fact(rows):
        rr = rows[0]
        assert len(rr) == 66000 > 65536
        first = [(r["forward"] - 1) * 220 + r["reverse"] - 1 for r in rr]         # (the pair's place in the aligned list)
        acc = [r["accept"] for r in rr]
        assert any(a and p < 65536 for a, p in zip(acc, first)) and any(a and p >= 65536 for a, p in zip(acc, first))
        assert any(not a and p >= 65536 for a, p in zip(acc, first))
        assert max(first[:13200]) >= 65536 and min(first[:13200]) == 0          # (the 13 200 doubled pairs come first)
    return dict(name="pairs_66000", seqsF=seqsF, seqsR=seqsR, fwd=fwd, rev=rev, n0F=rng.integers(1, 50, size=300).astype(np.int32),
                n0R=rng.integers(1, 50, size=220).astype(np.int32), options=[dict(max_mismatch=1)], fact=fact)


def ring_case():
    """30 forward x 20 reverse sequences of 45-125 nt cut from three templates of 150 nt, every combination a read pair: 600
    unique pairs in one device call, long pairs beside short ones - what the aligner's scratch ring wraps on when
    DADA2HIP_NW_RING makes it four waves (ten chunks of 64 pairs, the last of 24)."""
    rng = np.random.default_rng(600)
    tpl = [_rnd(rng, 150) for _ in range(3)]
    seqsF, seqsR = [], []
    for i in range(30):
        t = tpl[i % 3]
        n = (45, 125, 80, 60, 110)[i % 5] - i % 4
        a = int(rng.integers(0, 20))
        seqsF.append(t[a: a + n] if i % 4 else _flip(t[a: a + n], int(rng.integers(0, n))))
    for j in range(20):
        t = tpl[j % 3]
        n = (120, 50, 95, 70)[j % 4] - j % 3
        a = int(rng.integers(150 - n - 20, 150 - n + 1))
        seqsR.append(rc(t[a: a + n]))
    fwd = np.repeat(np.arange(1, 31, dtype=np.int32), 20)
    rev = np.tile(np.arange(1, 21, dtype=np.int32), 30)
    again = np.arange(0, fwd.size, 5)
    fwd, rev = np.concatenate([fwd, fwd[again]]), np.concatenate([rev, rev[again]])

    def fact(rows):
        for rr in rows.values():
            assert len(rr) == 600
            assert sum(r["accept"] for r in rr) >= 40 and sum(not r["accept"] for r in rr) >= 300, sum(r["accept"] for r in rr)
        assert any(r["accept"] and r["nmismatch"] == 1 for r in rows[1])
    return dict(name="pairs_600_ring", seqsF=seqsF, seqsR=seqsR, fwd=fwd, rev=rev, n0F=rng.integers(1, 50, size=30).astype(np.int32),
                n0R=rng.integers(1, 50, size=20).astype(np.int32), options=[dict(), dict(max_mismatch=1)], fact=fact)
