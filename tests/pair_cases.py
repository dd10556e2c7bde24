"""The case table of the pairwise alignment exports (dada2hip_nwvec, dada2hip_nwalign; dada2hip_merge_pairs rides on the
first): seeded, pure numpy, nothing on disk.  Used by tests/test_gpu_pairwise_exports.py on the MI355X, tests/test_emu.py under
the emulator and tests/test_oracle.py for the restatement against the reference.

The three exports go through nwvec_any (driver.cpp), which always launches the PAIR form of the lane kernels: a centre per work
item (NwArgs::pair_centre), 64 unrelated pairs to a wave, the alignment handed back as a move string per pair.  A batch's
kernel follows from the WHOLE batch: W = 2 band + (batch maxlen - batch minlen) + 1 picks k_nw<33|65|129|193|257, pair>, and
k_nw_gen<pair> beyond 257 and for band -1 (nw_class, kernels.hip).  The expected instance is written out per case; what the tests
assert is the library's launch ledger.

One NWVEC CASE = (band, minlen, maxlen, n pairs, scores, endsfree).  Pair 0 is (a string of maximal length, one of minimal
length) - it pins the class, for n = 1 too -, pair 1 the reverse; the others cycle through the pair classes of `_KINDS` with the
two sides swapped on every other turn, so the lanes of one wave differ in L1 and both lband > rband and the reverse occur.
Strings of 2-5 nt have cases of their own (short_*): one of them in a batch of 40 nt reads would be the batch's minlen and move
the batch to another class.  Scores 1/-64/-64 are given to batches with reads of 168 nt or more only: with ends free a gap
pays there only between two flanks of more than 64 matches, and every batch has to hold interior gaps (check_facts).  The
GLOBAL aligner gets them on reads of at most 105 nt only: past 155 nt x 64 its scores fall below the -9999 with which the scalar
aligners mark the band's edge, and from there on the reference's C_nwalign and its C_nwvec give different alignments (DESIGN
section 8; tests/test_oracle.py keeps one such pair).

One NWALIGN CASE = one pair through dada2hip_nwalign with a homopolymer gap penalty; the call's class comes from that pair
alone, so the pair's own W = 2 band + |len1 - len2| + 1 sits on the class boundary."""
from collections import namedtuple

import numpy as np

from aligner_cases import GAPLESS_BITS, _repeat_rich, _rnd, _sub, bit_gen, bit_nw, describe, read_ledger  # noqa: F401

SCORES = {"default": (5, -4, -8), "merge0": (1, -64, -64), "merge": (1, -8, -8), "flat": (6, -3, -3)}

VecCase = namedtuple("VecCase", "name band minlen maxlen n score endsfree expect seed small letters")
AlignCase = namedtuple("AlignCase", "name band homo_gap expect seed small pairs")


def _seed(name):
    return (sum(ord(c) * (i + 1) for i, c in enumerate(name)) * 2654435761) % (2 ** 31)   # (stable across processes)


def _expect(band, minlen, maxlen):
    """The pair instance by nw_class's thresholds, restated: the ledger assertion is what checks them."""
    if band < 0:
        return bit_gen(True)
    w = 2 * band + (maxlen - minlen) + 1
    for wclass in (33, 65, 129, 193, 257):
        if w <= wclass:
            return bit_nw(wclass, "pair")
    return bit_gen(True)


# (name, band, minlen, maxlen, the instance): W either side of every class boundary, W in the name
GEOMETRY = [
    ("w33", 6, 40, 60, bit_nw(33, "pair")), ("w34", 7, 41, 60, bit_nw(65, "pair")),
    ("w65", 16, 40, 72, bit_nw(65, "pair")), ("w66", 16, 40, 73, bit_nw(129, "pair")),
    ("w129", 32, 40, 104, bit_nw(129, "pair")), ("w130", 32, 40, 105, bit_nw(193, "pair")),
    ("w193", 32, 40, 168, bit_nw(193, "pair")), ("w194", 32, 40, 169, bit_nw(257, "pair")),
    ("w257", 32, 40, 232, bit_nw(257, "pair")), ("w258", 32, 40, 233, bit_gen(True)),
    ("unbanded", -1, 40, 100, bit_gen(True)),
    ("unbanded300", -1, 280, 300, bit_gen(True)),       # W = 601: what mergePairs sees on 2 x 300 reads
]
# ... and the classes past 129 at reads of at most 130 nt (the emulator's table): the band does what the length spread cannot
SMALL_GEOMETRY = [("s193", 45, 40, 130, bit_nw(193, "pair")), ("s257", 70, 40, 130, bit_nw(257, "pair")), ("sgen", 90, 40, 130, bit_gen(True))]
# scores of (n = 65, ends free) and of (n = 257, global) per geometry
_SCORE_OF = {
    "w33": ("default", "flat"), "w34": ("merge", "default"), "w65": ("flat", "merge"), "w66": ("default", "flat"),
    "w129": ("merge", "default"), "w130": ("flat", "merge0"), "w193": ("merge0", "default"), "w194": ("default", "merge"),
    "w257": ("merge0", "flat"), "w258": ("merge", "default"), "unbanded": ("default", "merge"), "unbanded300": ("merge", "default"),
}


def _vec(name, band, minlen, maxlen, n, score, endsfree, expect, small=False, letters=False):
    assert expect == _expect(band, minlen, maxlen) or letters, name
    return VecCase(name, band, minlen, maxlen, n, score, endsfree, expect, _seed(name), small, letters)


def vec_cases():
    """Every dada2hip_nwvec case."""
    out = []
    for name, band, lo, hi, bit in GEOMETRY:
        s65, s257 = _SCORE_OF[name]
        out.append(_vec("%s_n65_%s_ef1" % (name, s65), band, lo, hi, 65, s65, True, bit, small=hi <= 130))
        out.append(_vec("%s_n257_%s_ef0" % (name, s257), band, lo, hi, 257, s257, False, bit))
    # every batch size on two classes: one pair, a wave less one, a full wave (65: a second chunk of one pair; 257: ragged fifth)
    for name, band, lo, hi, bit in (GEOMETRY[0], GEOMETRY[9]):
        for n in (1, 63, 64):
            out.append(_vec("%s_n%d_default_ef1" % (name, n), band, lo, hi, n, "default", True, bit, small=hi <= 130 and n > 1))
    for k, (name, band, lo, hi, bit) in enumerate(SMALL_GEOMETRY):
        out.append(_vec("%s_n65_%s_ef1" % (name, ("default", "flat", "merge")[k]), band, lo, hi, 65, ("default", "flat", "merge")[k], True, bit, small=True))
    # the global aligner on every class at the emulator's size
    for k, (name, band, lo, hi, bit) in enumerate([GEOMETRY[0], GEOMETRY[2], GEOMETRY[4]] + SMALL_GEOMETRY + [GEOMETRY[10]]):
        sc = ("default", "merge", "flat")[k % 3]
        out.append(_vec("%s_n40_%s_ef0" % (name, sc), band, lo, hi, 40, sc, False, bit, small=True))
    # strings of 2-5 nt: band 14 gives W = 32, band 16 W = 36
    out.append(_vec("short_b14_n65_default_ef1", 14, 2, 5, 65, "default", True, bit_nw(33, "pair"), small=True))
    out.append(_vec("short_b16_n65_merge_ef0", 16, 2, 5, 65, "merge", False, bit_nw(65, "pair"), small=True))
    out.append(_vec("short_unbanded_n65_flat_ef1", -1, 2, 5, 65, "flat", True, bit_gen(True), small=True))
    # letters outside ACGT: two 2-bit planes per string, always the generic kernel (launch_nw), wider than two waves
    out.append(_vec("letters_n130_default_ef1", 16, 40, 60, 130, "default", True, bit_gen(True), small=True, letters=True))
    names = [c.name for c in out]
    assert len(set(names)) == len(names)
    return out


def small_vec_cases():
    """The thinned table (n <= 65, reads <= 130 nt; every class, ends free and global): the emulator's."""
    return [c for c in vec_cases() if c.small]


# ---- the pairs of a batch --------------------------------------------------------------------------------------------------------
def _mid_lengths(rng, lo, hi, k):
    return (hi, lo, (lo + hi) // 2, int(rng.integers(lo, hi + 1)))[k % 4]


def _k_identical(rng, c, lo, hi, band):
    return c, c


def _k_subs(rng, c, lo, hi, band):
    return c, _sub(rng, c, rng.choice(len(c), size=min(len(c), int(rng.integers(1, 7))), replace=False))


def _indel(rng, c, p, lo, hi):
    """`c` with a base deleted at p, or one inserted where the deletion would leave the length range."""
    if len(c) - 1 >= lo and (len(c) + 1 > hi or rng.random() < 0.5):
        return c[:p] + c[p + 1:]
    return c[:p] + "ACGT"[("ACGT".index(c[p]) + 1 + int(rng.integers(0, 3))) & 3] + c[p:]


def _k_indel_start(rng, c, lo, hi, band):
    return c, _indel(rng, c, int(rng.integers(2, 6)), lo, hi)


def _k_indel_end(rng, c, lo, hi, band):
    return c, _indel(rng, c, len(c) - 1 - int(rng.integers(2, 6)), lo, hi)


def _k_indel_mid(rng, c, lo, hi, band):
    return c, _indel(rng, c, len(c) // 2, lo, hi)


def _k_two_indels(rng, c, lo, hi, band):
    """A base deleted and one inserted 20 positions on: equal lengths, a gap in each string."""
    p = len(c) // 3
    s = c[:p] + c[p + 1:]
    q = min(p + 20, len(s) - 2)
    return c, s[:q] + "ACGT"[("ACGT".index(s[q]) + 1) & 3] + s[q:]


def _shift(rng, c, sh):
    return c[sh:] + _rnd(rng, sh)


def _k_shift_band(rng, c, lo, hi, band):
    """Equal lengths, the second string moved by exactly `band` bases: the path runs along the band's last diagonal."""
    sh = band if 0 < band < len(c) - 12 else max(1, len(c) // 4)
    return c, _shift(rng, c, sh)


def _k_shift_band1(rng, c, lo, hi, band):
    """... and by band + 1: the true path is out of the band."""
    sh = band + 1 if 0 < band + 1 < len(c) - 12 else max(1, len(c) // 3)
    return c, _shift(rng, c, sh)


def _k_overhang5(rng, c, lo, hi, band):
    d = int(rng.integers(1, 9))
    return c, (_rnd(rng, d) + c)[: len(c)]


def _k_overhang3(rng, c, lo, hi, band):
    d = int(rng.integers(1, 9))
    return c, (c + _rnd(rng, d))[d:]


def _k_substring(rng, c, lo, hi, band):
    a = int(rng.integers(0, len(c) - lo + 1))
    return c, c[a: a + lo]


def _k_tie_prone(rng, c, lo, hi, band):
    """Homopolymers and di- / tri-nucleotide repeats with an indel inside a repeat: only up > left > diagonal decides the strings."""
    c = _repeat_rich(rng, len(c))
    runs = [p for p in range(2, len(c) - 2) if c[p - 1] == c[p] == c[p + 1] or c[p - 2: p] == c[p: p + 2]]
    p = int(rng.choice(runs)) if runs else len(c) // 2
    if len(c) - 1 >= lo and (len(c) + 1 > hi or rng.random() < 0.5):
        return c, c[:p] + c[p + 1:]
    return c, c[:p] + c[p] + c[p:]


def _k_unrelated(rng, c, lo, hi, band):
    return c, _rnd(rng, _mid_lengths(rng, lo, hi, int(rng.integers(0, 4))))


_KINDS = [("identical", _k_identical), ("subs", _k_subs), ("indel_start", _k_indel_start), ("indel_end", _k_indel_end),
          ("indel_mid", _k_indel_mid), ("two_indels", _k_two_indels), ("shift_band", _k_shift_band), ("shift_band+1", _k_shift_band1),
          ("overhang5", _k_overhang5), ("overhang3", _k_overhang3), ("substring", _k_substring), ("tie_prone", _k_tie_prone),
          ("unrelated", _k_unrelated)]
_LETTERS = "ACGTNRYKMSWBDHV"

Built = namedtuple("Built", "case s1 s2 kinds")
_BUILT = {}


def build(case):
    """The n pairs of a case: (s1, s2, kind) lists.  Built once per process."""
    if case.name in _BUILT:
        return _BUILT[case.name]
    rng = np.random.default_rng(case.seed)
    lo, hi, band = case.minlen, case.maxlen, case.band
    s1, s2, kinds = [], [], []
    if hi <= 5:                                           # the 2-5 nt cases
        strs = [_rnd(rng, hi), _rnd(rng, lo)]
        s1, s2, kinds = [strs[0], strs[1]], [strs[1], strs[0]], ["long_short", "short_long"]
        while len(s1) < case.n:
            a = _rnd(rng, int(rng.integers(lo, hi + 1)))
            k = len(s1) % 4
            b = (a, a[1:] if len(a) > lo else a + "A", _rnd(rng, int(rng.integers(lo, hi + 1))), a[:-1] if len(a) > lo else "C" + a)[k]
            s1.append(a); s2.append(b)
            kinds.append(("identical", "drop5", "unrelated", "drop3")[k])
    else:
        cmax = _rnd(rng, hi)
        d = hi - lo
        cmin = _sub(rng, cmax[d // 2: d // 2 + lo], rng.choice(lo, size=2, replace=False))
        s1, s2, kinds = [cmax, cmin], [cmin, _sub(rng, cmax, [hi // 2])], ["long_short", "short_long"]
        t = 0
        while len(s1) < case.n:
            kind, fn = _KINDS[t % len(_KINDS)]
            turn = t // len(_KINDS)
            c = _rnd(rng, _mid_lengths(rng, lo, hi, t + turn))
            a, b = fn(rng, c, lo, hi, band)
            if (t + turn) % 2:
                a, b = b, a
            s1.append(a); s2.append(b); kinds.append(kind)
            t += 1
    s1, s2, kinds = s1[: case.n], s2[: case.n], kinds[: case.n]
    if case.letters:
        # N and IUPAC codes over the same pairs: one to four of the bases renamed throughout the pair (it stays as similar as it
        # was), and letters dropped on a few positions of either string; at most 4 + 6 distinct bytes in a pair
        for i in range(case.n):
            extras = [_LETTERS[4 + int(x)] for x in rng.permutation(len(_LETTERS) - 4)]
            m = {"ACGT"[int(x)]: extras[j] for j, x in enumerate(rng.permutation(4)[: 1 + i % 4])}
            pair = []
            for s in (s1[i], s2[i]):
                s = [m.get(ch, ch) for ch in s]
                for p in rng.choice(len(s), size=min(3, len(s)), replace=False):
                    s[int(p)] = extras[4 + int(rng.integers(0, 3))]
                pair.append("".join(s))
            s1[i], s2[i] = pair
        assert all(set(a + b) - set("ACGT") for a, b in zip(s1, s2))
    lens = [len(s) for s in s1 + s2]
    assert min(lens) == lo and max(lens) == hi, (case.name, min(lens), max(lens))
    b = Built(case, s1, s2, kinds)
    _BUILT[case.name] = b
    return b


_EXPECTED = {}


def expected(oracle, case, ref=None):
    """The oracle's alignment of every pair of the case, computed once per process: cport.C_nwalign (the plain-C restatement of
    nwalign_endsfree and the global nwalign) for A/C/G/T, the reference's own C_nwvec call on raw bytes (`ref`) for letters."""
    if case.name not in _EXPECTED:
        b = build(case)
        sc = SCORES[case.score]
        if case.letters:
            _EXPECTED[case.name] = [tuple(ref.nwvec_raw(a, c, sc[0], sc[1], sc[2], case.band, case.endsfree)) for a, c in zip(b.s1, b.s2)]
        else:
            _EXPECTED[case.name] = [tuple(oracle.C_nwalign(a, c, sc[0], sc[1], sc[2], None, case.band, case.endsfree)) for a, c in zip(b.s1, b.s2)]
    return _EXPECTED[case.name]


def interior_gaps(al):
    """(string 0 has a gap between two of its bases, string 1 has)."""
    return tuple("-" in s.strip("-") for s in al)


def py_nw(s1, s2, sc, band, endsfree, perturbed=False):
    """The aligners' recurrence in plain Python with the tie order as a parameter: up > left > diagonal as the reference has it
    (nwalign_endsfree.cpp:146-156), or diagonal > left > up.  Only to show that a pair HAS two optimal alignments."""
    match, mismatch, gap = sc
    L1, L2 = len(s1), len(s2)
    B = max(L1, L2) if band < 0 else band
    lband, rband = B + max(L1 - L2, 0), B + max(L2 - L1, 0)
    SENT = -9999
    D = [[SENT] * (L2 + 1) for _ in range(L1 + 1)]
    P = [[0] * (L2 + 1) for _ in range(L1 + 1)]
    for j in range(min(rband, L2) + 1):
        D[0][j] = 0 if endsfree else j * gap
    for i in range(1, L1 + 1):
        if i <= lband:
            D[i][0] = 0 if endsfree else i * gap
        row, prev = D[i], D[i - 1]
        for j in range(max(1, i - lband), min(L2, i + rband) + 1):
            diag = prev[j - 1] + (match if s1[i - 1] == s2[j - 1] else mismatch)
            up = (prev[j] if j - (i - 1) <= rband else SENT) + (0 if endsfree and j == L2 else gap)
            left = (row[j - 1] if i - (j - 1) <= lband else SENT) + (0 if endsfree and i == L1 else gap)
            if perturbed:
                p, v = (1, diag) if diag >= left and diag >= up else ((2, left) if left >= up else (3, up))
            else:
                p, v = (3, up) if up >= left and up >= diag else ((2, left) if left >= diag else (1, diag))
            row[j], P[i][j] = v, p
    i, j, a0, a1 = L1, L2, [], []
    while i > 0 or j > 0:
        p = 2 if i == 0 else (3 if j == 0 else P[i][j])
        if p == 3:
            i -= 1; a0.append(s1[i]); a1.append("-")
        elif p == 2:
            j -= 1; a0.append("-"); a1.append(s2[j])
        else:
            i -= 1; j -= 1; a0.append(s1[i]); a1.append(s2[j])
    return "".join(reversed(a0)), "".join(reversed(a1))


_FACTS = set()


def check_facts(oracle, case, want):
    """What a batch of a wave or more has to hold, from the oracle's alignments: an interior gap in each string (but in the
    2-5 nt cases, where no gap pays), and a pair whose gapped strings change when the tie order is perturbed - py_nw gives
    the oracle's alignment in the reference's order and another one in the opposite order."""
    if case.n < 63 or case.letters or case.name in _FACTS:
        return
    b = build(case)
    sc = SCORES[case.score]
    if case.maxlen > 5:
        g0 = sum(interior_gaps(al)[0] for al in want)
        g1 = sum(interior_gaps(al)[1] for al in want)
        assert g0 > 0 and g1 > 0, (case.name, "interior gaps in string 0 / string 1 of", g0, g1, "alignments")
    order = sorted(range(case.n), key=lambda i: (b.kinds[i] != "tie_prone", i))
    for i in order[:24]:
        if py_nw(b.s1[i], b.s2[i], sc, case.band, case.endsfree) == tuple(want[i]) and \
                py_nw(b.s1[i], b.s2[i], sc, case.band, case.endsfree, perturbed=True) != tuple(want[i]):
            _FACTS.add(case.name)
            return
    raise AssertionError((case.name, "no pair whose alignment depends on the tie order"))


def check_alignment(name, i, a, c, got, want=None):
    """The checks that need no oracle, then the oracle's strings."""
    g0, g1 = got
    assert len(g0) == len(g1), (name, i, a, c, got)
    assert not any(x == "-" and y == "-" for x, y in zip(g0, g1)), (name, i, "gap-gap column", got)
    assert g0.replace("-", "") == a and g1.replace("-", "") == c, (name, i, "degapped outputs are not the inputs", a, c, got)
    if want is not None:
        assert tuple(got) == tuple(want), (name, i, a, c, "got", got, "expected", want)


def run_vec_case(api, oracle, case, ref=None, nalone=8):
    """dada2hip_nwvec on the whole batch: every pair's two strings against the oracle, the ledger shows exactly the case's pair
    instance; then `nalone` pairs of the batch alone through dada2hip_nwalign (the batch layout does not leak between lanes).
    Returns the ledger of the batch call."""
    b = build(case)
    sc = SCORES[case.score]
    want = expected(oracle, case, ref)
    check_facts(oracle, case, want)
    read_ledger()
    got = api.nwvec(b.s1, b.s2, sc[0], sc[1], sc[2], case.band, case.endsfree)
    ran = read_ledger() & ~GAPLESS_BITS
    assert len(got) == case.n
    for i in range(case.n):
        check_alignment(case.name + ":" + b.kinds[i], i, b.s1[i], b.s2[i], got[i], want[i])
    assert ran == case.expect, (case.name, "ran", describe(ran), "expected", describe(case.expect))
    if not case.letters:
        for i in sorted({int(x) for x in np.linspace(0, case.n - 1, num=min(nalone, case.n))}):
            alone = api.nwalign(b.s1[i], b.s2[i], sc[0], sc[1], sc[2], None, case.band, case.endsfree)
            assert tuple(alone) == tuple(got[i]), (case.name, i, b.kinds[i], "alone", alone, "in the batch", got[i])
        read_ledger()
    return ran


# ---- the scratch ring's wrap: a wave's second and third chunk in the slot it has used ---------------------------------------------
# launch_nw caps its waves at the ring ensure_scratch sized (4 096 waves, fewer for long unbanded reads), and a wave that gets a
# second chunk of 64 pairs finds the first one's pointer rows, t-codes and DP row in its slot.  DADA2HIP_NW_RING=4 makes that
# happen on 600 pairs: ten chunks on four waves, two waves with a third trip, the last chunk of 24 pairs.  The pair classes cycle
# as in every batch (13 kinds against chunks of 64), so a lane of a reused slot goes from a long pair to a short one and back.
RING_N = 600
_RING_GEOMETRY = [GEOMETRY[0], GEOMETRY[2], GEOMETRY[4]] + SMALL_GEOMETRY + [GEOMETRY[10]]     # every pair instance at <= 130 nt; banded and unbanded k_nw_gen


def ring_vec_cases():
    """600 pairs per pair instance, ends free and global, plus the two-plane letters batch: the cases of the ring's wrap."""
    out = []
    for k, (name, band, lo, hi, bit) in enumerate(_RING_GEOMETRY):
        for ef in (True, False):
            sc = ("default", "flat", "merge")[(k + ef) % 3]
            out.append(_vec("ring_%s_n%d_%s_ef%d" % (name, RING_N, sc, ef), band, lo, hi, RING_N, sc, ef, bit))
    out.append(_vec("ring_letters_n%d_default_ef1" % RING_N, 16, 40, 60, RING_N, "default", True, bit_gen(True), letters=True))
    names = [c.name for c in out]
    assert len(set(names)) == len(names)
    return out


def run_ring_vec_case(api, oracle, case, ref=None):
    """dada2hip_nwvec on the whole batch under a ring of four waves: both strings of every pair against the oracle, the ledger
    shows the case's pair instance, dada2hip_nw_ring_trips says the launch was sized for three trips (an ignored knob fails
    here); then the same call with the knob unset - one trip, identical strings.  Returns the ledger of the call."""
    from aligner_cases import RING_MIN_WORK, RING_WAVES, read_ring_trips, ring
    assert case.n >= RING_MIN_WORK and case.n % 64
    b = build(case)
    sc = SCORES[case.score]
    want = expected(oracle, case, ref)
    check_facts(oracle, case, want)
    kinds_by_lane = {(i % 64): set() for i in range(case.n)}
    for i in range(case.n):
        kinds_by_lane[i % 64].add(len(b.s1[i]) + len(b.s2[i]) > case.minlen + case.maxlen)
    assert all(len(v) == 2 for v in kinds_by_lane.values()), (case.name, "a lane whose pairs are all long or all short")
    with ring(RING_WAVES):
        read_ledger()
        got = api.nwvec(b.s1, b.s2, sc[0], sc[1], sc[2], case.band, case.endsfree)
        ran = read_ledger() & ~GAPLESS_BITS
        trips = read_ring_trips()
    assert len(got) == case.n
    for i in range(case.n):
        check_alignment(case.name + ":" + b.kinds[i], i, b.s1[i], b.s2[i], got[i], want[i])
    assert ran == case.expect, (case.name, "ran", describe(ran), "expected", describe(case.expect))
    assert trips >= 3, (case.name, "the launch was sized for", trips, "trips: DADA2HIP_NW_RING ignored?")
    with ring(None):
        plain = api.nwvec(b.s1, b.s2, sc[0], sc[1], sc[2], case.band, case.endsfree)
        assert read_ring_trips() == 1, case.name
    assert [tuple(x) for x in plain] == [tuple(x) for x in got], (case.name, "the ring's size changed an alignment")
    return ran


# ---- the wrap at the ring's AUTOMATIC size: unbanded pairs of 1 400-1 500 nt --------------------------------------------------------
# ensure_scratch halves the ring while its pointer scratch would pass 6 x 2^28 words: at 1 500 nt unbanded (W = 3 001, 188 pointer
# words per row, 1 501 x 188 x 64 words per wave) that leaves 64 waves, so a call of more than 4 096 pairs wraps with no knob set.
# 4 200 pairs: 66 chunks on 64 waves, waves 0 and 1 take a second one, the last chunk holds 40 pairs.  The oracle aligns the
# 24 distinct pairs of the pool once each; item i is pool pair i mod 24, and 4 096 mod 24 = 16: the pair a lane finds in its slot
# from the first trip is another one.
LONG_N = 4200
LONG_RING_ITEMS = 64 * 64          # alignments per trip of the automatic ring at this geometry
LONG_POOL = 24


def long_pool(seed=1500):
    """[(s1, s2, kind)]: 24 pairs of 1 400-1 500 nt - identical, substitutions, insertions and deletions inside, one side a prefix
    of the other, unrelated; either side the longer one.  Both extreme lengths occur (the batch's window is 2 x 1 500 + 1)."""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(LONG_POOL):
        L = (1500, 1400, 1450, 1473, 1500, 1427)[(k + k // 6) % 6]
        c = _rnd(rng, L)
        kind = ("identical", "subs", "indels", "prefix", "unrelated", "subs+indels")[k % 6]
        if kind == "identical":
            b = c
        elif kind == "subs":
            b = _sub(rng, c, rng.choice(L, size=3 + 4 * k, replace=False))
        elif kind in ("indels", "subs+indels"):
            s = list(c)
            for _ in range(2 + k % 7):                       # deletions and insertions of 1-9 bases inside the read
                p, m = int(rng.integers(30, len(s) - 40)), int(rng.integers(1, 10))
                if len(s) - m >= 1400 and (len(s) + m > 1500 or rng.random() < 0.5):
                    del s[p: p + m]
                else:
                    s[p:p] = list(_rnd(rng, m))
            b = "".join(s)
            if kind == "subs+indels":
                b = _sub(rng, b, rng.choice(len(b), size=12, replace=False))
        elif kind == "prefix":
            c = c if L > 1400 else _rnd(rng, 1500)
            b = c[:1400]
        else:
            b = _rnd(rng, (1400, 1500, 1461)[k % 3])
        out.append((c, b, kind) if k % 2 else (b, c, kind))
    lens = [len(s) for a, b, _ in out for s in (a, b)]
    assert min(lens) == 1400 and max(lens) == 1500 and len({(a, b) for a, b, _ in out}) == LONG_POOL
    assert {k for _, _, k in out} == {"identical", "subs", "indels", "prefix", "unrelated", "subs+indels"}
    return out


def long_batch():
    """(s1, s2, pool index of every item): LONG_N items, items one trip of the automatic ring apart hold different pairs."""
    pool = long_pool()
    idx = np.arange(LONG_N) % LONG_POOL
    assert (idx[LONG_RING_ITEMS:] != idx[:-LONG_RING_ITEMS]).all() and LONG_N > LONG_RING_ITEMS and LONG_N % 64
    return [pool[k][0] for k in idx], [pool[k][1] for k in idx], idx


def run_long_batch(api, oracle):
    """dada2hip_nwvec, band -1, ends free, default scores, on the 4 200 pairs with NO knob set: every item's two strings
    against the oracle's alignment of its pool pair, k_nw_gen<pair> by the ledger, and dada2hip_nw_ring_trips >= 2 - the
    automatic ring was smaller than the call.  Returns (trips, seconds of the call)."""
    import time
    from aligner_cases import read_ring_trips, ring
    pool = long_pool()
    s1, s2, idx = long_batch()
    want = [tuple(oracle.C_nwalign(a, b, 5, -4, -8, None, -1, True)) for a, b, _ in pool]
    assert sum(interior_gaps(al)[0] or interior_gaps(al)[1] for al in want) >= 6
    with ring(None):
        read_ledger()
        t0 = time.time()
        got = api.nwvec(s1, s2, 5, -4, -8, -1, True)
        dt = time.time() - t0
        ran = read_ledger() & ~GAPLESS_BITS
        trips = read_ring_trips()
    assert len(got) == LONG_N
    for i in range(LONG_N):
        k = int(idx[i])
        if tuple(got[i]) != want[k]:
            check_alignment("long:%s" % pool[k][2], i, s1[i], s2[i], got[i], want[k])
    assert ran == bit_gen(True), describe(ran)
    assert trips >= 2, ("the launch was sized for", trips, "trip: the automatic ring holds the whole call")
    return trips, dt


# ---- dada2hip_nwalign with homopolymer gaps: one pair per call, the pair's own W on the class boundary ------------------------------
def _homo_pair(rng, long_len, short_len, swap):
    """A homopolymer-rich string and a stretch of it with run lengths changed by one and with the boundary between two adjacent
    runs of four or more moved by a base: a mismatch to the plain aligner, two cheap gaps to nwalign_endsfree_homo."""
    while True:
        c = ""
        while len(c) < long_len:
            c += "ACGT"[int(rng.integers(0, 4))] * int(rng.choice([1, 1, 2, 4, 4, 5, 6]))
        c = c[:long_len]
        a0 = (long_len - short_len) // 2
        s = list(c[a0: a0 + short_len])
        bounds = [p for p in range(6, len(s) - 6) if len(set(s[p - 4: p])) == 1 and len(set(s[p: p + 4])) == 1 and s[p - 1] != s[p]]
        if bounds:
            break
    for p in bounds[:: max(1, len(bounds) // 3)]:
        s[p] = s[p - 1]
    for _ in range(2):                                    # lengthen / shorten a run inside the stretch: the length stays
        runs = [p for p in range(8, len(s) - 8) if s[p - 1] == s[p] == s[p + 1]]
        if len(runs) < 2:
            break
        p, q = sorted(int(x) for x in rng.choice(runs, size=2, replace=False))
        s.insert(q, s[q])
        del s[p]
    s = "".join(s)
    assert len(s) == short_len
    return (s, c) if swap else (c, s)


def align_cases():
    """(band, long, short) with W = 2 band + long - short + 1 on each side of every class boundary, homopolymer gap -1 and 0."""
    rows = [("w33", 6, 60, 40, bit_nw(33, "pair")), ("w34", 7, 60, 41, bit_nw(65, "pair")), ("w65", 16, 72, 40, bit_nw(65, "pair")),
            ("w66", 16, 73, 40, bit_nw(129, "pair")), ("w129", 32, 104, 40, bit_nw(129, "pair")), ("w130", 32, 105, 40, bit_nw(193, "pair")),
            ("w193", 32, 168, 40, bit_nw(193, "pair")), ("w194", 32, 169, 40, bit_nw(257, "pair")), ("w257", 32, 232, 40, bit_nw(257, "pair")),
            ("w258", 32, 233, 40, bit_gen(True)), ("unbanded", -1, 90, 60, bit_gen(True)),
            # equal lengths: the class by the band alone
            ("w33_eq", 16, 57, 57, bit_nw(33, "pair")), ("w129_eq", 64, 120, 120, bit_nw(129, "pair")), ("w193_eq", 96, 130, 130, bit_nw(193, "pair")),
            ("w257_eq", 128, 130, 130, bit_nw(257, "pair")), ("w259_eq", 129, 130, 130, bit_gen(True))]
    out = []
    for name, band, hi, lo, bit in rows:
        for hg in (-1, 0):
            nm = "%s_homo%d" % (name, hg)
            seed = _seed(nm)
            rng = np.random.default_rng(seed)
            pairs = [_homo_pair(rng, hi, lo, swap) for swap in (False, True, False, True)]
            assert _expect(band, lo, hi) == bit, nm
            out.append(AlignCase(nm, band, hg, bit, seed, hi <= 130, pairs))
    return out


def small_align_cases():
    return [c for c in align_cases() if c.small]


def run_align_case(api, oracle, case):
    """Each pair of the case alone through dada2hip_nwalign (default scores, ends free, the case's homopolymer gap penalty)
    against the oracle; the ledger shows the case's pair instance after every call.  Returns the ledger."""
    seen = 0
    changed = 0
    for i, (a, c) in enumerate(case.pairs):
        want = oracle.C_nwalign(a, c, 5, -4, -8, case.homo_gap, case.band, True)
        read_ledger()
        got = api.nwalign(a, c, 5, -4, -8, case.homo_gap, case.band, True)
        ran = read_ledger() & ~GAPLESS_BITS
        check_alignment(case.name, i, a, c, got, want)
        assert ran == case.expect, (case.name, i, "ran", describe(ran), "expected", describe(case.expect))
        seen |= ran
        changed += tuple(want) != tuple(oracle.C_nwalign(a, c, 5, -4, -8, None, case.band, True))
    assert changed > 0, (case.name, "the homopolymer gap penalty changes no alignment of the case")
    return seen


def pair_instances():
    """The six pair instances of the build."""
    return [bit_nw(w, "pair") for w in (33, 65, 129, 193, 257)] + [bit_gen(True)]
