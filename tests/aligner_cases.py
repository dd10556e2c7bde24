"""The shared case table of the alignment-level tests (tests/test_gpu_aligner_instances.py on the MI355X, tests/test_emu.py
under the emulator, tests/test_oracle.py for the restatement against the reference): seeded, pure numpy, nothing on disk.

One GEOMETRY CASE = (band, maxlen, maxlen - minlen, score mode, route) plus the compiled aligner instance the launch must
choose for it.  The expectation is written out here; what a test asserts is the library's own launch ledger
(dada2hip_launch_ledger, include/dada2hip.h), so a threshold that moves in the dispatcher turns the test red instead of being
followed silently.  One sample per geometry case: two or three centres (of maximal, minimal and middle length, so the pair's
length difference takes both signs and the band's origin shift both parities) and, per centre, reads of every class listed in
`_reads_of`; all uniques of the sample are compared with each centre.

W = 2 band + (maxlen - minlen) + 1 is the band window.  k_nw_ad takes 21 / 32 / 64 lanes per alignment for W <= 41 / <= 63 /
<= 127 and its EDGE form when W + 4 > 2 GL; k_nw_adw 21 / 32 / 64 lanes for W + 1 <= 168 / 256 / 512; k_nw<WMAX> the classes
33 / 65 / 129 / 193 / 257, k_nw_gen beyond and for band -1."""
from collections import namedtuple

import numpy as np

from dada2_amd.io import extend_err
from dada2_amd.opts import DadaOpts

# ---- the launch ledger's bit layout (include/dada2hip.h) ----------------------------------------------------------------------
_GL = {21: 0, 32: 1, 64: 2}
AD_MODES = ("default", "generic", "homo", "fast")
NW_CLASSES = (33, 65, 129, 193, 257)
GAPLESS_BITS = (1 << 96) | (1 << 97)


def bit_ad(gl, edge, mode):
    return 1 << (8 * _GL[gl] + 4 * int(edge) + AD_MODES.index(mode))


def bit_lr(gl, edge, generic):
    return 1 << (32 + 4 * _GL[gl] + 2 * int(edge) + int(generic))


def bit_adw(gl, generic):
    return 1 << (64 + 2 * _GL[gl] + int(generic))


def bit_nw(wclass, form):
    """form: 'plain', 'nonplain' or 'pair' (a centre per work item)."""
    return 1 << (72 + 3 * NW_CLASSES.index(wclass) + ("plain", "nonplain", "pair").index(form))


def bit_gen(pair=False):
    return 1 << (88 + int(pair))


def instance_names():
    """{bit: name} of every aligner instance the ledger knows."""
    out = {}
    for gl in (21, 32, 64):
        for edge in (0, 1):
            for mode in AD_MODES:
                out[bit_ad(gl, edge, mode)] = "k_nw_ad<%d%s, %s>" % (gl, ", EDGE" if edge else "", mode)
            for g in (0, 1):
                out[bit_lr(gl, edge, g)] = "k_nw_ad<%d%s, LR, %s>" % (gl, ", EDGE" if edge else "", "generic" if g else "default")
        for g in (0, 1):
            out[bit_adw(gl, g)] = "k_nw_adw<%d, %s>" % (gl, "generic" if g else "default")
    for w in NW_CLASSES:
        for form in ("plain", "nonplain", "pair"):
            out[bit_nw(w, form)] = "k_nw<%d, %s>" % (w, form)
    out[bit_gen(False)] = "k_nw_gen"
    out[bit_gen(True)] = "k_nw_gen<pair>"
    return out


def read_ledger(clear=True):
    """The library's launch ledger as one Python integer (bit b = bit b of include/dada2hip.h's layout)."""
    import ctypes as C

    from dada2_amd import _lib
    m = (C.c_uint64 * 2)()
    assert _lib.lib().dada2hip_launch_ledger(m, 2, int(clear)) == 2
    return int(m[0]) | (int(m[1]) << 64)


def read_ring_trips(clear=True):
    """dada2hip_nw_ring_trips: the most trips through its chunk loop a lane launch was sized for since the last clear."""
    from dada2_amd import _lib
    return int(_lib.lib().dada2hip_nw_ring_trips(int(clear)))


RING_WAVES = 4          # the ring the wrap tests ask for: 4 waves = 256 alignments per trip
RING_MIN_WORK = 513     # ... and the least work of a launch under it: a third trip for some waves


class ring(object):
    """with ring(4): DADA2HIP_NW_RING for the calls inside (the library reads its knobs at every boundary call); ring(None): unset."""

    def __init__(self, waves):
        self.waves = waves

    def __enter__(self):
        import os
        self.old = os.environ.get("DADA2HIP_NW_RING")
        if self.waves is None:
            os.environ.pop("DADA2HIP_NW_RING", None)
        else:
            os.environ["DADA2HIP_NW_RING"] = str(self.waves)
        read_ring_trips()
        return self

    def __exit__(self, *exc):
        import os
        if self.old is None:
            os.environ.pop("DADA2HIP_NW_RING", None)
        else:
            os.environ["DADA2HIP_NW_RING"] = self.old
        return False


def describe(mask):
    names = instance_names()
    return [names.get(1 << b, "bit %d" % b) for b in range(128) if (mask >> b) & 1 and not (GAPLESS_BITS >> b) & 1]


# ---- score modes --------------------------------------------------------------------------------------------------------------
SCORE_MODES = {
    "default": dict(),
    "generic_a": dict(MATCH=4, MISMATCH=-5, GAP_PENALTY=-7),
    "generic_b": dict(MATCH=6, MISMATCH=-3, GAP_PENALTY=-3),       # a gap costs what a mismatch costs
    "homo_1": dict(HOMOPOLYMER_GAP_PENALTY=-1),
    "homo_0": dict(HOMOPOLYMER_GAP_PENALTY=0),
}


def _ad_mode(score):
    return "default" if score == "default" else ("homo" if score.startswith("homo") else "generic")


Case = namedtuple("Case", "name band maxlen diff score route expect seed small gapruns")
# route: the value of DADA2HIP_NW_KERNEL ("" = the dispatcher's own choice); expect: the one ledger bit of the aligner families
# small: part of the thinned table the emulator and the reference check run: reads of at most 130 nt, but for one wide case of
# 220 nt (wide_we256_default: the only small case whose diagonal offsets pass 127, what an 8-bit run descriptor would lose)


def _mk(name, band, maxlen, diff, score, route, expect, small=False, gapruns=False):
    seed = (sum(ord(c) * (i + 1) for i, c in enumerate(name)) * 2654435761) % (2 ** 31)   # (stable across processes)
    return Case(name, band, maxlen, diff, score, route, expect, seed, small, gapruns)


# (band, maxlen - minlen, GL, EDGE) of the anti-diagonal kernel: first / last W of every (GL, EDGE), W in the comment
AD_ROWS = [
    (1, 0, 21, 0),      # 3
    (16, 0, 21, 0),     # 33  the default band
    (18, 1, 21, 0),     # 38  last non-edge of 21 lanes
    (19, 0, 21, 1),     # 39  first EDGE
    (20, 0, 21, 1),     # 41  last of 21 lanes
    (19, 2, 21, 1),     # 41  ... with an odd left band: the origin shift is 1 and the band reaches the group's last cell, next to
                        #     alignments of the same wave whose left band is even and whose first cell is in band (the EDGE masks)
    (20, 1, 32, 0),     # 42  first of 32 lanes
    (16, 9, 32, 0),     # 42  ... by the length spread
    (29, 1, 32, 0),     # 60  last non-edge
    (30, 0, 32, 1),     # 61
    (31, 0, 32, 1),     # 63
    (29, 4, 32, 1),     # 63  ... with an odd left band (as 19, 2)
    (31, 1, 64, 0),     # 64  first of 64 lanes
    (32, 0, 64, 0),     # 65
    (61, 1, 64, 0),     # 124 last non-edge
    (62, 0, 64, 1),     # 125
    (32, 60, 64, 1),    # 125 the shape of bench.py's long-read configuration
    (63, 0, 64, 1),     # 127 last of the kernel
    (61, 4, 64, 1),     # 127 ... with an odd left band
]
# W = 128: past k_nw_ad.  The dispatcher's own choice is k_nw_adw<21> (plain scores) or k_nw<129> (homopolymer gaps)
PAST_AD_ROWS = [(63, 1), (32, 63)]


def _maxlen_for(i, small):
    # lengths either side of a multiple of 8 (the 16-step pointer blocks) and of 16
    return (104, 111, 112, 113, 121, 127, 128, 129)[i % 8] if small else (159, 160, 161, 200, 207, 208, 255, 256, 257, 260)[i % 10]


def aligner_cases():
    """Every geometry case of the aligner sweep."""
    cases = []
    k = 0
    for band, diff, gl, edge in AD_ROWS:
        for score in SCORE_MODES:
            k += 1
            for small in (False, True):
                ml = max(_maxlen_for(k, small), diff + 40)
                cases.append(_mk("ad_b%d_d%d_%s_%s" % (band, diff, score, "s" if small else "l"), band, ml, diff, score, "",
                                 bit_ad(gl, edge, _ad_mode(score)), small=small))
    for band, diff in PAST_AD_ROWS:
        for score in SCORE_MODES:
            k += 1
            for small in (False, True):
                ml = max(_maxlen_for(k, small), diff + 40)
                exp = bit_nw(129, "nonplain") if score.startswith("homo") else bit_adw(21, score != "default")
                cases.append(_mk("past_b%d_d%d_%s_%s" % (band, diff, score, "s" if small else "l"), band, ml, diff, score, "", exp, small=small))
    # many gap runs (>= 3 AD_RCAP = 192 merged runs inside the band: the traceback goes through several chunks of run descriptors)
    for band, diff, gl, edge in ((16, 0, 21, 0), (20, 0, 21, 1), (30, 0, 32, 1), (32, 0, 64, 0), (32, 60, 64, 1)):
        for score in ("default", "generic_a", "homo_1"):
            cases.append(_mk("runs_b%d_d%d_%s" % (band, diff, score), band, 1900, diff, score, "", bit_ad(gl, edge, _ad_mode(score)), gapruns=True))
    cases.append(_mk("runs_wide_b32_d150", 32, 1900, 150, "default", "", bit_adw(32, False), gapruns=True))
    # the longest reads k_nw_ad stages (nw_ad_lds_bytes: maxlen <= 2047), and one base more: the lane kernel of the default band
    cases.append(_mk("ad_maxlen2047", 16, 2047, 0, "default", "", bit_ad(21, 0, "default")))
    cases.append(_mk("ad_maxlen2047_edge_generic", 20, 2047, 0, "generic_a", "", bit_ad(21, 1, "generic")))
    cases.append(_mk("ad_maxlen2048", 16, 2048, 0, "default", "", bit_nw(33, "plain")))
    # the wide kernel: W + 1 either side of its lane-group sizes, default and generic scores; 513 falls to the lane kernels
    for we, gl in ((167, 21), (168, 21), (169, 32), (255, 32), (256, 32), (257, 64), (511, 64), (512, 64)):
        for score in ("default", "generic_a"):
            diff = we - 2 - 2 * 32
            small = we <= 169 or (we == 256 and score == "default")
            cases.append(_mk("wide_we%d_%s" % (we, score), 32, diff + (27 if we <= 169 else 30) if small else max(diff + 40, 230), diff, score, "",
                             bit_adw(gl, score != "default"), small=small))
    for we, gl in ((255, 32), (257, 64)):       # ... reached by the band instead of the length spread
        band = (we - 2 - 53) // 2
        cases.append(_mk("wide_we%d_band%d" % (we, band), band, 123, we - 2 - 2 * band, "generic_b", "", bit_adw(gl, True), small=True))
    cases.append(_mk("wide_we513_falls_to_lane", 32, 600, 447, "default", "", bit_gen()))
    cases.append(_mk("wide_maxlen4095", 32, 4095, 200, "default", "", bit_adw(64, False)))
    # the lane kernels (DADA2HIP_NW_KERNEL=lane): W either side of every class, plain and non-plain; band -1
    for w, wclass in ((33, 33), (34, 65), (65, 65), (66, 129), (129, 129), (130, 193), (193, 193), (194, 257), (257, 257), (258, 0)):
        band = 16 if w <= 34 else 32
        diff = w - 1 - 2 * band
        for score in ("default", "generic_b", "homo_1"):
            form = "nonplain" if score.startswith("homo") else "plain"
            exp = bit_gen() if wclass == 0 else bit_nw(wclass, form)
            cases.append(_mk("lane_w%d_%s" % (w, score), band, max(diff + 40, 120), diff, score, "lane", exp, small=(w <= 130)))
    for score in ("default", "homo_1"):
        cases.append(_mk("lane_unbanded_%s" % score, -1, 120, 30, score, "lane", bit_gen(), small=True))
    names = [c.name for c in cases]
    assert len(set(names)) == len(names)
    return cases


def small_cases():
    return [c for c in aligner_cases() if c.small]


# ---- reads -------------------------------------------------------------------------------------------------------------------
def _rnd(rng, n):
    return "".join("ACGT"[int(x)] for x in rng.integers(0, 4, size=n))


def _sub(rng, s, positions):
    s = list(s)
    for p in positions:
        s[p] = "ACGT"[("ACGT".index(s[p]) + int(rng.integers(1, 4))) & 3]
    return "".join(s)


def _repeat_rich(rng, n):
    """Homopolymer runs, dinucleotide and period-3 repeats between short random stretches: where the DP is full of ties."""
    out = ""
    while len(out) < n:
        kind = int(rng.integers(0, 4))
        if kind == 0:
            out += "ACGT"[int(rng.integers(0, 4))] * int(rng.integers(3, 12))
        elif kind == 1:
            out += _rnd(rng, 2) * int(rng.integers(3, 9))
        elif kind == 2:
            out += _rnd(rng, 3) * int(rng.integers(2, 6))
        else:
            out += _rnd(rng, int(rng.integers(2, 9)))
    return out[:n]


def _fit(rng, s, length):
    """`s` at exactly `length` bases: the 3' end cut off or random bases appended."""
    return s[:length] if len(s) >= length else s + _rnd(rng, length - len(s))


def _reads_of(rng, c, band, minlen, maxlen, lean, gapruns):
    """The reads of one centre `c`: (class, sequence), each fitted to a length of the sample's range."""
    L = len(c)
    out = []
    pick = [0]

    def tlen():
        pick[0] += 1
        return (minlen, maxlen, int(rng.integers(minlen, maxlen + 1)))[pick[0] % 3]

    def add(kind, s, length=None):
        out.append((kind, _fit(rng, s, tlen() if length is None else length)))

    # substitutions only; the first / the last base only
    for k in ((0, 1, 3, 10) if lean else range(0, 11)):
        add("subs%d" % k, _sub(rng, c, rng.choice(L, size=k, replace=False)), L)
    add("first_base", _sub(rng, c, [0]), L)
    add("last_base", _sub(rng, c, [L - 1]), L)
    # one indel 1, 2, band - 1, band, band + 1 bases from either end, and mid-read
    b = max(band, 2)
    offs = sorted({1, 2, b - 1, b, b + 1})
    for j, o in enumerate(offs):
        if o >= L // 2:
            continue
        for end in (0, 1):
            p = o if end == 0 else L - 1 - o
            if (j + end) % 2 == 0 or not lean:
                add("del@%d" % p, c[:p] + c[p + 1:])
            if (j + end) % 2 == 1 or not lean:
                add("ins@%d" % p, c[:p] + "ACGT"[int(rng.integers(0, 4))] + c[p:])
    add("del@mid", c[: L // 2] + c[L // 2 + 1:])
    add("ins@mid", _sub(rng, c[: L // 2] + "ACGT"[int(rng.integers(0, 4))] + c[L // 2:], [L // 3]))
    # a net shift of band - 1, band, band + 1: the path on and past the band's edge
    if band > 0:
        for sh in (band - 1, band, band + 1):
            if sh <= 0 or sh + 12 >= L:
                continue
            add("shift-%d" % sh, c[:10] + c[10 + sh:])                                   # a run of deletions
            add("shift+%d" % sh, c[:10] + _rnd(rng, sh) + c[10:])                        # a run of insertions
            if not lean:
                add("shift-%d@3'" % sh, c[: L - 10 - sh] + c[L - 10:])
    # an indel inside each kind of repeat of the centre (tie order up > left > diagonal decides where the gap goes)
    runs = [p for p in range(2, L - 2) if c[p - 1] == c[p] == c[p + 1] or c[p - 2: p] == c[p: p + 2] or c[p - 3: p] == c[p: p + 3]]
    for p in (rng.choice(runs, size=min(len(runs), 3 if lean else 8), replace=False) if runs else ()):
        p = int(p)
        add("del@repeat", c[:p] + c[p + 1:])
        add("ins@repeat", c[:p] + c[p] + c[p:])
    # many gap runs: a base deleted and one inserted six positions later (far enough apart that two gaps beat the mismatches
    # under every score mode of the table), every twelve positions along the read; run_case counts the runs of the expected alignment
    if gapruns or not lean:
        s, p = list(c), 5
        while p + 12 < len(s):
            del s[p]
            s.insert(p + 6, "ACGT"[int(rng.integers(0, 4))])
            p += 12
        add("gapruns", "".join(s), L)
        if gapruns:
            s, p = list(c), 3
            while p + 12 < len(s):
                s.insert(p, "ACGT"[int(rng.integers(0, 4))])
                del s[p + 7]
                p += 12
            add("gapruns2", _sub(rng, "".join(s), rng.choice(L - 1, size=3, replace=False)), L)
    # 5' / 3' truncations to minlen, both ends ragged
    if L > minlen:
        d = L - minlen
        add("trunc5", _sub(rng, c[d:], [3]), minlen)
        add("trunc3", _sub(rng, c[:minlen], [minlen // 2]), minlen)
        add("ragged", c[d // 2: d // 2 + minlen], minlen)
        add("trunc5+indel", c[d: d + 20] + c[d + 21:], None)
    if L < maxlen:
        d = maxlen - L
        add("extend5", _rnd(rng, d) + c, maxlen)
        add("extend3", c + _rnd(rng, d), maxlen)
        add("extend_both", _rnd(rng, d // 2) + c + _rnd(rng, d - d // 2), maxlen)
    # unrelated, at full length
    add("unrelated", _rnd(rng, maxlen), maxlen)
    # The EDGE masks.  A: a read of minimal length whose path runs along the band's LAST cell against a centre of maximal length
    # (with an odd left band that is the last cell of the lane group), costly enough that a neighbour seen by mistake would win;
    # B, right behind it in the work list: a read one base short of the centre whose path runs, free of cost, along the band's
    # FIRST cell (its left band is even: the first cell of the next lane group).  Pairs of them in every phase of the wave.
    if L == maxlen and maxlen - minlen >= 2 and band >= 2 and minlen > band + 45:
        for k in range(4 if lean else 12):
            body = _sub(rng, c[: minlen - band], rng.choice(40, size=3 + k % 3, replace=False))
            out.append(("edgeA", _rnd(rng, band) + body))
            out.append(("edgeB", c[band + 1:] + _rnd(rng, band)))
            for _ in range(k % 3):
                out.append(("edge_filler", _sub(rng, c, rng.choice(L, size=2, replace=False))))
    return out


Built = namedtuple("Built", "case seqs kinds quals abundances centres err opts skip")


def _quals(rng, seqs, maxlen, qmax):
    n = len(seqs)
    q = np.full((n, maxlen), np.nan)
    for i, s in enumerate(seqs):
        row = rng.integers(0, qmax + 1, size=len(s)).astype(np.float64)
        if i % 3 == 1:                                   # mean qualities of several reads: fractions, exact halves
            frac = rng.choice([0.0, 0.25, 0.5, 0.5, 0.75, 1.0 / 3.0], size=len(s))
            row = np.minimum(row + frac, float(qmax))
        q[i, : len(s)] = row
    return q


def seeded_err(rng, qmax):
    """A 16 x (qmax + 1) matrix with entries from 1e-12 to 1, exact zeros included (lambda = 0 exactly)."""
    e = 10.0 ** rng.uniform(-12, 0, size=(16, qmax + 1))
    e[rng.random(e.shape) < 0.03] = 0.0
    e[rng.random(e.shape) < 0.03] = 1.0
    return e


def build(case, lean=False, grow=0):
    """The sample of a geometry case.  lean: fewer reads per class (the emulator / the reference check).  grow: every centre
    gets lightly changed copies of itself on top (substitutions, an indel in every other one, lengths over the sample's range)
    until the sample has `grow` uniques per centre - the ring's wrap needs more than 512 alignments in one launch."""
    from helpers import tperr1
    rng = np.random.default_rng(case.seed)
    maxlen, minlen = case.maxlen, case.maxlen - case.diff
    big = maxlen > 1000
    lean = lean or big
    cmax = _rnd(rng, maxlen)
    centres = [cmax]
    if case.diff == 0:
        centres.append(_repeat_rich(rng, maxlen))
    else:
        d = case.diff
        centres.append(_sub(rng, cmax[d // 2: d // 2 + minlen], rng.choice(minlen, size=3, replace=False)))       # minimal length
        if not big:
            mid = minlen + (d + 1) // 2
            centres.append(_repeat_rich(rng, mid))                                                              # middle length
    seqs, kinds = [], []
    for ci, c in enumerate(centres):
        seqs.append(c)
        kinds.append("centre%d" % ci)
        if big and ci > 0:
            continue
        for kind, s in _reads_of(rng, c, case.band, minlen, maxlen, lean, case.gapruns):
            seqs.append(s)
            kinds.append("c%d:%s" % (ci, kind))
        for k in range(grow if not (big and ci > 0) else 0):
            s = _sub(rng, c, rng.choice(len(c), size=1 + k % 6, replace=False))
            if k % 2:
                p = int(rng.integers(1, len(s) - 1))
                s = s[:p] + s[p + 1:] if k % 4 == 1 else s[:p] + "ACGT"[int(rng.integers(0, 4))] + s[p:]
            seqs.append(_fit(rng, s, (minlen, maxlen, int(rng.integers(minlen, maxlen + 1)), len(c))[k % 4]))
            kinds.append("c%d:grown%d" % (ci, k % 4))
    keep = {}
    for i, s in enumerate(seqs):
        keep.setdefault(s, i)
    idx = sorted(keep.values())
    seqs, kinds = [seqs[i] for i in idx], [kinds[i] for i in idx]
    lens = [len(s) for s in seqs]
    assert min(lens) == minlen and max(lens) == maxlen, (case.name, min(lens), max(lens), minlen, maxlen)
    centre_idx = [seqs.index(c) for c in centres]
    qmax = 93 if case.seed % 2 else 40
    quals = _quals(rng, seqs, maxlen, qmax)
    err = seeded_err(rng, qmax) if case.seed % 3 == 0 else extend_err(tperr1(), qmax)
    ab = np.array([int(x) for x in rng.integers(1, 50, size=len(seqs))], dtype=np.int32)
    opts = DadaOpts(BAND_SIZE=case.band, GAPLESS=False, **SCORE_MODES[case.score])
    skip = (rng.random(len(seqs)) < 0.3).astype(np.uint8)
    return Built(case, seqs, kinds, quals, ab, centre_idx, err, opts, skip)


# ---- the sweep itself: shared by the GPU module and the emulator job -------------------------------------------------------------
def run_case(api, oracle, case, lean=False):
    """All uniques of the case's sample against each of its centres through dada2hip_sample_compare with every unmasked unique
    sent to the aligner (GAPLESS off, k-mer cutoff 1), pair by pair against `oracle.compare`: lambda bit-equal, hamming equal;
    the launch ledger shows exactly the expected instance.  Returns the number of pairs compared."""
    import os
    b = build(case, lean)
    n = len(b.seqs)
    old = os.environ.get("DADA2HIP_NW_KERNEL")
    if case.route:
        os.environ["DADA2HIP_NW_KERNEL"] = case.route
    else:
        os.environ.pop("DADA2HIP_NW_KERNEL", None)
    npairs = nchecked_runs = 0
    try:
        smp = api.Sample(b.seqs, b.abundances, None, b.quals)
        try:
            read_ledger()
            for k, ci in enumerate(b.centres):
                skip = b.skip if k == len(b.centres) - 1 else None
                lam, ham, cls, st = smp.compare(ci, b.err, b.opts, kdist_cutoff=1.0, skip=skip)
                nskip = int(skip.sum()) if skip is not None else 0
                assert st["nnw"] == n - nskip and st["ngapless"] == 0 and st["nshroud"] == 0, (case.name, st["nnw"], n, nskip)
                L1 = len(b.seqs[ci])
                for i in range(n):
                    if skip is not None and skip[i]:
                        assert cls[i] == 0 and lam[i] == 0.0 and ham[i] == 0xFFFFFFFF, (case.name, i, cls[i], lam[i], ham[i])
                        continue
                    L2 = len(b.seqs[i])
                    wl, wh, _, _ = oracle.compare(b.seqs[ci], b.quals[ci, :L1], b.seqs[i], b.quals[i, :L2], b.err, b.opts, kdist_cutoff=1.0)
                    if not (cls[i] == 3 and int(ham[i]) == wh and lam[i] == wl):
                        raise AssertionError(mismatch_report(oracle, b, ci, i, lam[i], int(ham[i]), wl, wh, read_ledger(False)))
                    npairs += 1
                    if case.gapruns and k == 0 and b.kinds[i] == "c0:gapruns":      # (centre 0 is the random one)
                        nruns = gap_runs(oracle, b, ci, i)
                        assert nruns >= 3 * 64, (case.name, b.kinds[i], "only %d gap runs in the expected alignment" % nruns)
                        nchecked_runs += 1
            if case.gapruns:
                assert nchecked_runs > 0, (case.name, "no gapruns read was checked")
            got = read_ledger() & ~GAPLESS_BITS
            assert got == case.expect, (case.name, "ran", describe(got), "expected", describe(case.expect))
        finally:
            smp.close()
    finally:
        if old is None:
            os.environ.pop("DADA2HIP_NW_KERNEL", None)
        else:
            os.environ["DADA2HIP_NW_KERNEL"] = old
    return npairs, got


RING_GROW = 200        # uniques added per centre: 600 and more in a sample of three centres, 400 and more with two


def ring_cases(small_only=False):
    """The lane cases of every class (plain, generic-score and homopolymer forms) and the unbanded ones: the cases of the wrap."""
    return [c for c in aligner_cases() if c.name.startswith("lane_") and (c.small or not small_only)]


def run_ring_case(api, oracle, case, lean=False):
    """The case's sample grown past 512 uniques, every one of them aligned with each centre (k-mer cutoff 1, GAPLESS off, no skip
    mask: the launch's work is the sample) under a scratch ring of four waves: three trips by dada2hip_nw_ring_trips, every pair
    against the oracle as run_case does (lambda bit-equal, hamming equal), and the same compare with the knob unset - one trip,
    the same bits.  The resident sample's ring is rebuilt at every change of the knob.  One centre per launch (no chunk_centre,
    no view): the cases cover stale slots and second-trip indices, not a per-chunk centre.  Returns (pairs compared, ledger)."""
    import os
    b = build(case, lean, grow=RING_GROW if case.diff else RING_GROW * 3 // 2)
    if len(b.seqs) % 64 == 0:                       # (the last chunk is to be ragged: without the last grown read)
        b = b._replace(seqs=b.seqs[:-1], kinds=b.kinds[:-1], quals=b.quals[:-1], abundances=b.abundances[:-1], skip=b.skip[:-1])
    n = len(b.seqs)
    assert n >= RING_MIN_WORK and n % 64 and max(b.centres) < n, (case.name, n)
    old = os.environ.get("DADA2HIP_NW_KERNEL")
    os.environ["DADA2HIP_NW_KERNEL"] = case.route
    npairs = 0
    try:
        smp = api.Sample(b.seqs, b.abundances, None, b.quals)
        try:
            read_ledger()
            for ci in b.centres:
                with ring(RING_WAVES):
                    lam, ham, cls, st = smp.compare(ci, b.err, b.opts, kdist_cutoff=1.0)
                    trips = read_ring_trips()
                assert st["nnw"] == n and st["ngapless"] == 0 and st["nshroud"] == 0, (case.name, st["nnw"], n)
                assert trips == -(-(-(-n // 64)) // RING_WAVES) >= 3, (case.name, n, "the launch was sized for", trips, "trips: DADA2HIP_NW_RING ignored?")
                with ring(None):
                    lam0, ham0, cls0, _ = smp.compare(ci, b.err, b.opts, kdist_cutoff=1.0)
                    assert read_ring_trips() == 1, case.name
                same = (np.asarray(lam).view(np.uint64) == np.asarray(lam0).view(np.uint64)) & (np.asarray(ham) == np.asarray(ham0)) & (np.asarray(cls) == np.asarray(cls0))
                assert same.all(), (case.name, ci, "the ring's size changed unique", int(np.flatnonzero(~same)[0]))
                L1 = len(b.seqs[ci])
                for i in range(n):
                    wl, wh, _, _ = oracle.compare(b.seqs[ci], b.quals[ci, :L1], b.seqs[i], b.quals[i, : len(b.seqs[i])], b.err, b.opts, kdist_cutoff=1.0)
                    if not (cls[i] == 3 and int(ham[i]) == wh and lam[i] == wl):
                        raise AssertionError(mismatch_report(oracle, b, ci, i, lam[i], int(ham[i]), wl, wh, read_ledger(False)))
                    npairs += 1
            got = read_ledger() & ~GAPLESS_BITS
            assert got == case.expect, (case.name, "ran", describe(got), "expected", describe(case.expect))
        finally:
            smp.close()
    finally:
        if old is None:
            os.environ.pop("DADA2HIP_NW_KERNEL", None)
        else:
            os.environ["DADA2HIP_NW_KERNEL"] = old
    return npairs, got


def run_ring_bimera(api, oracle, n=600, L=120):
    """api.bimera_pairs on n pairs of helpers.bimera_pair_cases under DADA2HIP_NW_KERNEL=lane (k_nw with its move strings kept,
    k_bimera_lr behind it) and a ring of four waves, under every option set of helpers.BIMERA_PAIR_OPTIONS against the oracle.
    The export gives every pair a chunk of its own (one query per chunk, 63 empty slots): n chunks on four waves, the chunk's
    query read through chunk_centre (no view is passed: view_by_chunk is run_ring_whole_path's).  The ledger shows lane instances only; the call with the knob unset gives the same rows
    (its own ring holds ceil(n / 64) waves: it wraps too, which is how the export has always run).  Returns n."""
    import os
    from helpers import BIMERA_PAIR_OPTIONS, bimera_pair_cases
    qs, ps = bimera_pair_cases(21, n, L)
    lane_bits = sum(bit_nw(w, f) for w in NW_CLASSES for f in ("plain", "nonplain", "pair")) | bit_gen(False) | bit_gen(True)
    old = os.environ.get("DADA2HIP_NW_KERNEL")
    os.environ["DADA2HIP_NW_KERNEL"] = "lane"
    try:
        for oo, ms, sc in BIMERA_PAIR_OPTIONS:
            want = oracle.bimera_pairs(qs, ps, oo, *sc, ms)
            with ring(RING_WAVES):
                read_ledger()
                got = api.bimera_pairs(qs, ps, oo, *sc, ms)
                ran = read_ledger() & ~GAPLESS_BITS
                trips = read_ring_trips()
            bad = np.nonzero((got != want).any(axis=1))[0]
            assert bad.size == 0, (oo, ms, sc, describe(ran), [(int(i), qs[i], ps[i], got[i].tolist(), want[i].tolist()) for i in bad[:3]])
            assert ran and not ran & ~lane_bits, describe(ran)
            assert trips == -(-n // RING_WAVES) >= 3, (trips, "trips: DADA2HIP_NW_RING ignored?")
            with ring(None):
                plain = api.bimera_pairs(qs, ps, oo, *sc, ms)
                assert read_ring_trips() < trips
            assert np.array_equal(plain, got), (oo, ms, sc, "the ring's size changed a row")
        # ... and the table form, where a query's parents FILL its chunks (64 lanes live, the query read through chunk_centre)
        mat, seqs = ring_bimera_table()
        for oo, ms in ((False, 16), (True, 8)):
            want = oracle.table_bimera2(mat, seqs, min_fold=1.5, min_abund=2, allow_one_off=oo, max_shift=ms)
            assert 0 < int((want[0] > 0).sum()) < len(seqs)
            with ring(RING_WAVES):
                read_ledger()
                got = api.table_bimera2(mat, seqs, min_fold=1.5, min_abund=2, allow_one_off=oo, max_shift=ms)
                ran = read_ledger() & ~GAPLESS_BITS
                trips = read_ring_trips()
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (oo, ms, np.flatnonzero(got[0] != want[0])[:5])
            assert ran and not ran & ~lane_bits and trips >= 3, (describe(ran), trips)
            with ring(None):
                plain = api.table_bimera2(mat, seqs, min_fold=1.5, min_abund=2, allow_one_off=oo, max_shift=ms)
            assert np.array_equal(plain[0], got[0]) and np.array_equal(plain[1], got[1])
    finally:
        if old is None:
            os.environ.pop("DADA2HIP_NW_KERNEL", None)
        else:
            os.environ["DADA2HIP_NW_KERNEL"] = old
    return n


# the goldens a whole dada() run wraps the ring on: nine and more births (one chunk per birth pair on four waves: three trips)
RING_WHOLE_PATH = ("sam1F_default", "synth3000_default", "sam1F_homogap", "samPB_band32")     # (the last: 1.5 kb reads, ragged)


def run_ring_whole_path(api, oracle, name):
    """dada_uniques on a golden case under DADA2HIP_NW_KERNEL=lane and a ring of four waves.  The two launches of the run's
    finish are the only lane launches that write aligned VIEWS: the final alignments (a centre per chunk through chunk_centre,
    view rows by unique) and the birth pairs (one chunk per birth, view_by_chunk = 1: row = chunk).  With nine births and more
    the birth launch makes three trips and more on four waves and the final one at least as many (a chunk and more per partition), so a view row or a chunk's centre taken from the
    wave's number instead of the chunk's lands in birth_subs, the transition table and the quality tables - all compared, with
    everything else, against the reference's golden and the oracle.  Then the same run with the knob unset: identical."""
    import os
    from helpers import P_RTOL, assert_results_equal, case_inputs
    d, err, pri, opts, exp, meta = case_inputs(name)
    nb = meta["nclust"] - 1
    assert -(-nb // RING_WAVES) >= 3 and len(d.seqs) > 64 * RING_WAVES, (name, nb, len(d.seqs))
    lane_bits = sum(bit_nw(w, f) for w in NW_CLASSES for f in ("plain", "nonplain")) | bit_gen(False)
    env = {"DADA2HIP_NW_KERNEL": "lane"}
    if opts.normalised().HOMOPOLYMER_GAP_PENALTY != opts.normalised().GAP_PENALTY:
        env["DADA2HIP_AD_HOMO"] = "0"                  # (homopolymer gaps on the lane kernels)
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        with ring(RING_WAVES):
            read_ledger()
            got = api.dada_uniques(d.seqs, d.abundances, pri, err, d.quals, opts)
            ran = read_ledger() & ~GAPLESS_BITS
            trips = read_ring_trips()
        assert ran and not ran & ~lane_bits, (name, describe(ran))
        assert trips >= 3, (name, "sized for", trips, "trips: DADA2HIP_NW_RING ignored?")
        assert got.nclust == meta["nclust"] and len(got.birth_subs["pos"]) > 0
        assert_results_equal(got, exp, p_rtol=P_RTOL, check_birth_from="priors" not in meta)
        assert_results_equal(got, oracle.dada_uniques(d.seqs, d.abundances, pri, err, d.quals, opts), p_rtol=P_RTOL, check_birth_from="priors" not in meta)
        with ring(None):
            plain = api.dada_uniques(d.seqs, d.abundances, pri, err, d.quals, opts)
        assert_results_equal(got, plain, exact_float=True)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    return trips


def ring_bimera_table(seed=77, nseq=100, L=110, nsam=3):
    """(mat [samples, sequences], seqs): fourteen variants of one ancestor and two-parent chimeras of them - exact, with a
    substitution, 5' trimmed - with the variants abundant and the chimeras rare, so that a chimera has up to a hundred candidate
    parents: its chunks of 64 are full."""
    rng = np.random.default_rng(seed)
    anc = _rnd(rng, L)
    true = list(dict.fromkeys(_sub(rng, anc, rng.choice(L, size=int(rng.integers(4, 13)), replace=False))[: L - int(rng.integers(0, 6))] for _ in range(14)))
    seqs = list(true)
    while len(seqs) < nseq:
        a, b = (int(x) for x in rng.choice(len(true), 2, replace=False))
        cut = int(rng.integers(10, L - 20))
        ch = true[a][:cut] + true[b][cut:]
        kind = int(rng.integers(0, 3))
        if kind == 1:
            ch = _sub(rng, ch, [int(rng.integers(0, len(ch)))])
        elif kind == 2:
            ch = ch[int(rng.integers(1, 12)):]
        if ch not in seqs:
            seqs.append(ch)
    mat = np.zeros((nsam, len(seqs)), dtype=np.int32)
    nt = len(true)
    mat[:, :nt] = rng.integers(50, 400, size=(nsam, nt))
    mat[:, nt:] = np.sort(rng.integers(2, 40, size=(nsam, len(seqs) - nt)), axis=1)[:, ::-1]
    return mat, seqs


def gap_runs(oracle, b, ci, i):
    """Gap runs (maximal stretches of '-' in either row) of the expected alignment of unique i on centre ci, ends excluded: what
    the many-gap-runs cases exist for (>= 3 AD_RCAP = 192: the traceback's run descriptors go through several chunks)."""
    o = b.opts.normalised()
    a0, a1 = oracle.C_nwalign(b.seqs[ci], b.seqs[i], o.MATCH, o.MISMATCH, o.GAP_PENALTY, o.HOMOPOLYMER_GAP_PENALTY, o.BAND_SIZE, True)
    cols = "".join("0" if x == "-" else ("1" if y == "-" else "m") for x, y in zip(a0, a1)).strip("01")
    return sum(1 for k in range(len(cols)) if cols[k] != "m" and (k == 0 or cols[k - 1] != cols[k]))


def mismatch_report(oracle, b, ci, i, lam, ham, wl, wh, ledger):
    o = b.opts.normalised()
    try:
        al = oracle.C_nwalign(b.seqs[ci], b.seqs[i], o.MATCH, o.MISMATCH, o.GAP_PENALTY, o.HOMOPOLYMER_GAP_PENALTY, o.BAND_SIZE, True)
    except Exception as ex:   # noqa: BLE001
        al = ("(no alignment: %s)" % ex, "")
    return ("case %s, centre %d (%s), unique %d (%s): lambda %r / hamming %d, expected %r / %d\ninstances run: %s\ncentre %s\nraw    %s\n"
            "expected alignment:\n%s\n%s" % (b.case.name, ci, b.kinds[ci], i, b.kinds[i], lam, ham, wl, wh, describe(ledger),
                                             b.seqs[ci], b.seqs[i], al[0], al[1]))


# ---- bimera mode: pair sets on the same W rows (band = max_shift) ------------------------------------------------------------------
# (max_shift, maxlen - minlen, the ledger bit for default scores, ... for user scores): every row of AD_ROWS in the kernel's bimera
# mode, and the two windows past it, where the pairs go to the lane kernel of class 129 (with k_bimera_lr behind it)
LR_ROWS = [(band, diff, bit_lr(gl, edge, False), bit_lr(gl, edge, True)) for band, diff, gl, edge in AD_ROWS] + [
    (band, diff, bit_nw(129, "plain"), bit_nw(129, "plain")) for band, diff in PAST_AD_ROWS]
LR_SCORES = ((5, -4, -8), (4, -5, -7))


def bimera_pair_set(max_shift, diff, seed, L=140, lean=False):
    """(queries, parents): every string between L - diff and L bases (the pair set's window is 2 max_shift + diff + 1), reads of
    every class of `_reads_of` against their centre, either one as the query, plus two-parent chimeras of the centres."""
    rng = np.random.default_rng(seed)
    maxlen, minlen = L, L - diff
    a, b = _rnd(rng, maxlen), _rnd(rng, maxlen)
    centres = [a, _sub(rng, a[: maxlen // 2] + b[maxlen // 2:], [7])]
    if diff:
        centres.append(_sub(rng, a[diff:], [5, 9]))
    qs, ps = [], []
    for c in centres:
        for k, (kind, s) in enumerate(_reads_of(rng, c, max_shift, minlen, maxlen, lean, False)):
            q, p = (c, s) if k % 2 else (s, c)
            qs.append(q); ps.append(p)
    qs += [centres[1], centres[0], centres[-1]]
    ps += [centres[0], centres[1], centres[1]]
    lens = [len(s) for s in qs + ps]
    assert min(lens) == minlen and max(lens) == maxlen, (min(lens), max(lens))
    return qs, ps


# ---- the screen sweep: class (skipped / shrouded / gapless / NW), lambda and hamming of every unique ----------------------------------
SCREEN_OPTIONS = [   # (DadaOpts keywords, k-mer cutoff): cutoffs 1 - dot/d hits exactly, every SSE form, the screens on and off, band 0
    (dict(), 0.42), (dict(), 0.5), (dict(), 0.25),
    (dict(SSE=1), 0.42), (dict(SSE=1), 0.5), (dict(SSE=0), 0.42), (dict(SSE=0), 0.25),      # (SSE 0: ordered distance -1 on unequal lengths)
    (dict(GAPLESS=False), 0.42), (dict(GAPLESS=False, SSE=0), 0.5),
    (dict(USE_KMERS=False), 0.42), (dict(USE_KMERS=False, GAPLESS=False), 0.42),
    (dict(BAND_SIZE=0), 0.42), (dict(BAND_SIZE=0, USE_KMERS=False), 0.42), (dict(BAND_SIZE=0, SSE=1), 0.25),
]
Screen = namedtuple("Screen", "name seqs quals abundances centres err band")


def kdist(a, b):
    """kmer_dist (kmers.cpp:29-51): 1 - (shared 5-mers, with multiplicity) / (5-mers of the shorter read)."""
    code = {"A": 0, "C": 1, "G": 2, "T": 3}

    def counts(s):
        v = np.zeros(1024, dtype=np.int64)
        for p in range(len(s) - 4):
            v[sum(code[s[p + q]] << (2 * (4 - q)) for q in range(5))] += 1
        return v
    return 1. - float(np.minimum(counts(a), counts(b)).sum()) / float(min(len(a), len(b)) - 4)


def _at_cutoffs(rng, c):
    """Reads whose k-mer distance from `c` (the sample's first centre) is EXACTLY 0.5 and exactly 0.25 (the screen shrouds on
    kdist > cutoff: these stay), and their neighbours one shared 5-mer either side: a prefix of `c` and a seeded tail, drawn
    until the distance is the one wanted.  As long as `c`, cut to a multiple of four 5-mers."""
    L = 4 + (len(c) - 4) // 4 * 4
    d = L - 4
    out = []
    for cut in (0.5, 0.25):
        for want in (int(d * (1 - cut)) - 1, int(d * (1 - cut)), int(d * (1 - cut)) + 1):
            for attempt in range(400):
                m = want - attempt % 40
                if m < 1:
                    continue
                s = c[: m + 4] + _rnd(rng, L - m - 4)
                if len(s) == L and kdist(c, s) == 1. - float(want) / float(d):
                    out.append(s)
                    break
    return out


def _screen_from(name, seqs, centres, rng, band, qmax=40):
    from helpers import tperr1
    keep = {}
    for i, s in enumerate(seqs):
        keep.setdefault(s, i)
    seqs = [seqs[i] for i in sorted(keep.values())]
    maxlen = max(len(s) for s in seqs)
    return Screen(name, seqs, _quals(rng, seqs, maxlen, qmax), np.array(rng.integers(1, 50, size=len(seqs)), dtype=np.int32),
                  [seqs.index(c) for c in centres], extend_err(tperr1(), qmax), band)


def screen_samples():
    out = []
    by_name = {c.name: c for c in aligner_cases()}
    for name in ("ad_b16_d0_default_l", "ad_b16_d9_default_l", "ad_b32_d60_default_l", "past_b32_d63_default_l", "wide_we256_default"):
        b = build(by_name[name])
        rng = np.random.default_rng(by_name[name].seed + 1)
        # + reads at every k-mer distance from a centre: d = len - 4 k-mers, a block of changed bases removes about as many as it is long
        c = b.seqs[b.centres[0]]
        far = [c[:p] + _rnd(rng, n) + c[p + n:] for n in range(5, len(c) - 10, 7) for p in (3, len(c) // 3)]
        out.append(_screen_from(name, b.seqs + far + _at_cutoffs(rng, c), [b.seqs[i] for i in b.centres], rng, by_name[name].band))
    # reads of 6-20 nt
    rng = np.random.default_rng(606)
    cs = [_rnd(rng, 20), _rnd(rng, 6), _rnd(rng, 13)]
    seqs = list(cs)
    for c in cs:
        for _ in range(25):
            s = list(c)
            for _ in range(int(rng.integers(0, 3))):
                s[int(rng.integers(0, len(s)))] = "ACGT"[int(rng.integers(0, 4))]
            s = "".join(s)[int(rng.integers(0, 3)):]
            seqs.append(_fit(rng, s, int(rng.integers(6, 21))))
    seqs += [_rnd(rng, int(rng.integers(6, 21))) for _ in range(30)] + _at_cutoffs(rng, cs[0])
    out.append(_screen_from("short_6_20", seqs, cs, rng, 16))
    # low complexity: one 5-mer more than 63 and more than 255 times in a read (the 8-bit tables of the reference saturate and it
    # falls back to the 16-bit ones; the device corrects its rank-capped overlap exactly)
    rng = np.random.default_rng(707)
    cs = []
    for run in (70, 130, 300):
        cs.append(_rnd(rng, 40) + "A" * run + _rnd(rng, 40))
        cs.append(_rnd(rng, 30) + "AC" * (run // 2) + "ACGTT" * (run // 5) + _rnd(rng, 20))
    seqs = list(cs)
    for c in cs:
        L = len(c)
        for k in range(14):
            s = _sub(rng, c, rng.choice(L, size=k % 5, replace=False))
            if k % 3 == 1:
                s = s[: L // 2] + s[L // 2 + 1 + k % 2:]               # a base or two less inside the repeat
            if k % 3 == 2:
                s = s[: L // 2] + c[L // 2] * (1 + k % 4) + s[L // 2:]
            seqs.append(s)
        seqs.append("A" * (L - 7))
    seqs += _at_cutoffs(rng, cs[0])
    out.append(_screen_from("low_complexity", seqs, cs, rng, 16))
    return out


def run_screen(api, oracle, smp_case, kw, cutoff):
    """One sample of the screen sweep under one option set: every unique's class, lambda and hamming against the oracle, the class
    by raw_align's rule from the oracle's kdist / kodist.  Returns (the number of comparisons of each class, the number whose k-mer
    distance equals the cutoff exactly)."""
    s = smp_case
    opts = DadaOpts(**dict(dict(BAND_SIZE=s.band), **kw))
    o = opts.normalised()
    n = len(s.seqs)
    rng = np.random.default_rng(n)
    skip = (rng.random(n) < 0.1).astype(np.uint8)
    counts = [0, 0, 0, 0]
    at_cutoff = 0
    smp = api.Sample(s.seqs, s.abundances, None, s.quals)
    try:
        for k, ci in enumerate(s.centres):
            sk = skip if k == len(s.centres) - 1 else None      # (the reads at the exact cutoffs belong to the first centre)
            lam, ham, cls, st = smp.compare(ci, s.err, opts, kdist_cutoff=cutoff, skip=sk)
            L1 = len(s.seqs[ci])
            for i in range(n):
                if sk is not None and sk[i]:
                    want = (0, 0.0, 0xFFFFFFFF)
                else:
                    wl, wh, kd, ko = oracle.compare(s.seqs[ci], s.quals[ci, :L1], s.seqs[i], s.quals[i, : len(s.seqs[i])], s.err, opts, kdist_cutoff=cutoff)
                    at_cutoff += int(o.USE_KMERS and kd == cutoff)
                    if o.USE_KMERS and kd > cutoff:
                        assert wh < 0, (s.name, i, kd, wh)
                        want = (1, 0.0, 0xFFFFFFFF)
                    else:
                        want = (2 if (o.BAND_SIZE == 0 or (o.GAPLESS and o.USE_KMERS and ko == kd)) else 3, wl, wh)
                got = (int(cls[i]), float(lam[i]), int(ham[i]))
                assert got == want, (s.name, kw, cutoff, "centre", ci, "unique", i, s.seqs[i], got, want)
                counts[want[0]] += 1
            assert (st["nskipped"], st["nshroud"], st["ngapless"], st["nnw"]) == tuple(
                int(np.sum(cls == v)) for v in range(4)), (s.name, kw, cutoff, st)
    finally:
        smp.close()
    return counts, at_cutoff
