"""removePrimers restated (R/filter.R:81-233) on Python strings, and the cases the CPU, emulator and GPU tests run against it.

The restatement follows the R wrapper line by line (the references in the comments are to R/filter.R).  What the wrapper calls
and this file has to restate from documentation is vmatchPattern(primer, reads, max.mismatch, with.indels = FALSE, fixed =
C_isACGT(primer)): `vmatch` below, the naive double loop over starts and letters - deliberately another algorithm than the
kernel's bit planes and bit-sliced counter.  The range of match starts (Biostrings' "out of limits" matches) is start_range(), and
nowhere else.

A case takes the module dada2_amd.primers and raises AssertionError.  CASES / CASE_NAMES / emu_run() as in tests/filter_cases.py:
tests/test_gpu_primers.py runs every case on the card, tests/test_emu_primers.py under the emulator; check_strided_batch is the
card's alone."""
import gzip
import os
import random

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
EXAMPLE = os.path.join(GOLDEN, "samPBprimers.fastq.gz")
F27 = "AGRGTTYGATYMTGGCTCAG"            # the reference's documented call (:74-78)
R1492 = "RGYTACCTTGTTACGACTT"
NA = -2 ** 31
CODES = ("kept", "no_fwd", "no_rev", "nothing_left", "bad_letter")

IUPAC = {"A": 1, "C": 2, "G": 4, "T": 8, "M": 3, "R": 5, "W": 9, "S": 6, "Y": 10, "K": 12, "V": 7, "H": 11, "D": 13, "B": 14, "N": 15}
_COMP = {"A": "T", "C": "G", "G": "C", "T": "A", "M": "K", "K": "M", "R": "Y", "Y": "R", "V": "B", "B": "V", "H": "D", "D": "H",
         "W": "W", "S": "S", "N": "N"}
SETS = {c: "".join(b for b in "ACGT" if IUPAC[c] & IUPAC[b]) for c in IUPAC}


def rc(s):
    """reverseComplement with Biostrings' complement of the IUPAC codes."""
    return "".join(_COMP[c] for c in reversed(s))


def is_acgt(s):
    """C_isACGT (:111-112)."""
    return all(c in "ACGT" for c in s)


def start_range(n, L, mm):
    """THE range of match starts, 0-based and inclusive: up to mm letters of a match may lie outside the read."""
    return -mm, n - L + mm


def vmatch(primer, read, mm, fixed):
    """The starts (0-based, ascending) at which at most mm of the primer's letters mismatch; a position outside the read is a
    mismatch; fixed: equal bytes, otherwise the letters' IUPAC sets intersect."""
    n, L = len(read), len(primer)
    lo, hi = start_range(n, L, mm)
    out = []
    for st in range(lo, hi + 1):
        bad = 0
        for i in range(L):
            p = st + i
            if p < 0 or p >= n:
                bad += 1
            elif fixed:
                bad += primer[i] != read[p]
            else:
                bad += (IUPAC[primer[i]] & IUPAC[read[p]]) == 0
            if bad > mm:
                break
        if bad <= mm:
            out.append(st)
    return out


def restate_read(seq, primer_fwd, primer_rev=None, max_mismatch=2, orient=True, trim_fwd=True, trim_rev=True):
    """One read through :126-211.  first / last: 1-based, inclusive, in the kept orientation (0 for codes 1, 2 and 4); hits and
    starts in the order fwd, rev, fwd on rc, rev on rc, the starts 1-based on their strand, NA without a match."""
    if any(c not in IUPAC for c in seq):
        return dict(code=4, flip=0, first=0, last=0, hits=(0,) * 4, starts=(NA,) * 8)
    n, has_rev = len(seq), primer_rev is not None
    m = [vmatch(primer_fwd, seq, max_mismatch, is_acgt(primer_fwd)),                               # :126
         vmatch(primer_rev, seq, max_mismatch, is_acgt(primer_rev)) if has_rev else [], [], []]   # :132
    if orient:                                                                                     # :136-150
        seq_rc = rc(seq)
        m[2] = vmatch(primer_fwd, seq_rc, max_mismatch, is_acgt(primer_fwd))
        if has_rev:
            m[3] = vmatch(primer_rev, seq_rc, max_mismatch, is_acgt(primer_rev))
    hits = tuple(len(x) for x in m)
    starts = tuple(v for x in m for v in ((x[0] + 1, x[-1] + 1) if x else (NA, NA)))
    flip = int(bool(orient and not m[0] and m[2]))                                                 # :181
    mf, mr = (m[2], m[3]) if flip else (m[0], m[1])                                                # :184-188
    code, first, last = 0, 0, 0
    if not mf:                                                                                     # :193
        code = 1
    elif has_rev and not mr:                                                                       # :194
        code = 2
    else:
        first = (mf[0] + 1) + len(primer_fwd) - 1 + 1 if trim_fwd else 1                           # :164, :202: end(first match) + 1
        last = (mr[-1] + 1) - 1 if (has_rev and trim_rev) else n                                   # :165, :207: start(last match) - 1
        if not last > first:                                                                       # :211
            code = 3
    return dict(code=code, flip=flip, first=first, last=last, hits=hits, starts=starts)


def restate_fastq(records, primer_fwd, primer_rev=None, **kw):
    """(reads in, the records written) of one file: `records` are (id line, sequence, qualities)."""
    want = [restate_read(s, primer_fwd, primer_rev, **kw) for _, s, _ in records]
    if any(w["code"] == 4 for w in want):
        raise ValueError("a letter outside the IUPAC codes")
    if sum(w["hits"][0] for w in want) == 0 or (primer_rev is not None and sum(w["hits"][1] for w in want) == 0):   # :157-158
        return len(records), []
    out = []
    for (h, s, q), w in zip(records, want):
        if w["code"] != 0:
            continue
        if w["flip"]:                                                                              # :183
            s, q = rc(s), q[::-1]
        out.append((h, s[w["first"] - 1: w["last"]], q[w["first"] - 1: w["last"]]))                # :213
    return len(records), out


# ---- files -----------------------------------------------------------------------------------------------------------------------

def read_fastq(path):
    op = gzip.open if open(path, "rb").read(2) == b"\x1f\x8b" else open
    with op(path, "rt") as fh:
        lines = fh.read().split("\n")
    return [(lines[i], lines[i + 1], lines[i + 3]) for i in range(0, len(lines) - 3, 4)]


def fastq_text(records):
    return "".join("%s\n%s\n+\n%s\n" % r for r in records)


def write_fastq(path, records, gz=False):
    with (gzip.open if gz else open)(path, "wt") as fh:
        fh.write(fastq_text(records))


def read_text(path):
    with open(path, "rb") as fh:
        data = fh.read()
    return (gzip.decompress(data) if data[:2] == b"\x1f\x8b" else data).decode()


# ---- reads with primers in them ----------------------------------------------------------------------------------------------------

def rand_seq(rng, n, letters="ACGT"):
    return "".join(rng.choice(letters) for _ in range(n))


def instance(rng, primer, nmis=0, where=None):
    """A concrete A/C/G/T word the primer matches with exactly nmis mismatches, placed at the positions `where` allows."""
    w = [rng.choice(SETS[c]) for c in primer]
    can = [i for i, c in enumerate(primer) if c != "N" and (where is None or where(i))]
    for i in rng.sample(can, nmis):
        w[i] = rng.choice([b for b in "ACGT" if b not in SETS[primer[i]]])
    return "".join(w)


def plant(read, word, st):
    """`read` with `word` written from start st on (the letters that fall outside the read are dropped)."""
    r = list(read)
    for i, ch in enumerate(word):
        if 0 <= st + i < len(r):
            r[st + i] = ch
    return "".join(r)


def amplicon(rng, n, fwd, rev, mis=(0, 0), flip=False, lead=None, tail=None):
    """lead + fwd + insert + rev + tail, n letters in all, as given or reverse-complemented."""
    lead = rng.randrange(0, 30) if lead is None else lead
    tail = rng.randrange(0, 30) if tail is None else tail
    body = max(0, n - lead - tail - len(fwd) - (len(rev) if rev else 0))
    s = rand_seq(rng, lead) + instance(rng, fwd, mis[0]) + rand_seq(rng, body) + (instance(rng, rev, mis[1]) if rev else "") + rand_seq(rng, tail)
    return rc(s) if flip else s


# ---- the library against the restatement -------------------------------------------------------------------------------------------

def with_env(env, f):
    env = {k: str(v) for k, v in (env or {}).items()}
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return f()
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def check_reads(pr, seqs, fwd, rev=None, what="", stats=None, **kw):
    """Every output of dada2hip_primers_reads for every read, against restate_read.  Returns the restated reads."""
    st = {} if stats is None else stats
    got = pr.primer_hits(seqs, fwd, rev, stats=st, **kw)
    want = [restate_read(s, fwd, rev, **kw) for s in seqs]
    assert len(got["code"]) == len(seqs)
    for i, w in enumerate(want):
        g = (int(got["code"][i]), int(got["flip"][i]), int(got["first"][i]), int(got["last"][i]), tuple(got["hits"][i].tolist()),
             tuple(got["starts"][i].reshape(-1).tolist()))
        e = (w["code"], w["flip"], w["first"], w["last"], w["hits"], w["starts"])
        assert g == e, (what, i, len(seqs[i]), "got", g, "want", e)
    codes = [w["code"] for w in want]
    assert st["reads_in"] == len(seqs) and st["reads_kept"] == codes.count(0), (what, st)
    for c in (1, 2, 3):
        assert st["dropped_" + CODES[c]] == codes.count(c), (what, c, st)
    assert st["flipped"] == sum(w["flip"] for w in want), (what, st)
    assert st["multiple_matches"] == sum(1 for w in want if max(w["hits"]) > 1), (what, st)
    assert st["hits_fwd"] == sum(w["hits"][0] for w in want) and st["hits_rev"] == sum(w["hits"][1] for w in want), (what, st)
    return want


LENGTHS = (0, 1, 19, 20, 21, 63, 64, 65, 127, 128, 129, 2129, 5000)      # L - 1, L, L + 1 of the 20-letter primer among them


def case_lengths(pr):
    rng = random.Random(201)
    rev = rc(R1492)
    seqs = []
    for n in LENGTHS:
        seqs += [rand_seq(rng, n), plant(rand_seq(rng, n), instance(rng, F27), 0), plant(rand_seq(rng, n), instance(rng, F27, 1), max(0, n - 20)),
                 amplicon(rng, n, F27, rev, flip=bool(n & 1)) if n >= 45 else rc(plant(rand_seq(rng, n), instance(rng, F27), 0))]
    want = check_reads(pr, seqs, F27, rev, "lengths")
    assert {0, 1, 2} <= {w["code"] for w in want} and any(w["flip"] for w in want)
    check_reads(pr, seqs, F27, None, "lengths, no reverse primer")
    check_reads(pr, seqs, F27, rev, "lengths, as given", orient=False, max_mismatch=0)
    check_reads(pr, seqs, "ACGTTGCAAGGTCCAT", None, "lengths, fixed primer", max_mismatch=3)


def case_batches(pr):
    rng = random.Random(202)
    rev = rc(R1492)
    for n in (1, 63, 64, 65, 4097):
        seqs = [amplicon(rng, rng.choice((60, 64, 65, 90, 131)), F27, rev, mis=(rng.randrange(4), rng.randrange(4)), flip=rng.random() < 0.5)
                for _ in range(n)]
        want = check_reads(pr, seqs, F27, rev, "batch of %d" % n)
        assert n < 60 or {0, 1, 2} <= {w["code"] for w in want}
    assert pr.primer_hits([], F27)["code"].shape == (0,)


def case_chunk_boundaries(pr):
    """A planted primer at every start around a word boundary, at both ends of the read and hanging over them."""
    rng = random.Random(203)
    for primer, mm in ((F27, 2), ("ACGTTGCAAGGTCCATCAGT", 2), ("ACGTTGCAAGGTCCATCAGTTGACCA" + "GATTACAGATTACAGG", 3)):
        L, n = len(primer), 200
        seqs, planted = [], []
        for st in list(range(64 - L - 1, 66)) + list(range(128 - L - 1, 130)) + [0, n - L]:
            seqs.append(plant(rand_seq(rng, n), instance(rng, primer, rng.randrange(mm + 1)), st))
            planted.append(st)
        inside = lambda st: (lambda i: 0 <= st + i < n)   # noqa: E731
        for k in range(1, mm + 2):                        # k letters outside: a match while k <= mm, with exactly mm - k mismatches inside
            for st in (-k, n - L + k):
                seqs.append(plant(rand_seq(rng, n), instance(rng, primer, max(0, mm - k), inside(st)), st))
                planted.append(st if k <= mm else None)
        want = check_reads(pr, seqs, primer, None, "boundaries of %s" % primer, max_mismatch=mm, orient=False)
        for w, st in zip(want, planted):
            assert w["hits"][0] == (0 if st is None else 1) and (st is None or w["starts"][0] == st + 1), (primer, st, w)
        check_reads(pr, [rc(s) for s in seqs], primer, None, "boundaries of %s on rc" % primer, max_mismatch=mm)


def case_mismatch_budget(pr):
    """Exactly mm and mm + 1 mismatches; windows that mismatch everywhere must not wrap the counter into a match."""
    rng = random.Random(204)
    primer = "ACGTTGCAAGGTCCATCAGTTGACCAGATTAC"      # 32 letters
    for mm in (0, 1, 2, 3, 7, 15):
        seqs = [plant(rand_seq(rng, 150), instance(rng, primer, k), rng.randrange(0, 150 - 32)) for k in (mm, mm + 1) for _ in range(4)]
        want = check_reads(pr, seqs, primer, None, "budget %d" % mm, max_mismatch=mm)
        # (15 of 32 letters may differ: a random window does that now and then, so there only the planted matches are asked for)
        assert [w["hits"][0] for w in want] == [1] * 4 + [0] * 4 if mm < 15 else all(w["hits"][0] >= 1 for w in want[:4]), (mm, want)
        deg = "ACGTTGCAAGGTCCATCAGTYGACCAGATTAC"
        want = check_reads(pr, seqs, deg, rc(primer[:18]), "budget %d, IUPAC" % mm, max_mismatch=mm)
    for L in (17, 32, 33, 64, 128):
        for mm in (0, 1, 3, 7, 15):
            want = check_reads(pr, ["C" * (L + 70), "C" * L, "CCG" * 50], "A" * L, "W" * L, "all %d mismatch, mm %d" % (L, mm), max_mismatch=mm)
            assert all(w["hits"] == (0, 0, 0, 0) for w in want), (L, mm)


def case_letters(pr):
    """Every IUPAC code of the primer against every letter of the read, under both comparison rules."""
    codes = "ACGTMRWSYKVHDBN"
    for pc in codes:
        primer = "NACGTTGCAAC" + pc                       # not fixed: it holds an N
        seqs = ["GG" + "TACGTTGCAAC" + rcode + "GG" for rcode in codes]
        want = check_reads(pr, seqs, primer, None, "letter %s" % pc, max_mismatch=0, orient=False)
        assert [w["hits"][0] for w in want] == [int((IUPAC[pc] & IUPAC[r]) != 0) for r in codes], pc
        check_reads(pr, seqs, primer, primer[::-1], "letter %s, both strands" % pc, max_mismatch=1)
    fixed, deg = "ACGTTGCAAGGT", "ACGTTGCAAGGY"
    seqs = ["TT" + "ACGTTGCAAGGT" + "CC", "TT" + "ACGTNGCAAGGT" + "CC", "TT" + "ACGTRGCAAGGT" + "CC", "N" * 30]
    want = check_reads(pr, seqs, fixed, None, "N under a fixed primer", max_mismatch=0)
    assert [w["hits"][0] for w in want] == [1, 0, 0, 0]
    want = check_reads(pr, seqs, deg, None, "N under a degenerate primer", max_mismatch=0)
    assert [w["hits"][0] for w in want] == [1, 1, 0, 30 - 12 + 1]
    E = pr._lib.Dada2HipError
    for bad in ("ACGTacgtACGTACGTACGTACGT", "ACGTACGTXACGTACGTACGTACG", "ACGT-ACGTTGCAAGGT", "U" + "ACGTTGCAAGGT"):
        _raises(E, lambda: pr.primer_hits(seqs[:2] + [bad], fixed), "read 3", code=4)
        assert restate_read(bad, fixed)["code"] == 4
    for p in ("ACGTacgt", "ACGTXACG", "ACGU"):
        _raises(E, lambda: pr.primer_hits(seqs, p, max_mismatch=0), code=4)
        _raises(E, lambda: pr.primer_hits(seqs, fixed, p, max_mismatch=0), code=4)


def case_multiple_hits(pr):
    """The first forward and the last reverse match, on both strands; an all-N primer matches at every start."""
    rng = random.Random(206)
    fwd, rev = "ACGTTGCAAGGTCCATCA", "GGATTACAGATTACAGCC"
    seqs = []
    for nf in (1, 2, 3):
        for nr in (1, 2, 3):
            parts = [rand_seq(rng, 7)]
            for _ in range(nf):
                parts += [instance(rng, fwd, rng.randrange(2)), rand_seq(rng, rng.randrange(5, 40))]
            for _ in range(nr):
                parts += [instance(rng, rev, rng.randrange(2)), rand_seq(rng, rng.randrange(5, 40))]
            s = "".join(parts)
            seqs += [s, rc(s)]
    want = check_reads(pr, seqs, fwd, rev, "multiple hits", max_mismatch=1)
    assert {(w["hits"][0] + w["hits"][2], w["hits"][1] + w["hits"][3]) for w in want} == {(a, b) for a in (1, 2, 3) for b in (1, 2, 3)}
    assert all(w["code"] == 0 for w in want) and [w["flip"] for w in want] == [0, 1] * 9
    check_reads(pr, seqs, fwd, rev, "multiple hits, untrimmed", max_mismatch=1, trim_fwd=False, trim_rev=False)
    for n in (5, 30, 64, 200, 4200):
        for mm in (0, 2):
            want = check_reads(pr, [rand_seq(rng, n)], "N" * 12, "N" * 30, "all-N primers on %d" % n, max_mismatch=mm)
            assert want[0]["hits"][0] == max(0, n - 12 + 2 * mm + 1) and want[0]["hits"][1] == max(0, n - 30 + 2 * mm + 1), want


def orientation_reads(rng, fwd, rev):
    body = lambda: rand_seq(rng, 120)   # noqa: E731
    forward = rand_seq(rng, 9) + instance(rng, fwd) + body() + instance(rng, rev) + rand_seq(rng, 6)
    both = rand_seq(rng, 9) + instance(rng, fwd) + body() + rc(instance(rng, fwd)) + body() + instance(rng, rev) + rand_seq(rng, 4)
    split = rand_seq(rng, 9) + instance(rng, fwd) + body() + rc(instance(rng, rev)) + rand_seq(rng, 6)   # rev on rc only: dropped
    return [forward, rc(forward), both, split, body()]


def case_orientation(pr):
    rng = random.Random(207)
    fwd, rev = F27, rc(R1492)
    seqs = orientation_reads(rng, fwd, rev)
    want = check_reads(pr, seqs, fwd, rev, "orientation")
    assert [(w["code"], w["flip"]) for w in want] == [(0, 0), (0, 1), (0, 0), (2, 0), (1, 0)], want
    assert want[2]["hits"][0] == 1 and want[2]["hits"][2] == 1 and want[3]["hits"] == (1, 0, 0, 1)
    want = check_reads(pr, seqs, fwd, rev, "orientation off", orient=False)
    assert [w["code"] for w in want] == [0, 1, 0, 2, 1] and all(w["hits"][2:] == (0, 0) for w in want)
    check_reads(pr, seqs, fwd, None, "orientation, no reverse primer")
    pal_f, pal_r = "ACGTTGCAATTGCAACGT", "GGATCCAAGCTTGGATCC"                 # their own reverse complements
    assert rc(pal_f) == pal_f and rc(pal_r) == pal_r
    seqs = orientation_reads(rng, pal_f, pal_r)
    want = check_reads(pr, seqs, pal_f, pal_r, "palindromic primers", max_mismatch=1)
    assert not any(w["flip"] for w in want) and want[0]["hits"][0] == want[0]["hits"][2] == 1


def case_window(pr):
    rng = random.Random(208)
    fwd, rev = "ACGTTGCAAGGTCCATCA", "GGATTACAGATTACAGCC"
    seqs = []
    for gap in (0, 1, 2, 3, 50):                          # letters between the primers: last - first + 1
        seqs.append(rand_seq(rng, 5) + fwd + rand_seq(rng, gap, "T") + rev + rand_seq(rng, 5))
    seqs.append(rand_seq(rng, 5) + rev + rand_seq(rng, 30, "T") + fwd + rand_seq(rng, 5))        # the reverse match left of the forward one
    seqs.append(fwd + rand_seq(rng, 40, "T") + rev)
    seqs.append(rand_seq(rng, 3, "T") + fwd[:10] + rev[8:] + "T")
    seqs += [rc(s) for s in seqs]
    want = check_reads(pr, seqs, fwd, rev, "window", max_mismatch=0)
    assert [w["code"] for w in want[:7]] == [3, 3, 0, 0, 0, 3, 0], want[:7]
    assert (want[1]["first"], want[1]["last"]) == (24, 24) and (want[2]["first"], want[2]["last"]) == (24, 25)
    for tf in (True, False):
        for tr in (True, False):
            check_reads(pr, seqs, fwd, rev, "window, trims %s %s" % (tf, tr), max_mismatch=1, trim_fwd=tf, trim_rev=tr)
            check_reads(pr, seqs, fwd, None, "window, no reverse primer %s" % tf, max_mismatch=1, trim_fwd=tf, trim_rev=tr)
    want = check_reads(pr, ["A", "AC", fwd, fwd + "A", fwd + "AC"], fwd, None, "short windows", max_mismatch=0, trim_fwd=False)
    want = check_reads(pr, ["A", "AC", fwd, fwd + "A", fwd + "AC"], fwd, None, "short windows", max_mismatch=0)
    assert [w["code"] for w in want] == [1, 1, 3, 3, 0]


def tile_reads(rng, fwd, rev):
    """100 to 400 letters: matches in the first and the last word of a tile, across its border, first and last hit tiles apart."""
    seqs = []
    for n in (100, 127, 128, 129, 191, 192, 193, 256, 300, 400):
        for st in (0, 44, 45, 63, 64, 100, 108, 109, 127, 128, 172, 173):
            if st + len(fwd) <= n:
                seqs.append(plant(plant(rand_seq(rng, n), instance(rng, fwd, 1), st), instance(rng, rev, 1), n - len(rev) - rng.randrange(3)))
        seqs.append(amplicon(rng, n, fwd, rev, flip=True))
        seqs.append(plant(plant(plant(rand_seq(rng, n), instance(rng, fwd), 2), instance(rng, fwd), 50), instance(rng, fwd), n - len(fwd) - 1))
    return seqs


def case_tiles_and_pieces(pr):
    rng = random.Random(209)
    fwd, rev = F27, rc(R1492)
    seqs = tile_reads(rng, fwd, rev)
    base = {}
    want = check_reads(pr, seqs, fwd, rev, "one tile", stats=base)
    assert base["pieces"] == 1 and base["tiles"] == len(seqs), base
    assert any(w["hits"][0] > 1 and w["starts"][1] - w["starts"][0] > 128 for w in want)
    for tile in (1, 2):
        st = {}
        with_env({"DADA2HIP_PRIMERS_TILE": tile}, lambda: check_reads(pr, seqs, fwd, rev, "tile %d" % tile, stats=st))
        chunks = [(max(0, len(s) - 19 + 2 * 2 + 1) + 63) // 64 for s in seqs]
        assert st["tiles"] == sum(max(1, -(-c // tile)) for c in chunks) > len(seqs), (tile, st)
        with_env({"DADA2HIP_PRIMERS_TILE": tile}, lambda: check_reads(pr, seqs[:40], "N" * 40, "ACGTTGCAAG", "tile %d, all-N" % tile, max_mismatch=3))
    for piece in (1, 2, 7, 64):
        st = {}
        with_env({"DADA2HIP_PRIMERS_PIECE": piece, "DADA2HIP_PRIMERS_TILE": 2}, lambda: check_reads(pr, seqs, fwd, rev, "piece %d" % piece, stats=st))
        assert st["pieces"] == -(-len(seqs) // piece), (piece, st)
    st = {}
    with_env({"DADA2HIP_PRIMERS_PIECE_BYTES": 1000}, lambda: check_reads(pr, seqs, fwd, rev, "pieces by bytes", stats=st))
    assert 1 < st["pieces"] < len(seqs), st
    long_read = plant(plant(plant(rand_seq(rng, 9000), instance(rng, fwd), 4085), instance(rng, fwd), 10), instance(rng, rev), 8900)
    st = {}
    want = check_reads(pr, [long_read, rc(long_read), seqs[0]], fwd, rev, "past the default tile", stats=st)
    assert st["tiles"] == 3 + 3 + 1 and want[0]["hits"][0] == 2 and want[1]["flip"] == 1, (st, want)


def case_random_sweep(pr):
    rng = random.Random(210)
    fwd, rev = F27, rc(R1492)
    seqs = []
    for _ in range(2500):
        n = rng.randrange(40, 260)
        kind = rng.random()
        if kind < 0.1:
            s = rand_seq(rng, n, "ACGTN" if rng.random() < 0.5 else "ACGT")
        else:
            s = rand_seq(rng, n)
            for primer in (fwd, rev):
                if rng.random() < 0.85:
                    s = plant(s, instance(rng, primer, rng.randrange(0, 5)), rng.randrange(-3, n - 15))
            if rng.random() < 0.5:
                s = rc(s)
        seqs.append(s)
    want = check_reads(pr, seqs, fwd, rev, "sweep")
    assert {0, 1, 2, 3} <= {w["code"] for w in want} and 200 < sum(w["flip"] for w in want)
    check_reads(pr, seqs[:800], "ACGTTGCAAGGTCCATCAGT", None, "sweep, fixed", max_mismatch=5)


# ---- files -------------------------------------------------------------------------------------------------------------------------

def check_file(pr, src, records, tmp, name, fwd, rev=None, compress=False, **kw):
    out = os.path.join(tmp, name)
    st = {}
    got = pr.primers_fastq(src, out, fwd, rev, compress=compress, stats=st, **kw)
    nin, want = restate_fastq(records, fwd, rev, **{k: v for k, v in kw.items() if k != "n"})
    assert got == (nin, len(want)), (name, got, nin, len(want))
    if not want:
        assert not os.path.exists(out), name
        return st
    with open(out, "rb") as fh:
        assert (fh.read(2) == b"\x1f\x8b") == bool(compress), name
    assert read_text(out) == fastq_text(want), name
    return st


def case_example_file(pr, tmp):
    records = read_fastq(EXAMPLE)
    rev = rc(R1492)
    plain = os.path.join(tmp, "example.fastq")
    write_fastq(plain, records)
    for src in (EXAMPLE, plain):
        for compress in (False, True):
            st = check_file(pr, src, records, tmp, "out.fastq" + (".gz" if compress else ""), F27, rev, compress=compress)
            assert (st["reads_in"], st["reads_kept"], st["flipped"]) == (50, 45, 25), st
    check_file(pr, EXAMPLE, records, tmp, "nr.fastq", F27, None)
    check_file(pr, EXAMPLE, records, tmp, "as_given.fastq", F27, rev, orient=False)
    check_file(pr, plain, records, tmp, "chunks.fastq", F27, rev, n=7)
    check_file(pr, plain, records, tmp, "untrimmed.fastq.gz", F27, rev, compress=True, trim_fwd=False, trim_rev=False, max_mismatch=1)
    from dada2_amd import api
    d = api.derep_fastq(os.path.join(tmp, "out.fastq.gz"))                     # the output feeds the next stage
    _, want = restate_fastq(records, F27, rev)
    assert sum(int(a) for a in d.abundances) == 45 and set(d.seqs) == {s for _, s, _ in want}


def case_file_rules(pr, tmp):
    rng = random.Random(212)
    fwd, rev = F27, rc(R1492)
    q = lambda s: "".join(chr(33 + (7 * i) % 40) for i in range(len(s)))   # noqa: E731
    recs = lambda seqs: [("@r%d some text" % i, s, q(s)) for i, s in enumerate(seqs)]   # noqa: E731
    src = os.path.join(tmp, "in.fastq")
    # the whole-file rule: reverse-oriented reads only - every read would flip, and nothing is written
    flipped = recs([amplicon(rng, 150, fwd, rev, flip=True) for _ in range(20)])
    write_fastq(src, flipped)
    assert all(restate_read(s, fwd, rev)["code"] == 0 for _, s, _ in flipped)
    st = check_file(pr, src, flipped, tmp, "rule.fastq", fwd, rev)
    assert st["flipped"] == 20 and st["hits_fwd"] == 0 and st["reads_kept"] == 0, st
    # ... and one read as given among them releases the file
    mixed = flipped[:10] + recs([amplicon(rng, 150, fwd, rev)]) + flipped[10:]
    write_fastq(src, mixed)
    check_file(pr, src, mixed, tmp, "rule.fastq", fwd, rev)
    assert len(read_fastq(os.path.join(tmp, "rule.fastq"))) == 21
    # the reverse primer's half of the rule (no read has a reverse match as given)
    half = recs([amplicon(rng, 150, fwd, None)] + [s for _, s, _ in flipped])
    write_fastq(src, half)
    check_file(pr, src, half, tmp, "half.fastq", fwd, rev)
    # nothing passes, over an output left from an earlier run
    left = os.path.join(tmp, "rule.fastq")
    assert os.path.exists(left)
    none = recs([rand_seq(rng, 100) for _ in range(9)])
    write_fastq(src, none, gz=True)
    check_file(pr, src, none, tmp, "rule.fastq", fwd, rev)
    assert not os.path.exists(left)
    # the wrapper: matrix, row names, directories, refusals, the warning
    import warnings
    write_fastq(src, mixed)
    src2 = os.path.join(tmp, "in2.fastq")
    write_fastq(src2, none)
    outs = [os.path.join(tmp, "new", "dir", "a.fastq.gz"), os.path.join(tmp, "new", "b.fastq.gz")]
    with warnings.catch_warnings(record=True) as wlist:
        warnings.simplefilter("always")
        rval, names = pr.remove_primers([src, src2], outs, fwd, rev)
    assert rval.tolist() == [[21, 21], [9, 0]] and names == ["in.fastq", "in2.fastq"] and not wlist
    assert os.path.exists(outs[0]) and not os.path.exists(outs[1])
    assert read_text(outs[0]) == fastq_text(restate_fastq(mixed, fwd, rev)[1])
    with warnings.catch_warnings(record=True) as wlist:
        warnings.simplefilter("always")
        rval, _ = pr.remove_primers(src2, outs[1], fwd, rev, verbose=False)
    assert rval.tolist() == [[9, 0]] and any("No reads passed the primer detection." in str(w.message) for w in wlist)
    E = pr._lib.Dada2HipError
    _raises(E, lambda: pr.primers_fastq(src, src, fwd), "distinct", code=1)
    _raises(E, lambda: pr.primers_fastq(os.path.join(tmp, "missing.fastq"), outs[1], fwd), "do not exist", code=1)
    _raises(ValueError, lambda: pr.remove_primers(src, src, fwd), "distinct from the input")
    _raises(ValueError, lambda: pr.remove_primers([src, src2], [outs[1], outs[1]], fwd), "must be distinct")
    _raises(ValueError, lambda: pr.remove_primers([src, src2], [outs[1]], fwd), "corresponding output file")
    _raises(ValueError, lambda: pr.remove_primers(os.path.join(tmp, "missing.fastq"), outs[1], fwd), "do not exist")
    _raises(NotImplementedError, lambda: pr.remove_primers(src, outs[1], fwd, allow_indels=True), "not supported")
    bad = recs([amplicon(rng, 150, fwd, rev), rand_seq(rng, 40) + "x" + rand_seq(rng, 40)])
    write_fastq(src2, bad)
    _raises(E, lambda: pr.primers_fastq(src2, outs[1], fwd, rev), "@r1 some text", code=4)
    assert not os.path.exists(outs[1])


def _raises(exc, fn, text=None, code=None):
    try:
        fn()
    except exc as e:
        assert text is None or text in str(e), str(e)
        assert code is None or e.code == code, (e.code, code)
        return
    raise AssertionError("no %s raised" % exc.__name__)


def case_refusals(pr):
    E = pr._lib.Dada2HipError
    seqs = ["ACGT" * 30]
    _raises(E, lambda: pr.primer_hits(seqs, "A" * 129), "128", code=4)
    _raises(E, lambda: pr.primer_hits(seqs, F27, "A" * 129), "128", code=4)
    _raises(E, lambda: pr.primer_hits(seqs, "A" * 40, max_mismatch=16), "15", code=4)
    _raises(E, lambda: pr.primer_hits(seqs, "ACGT", max_mismatch=4), "below", code=4)
    _raises(E, lambda: pr.primer_hits(seqs, F27, "ACG", max_mismatch=3), "below", code=4)
    _raises(E, lambda: pr.primer_hits(seqs, F27, max_mismatch=-1), code=1)
    _raises(E, lambda: pr.primer_hits(seqs, ""), code=1)
    _raises(ValueError, lambda: pr.primer_hits(seqs, None), "base R strings")
    p = pr._lib.CPrimerParams(F27.encode(), None, 2, 1, 1, 1, 1, 0)
    import ctypes as C
    eb = C.create_string_buffer(512)
    rv = pr._lib.lib().dada2hip_primers_reads(0, None, None, C.byref(p), 0, None, None, None, None, None, None, None, eb, 512)
    assert rv == 4 and b"not supported" in eb.value, (rv, eb.value)
    assert pr.rc("ACGTMRWSYKVHDBN") == rc("ACGTMRWSYKVHDBN") == "NVHDBMRSWYKACGT" and pr.is_acgt("ACGT") and not pr.is_acgt("ACGN")
    check_reads(pr, seqs * 3, "A" * 128, "ACGT" * 32, "128 letters", max_mismatch=15)


# ---- past one piece and one sweep of the grid (the card's alone) -------------------------------------------------------------------

STRIDED_POOL = 4096
PIECE_READS = 65536
GRID_BLOCKS = 4096                      # PR_GRID of csrc/engine.h: a block's next read is this many further on
STRIDED_N = PIECE_READS + GRID_BLOCKS + 1


def check_strided_batch(pr):
    """One call on more reads than a piece holds and, in each piece, more than the launch has blocks: 4 096 distinct reads restated
    once and laid out so that reads a block's stride or a piece apart differ."""
    rng = random.Random(213)
    fwd, rev = F27, rc(R1492)
    pool = []
    for i in range(STRIDED_POOL):
        n = rng.choice((30, 64, 65, 90, 129, 150))
        s = rand_seq(rng, n)
        for primer in (fwd, rev):
            if rng.random() < 0.9:
                s = plant(s, instance(rng, primer, rng.randrange(0, 4)), rng.randrange(-2, n - 17))
        pool.append(rc(s) if rng.random() < 0.5 else s)
    want = [restate_read(s, fwd, rev) for s in pool]
    i = np.arange(STRIDED_N, dtype=np.uint64)
    idx = ((i * np.uint64(2654435761) + i // np.uint64(STRIDED_POOL)) % np.uint64(STRIDED_POOL)).astype(np.int64)
    for d in (1, GRID_BLOCKS, 2 * GRID_BLOCKS, PIECE_READS):
        assert (idx[d:] != idx[:-d]).all(), d
    st = {}
    got = pr.primer_hits([pool[j] for j in idx], fwd, rev, stats=st)
    for k, width in (("code", 1), ("flip", 1), ("first", 1), ("last", 1), ("hits", 4), ("starts", 8)):
        w = np.array([want[j][k] for j in range(STRIDED_POOL)], dtype=np.int64).reshape(STRIDED_POOL, width)[idx]
        g = got[k].reshape(STRIDED_N, width)
        bad = np.flatnonzero((g != w).any(axis=1))
        assert bad.size == 0, (k, "first at read", int(bad[0]), "of", int(bad.size), g[bad[0]].tolist(), w[bad[0]].tolist())
    codes = np.array([w["code"] for w in want])[idx]
    assert st["pieces"] == 2 and st["reads_in"] == STRIDED_N and st["reads_kept"] == int((codes == 0).sum()) > 0, st
    return st


def _with_tmp(fn, **kw):
    def run(pr):
        import tempfile
        with tempfile.TemporaryDirectory() as tmp:
            fn(pr, tmp, **kw)
    return run


CASES = {"lengths": case_lengths, "batches": case_batches, "chunk_boundaries": case_chunk_boundaries,
         "mismatch_budget": case_mismatch_budget, "letters": case_letters, "multiple_hits": case_multiple_hits,
         "orientation": case_orientation, "window": case_window, "tiles_and_pieces": case_tiles_and_pieces,
         "random_sweep": case_random_sweep, "example_file": _with_tmp(case_example_file), "file_rules": _with_tmp(case_file_rules),
         "refusals": case_refusals}
CASE_NAMES = tuple(CASES)


def emu_run(names=None):
    """The emulator's job (tests/test_emu_primers.py): every case."""
    from dada2_amd import primers
    names = names or CASE_NAMES
    for name in names:
        CASES[name](primers)
    return "ok %d cases" % len(names)
