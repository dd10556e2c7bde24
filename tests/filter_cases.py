"""filterAndTrim: the restatement and the cases (tests/test_filter.py pins the restatement, tests/test_gpu_filter.py and
tests/test_emu_filter.py hold the library to it).

R is not available where the tests run, so the reference's two compiled routines - C_matchRef and C_matrixEE, src/filter.cpp - are
recorded in tests/golden/filter.npz by tests/golden/make_filter_golden.py, and the R-level flow around them is RESTATED here on
Python strings, line by line against R/filter.R:
  restate_read      fastqFilter's stages (:659-706) on one read -> the first stage it fails, the kept window, EE, the two counts
  match_ref         C_matchRef (src/filter.cpp:7-32), literally: a set of substrings, `j += word_size` and the loop's `j++`
  matrix_ee         C_matrixEE (:35-49): ee += pow(10.0, -q / 10.0) in order (math.pow is libm's pow)
  kmer_counts, complexity   oligonucleotideFrequency's bins and sindex (:1271-1275)
  restate_fastq, restate_paired   the file level: chunks only matter through the Auto quality offset (the first chunk's)
The pieces a call is cut into (DADA2HIP_FILTER_PIECE, DADA2HIP_FILTER_PIECE_BYTES) change no result: case_pieces runs one batch under
small pieces and counts them; strided_batch is the batch past one piece, 8 192 waves and 16 384 blocks (tests/test_gpu_filter.py).
Every comparison with the library is exact (integers, byte strings, bit-equal doubles) except the complexity value, relative 1e-12:
sixteen fp64 terms summed by R in long double, a few ulp at most."""
import gzip
import math
import os
import random

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
PHIX_FA = os.path.join(GOLDEN, "phix_genome.fa")
FASTQS = {k: os.path.join(GOLDEN, k + ".fastq.gz") for k in ("sam1F", "sam1R", "sam2F", "sam2R", "samPB")}
INF = float("inf")
DEFAULTS = dict(trunc_q=2, trunc_len=0, trim_left=0, trim_right=0, max_len=INF, min_len=20, max_n=0, min_q=0, max_ee=INF,
                rm_phix=False, rm_lowcomplex=0, min_matches=2, non_overlapping=True, kmer_size=0, quality_type=0)
STAGES = ("kept", "max_len", "trim_left", "trim_right", "trunc_q", "trunc_len", "min_len", "max_n", "min_q", "max_ee", "rm_phix",
          "rm_lowcomplex")

_PHIX = []


def phix():
    if not _PHIX:
        with open(PHIX_FA) as fh:
            _PHIX.append("".join(line.strip() for line in fh if not line.startswith(">")).upper())
    return _PHIX[0]


def rc(s):
    return s[::-1].translate(str.maketrans("ACGT", "TGCA"))


# ---- the restatement -----------------------------------------------------------------------------------------------------------

_WORDS = {}


def word_set(ref, word_size):
    key = (ref, word_size)
    if key not in _WORDS:
        ext = ref + ref[:word_size]                                       # src/filter.cpp:14
        _WORDS[key] = {ext[i: i + word_size] for i in range(len(ref))}    # :16-18
    return _WORDS[key]


def match_ref(seqs, ref, word_size=16, non_overlapping=True):
    words = word_set(ref, word_size)
    out = []
    for s in seqs:
        n = 0
        if len(s) >= word_size:                                           # :22
            j = 0
            while j <= len(s) - word_size:                                # :24
                if s[j: j + word_size] in words:
                    n += 1
                    if non_overlapping:
                        j += word_size                                    # :27
                j += 1
        out.append(n)
    return out


def matrix_ee(q):
    ee = 0.0
    for v in q:
        ee += math.pow(10.0, -v / 10.0)                                    # :44
    return ee


def kmer_counts(s, k):
    x = [0] * (4 ** k)
    for i in range(len(s) - k + 1):
        idx = 0
        for c in s[i: i + k]:
            j = "ACGT".find(c)
            if j < 0:
                idx = -1
                break
            idx = idx * 4 + j
        if idx >= 0:
            x[idx] += 1
    return x


def complexity(s, k=2):
    x = kmer_counts(s, k)
    tot = sum(x)
    if tot == 0:
        return float("nan")
    return math.exp(math.fsum(-(v / tot) * math.log(v / tot) for v in x if v > 0))   # :1272-1274


def auto_offset(quals):
    m = min((min(q.encode()) for q in quals if q), default=255)
    return 33 if m < 59 else 64


def restate_read(seq, qual, P, ref=None, offset=33, word_size=16):
    """{"code", "off", "len", "ee", "hits"} of one read under the parameters P (DEFAULTS' keys)."""
    start = max(1, P["trim_left"] + 1)                                    # :622
    skip = start - 1
    out = {"code": 0, "off": skip, "len": 0, "ee": 0.0, "hits": (0, 0)}
    w = len(seq)
    if P["max_len"] != INF and not w <= P["max_len"]:                     # :660
        return dict(out, code=1)
    if not w >= start:                                                    # :662
        return dict(out, code=2)
    s, q = seq[skip:], [c - offset for c in qual.encode()[skip:]]          # :663
    if P["trim_right"] > 0:                                               # :665-668
        if not len(s) > P["trim_right"]:
            return dict(out, code=3)
        s, q = s[: len(s) - P["trim_right"]], q[: len(q) - P["trim_right"]]
    for j, v in enumerate(q):                                             # :677 trimTails(fq, 1, truncQ)
        if v <= P["trunc_q"]:
            s, q = s[:j], q[:j]
            break
    if len(s) == 0:
        return dict(out, code=4)
    if P["trunc_len"] >= start:                                           # :623-625, :680-682
        end = P["trunc_len"] - start + 1
        if not len(s) >= end:
            return dict(out, code=5)
        s, q = s[:end], q[:end]
    if not len(s) >= P["min_len"]:                                        # :684
        return dict(out, code=6)
    out["len"] = len(s)
    out["ee"] = matrix_ee(q)
    if ref is not None:
        out["hits"] = (match_ref([s], ref, word_size, P["non_overlapping"])[0], match_ref([s], rc(ref), word_size, P["non_overlapping"])[0])
    code = 0
    if sum(1 for c in s if c not in "ACGT") > P["max_n"]:                 # :687
        code = 7
    elif P["min_q"] > P["trunc_q"] and not min(q) > P["min_q"]:           # :690
        code = 8
    elif P["max_ee"] < INF and not out["ee"] <= P["max_ee"]:              # :691-693
        code = 9
    elif P["rm_phix"] and (out["hits"][0] >= P["min_matches"] or out["hits"][1] >= P["min_matches"]):   # :697-700, :1186
        code = 10
    elif P["rm_lowcomplex"] > 0 and not complexity(s, P["kmer_size"] or 2) >= P["rm_lowcomplex"]:       # :703-706
        code = 11
    out["code"] = code
    return out


def params(**kw):
    bad = set(kw) - set(DEFAULTS)
    assert not bad, bad
    return dict(DEFAULTS, **kw)


def pick(P, which):
    return {k: (v[which if len(v) == 2 else 0] if isinstance(v, (list, tuple)) else v) for k, v in P.items()}


def read_fastq(path):
    with open(path, "rb") as fh:
        magic = fh.read(2)
    with (gzip.open if magic == b"\x1f\x8b" else open)(path, "rt") as fh:
        lines = fh.read().split("\n")
    if lines and lines[-1] == "":
        lines.pop()
    assert len(lines) % 4 == 0, path
    return [(lines[i], lines[i + 1], lines[i + 3]) for i in range(0, len(lines), 4)]


def fastq_text(records):
    return "".join("%s\n%s\n+\n%s\n" % r for r in records)


def write_fastq(path, records, gz=None):
    data = fastq_text(records).encode()
    if gz if gz is not None else path.endswith(".gz"):
        with gzip.open(path, "wb", compresslevel=1) as fh:
            fh.write(data)
    else:
        with open(path, "wb") as fh:
            fh.write(data)


def read_text(path):
    with open(path, "rb") as fh:
        magic = fh.read(2)
    with (gzip.open if magic == b"\x1f\x8b" else open)(path, "rb") as fh:
        return fh.read().decode()


def restate_fastq(records, P, ref=None, n=10**5):
    """The records fastqFilter writes, and (reads.in, reads.out)."""
    off = P["quality_type"] or auto_offset([r[2] for r in records[:n]])
    kept = []
    for hid, s, q in records:
        v = restate_read(s, q, P, ref if P["rm_phix"] else None, off)
        if v["code"] == 0:
            kept.append((hid, s[v["off"]: v["off"] + v["len"]], q[v["off"]: v["off"] + v["len"]]))
    return kept, (len(records), len(kept))


def restate_paired(rec_f, rec_r, P, ref=None, n=10**5):
    assert len(rec_f) == len(rec_r)
    PF, PR = pick(P, 0), pick(P, 1)
    of = PF["quality_type"] or auto_offset([r[2] for r in rec_f[:n]])
    orv = PR["quality_type"] or auto_offset([r[2] for r in rec_r[:n]])
    kf, kr = [], []
    for a, b in zip(rec_f, rec_r):
        va = restate_read(a[1], a[2], PF, ref if PF["rm_phix"] else None, of)
        vb = restate_read(b[1], b[2], PR, ref if PR["rm_phix"] else None, orv)
        if va["code"] == 0 and vb["code"] == 0:                           # :1083-1090: both directions
            kf.append((a[0], a[1][va["off"]: va["off"] + va["len"]], a[2][va["off"]: va["off"] + va["len"]]))
            kr.append((b[0], b[1][vb["off"]: vb["off"] + vb["len"]], b[2][vb["off"]: vb["off"] + vb["len"]]))
    return kf, kr, (len(rec_f), len(kf))


# ---- builders --------------------------------------------------------------------------------------------------------------------

LENGTHS = (0, 1, 15, 16, 17, 19, 20, 21, 63, 64, 65, 127, 128, 129, 250, 251, 301, 1500, 5000)


def rand_seq(rng, n):
    return "".join(rng.choice("ACGT") for _ in range(n))


def rand_qual(rng, n, lo=3, hi=40, offset=33):
    return "".join(chr(offset + rng.randint(lo, hi)) for _ in range(n))


def illumina_qual(rng, n, offset=33):
    """High at the start, decaying, with an occasional Q2 tail."""
    q = []
    tail = rng.random() < 0.3
    cut = rng.randint(0, n) if tail else n
    for i in range(n):
        v = 2 if i >= cut else max(3, min(40, int(38 - 25 * (i / max(n, 1)) ** 2 + rng.gauss(0, 4))))
        q.append(chr(offset + v))
    return "".join(q)


def genome_cut(rng, n, strand=None, at=None):
    g = phix()
    at = rng.randrange(len(g)) if at is None else at
    s = (g + g + g)[at: at + n] if n <= 2 * len(g) else None
    return rc(s) if (strand if strand is not None else rng.random() < 0.5) else s


def mixed_reads(rng, n, lengths=None, p_phix=0.15, p_n=0.15):
    """n reads: random or cut from the genome, some with N / IUPAC / lower-case letters, Illumina-like qualities."""
    seqs, quals = [], []
    for i in range(n):
        ln = lengths[i % len(lengths)] if lengths else rng.choice((30, 64, 100, 150, 250, 251))
        if rng.random() < p_phix and ln <= 5000:
            s = genome_cut(rng, ln)
            if ln > 40 and rng.random() < 0.5:                            # a genome piece inside random flanks
                a = rng.randint(0, ln - 36)
                s = rand_seq(rng, a) + s[a: a + 36] + rand_seq(rng, ln - a - 36)
        else:
            s = rand_seq(rng, ln)
        if ln and rng.random() < p_n:
            s = list(s)
            for _ in range(rng.choice((1, 1, 2, 4))):
                s[rng.randrange(ln)] = rng.choice("NNNRYKMa")
            s = "".join(s)
        seqs.append(s)
        quals.append(illumina_qual(rng, ln))
    return seqs, quals


# ---- the library against the restatement ---------------------------------------------------------------------------------------

def check_reads(api, ctx, seqs, quals, what="", kmers=False, **kw):
    """Every output of dada2hip_filter_reads for every read, against restate_read.  Returns the restated codes."""
    P = params(**kw)
    got = api.filter_reads(seqs, quals, ctx, kmers=kmers, **kw)
    off = P["quality_type"] or auto_offset(quals)
    ref = ctx.ref
    k = P["kmer_size"] or 2
    want = [restate_read(s, q, P, ref, off, ctx.word_size) for s, q in zip(seqs, quals)]
    assert len(got["code"]) == len(seqs)
    for i, w in enumerate(want):
        g = (int(got["code"][i]), int(got["window"][i, 0]), int(got["window"][i, 1]), float(got["ee"][i]).hex(),
             (int(got["hits"][i, 0]), int(got["hits"][i, 1])))
        e = (w["code"], w["off"], w["len"], w["ee"].hex(), w["hits"])
        assert g == e, (what, i, len(seqs[i]), "got", g, "want", e)
        if kmers:
            s = seqs[i][w["off"]: w["off"] + w["len"]]
            assert got["kmer_counts"][i].tolist() == kmer_counts(s, k), (what, i)
            c = complexity(s, k)
            gc = float(got["complexity"][i])
            assert (math.isnan(c) and math.isnan(gc)) or abs(gc - c) <= 1e-12 * abs(c), (what, i, gc, c)
    return [w["code"] for w in want]


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


def open_ctx(api, word_size=16, screen=True):
    return api.FilterContext(PHIX_FA if screen else None, word_size)


def case_lengths(api):
    rng = random.Random(101)
    seqs, quals = mixed_reads(rng, 3 * len(LENGTHS), lengths=LENGTHS, p_phix=0.4)
    with open_ctx(api) as ctx:
        codes = check_reads(api, ctx, seqs, quals, "defaults", rm_phix=True)
        assert {0, 2, 6, 10} <= set(codes), sorted(set(codes))
        check_reads(api, ctx, seqs, quals, "trunc 240 / ee 2", rm_phix=True, trunc_len=240, max_ee=2, max_n=1)
        check_reads(api, ctx, seqs, quals, "short", rm_phix=True, min_len=1, trunc_q=-1, max_n=5, kmers=True, kmer_size=3)
        check_reads(api, ctx, seqs, quals, "max_len", rm_phix=True, max_len=250, trim_left=10, trim_right=5, min_len=0)


def case_batches(api):
    rng = random.Random(102)
    with open_ctx(api) as ctx:
        for n in (1, 63, 64, 65, 4097):
            seqs, quals = mixed_reads(rng, n, lengths=(30, 64, 65, 100, 150) if n > 1000 else None)
            st = {}
            got = api.filter_reads(seqs, quals, ctx, stats=st, rm_phix=True, max_ee=3, trunc_len=50)
            codes = check_reads(api, ctx, seqs, quals, "batch of %d" % n, rm_phix=True, max_ee=3, trunc_len=50)
            assert got["code"].tolist() == codes
            assert st["reads_in"] == n and st["reads_kept"] == codes.count(0) and st["dropped_max_ee"] == codes.count(9), st
            assert st["table_keys"] == 10772 and st["table_in_lds"] == 1, st
        assert api.filter_reads([], [], ctx)["code"].shape == (0,)


def case_letters(api):
    rng = random.Random(103)
    seqs, quals = [], []
    for nn in (0, 1, 2, 3, 4):
        for letter in "NRYacgtn-":
            s = list(rand_seq(rng, 70))
            for p in rng.sample(range(70), nn):
                s[p] = letter
            seqs.append("".join(s))
            quals.append("I" * 70)
    seqs.append("N" * 64 + rand_seq(rng, 6))
    quals.append("I" * 70)
    with open_ctx(api, screen=False) as ctx:
        for mn in (0, 1, 3):
            codes = check_reads(api, ctx, seqs, quals, "maxN %d" % mn, max_n=mn)
            assert 0 in codes and 7 in codes
        # the letters behind the truncQ cut do not count
        s = rand_seq(rng, 30) + "NNNN"
        assert check_reads(api, ctx, [s, s], ["I" * 30 + "#III", "I" * 31 + "#II"], "N behind the cut") == [0, 7]


def case_truncq(api):
    rng = random.Random(104)
    seqs, quals = [], []
    for ln in (20, 64, 65, 130, 300):
        for cut in (0, 1, ln // 2, 63, 64, ln - 1, None):
            if cut is not None and cut >= ln:
                continue
            q = ["I"] * ln
            if cut is not None:
                q[cut] = "#"
                if cut + 5 < ln:
                    q[cut + 5] = "!"
            seqs.append(rand_seq(rng, ln))
            quals.append("".join(q))
    with open_ctx(api, screen=False) as ctx:
        codes = check_reads(api, ctx, seqs, quals, "truncQ 2", min_len=0)
        assert 4 in codes and 0 in codes
        check_reads(api, ctx, seqs, quals, "truncQ 2, minLen 20")
        check_reads(api, ctx, seqs, quals, "truncQ 0", trunc_q=0, min_len=1)
        check_reads(api, ctx, seqs, quals, "truncQ 1 behind trimLeft", trunc_q=1, trim_left=1, min_len=1)
        check_reads(api, ctx, seqs, quals, "truncQ 11", trunc_q=11, quality_type=33)
        q64 = [q.replace("I", "h").replace("#", "B").replace("!", "@") for q in quals]
        assert auto_offset(q64) == 64
        check_reads(api, ctx, seqs, q64, "offset 64 by Auto", min_len=0)
        check_reads(api, ctx, seqs, q64, "offset 64 given", min_len=0, quality_type=64)


def case_trims(api):
    rng = random.Random(105)
    lens = (1, 9, 10, 11, 12, 40, 41, 42, 100)
    seqs = [rand_seq(rng, n) for n in lens for _ in range(2)]
    quals = [rand_qual(rng, len(s), 5, 40) for s in seqs]
    with open_ctx(api, screen=False) as ctx:
        for tl in (0, 9, 10, 11, 40, 41):                                  # the width and the width - 1
            codes = check_reads(api, ctx, seqs, quals, "trimLeft %d" % tl, trim_left=tl, min_len=0)
            assert tl == 0 or 2 in codes
        for tr in (9, 10, 11, 40, 41, 99, 100):
            codes = check_reads(api, ctx, seqs, quals, "trimRight %d" % tr, trim_right=tr, min_len=0)
            assert 3 in codes
        check_reads(api, ctx, seqs, quals, "both", trim_left=5, trim_right=5, min_len=1)
        for tlen in (5, 6, 30, 31, 32, 36, 37):                            # below start, the trimmed width, one above it
            check_reads(api, ctx, seqs, quals, "truncLen %d" % tlen, trim_left=5, trunc_len=tlen, min_len=0)
        codes = check_reads(api, ctx, seqs, quals, "truncLen 41", trunc_len=41, min_len=0)
        assert codes.count(5) == 12 and codes.count(0) == 6, codes
        for ml in (10, 11, 12, 41):
            check_reads(api, ctx, seqs, quals, "minLen / maxLen %d" % ml, min_len=ml, max_len=ml)


def case_minq(api):
    rng = random.Random(106)
    seqs, quals = [], []
    for floor in (3, 4, 5, 6, 7, 10):
        for _ in range(3):
            q = [rng.randint(floor, 40) for _ in range(80)]
            q[rng.randrange(80)] = floor                                   # the minimum is exactly `floor`
            seqs.append(rand_seq(rng, 80))
            quals.append("".join(chr(33 + v) for v in q))
    with open_ctx(api, screen=False) as ctx:
        for tq, mq in ((5, 4), (5, 5), (5, 6), (2, 3), (2, 4), (2, 10), (0, 0), (2, 0)):
            codes = check_reads(api, ctx, seqs, quals, "truncQ %d minQ %d" % (tq, mq), trunc_q=tq, min_q=mq, min_len=0)
            assert (8 in codes) == (mq > tq), (tq, mq, codes)


def case_ee_threshold(api):
    rng = random.Random(107)
    seqs = [rand_seq(rng, 20), rand_seq(rng, 200), rand_seq(rng, 19), rand_seq(rng, 21), rand_seq(rng, 199)]
    quals = ["+" * 20, "5" * 200, "+" * 19, "+" * 21, "5" * 199]
    assert matrix_ee([10] * 20) == 2.0000000000000004 and sum([0.1] * 20) != math.fsum([0.1] * 20)   # in order, not a tree
    with open_ctx(api, screen=False) as ctx:
        codes = check_reads(api, ctx, seqs, quals, "on the threshold", max_ee=2, min_len=0)
        assert codes[0] == 9 and codes[2] == 0 and codes[3] == 9 and codes[4] == 0, codes
        assert codes[1] == (0 if matrix_ee([20] * 200) <= 2 else 9)
        s2, q2 = mixed_reads(rng, 150, p_phix=0, p_n=0)
        s2 += [rand_seq(rng, n) for n in (30, 64, 100, 150, 250) for _ in range(30)]
        q2 += [rand_qual(rng, len(s), 8, 40) for s in s2[150:]]            # about 0.023 expected errors per base: both sides of 1 / 2 / 5
        for me in (1, 2, 5, 0.5, 2.0000000000000004):
            codes = check_reads(api, ctx, s2, q2, "maxEE %r" % me, max_ee=me)
            assert 0 in codes and 9 in codes, me
        check_reads(api, ctx, s2, q2, "maxEE with truncLen", max_ee=2, trunc_len=60)


def screen_reads():
    """(sequences, {name: index}) for the screen's quirks, word size 16."""
    rng = random.Random(108)
    g = phix()
    n = len(g)
    w1, w2 = g[100:116], g[3000:3016]
    flank = "ACGTTGCAACGTTGCAAC"
    seqs, names = [], {}

    def add(name, s):
        names[name] = len(seqs)
        seqs.append(s)
    add("forward_250", g[1000:1250])
    add("reverse_250", rc(g[2000:2250]))
    add("junction_fwd", (g + g)[n - 40: n + 60])
    add("junction_rev", rc((g + g)[n - 25: n + 25]))
    add("back_to_back", w1 + w2)                                           # 1 hit under the + 1 skip
    add("one_between", w1 + "A" + w2)                                      # 2 hits
    add("fwd_and_rev", w1 + "A" + rc(w2))                                  # 1 + 1, never summed
    add("word_with_n", w1[:7] + "N" + w1[8:] + "A" + w2)
    add("word_lower", w1.lower() + "A" + w2)
    add("short_15", g[500:515])
    add("exactly_16", g[500:516])
    add("seventeen", g[500:517])
    add("thirty_two", g[500:532])                                          # windows 0 .. 16: a hit at 0 sends the scan to 17
    add("thirty_three", g[500:533])                                        # window 17 exists: a second hit
    add("empty", "")
    add("random_250", rand_seq(rng, 250))
    add("flanked", flank + w1 + flank + w2 + flank)
    add("hit_at_63_64", rand_seq(rng, 63) + g[700:740] + rand_seq(rng, 30))
    add("long_1500", rand_seq(rng, 700) + g[4000:4100] + rand_seq(rng, 700))
    add("long_5000", (g + g)[5000:5000 + 5000])
    for i in range(20):
        add("cut_%d" % i, genome_cut(rng, rng.choice((16, 17, 32, 33, 50, 64, 80, 128, 129)), at=None))
    return seqs, names


def case_screen(api):
    seqs, names = screen_reads()
    quals = ["I" * len(s) for s in seqs]
    g = phix()
    with open_ctx(api) as ctx:
        codes = check_reads(api, ctx, seqs, quals, "16 / 2 / TRUE", rm_phix=True, min_len=0, max_n=9)
        flagged = {k: codes[i] == 10 for k, i in names.items()}
        assert flagged["forward_250"] and flagged["reverse_250"] and flagged["junction_fwd"] and flagged["junction_rev"]
        assert not flagged["back_to_back"] and flagged["one_between"] and not flagged["fwd_and_rev"]
        assert not flagged["word_with_n"] and not flagged["word_lower"] and not flagged["short_15"] and not flagged["random_250"]
        assert not flagged["thirty_two"] and flagged["thirty_three"] and flagged["flanked"] and flagged["long_5000"]
        for mm in (1, 3):
            check_reads(api, ctx, seqs, quals, "minMatches %d" % mm, rm_phix=True, min_matches=mm, min_len=0, max_n=9)
        check_reads(api, ctx, seqs, quals, "overlapping", rm_phix=True, non_overlapping=False, min_len=0, max_n=9)
        check_reads(api, ctx, seqs, quals, "behind a trim", rm_phix=True, trim_left=3, trunc_len=40, min_len=0, max_n=9)
        got = api.is_phix(seqs, ctx)
        want = [a >= 2 or b >= 2 for a, b in zip(match_ref(seqs, g), match_ref(seqs, rc(g)))]
        assert got.tolist() == want
    for ws in (8, 20, 32, 1):
        with open_ctx(api, ws) as ctx:
            for no in (True, False):
                check_reads(api, ctx, seqs, quals, "word size %d" % ws, rm_phix=True, non_overlapping=no, min_len=0, max_n=9)
    for ws, no in ((16, True), (20, False)):
        assert api.match_ref(seqs, g, ws, no).tolist() == match_ref(seqs, g, ws, no)
    assert api.is_phix(seqs[:4], PHIX_FA, word_size=20, min_matches=1).tolist() == [True] * 4
    # a reference that is no genome: short, repetitive, and a word set of one
    for ref in ("ACGTACGTACGTACGTAC", "A" * 40, "ACGTTGCA" * 30 + "GGG"):
        qs = [ref * 3, ref[2:] + ref, "A" * 100, "ACGT" * 30, rc(ref) + "T" + ref]
        for ws in (4, 16):
            for no in (True, False):
                assert api.match_ref(qs, ref, ws, no).tolist() == match_ref(qs, ref, ws, no), (ref, ws, no)


def case_screen_in_global_memory(api):
    """A reference whose word table does not fit the LDS: the same search over global memory."""
    rng = random.Random(109)
    ref = rand_seq(rng, 9000)
    seqs = [ref[100:350], rc(ref[4000:4250]), rand_seq(rng, 250), (ref + ref)[8950:9100], ref[10:26] + ref[500:516], ref[10:26] + "C" + ref[500:516]]
    with api.FilterContext(ref, 16) as ctx:
        assert ctx.stats["table_keys"] > 16384 and ctx.stats["table_in_lds"] == 0, ctx.stats
        codes = check_reads(api, ctx, seqs, ["I" * len(s) for s in seqs], "global table", rm_phix=True)
        assert codes == [10, 10, 0, 10, 0, 10], codes


MAN_PAGE = ("TACGGAAGGTCCGGGCGTTATCCGGATTTATTGGGTTTAAAGGGAGCGTAGGCCGGAGATTAAGCGTGTTGTGA",
            "TCCTTCTTCTCCTCTCTTTCTCCTTCTTTCTTTTTTTTCCCTTTCTCTTCTTCTTTTTCTTCCTTCCTTTTTTC",
            "TTTTTCTTCTCCCCCTTCCCCTTTCCTTTTCTCCTTTTTTCCTTTAGTGCAGTTGAGGCAGGCGGAATTCGTGG")   # R/filter.R:1241-1243


def complexity_reads():
    rng = random.Random(110)
    seqs = list(MAN_PAGE) + ["A" * 60, "C" * 64, "AC" * 40, "GT" * 33 + "G", "ACG" * 30, "N" * 30, "ACNGT" * 20, "A", "AC", "ACG", "ACGT", ""]
    seqs += [rand_seq(rng, n) for n in (63, 64, 65, 130, 250, 1500)]
    return seqs


def lowcomplex_thresholds(seqs, k):
    """Thresholds between the restated values, none within 1e-9 of one."""
    vals = sorted(v for v in (complexity(s, k) for s in seqs) if not math.isnan(v))
    i = next(i for i in range(len(vals) // 3, len(vals) - 1) if vals[i + 1] - vals[i] > 0.01)
    ths = [round((vals[i] + vals[i + 1]) / 2, 3), round(0.7 * 4 ** k, 3)]
    for t in ths:
        assert all(abs(v - t) > 1e-9 for v in vals), (t, k)
    return ths


def case_complexity(api):
    seqs = complexity_reads()
    quals = ["I" * len(s) for s in seqs]
    cn, cl, cp = (complexity(s) for s in MAN_PAGE)
    assert cl < cp < cn <= 16                                              # low complexity, partly low, normal
    with open_ctx(api, screen=False) as ctx:
        for k in (1, 2, 3, 4):
            check_reads(api, ctx, seqs, quals, "k = %d" % k, kmers=True, kmer_size=k, min_len=0, max_n=99)
            got = api.seq_complexity(seqs, k)
            for s, v in zip(seqs, got):
                c = complexity(s, k)
                assert (math.isnan(c) and math.isnan(v)) or abs(v - c) <= 1e-12 * abs(c), (k, s[:20], v, c)
            for t in lowcomplex_thresholds(seqs, k):
                codes = check_reads(api, ctx, seqs, quals, "rm.lowcomplex %r" % t, rm_lowcomplex=t, kmer_size=k, min_len=0, max_n=99)
                assert 11 in codes and 0 in codes, (k, t, codes)
        codes = check_reads(api, ctx, ["N" * 30, "ACGT" * 10], ["I" * 30, "I" * 40], "no valid k-mer", rm_lowcomplex=0.5, max_n=99)
        assert codes == [11, 0]
        check_reads(api, ctx, seqs, quals, "behind a trim", kmers=True, trim_left=2, trunc_len=50, min_len=0, max_n=99)


def paired_records(n=400, seed=111):
    rng = random.Random(seed)
    sf, qf = mixed_reads(rng, n, p_phix=0.1, p_n=0.1)
    sr, qr = mixed_reads(rng, n, p_phix=0.1, p_n=0.1)
    rf = [("@read%d 1:N:0" % i, s, q) for i, (s, q) in enumerate(zip(sf, qf))]
    rr = [("@read%d 2:N:0" % i, s, q) for i, (s, q) in enumerate(zip(sr, qr))]
    return rf, rr


def case_paired(api, tmp):
    rf, rr = paired_records()
    inf, inr = os.path.join(tmp, "p_F.fastq"), os.path.join(tmp, "p_R.fastq.gz")
    write_fastq(inf, rf)
    write_fastq(inr, rr)
    P = params(trunc_len=(60, 50), max_ee=(2, 4), trim_left=(0, 5), max_n=(0, 1), rm_phix=True, trunc_q=(2, 5), min_q=(0, 6))
    kf, kr, counts = restate_paired(rf, rr, P, phix())
    # only F fails, only R fails, both at different stages: all present
    PF, PR = pick(P, 0), pick(P, 1)
    seen = set()
    for a, b in zip(rf, rr):
        ca = restate_read(a[1], a[2], PF, phix(), 33)["code"]
        cb = restate_read(b[1], b[2], PR, phix(), 33)["code"]
        seen.add("both" if ca and cb and ca != cb else "F" if ca and not cb else "R" if cb and not ca else "none" if not ca and not cb else "same")
    assert {"both", "F", "R", "none"} <= seen, seen
    kw = {k: v for k, v in P.items() if k not in ("rm_phix", "min_matches", "non_overlapping", "kmer_size", "quality_type")}
    with open_ctx(api) as ctx:
        for compress, n in ((True, 100), (False, 10**6)):
            of, orv = os.path.join(tmp, "o_F.fastq" + (".gz" if compress else "")), os.path.join(tmp, "o_R.fastq" + (".gz" if compress else ""))
            got = api.fastq_paired_filter((inf, inr), (of, orv), compress=compress, n=n, rm_phix=True, ctx=ctx, **kw)
            assert got == counts and 0 < counts[1] < counts[0], (got, counts)
            assert read_text(of) == fastq_text(kf) and read_text(orv) == fastq_text(kr)
        rval, names = api.filter_and_trim(inf, of, inr, orv, rm_phix=PHIX_FA, n=100, **kw)
        assert rval.tolist() == [list(counts)] and names == ["p_F.fastq"] and read_text(orv) == fastq_text(kr)
        short = os.path.join(tmp, "p_R_short.fastq")
        write_fastq(short, rr[:-1])
        for n in (100, 10**6):
            try:
                api.fastq_paired_filter((inf, short), (of, orv), n=n, ctx=ctx)
                raise AssertionError("unequal read counts were accepted")
            except api._lib.Dada2HipError as e:
                assert e.code == 1 and "Mismatched forward and reverse sequence files" in str(e), str(e)
            assert not os.path.exists(of) and not os.path.exists(orv)
        for bad in (((inf, inr), (inf, orv)), ((inf, inr), (of, of)), ((inf, inr), (of, inr))):
            try:
                api.fastq_paired_filter(*bad, ctx=ctx)
                raise AssertionError("equal paths were accepted")
            except api._lib.Dada2HipError as e:
                assert "must be different" in str(e)
        assert read_text(inf) == fastq_text(rf)


def case_files(api, tmp):
    rng = random.Random(112)
    seqs, quals = mixed_reads(rng, 1250, p_phix=0.1, p_n=0.1)
    recs = [("@r%d some text" % i, s, q) for i, (s, q) in enumerate(zip(seqs, quals))]
    plain, gz = os.path.join(tmp, "in.fastq"), os.path.join(tmp, "in.fastq.gz")
    write_fastq(plain, recs)
    write_fastq(gz, recs)
    P = params(trunc_len=60, max_ee=2, rm_phix=True)
    kept, counts = restate_fastq(recs, P, phix())
    assert 0 < counts[1] < counts[0]
    kw = dict(trunc_len=60, max_ee=2)
    with open_ctx(api) as ctx:
        for src in (plain, gz):
            for compress in (True, False):
                out = os.path.join(tmp, "out.fastq" + (".gz" if compress else ""))
                st = {}
                got = api.fastq_filter(src, out, compress=compress, n=100, rm_phix=True, ctx=ctx, stats=st, **kw)   # 12 chunks and a half
                assert got == counts and st["reads_in"] == counts[0] and st["reads_kept"] == counts[1], (got, counts, st)
                assert read_text(out) == fastq_text(kept)
                with open(out, "rb") as fh:
                    assert (fh.read(2) == b"\x1f\x8b") == compress
        # several gzip members: Python's gzip and the library's own reader take them as one file
        outgz = os.path.join(tmp, "members.fastq.gz")
        api.fastq_filter(gz, outgz, compress=True, n=100, rm_phix=True, ctx=ctx, **kw)
        with open(outgz, "rb") as fh:
            raw = fh.read()
        assert raw.count(b"\x1f\x8b\x08") >= 2
        assert read_text(outgz) == fastq_text(kept)
        d_got = api.derep_fastq(outgz)
        ref_file = os.path.join(tmp, "restated.fastq")
        write_fastq(ref_file, kept)
        d_want = api.derep_fastq(ref_file)
        assert list(d_got.seqs) == list(d_want.seqs) and np.array_equal(d_got.abundances, d_want.abundances)
        assert np.array_equal(d_got.map, d_want.map) and np.array_equal(d_got.quals, d_want.quals, equal_nan=True)
        # nothing passes: no file, and a stale one is removed
        stale = os.path.join(tmp, "stale.fastq.gz")
        write_fastq(stale, recs[:3])
        assert api.fastq_filter(plain, stale, min_len=10**6, ctx=ctx) == (1250, 0) and not os.path.exists(stale)
        import warnings
        with warnings.catch_warnings(record=True) as wlist:
            warnings.simplefilter("always")
            rval, _ = api.filter_and_trim(plain, stale, min_len=10**6, ctx=ctx)
        assert rval.tolist() == [[1250, 0]] and not os.path.exists(stale) and any("No reads passed" in str(w.message) for w in wlist)
        # the paths
        for call in (lambda: api.fastq_filter(plain, plain, ctx=ctx), ):
            try:
                call()
                raise AssertionError("input == output was accepted")
            except api._lib.Dada2HipError as e:
                assert e.code == 1 and "The output and input files must be different." in str(e)
        assert read_text(plain) == fastq_text(recs)
        for call, msg in ((lambda: api.filter_and_trim(plain, plain, ctx=ctx), "distinct from the input"),
                          (lambda: api.filter_and_trim([plain, gz], [stale, stale], ctx=ctx), "must be distinct"),
                          (lambda: api.filter_and_trim(os.path.join(tmp, "nope.fastq"), stale, ctx=ctx), "do not exist")):
            try:
                call()
                raise AssertionError(msg)
            except ValueError as e:
                assert msg in str(e), str(e)
        # lists of files into a directory that does not exist yet
        odir = os.path.join(tmp, "filtered", "deep")
        rval, names = api.filter_and_trim([plain, gz], odir, rm_phix=True, ctx=ctx, n=500, **kw)
        assert rval.tolist() == [list(counts)] * 2 and names == ["in.fastq", "in.fastq.gz"]
        assert read_text(os.path.join(odir, "in.fastq")) == fastq_text(kept) == read_text(os.path.join(odir, "in.fastq.gz"))
        # a damaged input is a read error
        cut = os.path.join(tmp, "cut.fastq.gz")
        with open(gz, "rb") as fh:
            data = fh.read()
        with open(cut, "wb") as fh:
            fh.write(data[: len(data) * 2 // 3])
        try:
            api.fastq_filter(cut, os.path.join(tmp, "cut_out.fastq.gz"), ctx=ctx)
            raise AssertionError("a truncated file was accepted")
        except api._lib.Dada2HipError as e:
            assert e.code == 1 and "error reading" in str(e), str(e)
        assert not os.path.exists(os.path.join(tmp, "cut_out.fastq.gz"))


def case_fixtures(api, tmp, names=("sam1F", "sam2R")):
    """Real reads at truncLen 240 / maxEE 2: the EE criterion both ways."""
    with open_ctx(api) as ctx:
        for name in names:
            recs = read_fastq(FASTQS[name])
            kept, counts = restate_fastq(recs, params(trunc_len=240, max_ee=2, rm_phix=True), phix())
            out = os.path.join(tmp, name + "_filt.fastq.gz")
            assert api.fastq_filter(FASTQS[name], out, trunc_len=240, max_ee=2, rm_phix=True, ctx=ctx) == counts
            assert read_text(out) == fastq_text(kept)
            check_reads(api, ctx, [r[1] for r in recs[:300]], [r[2] for r in recs[:300]], name, trunc_len=240, max_ee=2, rm_phix=True)


def case_vignette(api, tmp, denoise=True):
    """filter_and_trim -> derep_fastq -> dada -> merge_pairs on sam1F / sam1R; the derep of the filtered file equals the derep of
    the restatement's filtered file."""
    rf, rr = read_fastq(FASTQS["sam1F"]), read_fastq(FASTQS["sam1R"])
    P = params(trunc_len=(240, 160), max_ee=(2, 2), rm_phix=True)
    kf, kr, counts = restate_paired(rf, rr, P, phix())
    of, orv = os.path.join(tmp, "v", "F.fastq.gz"), os.path.join(tmp, "v", "R.fastq.gz")
    rval, _ = api.filter_and_trim(FASTQS["sam1F"], of, FASTQS["sam1R"], orv, trunc_len=(240, 160), max_ee=(2, 2), rm_phix=PHIX_FA)
    assert rval.tolist() == [list(counts)] and 0 < counts[1] < 1500
    dereps = []
    for out, kept in ((of, kf), (orv, kr)):
        want_file = out.replace(".fastq.gz", "_restated.fastq")
        write_fastq(want_file, kept)
        d, w = api.derep_fastq(out), api.derep_fastq(want_file)
        assert list(d.seqs) == list(w.seqs) and np.array_equal(d.abundances, w.abundances) and np.array_equal(d.map, w.map)
        assert np.array_equal(d.quals, w.quals, equal_nan=True)
        assert max(len(s) for s in d.seqs) == (240 if out == of else 160)
        dereps.append(d)
    if denoise:
        from helpers import tperr1
        dd = [api.dada(d, tperr1())[0] for d in dereps]
        m = api.merge_pairs(dd[0], dereps[0], dd[1], dereps[1])
        assert len(m) > 0 and sum(r["abundance"] for r in m) <= counts[1]


# ---- the pieces of a call ---------------------------------------------------------------------------------------------------------

PIECE_READS, PIECE_BYTES = 1 << 16, 32 << 20                               # the library's own limits, and what it uses unset


def cut_pieces(lens, reads=None, nbytes=None):
    """[(first read, one past the last)] of the pieces dada2hip_filter_reads cuts reads of these lengths into: a piece takes reads
    while it has fewer than `reads` and the next one still ends within `nbytes` of its start; its first read always."""
    reads = min(max(reads, 1), PIECE_READS) if reads is not None else PIECE_READS
    nbytes = min(max(nbytes, 1), PIECE_BYTES) if nbytes is not None else PIECE_BYTES
    out, r0, n = [], 0, len(lens)
    while r0 < n:
        r1, b = r0 + 1, lens[r0]
        while r1 < n and r1 - r0 < reads and b + lens[r1] <= nbytes:
            b += lens[r1]
            r1 += 1
        out.append((r0, r1))
        r0 = r1
    return out


def pieces_of(st, nbytes):
    """The pieces behind a call's stats: upload_bytes is 2 x bytes + (reads + pieces) x 8."""
    rest = st["upload_bytes"] - 2 * nbytes - 8 * st["reads_in"]
    assert rest >= 0 and rest % 8 == 0, (st, nbytes)
    return rest // 8


COUNTED = ("reads_in", "reads_kept") + tuple("dropped_" + s for s in STAGES[1:])


def same_outputs(got, base, what):
    assert sorted(got) == sorted(base), what
    for k in base:
        a, b = got[k], base[k]
        if a.dtype == np.float64:                                          # bit for bit (NaN included)
            a, b = a.view(np.uint64), b.view(np.uint64)
        bad = np.flatnonzero((a != b).reshape(len(a), -1).any(axis=1))
        assert bad.size == 0, (what, k, "first at read", int(bad[0]), got[k][bad[0]].tolist(), base[k][bad[0]].tolist())


def pieces_reads():
    """300 reads, the lengths 0, 1, 64 and 65 among them, one of 1 500 nt at index 137."""
    rng = random.Random(113)
    seqs, quals = mixed_reads(rng, 299, lengths=(0, 1, 16, 30, 47, 64, 65, 100, 150, 251), p_phix=0.3, p_n=0.5)
    ls, lq = mixed_reads(rng, 1, lengths=(1500,), p_phix=1.0)
    seqs[137:137] = ls
    quals[137:137] = lq
    return seqs, quals


def case_pieces(api, tmp):
    """One batch under small pieces: every output and every count is the default run's and the restatement's, and the pieces
    happened - the second piece, a slot used a second time, the stats summed over pieces, the cut by bytes; then the file level with
    four pieces per chunk."""
    seqs, quals = pieces_reads()
    lens = [len(s) for s in seqs]
    n, nbytes = len(seqs), sum(lens)
    assert n == 300 and {0, 1, 64, 65} <= set(lens) and lens.count(1500) == 1 and lens[137] == 1500
    kw = dict(rm_phix=True, max_ee=0.05, trunc_len=40, max_n=1, kmers=True)
    # (setting, the cut it stands for, the least number of pieces): 299 reads leave a second piece of one read, 1 499 bytes give
    # the long read a piece of its own
    settings = [({}, {}, 1)] + [({"DADA2HIP_FILTER_PIECE": r}, {"reads": r}, 2 if r == 299 else 3) for r in (1, 2, 7, 64, 299)]
    settings += [({"DADA2HIP_FILTER_PIECE_BYTES": b}, {"nbytes": b}, 3) for b in (400, 1499)]
    settings += [({"DADA2HIP_FILTER_PIECE": 10**9, "DADA2HIP_FILTER_PIECE_BYTES": 10**12}, {}, 1),      # past the limits: the limits
                 ({"DADA2HIP_FILTER_PIECE": 0, "DADA2HIP_FILTER_PIECE_BYTES": -5}, {"reads": 1, "nbytes": 1}, 3)]   # below 1: 1
    assert (137, 138) in cut_pieces(lens, nbytes=1499) and len(cut_pieces(lens, nbytes=400)) > n // 10
    assert all(b - a <= 12 for a, b in cut_pieces(lens, nbytes=400))       # "every few reads"
    with open_ctx(api) as ctx:
        base = None
        for env, cut, least in settings:
            st = {}
            got = with_env(env, lambda: api.filter_reads(seqs, quals, ctx, stats=st, **kw))
            codes = with_env(env, lambda: check_reads(api, ctx, seqs, quals, "pieces %r" % (env,), **kw))
            if base is None:
                base, base_st = got, st
                assert all(codes.count(c) >= 10 for c in (0, 5, 7, 9, 10)), [codes.count(c) for c in range(12)]
            same_outputs(got, base, env)
            assert got["code"].tolist() == codes, env
            for k in COUNTED:
                assert st[k] == base_st[k], (env, k, st[k], base_st[k])
            assert st["reads_in"] == n and st["reads_kept"] == codes.count(0), (env, st)
            for c in range(1, 12):
                assert st["dropped_" + STAGES[c]] == codes.count(c), (env, STAGES[c], st)
            want = len(cut_pieces(lens, **cut))
            assert pieces_of(st, nbytes) == want >= least, (env, pieces_of(st, nbytes), want, least)
        assert len(cut_pieces(lens, reads=7)) == 43 and len(cut_pieces(lens, reads=299)) == 2 and len(cut_pieces(lens)) == 1
        # ---- the file level: chunks of 100 reads in pieces of 30 -> 4 + 4 + 2 pieces (and twice that for a pair of files) ----
        rf, rr = paired_records(250, seed=114)
        inf, inr = os.path.join(tmp, "pc_F.fastq"), os.path.join(tmp, "pc_R.fastq")
        write_fastq(inf, rf)
        write_fastq(inr, rr)
        fkw = dict(trunc_len=60, max_ee=2)
        kept, counts = restate_fastq(rf, params(rm_phix=True, **fkw), phix())
        kf, kr, pcounts = restate_paired(rf, rr, params(rm_phix=True, **fkw), phix())
        assert 0 < counts[1] < counts[0] and 0 < pcounts[1] < counts[1]
        bf, br = sum(len(r[1]) for r in rf), sum(len(r[1]) for r in rr)
        outs = {}
        for env, npieces in (({}, 3), ({"DADA2HIP_FILTER_PIECE": 30}, 10)):
            out = os.path.join(tmp, "pc_out.fastq")
            st = {}
            got = with_env(env, lambda: api.fastq_filter(inf, out, compress=False, n=100, rm_phix=True, ctx=ctx, stats=st, **fkw))
            assert got == counts and st["reads_in"] == counts[0] and st["reads_kept"] == counts[1], (env, got, counts, st)
            assert read_text(out) == fastq_text(kept), env
            assert pieces_of(st, bf) == npieces, (env, pieces_of(st, bf))
            of, orv = os.path.join(tmp, "pc_oF.fastq.gz"), os.path.join(tmp, "pc_oR.fastq.gz")
            pst = {}
            got = with_env(env, lambda: api.fastq_paired_filter((inf, inr), (of, orv), n=100, rm_phix=True, ctx=ctx, stats=pst, **fkw))
            assert got == pcounts and pst["reads_in"] == pcounts[0] and pst["reads_kept"] == pcounts[1], (env, got, pcounts, pst)
            assert read_text(of) == fastq_text(kf) and read_text(orv) == fastq_text(kr), env
            rest = pst["upload_bytes"] - 2 * (bf + br) - 8 * 2 * len(rf)   # (the bytes are both files', reads_in the forward file's)
            assert rest == 8 * 2 * npieces, (env, rest)
            outs[bool(env)] = ({k: st[k] for k in COUNTED}, {k: pst[k] for k in COUNTED})
        assert outs[True] == outs[False]


# ---- past one piece, 8 192 waves and 16 384 blocks -----------------------------------------------------------------------------------

STRIDED_N, STRIDED_POOL = 2 * PIECE_READS + 1, 4096                        # three pieces; every wave of k_filter_scan takes 8 reads of a piece
STRIDED_LENGTHS = (0, 1, 15, 16, 17, 20, 30, 47, 64, 65, 100, 129, 150)
STRIDED_KW = dict(rm_phix=True, max_ee=0.05, trunc_len=40, max_n=1, kmer_size=2)
_STRIDED = {}


def strided_pool(which="phix"):
    """4 096 distinct reads and their restatement as arrays, once per process: ("phix") against the genome, whose word table the
    kernel keeps in LDS, or ("global") against the 9 000-nt random reference of case_screen_in_global_memory, every seventh read
    long enough replaced by a cut of it."""
    if which not in _STRIDED:
        rng = random.Random(115)
        seqs, quals = mixed_reads(rng, STRIDED_POOL - 2, lengths=STRIDED_LENGTHS, p_phix=0.25, p_n=0.3)
        ls, lq = mixed_reads(rng, 2, lengths=(1500,), p_phix=1.0)
        seqs[1000:1000] = ls[:1]
        quals[1000:1000] = lq[:1]
        seqs[3000:3000] = ls[1:]
        quals[3000:3000] = lq[1:]
        ref = phix()
        if which == "global":
            ref = rand_seq(random.Random(109), 9000)                       # case_screen_in_global_memory's
            r2 = random.Random(116)
            for i in range(3, len(seqs), 7):
                if len(seqs[i]) >= 47:
                    at = r2.randrange(9000 - len(seqs[i]))
                    cut = ref[at: at + len(seqs[i])]
                    seqs[i] = rc(cut) if r2.random() < 0.5 else cut
        # (distinct but for the few reads a length of 0 or 1 allows)
        assert len(seqs) == STRIDED_POOL and len(set(zip(seqs, quals))) >= STRIDED_POOL - 2 * (STRIDED_POOL // len(STRIDED_LENGTHS) + 1)
        assert auto_offset(quals) == 33
        P = params(**STRIDED_KW)
        want = [restate_read(s, q, P, ref, 33) for s, q in zip(seqs, quals)]
        kept = [s[w["off"]: w["off"] + w["len"]] for s, w in zip(seqs, want)]
        arr = {"code": np.array([w["code"] for w in want], dtype=np.int32),
               "window": np.array([(w["off"], w["len"]) for w in want], dtype=np.int32),
               "ee": np.array([w["ee"] for w in want], dtype=np.float64),
               "hits": np.array([w["hits"] for w in want], dtype=np.int32),
               "kmer_counts": np.array([kmer_counts(k, 2) for k in kept], dtype=np.int32),
               "complexity": np.array([complexity(k, 2) for k in kept], dtype=np.float64)}
        counts = np.bincount(arr["code"], minlength=12)
        assert all(counts[c] >= 20 for c in (0, 5, 7, 9, 10)), (which, counts.tolist())
        _STRIDED[which] = dict(seqs=seqs, quals=quals, ref=ref, want=arr)
    return _STRIDED[which]


def strided_order():
    """pool[(i * 2654435761 + i // 4096) % 4096]: neighbours differ, and so do reads 8 192 (a wave's next read), 16 384 (a block's)
    or a piece apart - the product alone has period 4 096, which divides all three, so every run of 4 096 is turned by one more."""
    i = np.arange(STRIDED_N, dtype=np.uint64)
    idx = ((i * np.uint64(2654435761) + i // np.uint64(STRIDED_POOL)) % np.uint64(STRIDED_POOL)).astype(np.int64)
    for d in (1, 4096, 8192, 16384, PIECE_READS, 2 * PIECE_READS):
        assert (idx[d:] != idx[:-d]).all(), d
    return idx


def check_strided_batch(api, which):
    """One dada2hip_filter_reads call on 131 073 reads against the tiled restatement of the pool, every output of every read."""
    d = strided_pool(which)
    idx = strided_order()
    seqs, quals = [d["seqs"][i] for i in idx], [d["quals"][i] for i in idx]
    nbytes = sum(len(s) for s in seqs)
    st = {}
    with api.FilterContext(d["ref"], 16) as ctx:
        assert ctx.stats["table_in_lds"] == (1 if which == "phix" else 0), ctx.stats
        got = api.filter_reads(seqs, quals, ctx, kmers=True, stats=st, **STRIDED_KW)
    want = {k: v[idx] for k, v in d["want"].items()}
    for k in ("code", "window", "hits", "kmer_counts"):
        bad = np.flatnonzero((got[k] != want[k]).reshape(STRIDED_N, -1).any(axis=1))
        assert bad.size == 0, (which, k, "first at read", int(bad[0]), "of", int(bad.size), got[k][bad[0]].tolist(), want[k][bad[0]].tolist())
    bad = np.flatnonzero(got["ee"].view(np.uint64) != want["ee"].view(np.uint64))
    assert bad.size == 0, (which, "ee", "first at read", int(bad[0]), "of", int(bad.size), got["ee"][bad[0]].hex(), want["ee"][bad[0]].hex())
    g, w = got["complexity"], want["complexity"]
    with np.errstate(invalid="ignore"):
        ok = (np.isnan(g) & np.isnan(w)) | (np.abs(g - w) <= 1e-12 * np.abs(w))
    bad = np.flatnonzero(~ok)
    assert bad.size == 0, (which, "complexity", "first at read", int(bad[0]), "of", int(bad.size), float(g[bad[0]]), float(w[bad[0]]))
    counts = np.bincount(want["code"], minlength=12)
    assert st["reads_in"] == STRIDED_N and st["reads_kept"] == counts[0], (st, counts.tolist())
    for c in range(1, 12):
        assert st["dropped_" + STAGES[c]] == counts[c], (STAGES[c], st, counts.tolist())
    assert pieces_of(st, nbytes) == 3 == len(cut_pieces([len(s) for s in seqs])), st
    return st


def check_strided_file(api, tmp):
    """The same batch as a FASTQ file through dada2hip_filter_fastq with its default chunk, plain in and plain out."""
    d = strided_pool("phix")
    idx = strided_order()
    w = d["want"]
    rec = ["%s\n+\n%s\n" % (s, q) for s, q in zip(d["seqs"], d["quals"])]
    kept = ["%s\n+\n%s\n" % (s[o: o + n], q[o: o + n]) for s, q, (o, n) in zip(d["seqs"], d["quals"], w["window"].tolist())]
    src, out = os.path.join(tmp, "strided.fastq"), os.path.join(tmp, "strided_out.fastq")
    with open(src, "w") as fh:
        fh.write("".join("@r%d\n%s" % (i, rec[p]) for i, p in enumerate(idx.tolist())))
    code = w["code"][idx]
    want_text = "".join("@r%d\n%s" % (i, kept[p]) for i, p in enumerate(idx.tolist()) if code[i] == 0)
    counts = np.bincount(code, minlength=12)
    st = {}
    kw = {k: v for k, v in STRIDED_KW.items() if k not in ("rm_phix", "kmer_size")}
    with api.FilterContext(d["ref"], 16) as ctx:
        got = api.fastq_filter(src, out, compress=False, rm_phix=True, ctx=ctx, stats=st, **kw)
    assert got == (STRIDED_N, int(counts[0])) and 0 < counts[0] < STRIDED_N, (got, counts.tolist())
    with open(out) as fh:
        text = fh.read()
    if text != want_text:
        a, b = text.split("\n"), want_text.split("\n")
        at = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
        raise AssertionError(("the written file differs", "first at line", at, a[at: at + 1], b[at: at + 1], len(a), len(b)))
    assert st["reads_in"] == STRIDED_N and st["reads_kept"] == counts[0], (st, counts.tolist())
    for c in range(1, 12):
        assert st["dropped_" + STAGES[c]] == counts[c], (STAGES[c], st, counts.tolist())
    assert pieces_of(st, sum(len(d["seqs"][p]) for p in idx.tolist())) == 3, st
    return st


def _raises(exc, fn, text=None, code=None):
    try:
        fn()
    except exc as e:
        assert text is None or text in str(e), str(e)
        assert code is None or e.code == code, (e.code, code)
        return
    raise AssertionError("no %s raised" % exc.__name__)


def case_input_errors(api, tmp):
    E = api._lib.Dada2HipError
    g = phix()
    _raises(E, lambda: api.FilterContext(g, 33), code=4)
    _raises(E, lambda: api.FilterContext(g, 0), code=4)
    _raises(E, lambda: api.FilterContext(g[:100] + "N" + g[100:], 16), code=4)
    _raises(E, lambda: api.FilterContext(g[:100].lower(), 16))
    _raises(E, lambda: api.FilterContext("ACGTACGT", 16), code=1)
    _raises(E, lambda: api.match_ref(["ACGT"], g, 33, True), code=4)
    _raises(NotImplementedError, lambda: api.seq_complexity(["ACGT" * 10], 2, window=25), "not supported")
    _raises(E, lambda: api.seq_complexity(["ACGT" * 10], 5), code=4)
    with open_ctx(api, screen=False) as ctx:
        _raises(E, lambda: api.filter_reads(["ACGT"], ["IIII"], ctx, rm_phix=True), code=1)
        _raises(E, lambda: api.filter_reads(["ACGT"], ["IIII"], ctx, quality_type=40), code=1)
        _raises(ValueError, lambda: api.filter_reads(["ACGT"], ["III"], ctx))
        for kw in ({"orient_fwd": "ACGT"}, {"match_ids": True}, {"id_sep": ":"}, {"id_field": 1}):
            _raises(NotImplementedError, lambda: api.filter_and_trim(FASTQS["sam1F"], os.path.join(tmp, "x.fastq.gz"), ctx=ctx, **kw), "not supported")
            _raises(NotImplementedError, lambda: api.fastq_filter(FASTQS["sam1F"], os.path.join(tmp, "x.fastq.gz"), ctx=ctx, **kw), "not supported")
        _raises(ValueError, lambda: api.filter_and_trim(FASTQS["sam1F"], os.path.join(tmp, "x.fastq.gz"), rm_phix=True), "ships no copy")
        _raises(ValueError, lambda: api.fastq_filter(FASTQS["sam1F"], os.path.join(tmp, "x.fastq.gz"), ctx=ctx, trunc_len=(240, 160)), "length 1")
        _raises(E, lambda: api.fastq_filter(os.path.join(tmp, "missing.fastq"), os.path.join(tmp, "x.fastq.gz"), ctx=ctx), code=1)
    assert not hasattr(api, "remove_primers") and not hasattr(api, "plot_complexity")
    assert not os.path.exists(os.path.join(tmp, "x.fastq.gz"))


def _with_tmp(fn, **kw):
    def run(api):
        import tempfile
        with tempfile.TemporaryDirectory() as tmp:
            fn(api, tmp, **kw)
    return run


CASES = {"lengths": case_lengths, "batches": case_batches, "letters": case_letters, "truncq": case_truncq, "trims": case_trims,
         "minq": case_minq, "ee_threshold": case_ee_threshold, "screen": case_screen,
         "screen_in_global_memory": case_screen_in_global_memory, "complexity": case_complexity, "paired": _with_tmp(case_paired),
         "files": _with_tmp(case_files), "pieces": _with_tmp(case_pieces), "fixtures": _with_tmp(case_fixtures), "vignette": _with_tmp(case_vignette),
         "input_errors": _with_tmp(case_input_errors)}
CASE_NAMES = tuple(CASES)


def emu_run(names=None):
    """The emulator's job (tests/test_emu_filter.py): every case; the vignette's front without the denoising, which the emulator
    has tests of its own for."""
    from dada2_amd import api
    emu = dict(CASES, vignette=_with_tmp(case_vignette, denoise=False), fixtures=_with_tmp(case_fixtures, names=("sam1F",)))
    names = names or CASE_NAMES
    for name in names:
        emu[name](api)
    return "ok %d cases" % len(names)
