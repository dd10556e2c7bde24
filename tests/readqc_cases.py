"""The read diagnostics restated in numpy, and the cases the CPU, emulator and GPU tests run against the restatement.

Restated, with the reference's lines beside the code (R/plot-methods.R for the quality profile, R/filter.R for the complexity):
  * ShortRead qa()'s perCycle$quality as plotQualityProfile reads it: the data frame Cycle / Score / Count with Count > 0 rows
    only, by cycle, then by ascending score (restate_table, long_df); `naive_counts` is an independent per-character count that
    tests/test_readqc.py holds restate_table to;
  * the statistics of R/plot-methods.R:178-205 (restate_profile), get_quant in double as R divides;
  * seqComplexity (R/filter.R:1248-1268) with sindex (:1271-1275), the sum in np.longdouble as R's sum() accumulates
    (restate_complexity): the loop over window starts literally, so its quirks come with it.
The stated deviations are restated too: `n` takes the FIRST n records, n=None all of them.

A case takes the module dada2_amd.readqc and raises AssertionError.  CASES / CASE_NAMES / emu_run() as in tests/primer_cases.py:
tests/test_gpu_readqc.py runs every case on the card, tests/test_emu_readqc.py under the emulator (the lighter form of the file
cases); check_strided_table is the card's alone."""
import gzip
import os
import random
import tempfile

import numpy as np

from primer_cases import _raises, with_env

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
FIXTURES = {name: os.path.join(GOLDEN, name + ".fastq.gz") for name in ("sam1F", "sam1R", "samPB")}
NSCORE = 94
PIECE_ENV = {"DADA2HIP_READQC_PIECE": 3, "DADA2HIP_READQC_PIECE_BYTES": 200}
CX_RTOL = 1e-12          # the issue's bound: <= 256 positive terms <= 1/e summed in double against long double, then exp
CX_SEEN = {"max_rel": 0.0}


# ---- files ---------------------------------------------------------------------------------------------------------------------------

def read_fastq(path):
    with open(path, "rb") as fh:
        data = fh.read()
    lines = (gzip.decompress(data) if data[:2] == b"\x1f\x8b" else data).decode("latin-1").split("\n")
    return [(lines[i], lines[i + 1], lines[i + 3]) for i in range(0, len(lines) - 3, 4)]


def write_fastq(path, records, gz=False):
    text = "".join("%s\n%s\n+\n%s\n" % r for r in records).encode("latin-1")
    with open(path, "wb") as fh:
        fh.write(gzip.compress(text) if gz else text)


# ---- the quality profile restated ----------------------------------------------------------------------------------------------------

def naive_counts(quals):
    """{(cycle, letter): count}, cycle 1-based, one character at a time."""
    out = {}
    for q in quals:
        for c, ch in enumerate(q):
            key = (c + 1, ord(ch))
            out[key] = out.get(key, 0) + 1
    return out


def restate_table(quals):
    """(ncycle, 94) int64: counts[cycle - 1][letter - 33]; a letter outside '!'..'~' raises ValueError with the read's number."""
    ncycle = max((len(q) for q in quals), default=0)
    tab = np.zeros((ncycle, NSCORE), dtype=np.int64)
    for i, q in enumerate(quals):
        a = np.frombuffer(q.encode("latin-1"), dtype=np.uint8).astype(np.int64) - 33
        if ((a < 0) | (a >= NSCORE)).any():
            raise ValueError("read %d" % (i + 1))
        np.add.at(tab, (np.arange(len(a)), a), 1)
    return tab


def auto_offset(quals):
    """derep.cpp's Auto rule: any letter below ';' means Phred+33, otherwise 64 (no letter at all: 33)."""
    m = min((ord(ch) for q in quals for ch in q), default=0)
    return 33 if m < 59 else 64


def long_df(tab, score0):
    """perCycle$quality: Cycle, Score, Count of the Count > 0 cells, by cycle, then by ascending score."""
    cyc, col = np.nonzero(tab)
    return {"cycle": cyc + 1, "score": col + score0, "count": tab[cyc, col]}


def get_quant(xx, yy, q):                                           # plot-methods.R:179
    return xx[np.flatnonzero(np.cumsum(yy).astype(np.float64) / np.float64(np.sum(yy)) >= q)[0]]


def restate_stats(df, denom):
    """plot-methods.R:178-192 on one data frame: rowsum / by() per cycle."""
    out = {k: [] for k in ("Cycle", "Mean", "Q25", "Q50", "Q75", "Cum")}
    for cyc in np.unique(df["cycle"]):
        m = df["cycle"] == cyc
        score, count = df["score"][m], df["count"][m]
        out["Cycle"].append(int(cyc))
        out["Mean"].append(np.float64(np.sum(score * count)) / np.float64(np.sum(count)))           # :178
        out["Q25"].append(float(get_quant(score, count, 0.25)))                                    # :180
        out["Q50"].append(float(get_quant(score, count, 0.5)))                                     # :181
        out["Q75"].append(float(get_quant(score, count, 0.75)))                                    # :182
        out["Cum"].append(10.0 * np.float64(np.sum(count)) / denom if denom else np.nan)          # :183, :192
    return {k: np.array(v, dtype=np.int64 if k == "Cycle" else np.float64) for k, v in out.items()}


def restate_profile(files, n=None, aggregate=False, quality_type=0):
    """plotQualityProfile's data for `files` = [(basename, [quality strings])]: the structure dada2_amd.readqc.quality_profile
    returns.  The first n records are profiled (n=None: all); rc counts the file (:171)."""
    cap = float("inf") if n is None else n
    entries, tabs = [], []
    for name, quals in files:
        rc = len(quals)
        prof = quals if n is None else quals[:n]
        off = quality_type or auto_offset(quals[:100000])
        tab = restate_table(prof)
        df = long_df(tab, 33 - off)
        entries.append({"file": name, "rc": rc, "profiled": len(prof), "qual_offset": off, "table": df,
                        "stats": restate_stats(df, min(rc, cap))})                                 # :192 min(rc, n)
        tabs.append((tab, 33 - off))
    mins = [int(e["table"]["score"].min()) for e in entries if len(e["table"]["score"])]
    min_score = min(mins) if mins else None                                                        # :195
    for e in entries:
        e["minScore"] = min_score
    agg = None
    if aggregate and entries:                                                                      # :198-205: Count ~ Cycle + Score, summed
        cells = {}
        for tab, s0 in tabs:
            for c, j in zip(*np.nonzero(tab)):
                cells[(c + 1, j + s0)] = cells.get((c + 1, j + s0), 0) + int(tab[c, j])
        keys = sorted(cells)
        df = {"cycle": np.array([k[0] for k in keys], dtype=np.int64), "score": np.array([k[1] for k in keys], dtype=np.int64),
              "count": np.array([cells[k] for k in keys], dtype=np.int64)}
        agg = {"table": df, "stats": restate_stats(df, sum(min(e["rc"], cap) for e in entries)), "rc": sum(e["rc"] for e in entries)}
    return {"files": entries, "minScore": min_score, "aggregate": agg}


def assert_same_frames(got, want, what):
    for part in ("table", "stats"):
        assert set(got[part]) == set(want[part]), (what, part)
        for k in want[part]:
            g, w = np.asarray(got[part][k]), np.asarray(want[part][k])
            assert g.shape == w.shape and np.array_equal(g, w, equal_nan=True), (what, part, k, g[:8], w[:8])


def assert_same_profile(got, want, what=""):
    assert got["minScore"] == want["minScore"] and len(got["files"]) == len(want["files"]), (what, got["minScore"], want["minScore"])
    for g, w in zip(got["files"], want["files"]):
        for k in ("file", "rc", "profiled", "qual_offset", "minScore"):
            assert g[k] == w[k], (what, k, g[k], w[k])
        assert_same_frames(g, w, (what, g["file"]))
    assert (got["aggregate"] is None) == (want["aggregate"] is None), what
    if want["aggregate"] is not None:
        assert got["aggregate"]["rc"] == want["aggregate"]["rc"], what
        assert_same_frames(got["aggregate"], want["aggregate"], (what, "aggregate"))


# ---- seqComplexity restated ----------------------------------------------------------------------------------------------------------

_CODE = {"A": 0, "C": 1, "G": 2, "T": 3}


def kmer_index(seq, k):
    """Per k-mer start the bin of oligonucleotideFrequency(width = k) (first letter most significant), -1 for a k-mer with a letter
    other than A/C/G/T: those are not counted."""
    code = np.array([_CODE.get(c, -1) for c in seq], dtype=np.int64)
    nk = len(seq) - k + 1
    if nk <= 0:
        return np.zeros(0, dtype=np.int64)
    idx, bad = np.zeros(nk, dtype=np.int64), np.zeros(nk, dtype=bool)
    for t in range(k):
        part = code[t:t + nk]
        bad |= part < 0
        idx = idx * 4 + np.maximum(part, 0)
    idx[bad] = -1
    return idx


def sindex(x):                                                      # filter.R:1271-1275
    x = np.asarray(x, dtype=np.float64)
    tot = x.sum()
    if tot == 0:                                                    # 0 / 0: y is NaN, y[y > 0] NA, the sum NA
        return float("nan")
    y = x / tot
    y = y[y > 0]
    acc = np.cumsum((-y * np.log(y)).astype(np.longdouble))[-1]    # (R's sum(): a long double accumulator, in order)
    return float(np.exp(np.float64(acc)))


def pmin(a, b):
    return float("nan") if (a != a or b != b) else min(a, b)


NO_START = "seq(1, max(width) - window, by)"
KMER_WINDOW = "The window over which kmer frequency is calculated must be larger than the kmerSize."


def restate_complexity(seqs, kmer_size=2, window=None, by=5):
    if window is not None and kmer_size >= window:                  # :1249
        raise ValueError(KMER_WINDOW)
    nb = 4 ** kmer_size                                             # :1255
    idx = [kmer_index(s, kmer_size) for s in seqs]
    freq = lambda a: np.bincount(a[a >= 0], minlength=nb)           # noqa: E731
    if window is None:                                              # :1257
        return np.array([sindex(freq(a)) for a in idx], dtype=np.float64)
    width = [len(s) for s in seqs]
    si = [float(nb)] * len(seqs)                                    # :1259
    if max(width, default=0) - window < 1:                          # :1260 seq(1, to < 1, by > 0) stops
        raise ValueError(NO_START)
    for i in range(1, max(width) - window + 1, by):                 # :1260
        for j, a in enumerate(idx):
            if width[j] >= i + window - 1:                          # :1261
                si[j] = pmin(si[j], sindex(freq(a[i - 1:i - 1 + window - kmer_size + 1])))   # :1262-1264
    return np.array(si, dtype=np.float64)


def assert_complexity(got, want, what=""):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.array_equal(np.isnan(got), np.isnan(want)), (what, "NaN positions", np.flatnonzero(np.isnan(got) != np.isnan(want))[:8])
    ok = ~np.isnan(want)
    rel = np.abs(got[ok] - want[ok]) / np.abs(want[ok])
    worst = float(rel.max()) if rel.size else 0.0
    CX_SEEN["max_rel"] = max(CX_SEEN["max_rel"], worst)
    print("complexity %s: %d values, %d NaN, largest relative difference %.3g" % (what, got.size, int((~ok).sum()), worst))
    assert worst <= CX_RTOL, (what, worst, int(np.argmax(rel)))


# ---- the cases: the quality table -------------------------------------------------------------------------------------------------

def rand_qual(rng, n, lo=33, hi=126):
    return "".join(chr(rng.randint(lo, hi)) for _ in range(n))


def check_table(rq, quals, what, stats=None):
    got = rq.quality_table(quals, stats=stats)
    want = restate_table(quals)
    assert got.shape == want.shape and got.dtype == np.int64, (what, got.shape, want.shape)
    bad = np.argwhere(got != want)
    assert bad.size == 0, (what, "first at (cycle, column)", bad[0].tolist(), int(got[tuple(bad[0])]), int(want[tuple(bad[0])]), len(bad))
    return got


def case_table_lengths(rq, light=False):
    rng = random.Random(301)
    lens = [0, 1, 63, 64, 65, 128, 129] * 3 + [0, 129, 1]
    rng.shuffle(lens)
    st = {}
    check_table(rq, [rand_qual(rng, n) for n in lens], "mixed lengths", stats=st)
    assert st["reads_in"] == len(lens) and st["cycles"] == 129 and st["pieces"] == 1, st
    check_table(rq, ["", "", ""], "empty reads only")
    assert rq.quality_table([]).shape == (0, NSCORE)
    check_table(rq, ["!" * 70, "~" * 65, "!~" * 40, "~"], "the first and the last letter")
    got = check_table(rq, ["!" * 64 + "~"] * 5, "one letter per cycle")
    assert got[:64, 0].tolist() == [5] * 64 and got[64, 93] == 5 and got.sum() == 5 * 65


def case_table_pieces(rq, light=False):
    rng = random.Random(302)
    grow = [rand_qual(rng, n) for n in (5, 10, 20, 70, 64, 65, 200, 130, 129)]   # three pieces of three reads, each reaching further
    st = {}
    with_env({"DADA2HIP_READQC_PIECE": 3}, lambda: check_table(rq, grow, "pieces that grow", stats=st))
    assert st["pieces"] == 3 and st["cycles"] == 200, st
    shrink = grow[::-1]
    with_env({"DADA2HIP_READQC_PIECE": 3}, lambda: check_table(rq, shrink, "pieces that shrink"))
    lens = [0, 1, 63, 64, 65, 128, 129, 199, 200, 201, 0, 77]
    st = {}
    with_env(PIECE_ENV, lambda: check_table(rq, [rand_qual(rng, n) for n in lens], "3 reads and 200 bases", stats=st))
    assert st["pieces"] >= 7, st                                   # (a read above 200 bases is a piece of its own)


def case_table_refusals(rq, light=False):
    rng = random.Random(303)
    E = rq._lib.Dada2HipError
    quals = [rand_qual(rng, 70) for _ in range(9)]
    for ch in (" ", "\x7f", "\xe9", "\x00"):
        bad = list(quals)
        bad[4] = bad[4][:66] + ch + bad[4][67:]
        _raises(E, lambda: rq.quality_table(bad), "read 5 ", code=1)
        with_env(PIECE_ENV, lambda: _raises(E, lambda: rq.quality_table(bad), "read 5 ", code=1))
    import ctypes as C
    L, eb = rq._lib.lib(), C.create_string_buffer(512)
    off = np.array([0, 4], dtype=np.int64)
    small = np.zeros((3, NSCORE), dtype=np.int64)
    rv = L.dada2hip_qprofile_reads(1, b"IIII", off.ctypes.data, 0, 3, small.ctypes.data, None, eb, 512)
    assert rv == 1 and b"fewer cycles" in eb.value, (rv, eb.value)
    wide = np.full((6, NSCORE), 7, dtype=np.int64)                  # a table with more cycles than the longest read: set, not added to
    rv = L.dada2hip_qprofile_reads(1, b"IIII", off.ctypes.data, 0, 6, wide.ctypes.data, None, eb, 512)
    assert rv == 0 and wide.sum() == 4 and wide[:4, ord("I") - 33].tolist() == [1] * 4, (rv, eb.value)


def _plain_copy(tmp, name):
    path = os.path.join(tmp, name + ".fastq")
    if not os.path.exists(path):
        with open(FIXTURES[name], "rb") as fh, open(path, "wb") as out:
            out.write(gzip.decompress(fh.read()))
    return path


def case_profile_files(rq, light=False):
    """The three fixtures as files, plain and gzip, in chunks of 400 and of 10^6 records: equal to one another and to the restatement."""
    with tempfile.TemporaryDirectory() as tmp:
        for name in (("sam1F",) if light else ("sam1F", "sam1R", "samPB")):
            quals = [q for _, _, q in read_fastq(FIXTURES[name])]
            want = restate_table(quals)
            first = None
            for path in (FIXTURES[name], _plain_copy(tmp, name)):
                for chunk in ((400,) if light else (400, 10 ** 6)):
                    st = {}
                    got = rq.quality_table_fastq(path, chunk_reads=chunk, stats=st)
                    assert (got["rc"], got["profiled"], got["qual_offset"]) == (len(quals), len(quals), 33), (name, path, chunk, got)
                    assert np.array_equal(got["counts"], want), (name, path, chunk)
                    assert st["reads_in"] == len(quals) and st["cycles"] == want.shape[0], st
                    first = got["counts"] if first is None else first
                    assert np.array_equal(got["counts"], first)
            prof = rq.quality_profile(FIXTURES[name])
            assert_same_profile(prof, restate_profile([(name + ".fastq.gz", quals)]), name)
        # samPB's reads are of 1 456 to 1 511 cycles: in chunks of 7 records the table grows under later chunks
        if not light:
            quals = [q for _, _, q in read_fastq(FIXTURES["samPB"])][:60]
            small = os.path.join(tmp, "pb60.fastq")
            write_fastq(small, read_fastq(FIXTURES["samPB"])[:60])
            got = with_env(PIECE_ENV, lambda: rq.quality_table_fastq(small, chunk_reads=7))
            assert np.array_equal(got["counts"], restate_table(quals)) and got["rc"] == 60


def case_profile_n_and_aggregate(rq, light=False):
    qf = [q for _, _, q in read_fastq(FIXTURES["sam1F"])]
    qr = [q for _, _, q in read_fastq(FIXTURES["sam1R"])]
    for n in (1000, 1500, 5000):                                    # below, at and above rc
        got = rq.quality_profile(FIXTURES["sam1F"], n=n)
        assert_same_profile(got, restate_profile([("sam1F.fastq.gz", qf)], n=n), "n = %d" % n)
        assert got["files"][0]["rc"] == 1500 and got["files"][0]["profiled"] == min(n, 1500)
    got = rq.quality_table_fastq(FIXTURES["sam1F"], n=1000, chunk_reads=300)   # the limit falls inside a chunk
    assert got["profiled"] == 1000 and got["rc"] == 1500 and np.array_equal(got["counts"], restate_table(qf[:1000]))
    if light:
        return
    files = [FIXTURES["sam1F"], FIXTURES["sam1R"]]
    named = [("sam1F.fastq.gz", qf), ("sam1R.fastq.gz", qr)]
    for n in (None, 1000):
        got = rq.quality_profile(files, n=n, aggregate=True)
        assert_same_profile(got, restate_profile(named, n=n, aggregate=True), "aggregate, n = %s" % n)
        assert got["aggregate"]["rc"] == 3000
    assert rq.quality_profile(files)["aggregate"] is None


def case_profile_phred64_and_rules(rq, light=False):
    rng = random.Random(305)
    E = rq._lib.Dada2HipError
    with tempfile.TemporaryDirectory() as tmp:
        recs = [("@r%d some text" % i, "ACGT" * 20, rand_qual(rng, 80, 64, 104)) for i in range(40)]
        recs[7] = (recs[7][0], "ACG", "hhh")
        p64 = os.path.join(tmp, "p64.fastq")
        write_fastq(p64, recs)
        quals = [q for _, _, q in recs]
        got = rq.quality_profile(p64)
        assert got["files"][0]["qual_offset"] == 64 and 0 <= got["minScore"] <= 40
        assert_same_profile(got, restate_profile([("p64.fastq", quals)]), "Phred+64, Auto")
        got = rq.quality_profile(p64, quality_type=33)             # the offset given: the same letters as scores 31..71
        assert_same_profile(got, restate_profile([("p64.fastq", quals)], quality_type=33), "offset given")
        assert got["minScore"] >= 31
        mixed = os.path.join(tmp, "mixed.fastq.gz")
        write_fastq(mixed, [("@m%d" % i, "A" * 30, rand_qual(rng, 30, 35, 73)) for i in range(25)], gz=True)
        both = rq.quality_profile([p64, mixed], aggregate=True)   # two offsets: the tables are summed by score
        assert_same_profile(both, restate_profile([("p64.fastq", quals), ("mixed.fastq.gz", [q for _, _, q in read_fastq(mixed)])], aggregate=True),
                            "two offsets")
        bad = list(recs)
        bad[11] = (bad[11][0], bad[11][1], bad[11][2][:40] + " " + bad[11][2][41:])
        pbad = os.path.join(tmp, "bad.fastq")
        write_fastq(pbad, bad)
        _raises(E, lambda: rq.quality_table_fastq(pbad), "read 12 (@r11 some text)", code=1)
        _raises(E, lambda: rq.quality_table_fastq(pbad, chunk_reads=5), "read 12 (@r11 some text)", code=1)
        assert rq.quality_table_fastq(pbad, n=11)["profiled"] == 11   # (the record is never profiled)
        _raises(ValueError, lambda: rq.quality_profile(tmp), "directory")
        _raises(E, lambda: rq.quality_table_fastq(tmp), "directory", code=1)
        _raises(E, lambda: rq.quality_table_fastq(os.path.join(tmp, "missing.fastq")), "do not exist", code=1)
        _raises(E, lambda: rq.quality_table_fastq(p64, quality_type=50), "offset", code=1)
        empty = os.path.join(tmp, "empty.fastq")
        write_fastq(empty, [])
        got = rq.quality_profile(empty)
        assert got["files"][0]["rc"] == 0 and got["minScore"] is None and len(got["files"][0]["stats"]["Cycle"]) == 0


# ---- the cases: the complexity ------------------------------------------------------------------------------------------------------

SQ_NORM = "TACGGAAGGTCCGGGCGTTATCCGGATTTATTGGGTTTAAAGGGAGCGTAGGCCGGAGATTAAGCGTGTTGTGA"   # filter.R:1241-1243
SQ_LOWC = "TCCTTCTTCTCCTCTCTTTCTCCTTCTTTCTTTTTTTTCCCTTTCTCTTCTTCTTTTTCTTCCTTCCTTTTTTC"
SQ_PART = "TTTTTCTTCTCCCCCTTCCCCTTTCCTTTTCTCCTTTTTTCCTTTAGTGCAGTTGAGGCAGGCGGAATTCGTGG"


def rand_seq(rng, n, letters="ACGT"):
    return "".join(rng.choice(letters) for _ in range(n))


def check_complexity(rq, seqs, what, **kw):
    got = rq.seq_complexity(seqs, **kw)
    want = restate_complexity(seqs, **kw)
    assert_complexity(got, want, what)
    return want


def case_complexity_null(rq, light=False):
    """window = None is api.seq_complexity, bit for bit."""
    from dada2_amd import api
    rng = random.Random(311)
    seqs = [SQ_NORM, SQ_LOWC, SQ_PART, "", "N" * 30, "ACGTN" * 20] + [rand_seq(rng, rng.randrange(1, 200), "ACGTN") for _ in range(40)]
    for k in (1, 2, 3, 4):
        got, ref = rq.seq_complexity(seqs, kmer_size=k), api.seq_complexity(seqs, kmer_size=k)
        assert got.tobytes() == ref.tobytes(), k
        assert_complexity(got, restate_complexity(seqs, kmer_size=k), "window = None, k = %d" % k)
    _raises(NotImplementedError, lambda: api.seq_complexity(seqs, window=25))
    assert not hasattr(api, "plot_complexity")


def case_complexity_example(rq, light=False):
    want = check_complexity(rq, [SQ_NORM, SQ_LOWC, SQ_PART], "the reference's example", kmer_size=3, window=25)
    whole = restate_complexity([SQ_NORM, SQ_LOWC, SQ_PART])
    assert whole[0] > 12 and whole[1] < 5 and whole[2] > 8 and want[0] > 2 * want[2] and abs(want[2] - want[1]) < 1, (whole, want)   # the window finds the low-complexity half


def case_complexity_steps(rq, light=False):
    rng = random.Random(312)
    seqs = [rand_seq(rng, n, "ACGGTTTT") for n in (40, 41, 63, 64, 65, 90, 127, 128, 129, 130, 200, 200)]
    for by in (1, 5, 50):                                           # 50: above the window
        check_complexity(rq, seqs, "by = %d" % by, window=30, by=by)
    for k in (1, 2, 3, 4):
        check_complexity(rq, seqs, "k = %d" % k, kmer_size=k, window=20, by=3)
    with_env(PIECE_ENV, lambda: check_complexity(rq, seqs, "3 reads and 200 bases", window=30, by=5))
    check_complexity(rq, seqs, "window 40 = the shortest read", window=40, by=1)
    check_complexity(rq, seqs + [rand_seq(rng, 300)], "a wide window", kmer_size=4, window=256 + 3, by=7)
    if not light:
        check_complexity(rq, [rand_seq(rng, 700, "ACCGT"), rand_seq(rng, 1100)], "window 1 024", kmer_size=4, window=1024, by=11)


def case_complexity_quirks(rq, light=False):
    rng = random.Random(313)
    low = "T" * 12
    # a read shorter than the window beside longer ones keeps 4^k
    want = check_complexity(rq, ["ACGTACGTAC", rand_seq(rng, 50), rand_seq(rng, 60)], "shorter than the window", window=20, by=1)
    assert want[0] == 16.0
    # two reads of the maximal length end in a low-complexity window that is never tested; one base shorter, and it is
    body = "G" + rand_seq(rng, 47) + "G"                            # (no T next to the tail: only the last window is all T)
    seqs = [body + low, body[::-1] + low, body[1:] + low, rand_seq(rng, 30)]
    want = check_complexity(rq, seqs, "the last window of the longest reads", window=12, by=1)
    assert want[2] == 1.0 and want[0] > 1.0 and want[1] > 1.0, want
    with_env({"DADA2HIP_READQC_PIECE": 1}, lambda: check_complexity(rq, seqs, "... a read a piece", window=12, by=1))
    want = check_complexity(rq, seqs, "... its last start off the grid of by", window=12, by=5)   # start 49 is no 1 + 5 j
    assert want[2] > 1.0, want
    want = check_complexity(rq, seqs, "... and on it", window=12, by=6)                           # 49 = 1 + 6 * 8
    assert want[2] == 1.0, want
    # N inside a window: its k-mers are not counted; a tested window of N only makes the read NaN for good
    seqs = [rand_seq(rng, 30) + "N" + rand_seq(rng, 30), rand_seq(rng, 20) + "N" * 15 + rand_seq(rng, 26), "N" * 61, rand_seq(rng, 62),
            "ACGT" * 5 + "NANANANANANA" + "ACGT" * 7]
    want = check_complexity(rq, seqs, "N in windows", window=12, by=1)
    assert not np.isnan(want[0]) and np.isnan(want[1]) and np.isnan(want[2]) and not np.isnan(want[3]), want
    want = check_complexity(rq, seqs, "N, k = 3", kmer_size=3, window=12, by=1)
    assert np.isnan(want[4])                                        # NANANANANANA: no 3-mer without an N
    want = check_complexity(rq, seqs, "N, by = 5", window=12, by=5)
    check_complexity(rq, ["acgtacgtacgtacgtacgt", rand_seq(rng, 40)], "lower case is no A/C/G/T", window=10, by=2)


def case_complexity_refusals(rq, light=False):
    E = rq._lib.Dada2HipError
    seqs = [SQ_NORM, SQ_LOWC]
    for k, w in ((2, 2), (3, 2), (4, 4)):
        _raises(E, lambda: rq.seq_complexity(seqs, kmer_size=k, window=w), KMER_WINDOW, code=1)
        _raises(ValueError, lambda: restate_complexity(seqs, kmer_size=k, window=w), KMER_WINDOW)
    _raises(E, lambda: rq.seq_complexity(seqs, window=len(SQ_NORM)), NO_START, code=1)   # max(width) == window
    _raises(ValueError, lambda: restate_complexity(seqs, window=len(SQ_NORM)), NO_START)
    _raises(E, lambda: rq.seq_complexity(seqs, window=200), NO_START, code=1)
    _raises(E, lambda: rq.seq_complexity([], window=20), NO_START, code=1)
    check_complexity(rq, seqs, "max(width) = window + 1", window=len(SQ_NORM) - 1)
    _raises(E, lambda: rq.seq_complexity(seqs, kmer_size=5, window=25), "1..4", code=4)
    _raises(E, lambda: rq.seq_complexity(seqs, window=1025), "1024", code=4)
    _raises(E, lambda: rq.seq_complexity(seqs, window=25, by=0), "by", code=1)
    _raises(ValueError, lambda: rq.seq_complexity(seqs, window=0), KMER_WINDOW)


def case_complexity_files(rq, light=False):
    recs = read_fastq(FIXTURES["samPB"])
    n = 40 if light else None
    seqs = [s for _, s, _ in recs][:n]
    want = restate_complexity(seqs, window=100)
    got = rq.complexity_fastq(FIXTURES["samPB"], window=100, n=n, chunk_reads=16 if light else 150)
    assert_complexity(got, want, "samPB, window 100, from the file")
    if light:
        return
    st = {}
    got = rq.complexity_fastq(FIXTURES["samPB"], window=100, n=120, stats=st)   # the maximum is the profiled records'
    assert_complexity(got, restate_complexity(seqs[:120], window=100), "samPB, the first 120")
    assert st["reads_in"] == 500 and st["reads_profiled"] == 120, st
    prof = rq.complexity_profile([FIXTURES["sam1F"], FIXTURES["samPB"]], n=200)
    f = [s for _, s, _ in read_fastq(FIXTURES["sam1F"])][:200]
    assert prof["file"] == ["sam1F.fastq.gz"] * 200 + ["samPB.fastq.gz"] * 200
    assert_complexity(prof["complexity"], np.concatenate([restate_complexity(f), restate_complexity(seqs[:200])]), "plotComplexity's frame")
    from dada2_amd import api
    assert prof["complexity"][:200].tobytes() == api.seq_complexity(f).tobytes()
    E = rq._lib.Dada2HipError
    _raises(E, lambda: rq.complexity_fastq(FIXTURES["sam1F"], window=250), NO_START, code=1)   # every read has 250 letters
    _raises(E, lambda: rq.complexity_fastq(FIXTURES["sam1F"], kmer_size=3, window=3), KMER_WINDOW, code=1)
    _raises(E, lambda: rq.complexity_fastq(os.path.dirname(FIXTURES["sam1F"]), window=30), "directory", code=1)


# ---- more reads than one block's slice (the card's alone) ------------------------------------------------------------------------------

STRIDED_POOL = 4096
STRIDED_N = 70000
STRIDED_LEN = 70


def check_strided_table(rq):
    """70 000 reads of 70 cycles: two pieces of a call, and in the first 128 blocks per tile of cycles with 512 reads each.  4 096
    distinct quality strings, laid out so that reads a wave's stride or a piece apart differ; the table is the pool's, weighted."""
    rng = np.random.default_rng(306)
    pool = rng.integers(33, 127, size=(STRIDED_POOL, STRIDED_LEN), dtype=np.uint8)
    i = np.arange(STRIDED_N, dtype=np.uint64)
    idx = ((i * np.uint64(2654435761) + i // np.uint64(STRIDED_POOL)) % np.uint64(STRIDED_POOL)).astype(np.int64)
    for d in (1, 4, 512, 65536):
        assert (idx[d:] != idx[:-d]).all(), d
    mult = np.bincount(idx, minlength=STRIDED_POOL)
    want = np.zeros((STRIDED_LEN, NSCORE), dtype=np.int64)
    np.add.at(want, (np.broadcast_to(np.arange(STRIDED_LEN), pool.shape), pool.astype(np.int64) - 33), np.broadcast_to(mult[:, None], pool.shape))
    quals = [pool[j].tobytes() for j in idx]
    st = {}
    got = rq.quality_table(quals, stats=st)
    assert np.array_equal(got, want), np.argwhere(got != want)[:4]
    assert st["pieces"] == 2 and st["reads_in"] == STRIDED_N and got.sum() == STRIDED_N * STRIDED_LEN, st
    return st


CASES = {"table_lengths": case_table_lengths, "table_pieces": case_table_pieces, "table_refusals": case_table_refusals,
         "profile_files": case_profile_files, "profile_n_and_aggregate": case_profile_n_and_aggregate,
         "profile_phred64_and_rules": case_profile_phred64_and_rules, "complexity_null": case_complexity_null,
         "complexity_example": case_complexity_example, "complexity_steps": case_complexity_steps,
         "complexity_quirks": case_complexity_quirks, "complexity_refusals": case_complexity_refusals,
         "complexity_files": case_complexity_files}
CASE_NAMES = tuple(CASES)


def emu_run(names=None):
    """The emulator's job (tests/test_emu_readqc.py): every case, the file cases in their lighter form."""
    from dada2_amd import readqc
    names = names or CASE_NAMES
    for name in names:
        CASES[name](readqc, light=True)
    return "ok %d cases, largest relative difference of a complexity %.3g" % (len(names), CX_SEEN["max_rel"])
