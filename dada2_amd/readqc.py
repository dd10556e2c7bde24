"""Read diagnostics on the GPU: the numbers behind plotQualityProfile (R/plot-methods.R:163-243, on ShortRead qa()'s
perCycle$quality) and plotComplexity (:293-299), and seqComplexity with a sliding window (R/filter.R:1248-1275).

Only data is produced; nothing is drawn.  The entry points live in this module, and ``dada2_amd.api`` neither imports nor
re-exports them: ``tests/filter_cases.py`` pins that ``dada2_amd.api`` has no ``plot_complexity`` and that
``api.seq_complexity(..., window=...)`` raises.

Deviations from the reference, both stated in DESIGN §8h: where the reference profiles a uniform random sample of ``n`` reads,
``n=None`` profiles every read and a given ``n`` the FIRST ``n`` records (the whole file is still counted for ``rc``); a
directory is refused."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import _lib

_EB = 2048
NSCORE = _lib.QPROFILE_NSCORE
_KMER_WINDOW = "The window over which kmer frequency is calculated must be larger than the kmerSize."   # R/filter.R:1249


def _blob(strings):
    bs = [s if isinstance(s, bytes) else str(s).encode("latin-1") for s in strings]
    off = np.zeros(len(bs) + 1, dtype=np.int64)
    if bs:
        np.cumsum([len(b) for b in bs], out=off[1:])
    return b"".join(bs), off


def _stats_dict(st):
    return {k: int(st[i]) for i, k in enumerate(_lib.READQC_STATS)}


def quality_table(quals, device=0, stats: dict = None):
    """dada2hip_qprofile_reads on quality strings in memory: an (ncycle, 94) int64 array, ncycle the longest string, column =
    letter - 33 ('!' .. '~').  A letter outside that range is refused, and the message names the read."""
    qb, off = _blob([quals] if isinstance(quals, (str, bytes)) else quals)
    n = len(off) - 1
    ncycle = int(np.diff(off).max()) if n else 0
    counts = np.zeros((ncycle, NSCORE), dtype=np.int64)
    st = np.zeros(_lib.READQC_NSTATS, dtype=np.int64)
    eb = C.create_string_buffer(_EB)
    rv = _lib.lib().dada2hip_qprofile_reads(n, qb, off.ctypes.data, int(device), ncycle, counts.ctypes.data, st.ctypes.data, eb, _EB)
    if stats is not None:
        stats.update(_stats_dict(st))
    _lib.check(rv, eb)
    return counts


def quality_table_fastq(fn, n=None, quality_type=0, chunk_reads=0, device=0, stats: dict = None):
    """dada2hip_qprofile_fastq on one file (plain or gzip): a dict with ``counts`` (ncycle, 94; column = letter - 33), ``rc`` (the
    records of the file), ``profiled`` (the first ``n`` of them, all for ``n=None``) and ``qual_offset`` (33 or 64; ``quality_type``
    0 is Auto: any letter below ';' in the first chunk means 33)."""
    h = C.c_void_p()
    st = np.zeros(_lib.READQC_NSTATS, dtype=np.int64)
    eb = C.create_string_buffer(_EB)
    L = _lib.lib()
    rv = L.dada2hip_qprofile_fastq(os.fspath(fn).encode(), int(chunk_reads), 0 if n is None else max(int(n), 0), int(quality_type), int(device),
                                   C.byref(h), st.ctypes.data, eb, _EB)
    _lib.check(rv, eb)
    try:
        ncycle = L.dada2hip_qprofile_ncycle(h)
        counts = np.ctypeslib.as_array(L.dada2hip_qprofile_counts(h), shape=(ncycle, NSCORE)).copy() if ncycle else np.zeros((0, NSCORE), np.int64)
        out = {"counts": counts, "rc": int(L.dada2hip_qprofile_reads_total(h)), "profiled": int(L.dada2hip_qprofile_profiled(h)),
               "qual_offset": int(L.dada2hip_qprofile_qual_offset(h))}
    finally:
        L.dada2hip_qprofile_free(h)
    if stats is not None:
        stats.update(_stats_dict(st))
    return out


def long_table(by_score, score0):
    """The rows of qa()'s perCycle$quality with Count > 0, ordered by cycle, then by ascending score: ``by_score`` is (ncycle,
    nscore), its column j the score ``score0 + j``."""
    cyc, col = np.nonzero(by_score)                               # (row-major: by cycle, then by column)
    return {"cycle": (cyc + 1).astype(np.int64), "score": (col + score0).astype(np.int64), "count": by_score[cyc, col].astype(np.int64)}


def cycle_stats(by_score, score0, denom):
    """The statistics frame of R/plot-methods.R:178-192 for one count table: per cycle the mean score, get_quant's Q25 / Q50 / Q75
    (:179: the first score, ascending, at which cumsum(count) / sum(count) >= q, in double as R divides) and Cum = 10 * sum(count)
    / denom (:192).  Cycles without a count have no row."""
    tot = by_score.sum(axis=1)
    rows = np.flatnonzero(tot > 0)
    t, tf = by_score[rows], tot[rows].astype(np.float64)
    scores = np.arange(by_score.shape[1], dtype=np.int64) + score0
    out = {"Cycle": (rows + 1).astype(np.int64), "Mean": (t * scores).sum(axis=1).astype(np.float64) / tf}   # (integer sums: exact)
    frac = np.cumsum(t, axis=1).astype(np.float64) / tf[:, None]
    for name, q in (("Q25", 0.25), ("Q50", 0.5), ("Q75", 0.75)):
        out[name] = scores[np.argmax(frac >= q, axis=1)].astype(np.float64) if len(rows) else np.zeros(0)
    out["Cum"] = 10.0 * tf / float(denom) if denom else np.full(len(rows), np.nan)
    return out


def quality_profile(fl, n=None, aggregate=False, quality_type=0, device=0):
    """The data of plotQualityProfile(fl, n, aggregate).  Returns a dict: ``files``, one entry per file with ``file`` (its
    basename), ``table`` (the long table ``cycle`` / ``score`` / ``count``), ``stats`` (``Cycle``, ``Mean``, ``Q25``, ``Q50``,
    ``Q75``, ``Cum``), ``rc``, ``profiled``, ``qual_offset`` and ``minScore``; ``minScore``, the minimum over all files (:195);
    and ``aggregate``: None, or with ``aggregate=True`` the ``table`` and ``stats`` of the count tables summed over the files,
    with Cum over sum(min(rc, n)) (:198-205), and ``rc``, the total."""
    fl = [os.fspath(fl)] if (isinstance(fl, (str, bytes)) or hasattr(fl, "__fspath__")) else [os.fspath(f) for f in fl if f is not None]
    for f in fl:
        if os.path.isdir(f):
            raise ValueError("A directory is not profiled; name its files: " + str(f))
    cap = float("inf") if n is None else int(n)
    files = []
    for f in fl:
        got = quality_table_fastq(f, n=n, quality_type=quality_type, device=device)
        score0 = 33 - got["qual_offset"]                            # the score of column 0
        e = {"file": os.path.basename(f), "rc": got["rc"], "profiled": got["profiled"], "qual_offset": got["qual_offset"],
             "table": long_table(got["counts"], score0), "stats": cycle_stats(got["counts"], score0, min(got["rc"], cap)),
             "_counts": got["counts"], "_score0": score0}
        files.append(e)
    mins = [int(e["table"]["score"].min()) for e in files if len(e["table"]["score"])]
    min_score = min(mins) if mins else None
    agg = None
    if aggregate and files:
        lo = min(e["_score0"] for e in files)
        ncyc = max(e["_counts"].shape[0] for e in files)
        width = max(e["_score0"] - lo + NSCORE for e in files)
        total = np.zeros((ncyc, width), dtype=np.int64)
        for e in files:
            c = e["_counts"]
            total[:c.shape[0], e["_score0"] - lo:e["_score0"] - lo + NSCORE] += c
        agg = {"table": long_table(total, lo), "stats": cycle_stats(total, lo, sum(min(e["rc"], cap) for e in files)),
               "rc": sum(e["rc"] for e in files)}
    for e in files:
        e["minScore"] = min_score
        del e["_counts"], e["_score0"]
    return {"files": files, "minScore": min_score, "aggregate": agg}


def seq_complexity(seqs, kmer_size=2, window=None, by=5, device=0, stats: dict = None):
    """seqComplexity(seqs, kmerSize, window, by) (R/filter.R:1248-1268).  ``window=None`` is ``api.seq_complexity``, its bits.
    With a window the R loop is restated with its quirks: the starts run to max(width) - window over the sequences of THIS call,
    so a sequence of the maximal length never has its last window tested and one shorter than the window keeps 4^k; a tested
    window without a countable k-mer makes the value NaN."""
    seqs = [seqs] if isinstance(seqs, (str, bytes)) else list(seqs)
    seqs = [s.decode("latin-1") if isinstance(s, bytes) else str(s) for s in seqs]
    if window is None:
        from . import api
        return api.seq_complexity(seqs, kmer_size=kmer_size, device=device)
    if int(window) < 1:                                             # (0 is the C interface's window = NULL)
        raise ValueError(_KMER_WINDOW)
    sb, off = _blob(seqs)
    n = len(off) - 1
    out = np.zeros(n, dtype=np.float64)
    st = np.zeros(_lib.READQC_NSTATS, dtype=np.int64)
    eb = C.create_string_buffer(_EB)
    rv = _lib.lib().dada2hip_complexity_reads(n, sb, off.ctypes.data, int(kmer_size), int(window), int(by), int(device), out.ctypes.data,
                                              st.ctypes.data, eb, _EB)
    if stats is not None:
        stats.update(_stats_dict(st))
    _lib.check(rv, eb)
    return out


def complexity_fastq(fn, kmer_size=2, window=None, by=5, n=100000, chunk_reads=0, device=0, stats: dict = None):
    """dada2hip_complexity_fastq: seqComplexity of the first ``n`` records of one file (None: all), as a float64 array."""
    if window is not None and int(window) < 1:
        raise ValueError(_KMER_WINDOW)
    p, cnt = C.c_void_p(), C.c_int64()
    st = np.zeros(_lib.READQC_NSTATS, dtype=np.int64)
    eb = C.create_string_buffer(_EB)
    L = _lib.lib()
    rv = L.dada2hip_complexity_fastq(os.fspath(fn).encode(), int(chunk_reads), 0 if n is None else max(int(n), 0), int(kmer_size),
                                     0 if window is None else int(window), int(by), int(device), C.byref(p), C.byref(cnt), st.ctypes.data, eb, _EB)
    _lib.check(rv, eb)
    try:
        out = np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_double)), shape=(cnt.value,)).copy() if cnt.value else np.zeros(0)
    finally:
        L.dada2hip_complexity_free(p)
    if stats is not None:
        stats.update(_stats_dict(st))
    return out


def complexity_profile(fl, kmer_size=2, window=None, by=5, n=100000, device=0):
    """The data frame plotComplexity hands to ggplot (:300-301): ``complexity`` (float64) and ``file`` (the basename, once per
    value), over the first ``n`` records of every file.  No binning."""
    fl = [os.fspath(fl)] if (isinstance(fl, (str, bytes)) or hasattr(fl, "__fspath__")) else [os.fspath(f) for f in fl]
    for f in fl:
        if os.path.isdir(f):
            raise ValueError("A directory is not profiled; name its files: " + str(f))
    vals = [complexity_fastq(f, kmer_size, window, by, n, device=device) for f in fl]
    return {"complexity": np.concatenate(vals) if vals else np.zeros(0),
            "file": [os.path.basename(f) for f, v in zip(fl, vals) for _ in range(len(v))]}
