"""filterAndTrim with orient.fwd, matchIDs, id.sep and id.field (R/filter.R:648-658, :940-1007).

``dada2_amd.api``'s filter functions refuse these four arguments, and ``tests/filter_cases.py`` pins that they do.  The functions
here take every argument ``api``'s take, plus ``orient_fwd``, ``match_ids``, ``id_sep`` and ``id_field``; called without the new
ones they ARE ``api``'s (the same entry points, the same files).  ``dada2_amd.api`` neither imports nor re-exports this module.

orient_fwd, single-end: per chunk of ``n`` records, the reads that start with it are kept as given, those whose reverse complement
does (and who do not themselves) are reverse-complemented - before every stage, so the truncQ cut, the expected errors, the phiX
screen and the complexity are those of the flipped read - and written BEHIND the chunk's as-given reads; the rest is dropped (code
12, "orient").  The output order depends on ``n``, as the reference's does.  Paired: no reverse complement; a pair whose reverse
read starts with it (and whose forward read does not) is swapped, each read judged by and written to the other direction.
match_ids (paired only; ignored single-end, as in the reference): pairs are matched by the id field of their header lines, the
unmatched tail of each chunk carried into the next.

Departures from the reference, both documented in DESIGN.md: an empty ``orient_fwd`` is a ValueError (the reference would keep
every read), and duplicate ids that leave the two kept lists of a chunk unequal are an error (the reference goes on into
recycled indexing)."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import _lib, api

_EB = 2048
STAGES = _lib.FILTER_STAGES + ("orient",)   # a read's code indexes this: 12 is "in neither orientation"
# the int64 words of the stats of the entries below: _lib.FILTER_STATS and, from word 26 on, these
ORIENT_STATS = ("dropped_orient", "flipped", "dropped_ids", "orient_device_us", "id_join_us")
STATS = _lib.FILTER_STATS + ORIENT_STATS
ORIENT_MAX = 256                            # letters of orient_fwd (FT_ORIENT_MAX)
_NEW = ("orient_fwd", "match_ids", "id_sep", "id_field")
_REGEX_META = set(".\\|()[]{}^$*+?")


def _stats_out(stats, st):
    if stats is not None:
        stats.update({k: int(st[i]) for i, k in enumerate(STATS)})


def check_orient_fwd(orient_fwd):
    """None, or the barcode as bytes: non-empty upper-case A/C/G/T (R/filter.R:650), at most ORIENT_MAX letters."""
    if orient_fwd is None:
        return None
    b = str(orient_fwd)
    if b == "":
        raise ValueError("orient_fwd is empty (the reference would keep every read; pass None for no orientation).")
    if any(c not in "ACGT" for c in b):
        raise ValueError("Non-ACGT characters detected in orient.fwd")
    if len(b) > ORIENT_MAX:
        raise NotImplementedError(f"orient_fwd longer than {ORIENT_MAX} letters is not supported by this library.")
    return b.encode()


def check_id_args(id_sep, id_field):
    """(id_sep as the library takes it, id_field with 0 for "detect")."""
    sep = "\\s" if id_sep is None else str(id_sep)
    if sep != "\\s" and (len(sep) != 1 or sep in _REGEX_META):
        raise NotImplementedError("id_sep other than \"\\\\s\" or one literal character that is no regex metacharacter is not supported by "
                                  "this library.")
    if id_field is None:
        return sep.encode(), 0
    if int(id_field) != id_field or int(id_field) < 1:
        raise ValueError("id_field must be a positive integer (1-based), or None to detect it.")
    return sep.encode(), int(id_field)


def filter_reads(seqs, quals, ctx: api.FilterContext, params=None, *, orient_fwd=None, paired=False, kmers=False, stats: dict = None,
                 **kw):
    """api.filter_reads with ``orient_fwd``: dada2hip_filter_reads_oriented on reads in memory, results in INPUT order.  Beside
    api.filter_reads' arrays, ``orient``: 0 the read starts with orient_fwd, 1 only its reverse complement does (every other array
    is then the flipped read's, ``window[:, 0]`` counting from the read's end), 2 neither (code 12).  ``paired``: the forward test
    alone (orient 0 or 2, code 0 or 12), nothing else judged."""
    bar = check_orient_fwd(orient_fwd)
    if bar is None:
        if paired:
            raise ValueError("paired needs orient_fwd.")
        return api.filter_reads(seqs, quals, ctx, params, kmers=kmers, stats=stats, **kw)
    p = params if params is not None else api.filter_params(**kw)
    sb, off = api._blob(seqs)
    qb, qoff = api._blob(quals)
    if not np.array_equal(off, qoff):
        raise ValueError("Every read needs as many quality characters as bases.")
    n = len(off) - 1
    k = p.kmer_size or 2
    kmers = kmers and not paired
    out = {"code": np.zeros(n, dtype=np.int32), "window": np.zeros((n, 2), dtype=np.int32), "ee": np.zeros(n, dtype=np.float64),
           "hits": np.zeros((n, 2), dtype=np.int32), "orient": np.zeros(n, dtype=np.int8)}
    if kmers:
        out["kmer_counts"] = np.zeros((n, 4 ** k), dtype=np.int32)
        out["complexity"] = np.zeros(n, dtype=np.float64)
    st = np.zeros(_lib.FILTER_NSTATS, dtype=np.int64)
    eb = C.create_string_buffer(_EB)
    rv = _lib.lib().dada2hip_filter_reads_oriented(ctx._h, n, sb, qb, off.ctypes.data, C.byref(p), bar, int(bool(paired)),
                                                   out["code"].ctypes.data, out["window"].ctypes.data, out["ee"].ctypes.data,
                                                   out["hits"].ctypes.data, out["kmer_counts"].ctypes.data if kmers else None,
                                                   out["complexity"].ctypes.data if kmers else None, out["orient"].ctypes.data,
                                                   st.ctypes.data, eb, _EB)
    _lib.check(rv, eb)
    _stats_out(stats, st)
    return out


def _split_new(kw):
    new = {k: kw.pop(k, None) for k in _NEW}
    return new, not (new["orient_fwd"] is None and not new["match_ids"])


def fastq_filter(fn, fout, *, compress=True, n=10**6, quality_type=0, verbose=False, rm_phix=False, ctx: api.FilterContext = None,
                 device: int = 0, stats: dict = None, min_matches=2, non_overlapping=True, kmer_size=0, **kw):
    """fastqFilter (R/filter.R:613-730) with ``orient_fwd``: (reads_in, reads_out).  ``match_ids``, ``id_sep`` and ``id_field``
    are accepted and ignored, as the reference ignores them for single-end files."""
    new, _ = _split_new(kw)
    bar = check_orient_fwd(new["orient_fwd"])
    common = dict(compress=compress, n=n, quality_type=quality_type, verbose=verbose, rm_phix=rm_phix, ctx=ctx, device=device, stats=stats,
                  min_matches=min_matches, non_overlapping=non_overlapping, kmer_size=kmer_size)
    if bar is None:
        return api.fastq_filter(fn, fout, **common, **kw)
    for k_, v in kw.items():
        if k_ not in api._FILTER_DEFAULTS:
            raise TypeError(f"unexpected argument {k_!r}")
        if isinstance(v, (list, tuple, np.ndarray)) and len(v) > 1:
            raise ValueError("Filtering and trimming arguments should be of length 1 when processing single-end (rather than paired-end) data.")
    c, own = api._filter_ctx(rm_phix, ctx, device)
    try:
        p = api.filter_params(rm_phix=bool(rm_phix), min_matches=min_matches, non_overlapping=non_overlapping, kmer_size=kmer_size,
                              quality_type=quality_type, **kw)
        rin, rout = C.c_int64(), C.c_int64()
        st = np.zeros(_lib.FILTER_NSTATS, dtype=np.int64)
        eb = C.create_string_buffer(_EB)
        _lib.check(_lib.lib().dada2hip_filter_fastq_oriented(c._h, os.fspath(fn).encode(), os.fspath(fout).encode(), C.byref(p), bar,
                                                             int(bool(compress)), int(n), C.byref(rin), C.byref(rout), st.ctypes.data, eb,
                                                             _EB), eb)
    finally:
        if own:
            c.close()
    _stats_out(stats, st)
    if verbose:
        print(f"Read in {rin.value}, output {rout.value} ({round(rout.value * 100 / max(rin.value, 1), 1)}%) filtered sequences.")
        if rout.value == 0:
            print(f"The filter removed all reads: {fout} not written.")
    return rin.value, rout.value


def fastq_paired_filter(fn, fout, *, compress=True, n=10**6, quality_type=0, verbose=False, rm_phix=False,
                        ctx: api.FilterContext = None, device: int = 0, stats: dict = None, min_matches=2, non_overlapping=True,
                        kmer_size=0, **kw):
    """fastqPairedFilter (R/filter.R:878-1140) with ``orient_fwd``, ``match_ids``, ``id_sep`` ("\\\\s" or one literal character)
    and ``id_field`` (1-based; None: detected from the first forward id)."""
    new, used = _split_new(kw)
    bar = check_orient_fwd(new["orient_fwd"])
    common = dict(compress=compress, n=n, quality_type=quality_type, verbose=verbose, rm_phix=rm_phix, ctx=ctx, device=device, stats=stats,
                  min_matches=min_matches, non_overlapping=non_overlapping, kmer_size=kmer_size)
    if not used:
        return api.fastq_paired_filter(fn, fout, **common, **kw)
    sep, field = check_id_args(new["id_sep"], new["id_field"]) if new["match_ids"] else (None, 0)
    if isinstance(fn, str) or len(fn) != 2:
        raise ValueError("Two paired input file names required.")
    if isinstance(fout, str) or len(fout) != 2:
        raise ValueError("Two paired output file names required.")
    for k_ in kw:
        if k_ not in api._FILTER_DEFAULTS:
            raise TypeError(f"unexpected argument {k_!r}")
    c, own = api._filter_ctx(rm_phix, ctx, device)
    try:
        ps = [api.filter_params(w, rm_phix=bool(rm_phix), min_matches=min_matches, non_overlapping=non_overlapping, kmer_size=kmer_size,
                                quality_type=quality_type, **kw) for w in (0, 1)]
        rin, rout = C.c_int64(), C.c_int64()
        st = np.zeros(_lib.FILTER_NSTATS, dtype=np.int64)
        eb = C.create_string_buffer(_EB)
        _lib.check(_lib.lib().dada2hip_filter_fastq_paired_ex(c._h, os.fspath(fn[0]).encode(), os.fspath(fn[1]).encode(),
                                                              os.fspath(fout[0]).encode(), os.fspath(fout[1]).encode(), C.byref(ps[0]),
                                                              C.byref(ps[1]), bar, int(bool(new["match_ids"])), sep, field,
                                                              int(bool(compress)), int(n), C.byref(rin), C.byref(rout), st.ctypes.data, eb,
                                                              _EB), eb)
    finally:
        if own:
            c.close()
    _stats_out(stats, st)
    if verbose:
        print(f"Read in {rin.value} paired-sequences, output {rout.value} ({round(rout.value * 100 / max(rin.value, 1), 1)}%) filtered paired-sequences.")
    return rin.value, rout.value


def filter_and_trim(fwd, filt, rev=None, filt_rev=None, *, orient_fwd=None, match_ids=False, id_sep=None, id_field=None, **kw):
    """filterAndTrim (R/filter.R:402-497) with the four arguments; everything else is api.filter_and_trim's, which does the path
    checks, the output directories and the reads.in / reads.out matrix, with this module's per-file functions underneath."""
    bar = check_orient_fwd(orient_fwd)
    if bar is None and not (match_ids and rev is not None):
        return api.filter_and_trim(fwd, filt, rev, filt_rev, **kw)
    if match_ids and rev is not None:
        check_id_args(id_sep, id_field)
    new = dict(orient_fwd=orient_fwd, match_ids=match_ids, id_sep=id_sep, id_field=id_field)
    per_file = (lambda *a, **k: fastq_filter(*a, **k, **new), lambda *a, **k: fastq_paired_filter(*a, **k, **new))
    return api.filter_and_trim(fwd, filt, rev, filt_rev, _per_file=per_file, **kw)
