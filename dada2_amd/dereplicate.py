"""derepFastq on the device (R/sequenceIO.R:45-183): reads in memory, or the reads filterAndTrim keeps, to a derep object.

``derep_reads`` dereplicates reads that are in memory; ``filter_and_derep`` filters a sample's file (or pair of files) and
dereplicates what passes in the same pass - the reads are on the device for the filter anyway, so with ``filt=None`` no file is
written, deflated, inflated or parsed a second time.  Both return ``api.NativeDerep`` objects, which ``Sample.from_native``,
``api.combine_dereps``, ``api.dada`` and ``api.merge_pairs`` take as they are, and which equal ``api.derep_fastq`` of the same
reads (of the filtered file) field for field.  ``dada2_amd.api`` neither imports nor re-exports this module.

``filter_and_derep`` takes ``api.filter_and_trim``'s arguments and gives its warnings; ``orient_fwd`` and ``match_ids`` are
refused - they stay with ``dada2_amd.filtering``, unfused.

The resident forms - ``derep_reads_resident``, ``filter_and_sample`` - end where ``dada()`` starts: they return ``ResidentDerep``
objects, each with the resident ``Sample`` that ``Sample.from_native`` would have made of it.  The dereplicator's quality sums
never leave the device: one kernel rounds them into the sample's quality bytes where they lie (byte for byte the rows of the
host route).  A ``ResidentDerep`` therefore has no quality matrix - sequences, abundances, map and ``qmax()`` are all
``dada()``, ``paired.merge_pairs`` and ``learn_errors`` read; ``to_derep``, ``Sample.from_native``, ``api.combine_dereps`` and
``dada(pool=True)`` refuse it and say why.  ``dada`` here is ``api.dada`` on the samples the dereps came with."""
from __future__ import annotations

import ctypes as C
import os
import warnings

import numpy as np

from . import _lib, api

_EB = 2048
STATS = _lib.DEREP_STATS                                  # the int64 words of dada2hip_derep_reads' stats
FUSED_STATS = _lib.FILTER_STATS + ("",) * (_lib.FILTER_NSTATS - len(_lib.FILTER_STATS)) + tuple("derep_" + k for k in STATS)
RESIDENT_STATS = _lib.RESIDENT_STATS                     # the int64 words of the resident entries' resident_stats
NO_MATRIX = ("a ResidentDerep has no quality matrix: its qualities were rounded on the device, into the sample it came with "
             "(.sample); filter_and_derep / derep_reads are the routes that keep the matrix.")


class ResidentDerep(api.NativeDerep):
    """The derep object of a resident entry: an ``api.NativeDerep`` without a quality matrix, and ``.sample``, the resident
    ``api.Sample`` of its uniques (rows byte for byte those of ``Sample.from_native`` on the full object).  ``qmax()`` is the
    word the device stored: the largest ``ceil(mean)`` it met while rounding."""

    def __init__(self, *a, **k):
        raise TypeError("ResidentDerep objects come from derep_reads_resident and filter_and_sample.")

    @classmethod
    def _from_handles(cls, h, hs, device):
        self = cls._from_handle(h)
        smp = api.Sample.__new__(api.Sample)
        smp._h, smp.nraw, smp.device = hs, self.nuniques, device
        self.sample = smp
        return self

    def to_derep(self):
        raise ValueError(NO_MATRIX)

    def close(self):
        smp = getattr(self, "sample", None)
        if smp is not None:
            smp.close()
        super().close()


def _resident_stats_out(stats, rs, prefixes):
    if stats is not None:
        for j, pre in enumerate(prefixes):
            stats.update({pre + k: int(rs[j * _lib.RESIDENT_NSTATS + i]) for i, k in enumerate(RESIDENT_STATS)})


def _bytes(strs):
    bs = [s if isinstance(s, bytes) else str(s).encode("latin-1") for s in strs]
    off = np.zeros(len(bs) + 1, dtype=np.int64)
    if bs:
        np.cumsum([len(b) for b in bs], out=off[1:])
    return b"".join(bs), off


def derep_reads(seqs, quals, n: int = 10**6, qual_offset: int = 0, device: int = 0, stats: dict = None) -> api.NativeDerep:
    """dada2hip_derep_reads: ``seqs`` and ``quals`` (the quality strings as in a FASTQ file) in chunks of ``n`` -> NativeDerep."""
    sb, off = _bytes(seqs)
    qb, qoff = _bytes(quals)
    if not np.array_equal(off, qoff):
        raise ValueError("Every read needs as many quality characters as bases.")
    h = C.c_void_p()
    st = np.zeros(_lib.DEREP_NSTATS, dtype=np.int64)
    eb = C.create_string_buffer(_EB)
    _lib.check(_lib.lib().dada2hip_derep_reads(len(off) - 1, sb, qb, off.ctypes.data, int(n), int(qual_offset), int(device), C.byref(h),
                                               st.ctypes.data, eb, _EB), eb)
    if stats is not None:
        stats.update({k: int(st[i]) for i, k in enumerate(STATS)})
    return api.NativeDerep._from_handle(h)


def derep_reads_resident(seqs, quals, n: int = 10**6, qual_offset: int = 0, device: int = 0, stats: dict = None) -> ResidentDerep:
    """dada2hip_derep_reads_resident: ``derep_reads``' arguments -> ResidentDerep (with ``.sample``).  ``stats`` gets
    ``derep_reads``' words and, as ``resident_<word>``, RESIDENT_STATS.  An input error of the sample (a letter outside A/C/G/T, a
    read of at most five bases, a mean quality that is no byte) fails the call - there is no derep object to look at."""
    sb, off = _bytes(seqs)
    qb, qoff = _bytes(quals)
    if not np.array_equal(off, qoff):
        raise ValueError("Every read needs as many quality characters as bases.")
    h, hs = C.c_void_p(), C.c_void_p()
    st = np.zeros(_lib.DEREP_NSTATS, dtype=np.int64)
    rs = np.zeros(_lib.RESIDENT_NSTATS, dtype=np.int64)
    eb = C.create_string_buffer(_EB)
    _lib.check(_lib.lib().dada2hip_derep_reads_resident(len(off) - 1, sb, qb, off.ctypes.data, int(n), int(qual_offset), int(device), C.byref(h),
                                                        C.byref(hs), st.ctypes.data, rs.ctypes.data, eb, _EB), eb)
    if stats is not None:
        stats.update({k: int(st[i]) for i, k in enumerate(STATS)})
    _resident_stats_out(stats, rs, ("resident_",))
    return ResidentDerep._from_handles(h, hs, int(device))


def _stats_out(stats, st):
    if stats is not None:
        stats.update({k: int(st[i]) for i, k in enumerate(FUSED_STATS) if k})


def _fused_single(found, n_derep, derep_qual_offset, resident=False):
    def run(fn, fout, *, compress=True, n=10**6, quality_type=0, verbose=False, rm_phix=False, ctx=None, device=0, stats=None,
            min_matches=2, non_overlapping=True, kmer_size=0, **kw):
        for k, v in kw.items():
            if k not in api._FILTER_DEFAULTS:
                raise TypeError(f"unexpected argument {k!r}")
            if isinstance(v, (list, tuple, np.ndarray)) and len(v) > 1:
                raise ValueError("Filtering and trimming arguments should be of length 1 when processing single-end (rather than paired-end) data.")
        c, own = api._filter_ctx(rm_phix, ctx, device)
        try:
            p = api.filter_params(rm_phix=bool(rm_phix), min_matches=min_matches, non_overlapping=non_overlapping, kmer_size=kmer_size,
                                  quality_type=quality_type, **kw)
            rin, rout, h, hs = C.c_int64(), C.c_int64(), C.c_void_p(), C.c_void_p()
            st = np.zeros(_lib.FILTER_NSTATS + _lib.DEREP_NSTATS, dtype=np.int64)
            rs = np.zeros(_lib.RESIDENT_NSTATS, dtype=np.int64)
            eb = C.create_string_buffer(_EB)
            fin, fo = os.fspath(fn).encode(), None if fout is None else os.fspath(fout).encode()
            if resident:
                _lib.check(_lib.lib().dada2hip_filter_derep_fastq_resident(c._h, fin, fo, C.byref(p), int(bool(compress)), int(n), int(n_derep),
                                                                           int(derep_qual_offset), C.byref(h), C.byref(hs), C.byref(rin),
                                                                           C.byref(rout), st.ctypes.data, rs.ctypes.data, eb, _EB), eb)
            else:
                _lib.check(_lib.lib().dada2hip_filter_derep_fastq(c._h, fin, fo, C.byref(p), int(bool(compress)), int(n), int(n_derep),
                                                                  int(derep_qual_offset), C.byref(h), C.byref(rin), C.byref(rout), st.ctypes.data,
                                                                  eb, _EB), eb)
            dev = c.device
        finally:
            if own:
                c.close()
        _stats_out(stats, st)
        if resident:
            _resident_stats_out(stats, rs, ("resident_",))
            found.append(ResidentDerep._from_handles(h, hs, dev) if h else None)
        else:
            found.append(api.NativeDerep._from_handle(h) if h else None)
        if verbose:
            print(f"Read in {rin.value}, output {rout.value} ({round(rout.value * 100 / max(rin.value, 1), 1)}%) filtered sequences.")
        return rin.value, rout.value
    return run


def _fused_pair(found, n_derep, derep_qual_offset, resident=False):
    def run(fn, fout, *, compress=True, n=10**6, quality_type=0, verbose=False, rm_phix=False, ctx=None, device=0, stats=None,
            min_matches=2, non_overlapping=True, kmer_size=0, **kw):
        if isinstance(fn, str) or len(fn) != 2:
            raise ValueError("Two paired input file names required.")
        if fout is not None and (isinstance(fout, str) or len(fout) != 2):
            raise ValueError("Two paired output file names required.")
        for k in kw:
            if k not in api._FILTER_DEFAULTS:
                raise TypeError(f"unexpected argument {k!r}")
        c, own = api._filter_ctx(rm_phix, ctx, device)
        try:
            ps = [api.filter_params(w, rm_phix=bool(rm_phix), min_matches=min_matches, non_overlapping=non_overlapping, kmer_size=kmer_size,
                                    quality_type=quality_type, **kw) for w in (0, 1)]
            rin, rout, hf, hr, sf, sr = C.c_int64(), C.c_int64(), C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
            st = np.zeros(_lib.FILTER_NSTATS + _lib.DEREP_NSTATS, dtype=np.int64)
            rs = np.zeros(2 * _lib.RESIDENT_NSTATS, dtype=np.int64)
            eb = C.create_string_buffer(_EB)
            outs = (None, None) if fout is None else tuple(os.fspath(f).encode() for f in fout)
            if resident:
                _lib.check(_lib.lib().dada2hip_filter_derep_fastq_paired_resident(
                    c._h, os.fspath(fn[0]).encode(), os.fspath(fn[1]).encode(), outs[0], outs[1], C.byref(ps[0]), C.byref(ps[1]), int(bool(compress)),
                    int(n), int(n_derep), int(derep_qual_offset), C.byref(hf), C.byref(hr), C.byref(sf), C.byref(sr), C.byref(rin), C.byref(rout),
                    st.ctypes.data, rs.ctypes.data, eb, _EB), eb)
            else:
                _lib.check(_lib.lib().dada2hip_filter_derep_fastq_paired(c._h, os.fspath(fn[0]).encode(), os.fspath(fn[1]).encode(), outs[0], outs[1],
                                                                         C.byref(ps[0]), C.byref(ps[1]), int(bool(compress)), int(n), int(n_derep),
                                                                         int(derep_qual_offset), C.byref(hf), C.byref(hr), C.byref(rin),
                                                                         C.byref(rout), st.ctypes.data, eb, _EB), eb)
            dev = c.device
        finally:
            if own:
                c.close()
        _stats_out(stats, st)
        if resident:
            _resident_stats_out(stats, rs, ("resident_", "resident_rev_"))
            found.append((ResidentDerep._from_handles(hf, sf, dev), ResidentDerep._from_handles(hr, sr, dev)) if hf and hr else None)
        else:
            found.append((api.NativeDerep._from_handle(hf), api.NativeDerep._from_handle(hr)) if hf and hr else None)
        if verbose:
            print(f"Read in {rin.value} paired-sequences, output {rout.value} ({round(rout.value * 100 / max(rin.value, 1), 1)}%) filtered paired-sequences.")
        return rin.value, rout.value
    return run


def filter_and_derep(fwd, filt=None, rev=None, filt_rev=None, *, n_derep: int = 10**6, derep_qual_offset: int = 0, stats: dict = None,
                     **filter_args):
    """filterAndTrim and derepFastq of ONE sample in one pass: ``(counts, NativeDerep | None)``, for a pair
    ``(counts, (NativeDerepF, NativeDerepR) | None)``; ``counts`` is (reads_in, reads_out).  ``filt`` (and ``filt_rev``) None: no
    filtered file is written; otherwise the files are api.filter_and_trim's byte for byte.  The derep objects are what
    api.derep_fastq(filt, n_derep, derep_qual_offset) gives for those files.  None when no read passes (with filterAndTrim's warning).
    ``filter_args``: api.filter_and_trim's (trunc_len, max_ee, ..., n, compress, rm_phix, ctx, device, verbose)."""
    return _filter_and("filter_and_derep", False, fwd, filt, rev, filt_rev, n_derep, derep_qual_offset, stats, filter_args)


def filter_and_sample(fwd, filt=None, rev=None, filt_rev=None, *, n_derep: int = 10**6, derep_qual_offset: int = 0, stats: dict = None,
                      **filter_args):
    """``filter_and_derep`` with the resident end: ``(counts, ResidentDerep | None)``, for a pair ``(counts, (ResidentDerepF,
    ResidentDerepR) | None)`` - every object with its resident ``.sample``, ready for ``dada``.  The arguments, the refusals, the
    files written and the warning are ``filter_and_derep``'s; ``stats`` also gets RESIDENT_STATS as ``resident_<word>`` (the reverse
    sample's as ``resident_rev_<word>``).  An input error of a sample (an N that ``max_n`` let through, a read of at most five bases)
    fails the call and leaves no file."""
    return _filter_and("filter_and_sample", True, fwd, filt, rev, filt_rev, n_derep, derep_qual_offset, stats, filter_args)


def _filter_and(name, resident, fwd, filt, rev, filt_rev, n_derep, derep_qual_offset, stats, filter_args):
    for k in ("orient_fwd", "match_ids"):
        v = filter_args.get(k)
        if v is not None and v is not False:
            raise NotImplementedError(f"{k} is not supported by {name}: filter with dada2_amd.filtering, then dereplicate the file.")
    if not (isinstance(fwd, (str, bytes)) or hasattr(fwd, "__fspath__")):
        raise ValueError(f"{name} takes one sample: one forward file (and one reverse file).")
    if rev is not None and not (isinstance(rev, (str, bytes)) or hasattr(rev, "__fspath__")):
        raise ValueError(f"{name} takes one sample: one forward file (and one reverse file).")
    paired = rev is not None
    if paired and (filt is None) != (filt_rev is None):
        raise ValueError("Output files for both directions, or for neither.")
    found = []
    per_file = (_fused_single(found, n_derep, derep_qual_offset, resident), _fused_pair(found, n_derep, derep_qual_offset, resident))
    if filt is not None:
        args = dict(filter_args)
        st = {}
        counts, _ = api.filter_and_trim(fwd, filt, rev, filt_rev, _per_file=(lambda *a, **k: per_file[0](*a, stats=st, **k),
                                                                                lambda *a, **k: per_file[1](*a, stats=st, **k)), **args)
        if stats is not None:
            stats.update(st)
        return (int(counts[0, 0]), int(counts[0, 1])), found[0]
    # no output files: api.filter_and_trim's checks of the inputs, its arguments and its warning, without its output paths
    args = dict(filter_args)
    api._refuse_filter_args({k: args.pop(k) for k in list(args) if k in api._FILTER_REFUSED})
    if not os.path.exists(os.fspath(fwd)):
        raise ValueError("Some input files do not exist.")
    if paired and not os.path.exists(os.fspath(rev)):
        raise ValueError("Some input files (rev) do not exist.")
    n = args.pop("n", 10**5)
    if paired:
        rin, rout = per_file[1]((fwd, rev), None, n=n, stats=stats, **args)
    else:
        rin, rout = per_file[0](fwd, None, n=n, stats=stats, **args)
    if rout == 0:
        warnings.warn("No reads passed the filter. Please revisit your filtering parameters.")
    return (rin, rout), found[0]


def dada(dereps, err, **kw):
    """``api.dada(dereps, err, samples=[d.sample ...], **kw)`` for ``ResidentDerep`` objects: the samples they came with are run as
    they lie (and stay open - they are the dereps').  ``pool="pseudo"`` works, the samples stay separate; ``pool=True`` needs the
    combined quality matrix and is refused with the combine's message."""
    single = isinstance(dereps, api.NativeDerep)
    ds = [dereps] if single else list(dereps)
    if not ds or not all(isinstance(d, ResidentDerep) for d in ds):
        raise ValueError("dereplicate.dada takes ResidentDerep objects (derep_reads_resident, filter_and_sample); api.dada takes the others.")
    if "samples" in kw:
        raise ValueError("dereplicate.dada runs the samples its dereps came with: samples= does not apply.")
    pool = kw.get("pool", False)
    if isinstance(pool, (bool, np.bool_)) and bool(pool) and len(ds) > 1:
        api._combine_native(ds)[0].close()                          # (raises: the combine says what is missing)
        raise ValueError(NO_MATRIX)
    return api.dada(dereps, err, samples=[d.sample for d in ds], **kw)
