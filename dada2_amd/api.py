"""Host-side mirror of the reference's operator interface for the hot path, over the C ABI.

* ``dada_uniques(...)``  — the ``.Call`` of R/RcppExports.R:8-10 (src/Rmain.cpp:30): same
  argument meaning, same six outputs, errors raised with the reference's messages.
* ``Sample``             — the same call split into "make the uniques resident in HBM" and
  "run with this error matrix", which is what the selfConsist loop of R/dada.R:256-405 needs.
* ``nwalign`` / ``nwvec`` — R/misc.R:179 ``nwalign()`` -> C_nwalign / C_nwvec; ``nweval`` / ``nwhamming`` (R/misc.R:216-225).
* ``make_sequence_table`` / ``collapse_no_mismatch`` — R/multiSample.R:31-55, :104-160.
* ``dada(...)``          — the per-sample loop + selfConsist loop of R/dada.R:144-487, reduced
  to what the hot path needs (single process; ``dada2_amd.multi`` shards samples over GPUs).

R is not installed in this image, so this Python layer stands where R/dada.R
stands; INTEGRATION.md shows the Rcpp stub that binds the same C ABI from R.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from .io import Derep, extend_err
from .opts import COpts, DadaOpts, DadaResult, NA_INTEGER

_EB = 2048


class HostInput:
    """Host-side inputs of one ``dada_uniques`` call laid out as the C ABI takes them — what R already holds in its
    own vectors when it issues the ``.Call``: ``char**`` strings, int32 abundances, uint8 priors and the column-major
    ``maxlen x nraw`` double quality matrix (here: row-major [nraw, maxlen], the same bytes).  Built once; timing a
    call on a ``HostInput`` measures the boundary call itself, not Python's marshalling."""

    def __init__(self, seqs, abundances, priors, quals):
        n = len(seqs)
        self.n = n
        if n and isinstance(seqs[0], bytes):
            parts = seqs
        else:
            parts = [s.encode("ascii") for s in seqs]
        self._blob = b"\0".join(parts) + b"\0"
        lens = np.fromiter((len(x) for x in parts), dtype=np.int64, count=n)
        off = np.zeros(n, dtype=np.int64)
        if n > 1:
            np.cumsum(lens[:-1] + 1, out=off[1:])
        base = np.frombuffer(self._blob, dtype=np.uint8).ctypes.data
        self._ptrs = (off + base).astype(np.uint64)             # const char *const *
        self.seqs_p = self._ptrs.ctypes.data if n else None
        self.ab = np.ascontiguousarray(abundances, dtype=np.int32)
        self.pr = None if priors is None else np.ascontiguousarray(priors, dtype=np.uint8)
        self.q = None if quals is None else np.ascontiguousarray(quals, dtype=np.float64)
        if self.q is not None and self.q.ndim == 2 and self.q.shape[0] != n:
            raise ValueError("derep$quals matrices must have one row for each derep$unique sequence.")
        self.qn = 0 if self.q is None else self.q.shape[1]

    @classmethod
    def from_derep(cls, d: Derep, priors=None):
        return cls(d.seqs, d.abundances, priors, d.quals)

    @property
    def nbytes(self):
        return len(self._blob) + self.ab.nbytes + (0 if self.q is None else self.q.nbytes) + 8 * self.n


def _pack(seqs, abundances, priors, quals):
    h = seqs if isinstance(seqs, HostInput) else HostInput(seqs, abundances, priors, quals)
    return h


def _err_colmajor(err):
    e = np.asarray(err, dtype=np.float64)
    if e.ndim != 2 or e.shape[0] != 16:
        raise _lib.Dada2HipError(1, "Error matrix must have 16 rows.")
    return np.ascontiguousarray(e.T), e.shape[1]


def _collect(L, h) -> DadaResult:
    Cn = L.dada2hip_result_nclust(h)
    N = L.dada2hip_result_nraw(h)
    ml = L.dada2hip_result_maxlen(h)
    nc = L.dada2hip_result_ncol(h)
    nb = L.dada2hip_result_nbirth_subs(h)

    def arr(name, n, dt):
        if n == 0:
            return np.zeros(0, dtype=dt)
        return np.ctypeslib.as_array(getattr(L, "dada2hip_result_" + name)(h), shape=(n,)).astype(dt, copy=True)

    clustering = {
        "sequence": [L.dada2hip_result_sequence(h, i).decode() for i in range(Cn)],
        "abundance": arr("abundance", Cn, np.int32), "n0": arr("n0", Cn, np.int32), "n1": arr("n1", Cn, np.int32),
        "nunq": arr("nunq", Cn, np.int32), "pval": arr("clust_pval", Cn, np.float64),
        "birth_from": arr("birth_from", Cn, np.int32), "birth_pval": arr("birth_pval", Cn, np.float64),
        "birth_fold": arr("birth_fold", Cn, np.float64), "birth_ham": arr("birth_ham", Cn, np.int32),
        "birth_qave": arr("birth_qave", Cn, np.float64),
    }
    ref = L.dada2hip_result_bs_ref(h)
    sub = L.dada2hip_result_bs_sub(h)
    birth_subs = {
        # (one block copy + one decode each: a per-element ctypes read cost 10 ms of the boundary call at 10^4 substitutions)
        "pos": arr("bs_pos", nb, np.int32), "ref": list(C.string_at(ref, nb).decode("ascii")) if nb else [],
        "sub": list(C.string_at(sub, nb).decode("ascii")) if nb else [], "qual": arr("bs_qual", nb, np.float64),
        "clust": arr("bs_clust", nb, np.int32),
    }
    subqual = arr("subqual", 16 * nc, np.int32).reshape(nc, 16).T.copy()
    cq = arr("clusterquals", ml * Cn, np.float64).reshape(Cn, ml).T.copy()
    st = _lib.CStats()
    L.dada2hip_result_stats(h, C.byref(st))
    stats = st.as_dict()
    stats["center"] = arr("center", Cn, np.int32)
    return DadaResult(clustering, birth_subs, subqual, cq, arr("map", N, np.int32), arr("pval", N, np.float64), stats)


def _copts(opts, max_clust, multithread, verbose, copts):
    if copts is not None:
        return copts
    return (opts or DadaOpts()).to_c(max_clust=max_clust, multithread=multithread, verbose=verbose)


def dada_uniques(seqs, abundances, priors, err, quals, opts: DadaOpts = None, *, max_clust=None, multithread=False,
                 verbose=False, copts: COpts = None, device: int = 0, log=None, should_abort=None) -> DadaResult:
    """One ``dada_uniques`` call (src/Rmain.cpp:30) on the GPU.  ``quals`` is the derep-side
    [N, maxlen] matrix (NaN past a short read's end); ``err`` is 16 x Q.  ``log(str)`` receives the ``verbose`` lines
    (Rprintf, src/Rmain.cpp:317-333), ``should_abort()`` is polled once per divisive round (Rcpp::checkUserInterrupt,
    src/Rmain.cpp:330): a true value ends the call with ``Dada2HipError(code=5)``."""
    L = _lib.lib()
    co = _copts(opts, max_clust, multithread, verbose, copts)
    hooks, keep = _lib.make_hooks(log, should_abort)
    hi = _pack(seqs, abundances, priors, quals)
    e, ncol = _err_colmajor(err)
    eb = C.create_string_buffer(_EB)
    h = C.c_void_p()
    rc = L.dada2hip_dada_uniques(hi.n, hi.seqs_p, hi.ab.ctypes.data, hi.pr.ctypes.data if hi.pr is not None else None,
                                 e.ctypes.data, ncol, hi.q.ctypes.data if hi.q is not None else None, hi.qn, C.byref(co),
                                 device, C.byref(hooks) if hooks is not None else None, C.byref(h), eb, _EB)
    if keep and keep["error"] is not None:
        if rc == 0:
            L.dada2hip_result_free(h)
        raise keep["error"]
    _lib.check(rc, eb)
    try:
        return _collect(L, h)
    finally:
        L.dada2hip_result_free(h)


def dada_uniques_multi(inputs, err, opts: DadaOpts = None, *, devices=(0,), copts: COpts = None):
    """``dada2hip_run_multi``: the per-sample loop of R/dada.R:266 over the GPUs of the node, one host thread per entry
    of ``devices`` inside the library.  ``inputs``: list of HostInput (or Derep).  Returns list[DadaResult]."""
    L = _lib.lib()
    co = _copts(opts, None, False, False, copts)
    his = [x if isinstance(x, HostInput) else HostInput.from_derep(x) for x in inputs]
    n = len(his)
    arr = (_lib.CSampleInput * max(n, 1))()
    for i, hi in enumerate(his):
        arr[i].nraw = hi.n
        arr[i].quals_nrow = hi.qn
        arr[i].seqs = C.cast(C.c_void_p(hi.seqs_p), C.POINTER(C.c_char_p))
        arr[i].abundances = hi.ab.ctypes.data
        arr[i].priors = hi.pr.ctypes.data if hi.pr is not None else None
        arr[i].quals = hi.q.ctypes.data if hi.q is not None else None
    e, ncol = _err_colmajor(err)
    devs = np.ascontiguousarray(devices, dtype=np.int32)
    outs = (C.c_void_p * max(n, 1))()
    eb = C.create_string_buffer(_EB)
    rc = L.dada2hip_run_multi(n, arr, e.ctypes.data, ncol, C.byref(co), devs.size, devs.ctypes.data, outs, eb, _EB)
    _lib.check(rc, eb)
    res = []
    try:
        for i in range(n):
            res.append(_collect(L, C.c_void_p(outs[i])))
    finally:
        for i in range(n):
            if outs[i]:
                L.dada2hip_result_free(C.c_void_p(outs[i]))
    return res


class NativeDerep:
    """derepFastq through the library's host-side dereplicator (dada2hip_derep_fastq; R/sequenceIO.R:45-124): the object
    stays in the library's memory; ``to_derep`` copies it into the numpy ``Derep`` mirror, ``Sample.from_native`` uploads it
    as a resident sample without a Python-side copy."""

    def __init__(self, path: str, n: int = 10**6, qual_offset: int = 0):
        L = _lib.lib()
        eb = C.create_string_buffer(_EB)
        self._h = C.c_void_p()
        _lib.check(L.dada2hip_derep_fastq(str(path).encode(), int(n), int(qual_offset), C.byref(self._h), eb, _EB), eb)
        self.nuniques = L.dada2hip_derep_nuniques(self._h)
        self.nreads = L.dada2hip_derep_nreads(self._h)
        self.maxlen = L.dada2hip_derep_maxlen(self._h)

    def to_derep(self) -> Derep:
        L = _lib.lib()
        n, ml = self.nuniques, self.maxlen
        sp = L.dada2hip_derep_seqs(self._h)
        seqs = [sp[i].decode("ascii") for i in range(n)]
        ab = np.ctypeslib.as_array(L.dada2hip_derep_abundances(self._h), (n,)).copy()
        q = np.ctypeslib.as_array(L.dada2hip_derep_quals(self._h), (n, ml)).copy()
        mp = np.ctypeslib.as_array(L.dada2hip_derep_map(self._h), (self.nreads,)).copy() if self.nreads else np.zeros(0, np.int32)
        mp[mp == np.iinfo(np.int32).min] = -1
        return Derep(seqs, ab, q, mp)

    @classmethod
    def _from_handle(cls, h):
        """A dada2hip_derep the library handed out (dada2hip_derep_combine)."""
        L = _lib.lib()
        self = cls.__new__(cls)
        self._h = h
        self.nuniques = L.dada2hip_derep_nuniques(h)
        self.nreads = L.dada2hip_derep_nreads(h)
        self.maxlen = L.dada2hip_derep_maxlen(h)
        return self

    def qmax(self) -> int:
        """``ceiling(max(derep$quals, na.rm=TRUE))`` (R/dada.R:290): dada2hip_derep_qmax, over the library's matrix in place - or,
        for an object without a matrix (dada2_amd.dereplicate.ResidentDerep), the word the device stored.  (In the library, not
        ``np.nanmax``: the matrix's NA is R's NA_real_, a signalling NaN, which numpy's vectorised fmax does not always skip.)"""
        return int(_lib.lib().dada2hip_derep_qmax(self._h))

    def close(self):
        if getattr(self, "_h", None):
            _lib.lib().dada2hip_derep_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _StrArray:
    """``const char *const *`` over one NUL-separated blob (HostInput's layout)."""

    def __init__(self, seqs):
        parts = [s if isinstance(s, bytes) else str(s).encode("ascii") for s in seqs]
        n = len(parts)
        self.n = n
        self._blob = b"\0".join(parts) + b"\0"
        lens = np.fromiter((len(x) for x in parts), dtype=np.int64, count=n)
        off = np.zeros(n, dtype=np.int64)
        if n > 1:
            np.cumsum(lens[:-1] + 1, out=off[1:])
        self._ptrs = (off + np.frombuffer(self._blob, dtype=np.uint8).ctypes.data).astype(np.uint64)
        self.p = self._ptrs.ctypes.data if n else None


def _derep_view(d, keep):
    """The dada2hip_derep_view of a Derep or a NativeDerep; what it points to is appended to ``keep``."""
    L = _lib.lib()
    v = _lib.CDerepView()
    if isinstance(d, NativeDerep):
        v.nuniques, v.maxlen, v.nreads = d.nuniques, d.maxlen, d.nreads
        v.seqs = C.cast(L.dada2hip_derep_seqs(d._h), C.c_void_p)
        v.abundances = C.cast(L.dada2hip_derep_abundances(d._h), C.c_void_p)
        v.quals = C.cast(L.dada2hip_derep_quals(d._h), C.c_void_p)
        v.map = C.cast(L.dada2hip_derep_map(d._h), C.c_void_p) if d.nreads else None
        keep.append(d)
        return v
    if not isinstance(d, Derep):
        raise ValueError("Requires derep-class objects.")
    sa = _StrArray(d.seqs)
    ab = np.ascontiguousarray(d.abundances, dtype=np.int32)
    q = np.ascontiguousarray(d.quals, dtype=np.float64)
    if q.ndim != 2 or q.shape[0] != sa.n or ab.shape != (sa.n,):
        raise ValueError("derep$quals matrices must have one row for each derep$unique sequence.")
    mp = np.array(d.map, dtype=np.int32, copy=True).ravel()
    mp[mp < 0] = NA_INTEGER                                     # the numpy Derep's -1 (and the library's NA) both mean NA
    keep.extend((sa, ab, q, mp))
    v.nuniques, v.maxlen, v.nreads = sa.n, q.shape[1], mp.size
    v.seqs, v.abundances, v.quals = sa.p, ab.ctypes.data, q.ctypes.data
    v.map = mp.ctypes.data if mp.size else None
    return v


def _combine_native(dereps):
    """dada2hip_derep_combine -> (NativeDerep of the pooled object, [unique_to_pool per sample])."""
    dereps = list(dereps)
    if not dereps:
        raise ValueError("Requires derep-class objects.")
    keep = []
    views = (_lib.CDerepView * len(dereps))(*[_derep_view(d, keep) for d in dereps])
    sizes = [int(v.nuniques) for v in views]
    u2p = np.zeros(max(sum(sizes), 1), dtype=np.int32)
    h = C.c_void_p()
    eb = C.create_string_buffer(_EB)
    _lib.check(_lib.lib().dada2hip_derep_combine(len(dereps), views, C.byref(h), u2p.ctypes.data, eb, _EB), eb)
    cuts = np.cumsum([0] + sizes)
    return NativeDerep._from_handle(h), [u2p[cuts[i]:cuts[i + 1]].copy() for i in range(len(sizes))]


def combine_dereps(dereps):
    """combineDereps2 (R/multiSample.R:165-203) through dada2hip_derep_combine: ``(Derep, [unique_to_pool per sample])``.  The pooled
    uniques are the union of the samples' in order of first appearance, stably ordered by decreasing summed abundance; a quality is
    the abundance-weighted mean of the samples' (NaN past a unique's length and past a narrower sample's width); the map is the
    samples' maps one after the other, renumbered (-1 = NA, as in every numpy ``Derep``).  ``unique_to_pool[i][j]`` is the 0-based
    pooled row of unique j of sample i.  ``dereps``: ``Derep`` and ``NativeDerep`` objects, mixed as they come."""
    nd, u2p = _combine_native(dereps)
    try:
        return nd.to_derep(), u2p
    finally:
        nd.close()


def derep_fastq(path: str, n: int = 10**6, qual_offset: int = 0) -> Derep:
    """derepFastq(fl, n) (R/sequenceIO.R:45) -> Derep, through dada2hip_derep_fastq."""
    nd = NativeDerep(path, n, qual_offset)
    try:
        return nd.to_derep()
    finally:
        nd.close()


class Sample:
    """Uniques of one sample resident in HBM (dada2hip_sample_*): 2-bit reads, rounded
    qualities and k-mer records are uploaded/built once and reused by every ``run``."""

    def __init__(self, seqs, abundances, priors, quals, device: int = 0):
        L = _lib.lib()
        hi = _pack(seqs, abundances, priors, quals)
        eb = C.create_string_buffer(_EB)
        self._h = C.c_void_p()
        rc = L.dada2hip_sample_create(hi.n, hi.seqs_p, hi.ab.ctypes.data, hi.pr.ctypes.data if hi.pr is not None else None,
                                      hi.q.ctypes.data if hi.q is not None else None, hi.qn, device, C.byref(self._h), eb, _EB)
        _lib.check(rc, eb)
        self.nraw = hi.n
        self.device = device

    @classmethod
    def from_derep(cls, d: Derep, priors=None, device: int = 0):
        return cls(d.seqs, d.abundances, priors, d.quals, device)

    @classmethod
    def from_native(cls, nd: "NativeDerep", priors=None, device: int = 0):
        """dada2hip_sample_from_derep: the library's derep object -> resident sample, no host copy in between."""
        self = cls.__new__(cls)
        eb = C.create_string_buffer(_EB)
        self._h = C.c_void_p()
        pr = None if priors is None else np.ascontiguousarray(priors, dtype=np.uint8)
        rc = _lib.lib().dada2hip_sample_from_derep(nd._h, pr.ctypes.data if pr is not None else None, device, C.byref(self._h), eb, _EB)
        _lib.check(rc, eb)
        self.nraw = nd.nuniques
        self.device = device
        return self

    def rows(self) -> dict:
        """dada2hip_sample_rows: the resident rows as they lie on the device, padding included - ``seq2`` (n, W2) uint32, ``len``,
        ``reads``, ``qual`` (n, LQ) uint8 - and the geometry words (_lib.SAMPLE_ROWS_GEOM)."""
        L = _lib.lib()
        eb = C.create_string_buffer(_EB)
        g = np.zeros(_lib.SAMPLE_ROWS_NGEOM, dtype=np.int32)
        _lib.check(L.dada2hip_sample_rows(self._h, g.ctypes.data, None, None, None, None, eb, _EB), eb)
        out = {k: int(g[i]) for i, k in enumerate(_lib.SAMPLE_ROWS_GEOM)}
        n = out["n"]
        out.update(seq2=np.zeros((n, out["W2"]), dtype=np.uint32), len=np.zeros(n, dtype=np.int32), reads=np.zeros(n, dtype=np.uint32),
                   qual=np.zeros((n, out["LQ"]), dtype=np.uint8))
        _lib.check(L.dada2hip_sample_rows(self._h, None, out["seq2"].ctypes.data, out["len"].ctypes.data, out["reads"].ctypes.data,
                                          out["qual"].ctypes.data, eb, _EB), eb)
        return out

    def set_priors(self, priors):
        eb = C.create_string_buffer(_EB)
        pr = np.ascontiguousarray(priors, dtype=np.uint8)
        _lib.check(_lib.lib().dada2hip_sample_set_priors(self._h, pr.ctypes.data, eb, _EB), eb)

    def set_prior_seqs(self, seqs, or_flags=None, want_match=False):
        """dada2hip_sample_set_prior_seqs: flag the resident uniques whose sequence is one of ``seqs`` (``names(uniques) %in% seqs``,
        R/dada.R:335; matched on the device), OR-ed with the per-unique ``or_flags`` where given.  Entries with a letter outside
        A/C/G/T match nothing; duplicates are allowed.  Returns the number of flags set, or with ``want_match``
        ``(nset, first_match)``: per unique the smallest index into ``seqs`` of an equal entry, -1 for none."""
        sa = _StrArray(seqs)
        orf = None
        if or_flags is not None:
            orf = np.ascontiguousarray(np.asarray(or_flags) != 0, dtype=np.uint8)
            if orf.shape != (self.nraw,):
                raise ValueError("or_flags must have one entry per unique.")
        fm = np.full(self.nraw, -1, dtype=np.int32) if want_match else None
        nset = C.c_int32(0)
        eb = C.create_string_buffer(_EB)
        _lib.check(_lib.lib().dada2hip_sample_set_prior_seqs(self._h, sa.n, sa.p, orf.ctypes.data if orf is not None else None,
                                                             fm.ctypes.data if fm is not None else None, C.byref(nset), eb, _EB), eb)
        return (int(nset.value), fm) if want_match else int(nset.value)

    def prior_seqs_stats(self) -> dict:
        """The words of this sample's last ``set_prior_seqs`` call (_lib.PRIOR_SEQS_STATS)."""
        st = np.zeros(_lib.PRIOR_SEQS_NSTATS, dtype=np.int64)
        _lib.lib().dada2hip_sample_prior_seqs_stats(self._h, st.ctypes.data)
        return {k: int(st[i]) for i, k in enumerate(_lib.PRIOR_SEQS_STATS)}

    def run(self, err, opts: DadaOpts = None, *, max_clust=None, multithread=False, verbose=False,
            copts: COpts = None, log=None, should_abort=None) -> DadaResult:
        L = _lib.lib()
        co = _copts(opts, max_clust, multithread, verbose, copts)
        e, ncol = _err_colmajor(err)
        eb = C.create_string_buffer(_EB)
        h = C.c_void_p()
        hooks, keep = _lib.make_hooks(log, should_abort)
        rc = L.dada2hip_sample_run(self._h, e.ctypes.data, ncol, C.byref(co), C.byref(hooks) if hooks is not None else None,
                                   C.byref(h), eb, _EB)
        if keep and keep["error"] is not None:
            if rc == 0:
                L.dada2hip_result_free(h)
            raise keep["error"]
        _lib.check(rc, eb)
        try:
            return _collect(L, h)
        finally:
            L.dada2hip_result_free(h)

    def run_sharded(self, err, opts: DadaOpts, rank: int, world: int, exchange, *, max_clust=None, copts: COpts = None) -> DadaResult:
        """``dada2hip_sample_run_sharded``: this process does the per-unique work of block ``rank`` of ``world``.  ``exchange(kind,
        send: bytes-like memoryview, recv: writable memoryview)`` is the collective of include/dada2hip.h's dada2hip_shard
        (kind 0 = all-gather of equal-size payloads in rank order, kind 1 = in-place all-reduce(sum) of int64);
        ``dada2_amd.shard`` provides it over torch.distributed.  Every rank gets the complete result."""
        L = _lib.lib()
        co = _copts(opts, max_clust, False, False, copts)
        e, ncol = _err_colmajor(err)
        failure = []

        def _cb(user, kind, send, nbytes, recv):
            try:
                n = int(nbytes)
                sv = (C.c_char * n).from_address(send) if n else (C.c_char * 0)()
                rv = (C.c_char * (n * world if kind == 0 else n)).from_address(recv) if n else (C.c_char * 0)()
                exchange(int(kind), memoryview(sv).cast("B"), memoryview(rv).cast("B"))
                return 0
            except BaseException as ex:   # never unwind through the C frames
                failure.append(ex)
                return 1
        cb = _lib.EXCHANGE_FN(_cb)
        sh = _lib.CShard(int(rank), int(world), cb, None)
        eb = C.create_string_buffer(_EB)
        h = C.c_void_p()
        rc = L.dada2hip_sample_run_sharded(self._h, e.ctypes.data, ncol, C.byref(co), None, C.byref(sh), C.byref(h), eb, _EB)
        if failure:
            raise failure[0]
        _lib.check(rc, eb)
        try:
            return _collect(L, h)
        finally:
            L.dada2hip_result_free(h)

    def compare(self, centre: int, err, opts: DadaOpts = None, kdist_cutoff=None, skip=None):
        """One b_compare round (cluster.cpp:90-149): (lambda[N], hamming[N], cls[N], stats)."""
        L = _lib.lib()
        o = opts or DadaOpts()
        co = o.to_c()
        e, ncol = _err_colmajor(err)
        lam = np.zeros(self.nraw)
        ham = np.zeros(self.nraw, dtype=np.uint32)
        cls = np.zeros(self.nraw, dtype=np.uint8)
        sk = None if skip is None else np.ascontiguousarray(skip, dtype=np.uint8)
        st = _lib.CStats()
        eb = C.create_string_buffer(_EB)
        rc = L.dada2hip_sample_compare(self._h, int(centre), e.ctypes.data, ncol, C.byref(co),
                                       float(o.KDIST_CUTOFF if kdist_cutoff is None else kdist_cutoff),
                                       sk.ctypes.data if sk is not None else None, lam.ctypes.data, ham.ctypes.data,
                                       cls.ctypes.data, C.byref(st), eb, _EB)
        _lib.check(rc, eb)
        return lam, ham, cls, st.as_dict()

    def close(self):
        if getattr(self, "_h", None):
            _lib.lib().dada2hip_sample_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def nwvec(s1, s2, match=5, mismatch=-4, gap=-8, band=-1, endsfree=True, device: int = 0):
    """C_nwvec (src/nwalign_vectorized.cpp:321): list of (al0, al1) for the pairs."""
    L = _lib.lib()
    n = len(s1)
    if n != len(s2):
        raise ValueError("Character vectors to be aligned must be of equal length.")
    a = (C.c_char_p * n)(*[x.encode() for x in s1])
    b = (C.c_char_p * n)(*[x.encode() for x in s2])
    bufs = [C.create_string_buffer(len(s1[i // 2]) + len(s2[i // 2]) + 2) for i in range(2 * n)]
    out = (C.c_char_p * (2 * n))(*[C.cast(x, C.c_char_p) for x in bufs])
    eb = C.create_string_buffer(_EB)
    _lib.check(L.dada2hip_nwvec(n, a, b, match, mismatch, gap, band, int(endsfree), device, out, eb, _EB), eb)
    return [(bufs[2 * i].value.decode(), bufs[2 * i + 1].value.decode()) for i in range(n)]


def nwalign(s1, s2, match=5, mismatch=-4, gap=-8, homo_gap=None, band=-1, endsfree=True, device: int = 0):
    """R/misc.R:179 nwalign(): one pair, returns (al0, al1)."""
    L = _lib.lib()
    o0 = C.create_string_buffer(len(s1) + len(s2) + 2)
    o1 = C.create_string_buffer(len(s1) + len(s2) + 2)
    eb = C.create_string_buffer(_EB)
    rc = L.dada2hip_nwalign(s1.encode(), s2.encode(), match, mismatch, gap, gap if homo_gap is None else homo_gap, band,
                            int(endsfree), device, o0, o1, eb, _EB)
    _lib.check(rc, eb)
    return o0.value.decode(), o1.value.decode()


def table_bimera2(mat, seqs, min_fold=1.5, min_abund=2, allow_one_off=False, min_one_off_par_dist=4, match=5, mismatch=-4,
                  gap_p=-8, max_shift=16, device: int = 0):
    """C_table_bimera2 (src/chimera.cpp:192; called by isBimeraDenovoTable, R/chimeras.R:236): ``mat`` is the
    [samples, sequences] count table; returns (nflag[nseq], nsam[nseq])."""
    L = _lib.lib()
    m = np.asfortranarray(np.asarray(mat, dtype=np.int32))
    nrow, ncol = m.shape
    if ncol != len(seqs):
        raise ValueError("The sequence table must have one column per sequence.")
    arr = (C.c_char_p * max(ncol, 1))(*[s.encode("ascii") for s in seqs])
    nflag, nsam = np.zeros(ncol, dtype=np.int32), np.zeros(ncol, dtype=np.int32)
    eb = C.create_string_buffer(_EB)
    _lib.check(L.dada2hip_table_bimera2(nrow, ncol, m.ctypes.data, arr, float(min_fold), int(min_abund), int(allow_one_off),
                                        int(min_one_off_par_dist), match, mismatch, gap_p, int(max_shift), device,
                                        nflag.ctypes.data, nsam.ctypes.data, eb, _EB), eb)
    return nflag, nsam


def is_bimera(sq, parents, allow_one_off=False, min_one_off_par_dist=4, match=5, mismatch=-4, gap_p=-8, max_shift=16, device: int = 0):
    """C_is_bimera (src/chimera.cpp:18; R/chimeras.R:43 isBimera)."""
    L = _lib.lib()
    arr = (C.c_char_p * max(len(parents), 1))(*[s.encode("ascii") for s in parents])
    out = C.c_int32(0)
    eb = C.create_string_buffer(_EB)
    _lib.check(L.dada2hip_is_bimera(sq.encode("ascii"), len(parents), arr, int(allow_one_off), int(min_one_off_par_dist), match,
                                    mismatch, gap_p, int(max_shift), device, C.byref(out), eb, _EB), eb)
    return bool(out.value)


def bimera_pairs(queries, parents, allow_one_off=False, match=5, mismatch=-4, gap_p=-8, max_shift=16, device: int = 0):
    """get_lr / get_ham_endsfree (src/chimera.cpp:211-293) of each (query, parent) alignment: int32 [n, 5] =
    left, right, left_oo, right_oo, hamming - what C_is_bimera / C_table_bimera2 reduce to a flag."""
    L = _lib.lib()
    n = len(queries)
    if n != len(parents):
        raise ValueError("queries and parents must have the same length")
    qa = (C.c_char_p * max(n, 1))(*[s.encode("ascii") for s in queries])
    pa = (C.c_char_p * max(n, 1))(*[s.encode("ascii") for s in parents])
    out = np.zeros((n, 5), dtype=np.int32)
    eb = C.create_string_buffer(_EB)
    _lib.check(L.dada2hip_bimera_pairs(n, qa, pa, int(allow_one_off), match, mismatch, gap_p, int(max_shift), device,
                                       out.ctypes.data, eb, _EB), eb)
    return out


def is_bimera_denovo_table(mat, seqs, min_sample_fraction=0.9, ignore_n_negatives=1, **kw):
    """isBimeraDenovoTable (R/chimeras.R:220-247): the consensus decision over samples on top of C_table_bimera2."""
    nflag, nsam = table_bimera2(mat, seqs, **kw)
    return (nflag >= nsam) | ((nflag > 0) & (nflag >= (nsam - ignore_n_negatives) * min_sample_fraction))


def _is_table(obj):
    """A (mat, seqs) sequence table: a two-dimensional array with its column names."""
    return (isinstance(obj, tuple) and len(obj) == 2 and getattr(obj[0], "ndim", 0) == 2 and not isinstance(obj[1], np.ndarray)
            and len(obj[1]) == obj[0].shape[1] and all(isinstance(s, str) for s in obj[1]))


def _input_uniques(obj, seqs=None):
    """(sequences, abundances) of ``obj`` as given - duplicates kept, input order: what getSequences sees."""
    if seqs is not None:
        obj = (np.asarray(obj), list(seqs))
    if isinstance(obj, DadaResult):
        s, a = obj.clustering["sequence"], obj.clustering["abundance"]
    elif isinstance(obj, Derep):
        s, a = obj.seqs, obj.abundances
    elif isinstance(obj, dict):
        s, a = list(obj.keys()), list(obj.values())
    elif _is_table(obj):
        s, a = obj[1], np.asarray(obj[0]).sum(axis=0, dtype=np.int64)   # as.integer(colSums(object))
    elif isinstance(obj, (tuple, list)) and len(obj) == 2 and not isinstance(obj[0], str) and len(obj[0]) == len(obj[1]):
        s, a = obj
    else:
        raise ValueError("Unrecognized format: Requires a {sequence: abundance} mapping, a (sequences, abundances) pair, a DadaResult, "
                         "a Derep or a (mat, seqs) sequence table.")
    s = [str(x) for x in s]
    a = np.asarray(a, dtype=np.int64).reshape(-1)
    if len(s) != a.size:
        raise ValueError("One abundance per sequence is required.")
    if a.size and (a.max() > np.iinfo(np.int32).max or a.min() < 0):
        raise _lib.Dada2HipError(1, "dada2hip: an abundance is negative or exceeds the integer range.")
    return s, a


def get_uniques(obj, seqs=None):
    """getUniques (R/misc.R:33-62): (sequences, int32 abundances) of a {sequence: abundance} mapping, a (sequences, abundances)
    pair, a DadaResult (its clustering's sequence / abundance), a Derep or a sequence table - ``(mat, seqs)``, or ``mat`` with
    ``seqs=`` - whose abundances are the column sums.  A sequence given more than once is merged and its abundances summed, the
    result then standing in ascending byte order of the sequences, as ``tapply(unqs, names(unqs), sum)`` leaves it (:55)."""
    s, a = _input_uniques(obj, seqs)
    if len(set(s)) == len(s):
        return s, a.astype(np.int32)
    summed = {}
    for x, v in zip(s, a):
        summed[x] = summed.get(x, 0) + int(v)
    keys = sorted(summed, key=lambda x: x.encode("ascii"))
    tot = np.array([summed[k] for k in keys], dtype=np.int64)
    if tot.max() > np.iinfo(np.int32).max:
        raise _lib.Dada2HipError(1, "dada2hip: an abundance is negative or exceeds the integer range.")
    return keys, tot.astype(np.int32)


def bimera_denovo_rows(mat, seqs, min_fold_parent_over_abundance=2, min_parent_abundance=8, allow_one_off=False,
                       min_one_off_parent_distance=4, max_shift=16, match=5, mismatch=-4, gap_p=-8, skip_zero=False, device: int = 0,
                       stats: dict = None):
    """dada2hip_bimera_denovo: isBimeraDenovo (R/chimeras.R:105-154) on every row of the [rows, sequences] table ``mat`` with the
    sequences resident once - bool [rows, sequences].  The sequences must be distinct.  ``skip_zero``: zero cells are FALSE without
    work.  ``stats`` (a dict) receives the library's counters (_lib.BIMERA_DENOVO_STATS)."""
    m = np.asfortranarray(np.asarray(mat, dtype=np.int32))
    if m.ndim != 2 or m.shape[1] != len(seqs):
        raise ValueError("The sequence table must have one column per sequence.")
    nrow, ncol = m.shape
    flags = np.zeros((nrow, ncol), dtype=np.uint8, order="F")
    st = np.zeros(_lib.BIMERA_DENOVO_NSTATS, dtype=np.int64)
    eb = C.create_string_buffer(_EB)
    _lib.check(_lib.lib().dada2hip_bimera_denovo(nrow, ncol, m.ctypes.data, _charpp(list(seqs)), float(min_fold_parent_over_abundance),
                                                 float(min_parent_abundance), int(bool(allow_one_off)), int(min_one_off_parent_distance),
                                                 int(match), int(mismatch), int(gap_p), int(max_shift), int(bool(skip_zero)), device,
                                                 flags.ctypes.data, st.ctypes.data, eb, _EB), eb)
    if stats is not None:
        stats.update({k: int(v) for k, v in zip(_lib.BIMERA_DENOVO_STATS, st)})
    return flags.astype(bool)


def is_bimera_denovo(unqs, min_fold_parent_over_abundance=2, min_parent_abundance=8, allow_one_off=False,
                     min_one_off_parent_distance=4, max_shift=16, match=5, mismatch=-4, gap_p=-8, device: int = 0, stats: dict = None,
                     seqs=None):
    """isBimeraDenovo (R/chimeras.R:105-154): a bool array with one entry per INPUT sequence of ``unqs`` (any form get_uniques
    takes), TRUE where the sequence is a two-parent bimera of sequences more than ``min_fold_parent_over_abundance`` times as
    abundant and more abundant than ``min_parent_abundance``.  A sequence given more than once gets the answer of its merged entry
    (``seqs.input %in% seqs[bims]``, :150)."""
    s_in, _ = _input_uniques(unqs, seqs)
    s, a = get_uniques(unqs, seqs)
    if not s:
        return np.zeros(0, dtype=bool)
    bim = bimera_denovo_rows(a.reshape(1, -1), s, min_fold_parent_over_abundance, min_parent_abundance, allow_one_off,
                             min_one_off_parent_distance, max_shift, match, mismatch, gap_p, False, device, stats)[0]
    if s_in == s:
        return bim
    flagged = {x for x, b in zip(s, bim) if b}
    return np.array([x in flagged for x in s_in], dtype=bool)


def remove_bimera_denovo(unqs, method="consensus", seqs=None, **kw):
    """removeBimeraDenovo (R/chimeras.R:294-346).  A sequence table - ``(mat, seqs)``, or ``mat`` with ``seqs=`` - comes back as
    (mat, seqs): with "pooled" (is_bimera_denovo on the column sums) and "consensus" (is_bimera_denovo_table, whose own defaults
    are 1.5 and 2) without the flagged columns; with "per-sample" every row is run on its own, the flagged cells are zeroed and the
    columns left without a count are dropped (:329-332).  Every other input goes through is_bimera_denovo whatever ``method`` says
    and comes back as (sequences, int32 abundances) in input order without the flagged entries.  ``kw`` goes to the function that
    decides."""
    table = seqs is not None or _is_table(unqs)
    if not table:
        s, a = _input_uniques(unqs)
        keep = ~is_bimera_denovo((s, a), **kw)
        return [x for x, k in zip(s, keep) if k], a[keep].astype(np.int32)
    mat, names = (np.asarray(unqs), list(seqs)) if seqs is not None else (np.asarray(unqs[0]), list(unqs[1]))
    if mat.ndim != 2 or mat.shape[1] != len(names):
        raise ValueError("The sequence table must have one column per sequence.")
    if method == "pooled":
        keep = ~is_bimera_denovo((mat, names), **kw)
    elif method == "consensus":
        keep = ~np.asarray(is_bimera_denovo_table(mat, names, **kw), dtype=bool)
    elif method == "per-sample":
        if len(set(names)) != len(names):
            raise ValueError("Duplicate sequences detected in input.")
        bim = bimera_denovo_rows(mat, names, skip_zero=True, **kw)
        out = np.array(mat, copy=True)
        out[bim] = 0
        keep = out.sum(axis=0, dtype=np.int64) != 0
        return np.ascontiguousarray(out[:, keep]), [x for x, k in zip(names, keep) if k]
    else:
        raise ValueError("Valid values for method: 'pooled', 'consensus', or 'per-sample'")
    return np.ascontiguousarray(mat[:, keep]), [x for x, k in zip(names, keep) if k]


def is_shift_denovo(unqs, min_overlap=20, flag_subseqs=False, device: int = 0, seqs=None):
    """isShiftDenovo (R/chimeras.R:380-399): a bool array with one entry per input sequence, TRUE where the sequence equals a more
    abundant one up to an overall shift - isShiftedPair (:412-417): the unbanded ends-free alignment with the default scores has no
    mismatch and no indel, at least ``min_overlap`` matches, and fewer matches than either sequence is long.  ``flag_subseqs`` is
    accepted and has NO effect, as in the reference: isShiftDenovo never passes it on to isShift (:391), so a strict subsequence is
    FALSE either way.  A pair whose best gapless diagonal cannot be an exact optimal alignment (dada2hip_collapse_pairs: m_max <
    min_overlap or G > match * m_max) is FALSE without an alignment; the others go through dada2hip_nweval."""
    del flag_subseqs
    s_in, _ = _input_uniques(unqs, seqs)
    s, a = get_uniques(unqs, seqs)
    n = len(s)
    order = np.argsort(-a.astype(np.int64), kind="stable")
    ra = a[order]
    npar = np.searchsorted(-ra.astype(np.int64), -a.astype(np.int64), side="left")    # parents of j: abunds > abund_j, ranks [0, npar[j])
    shift = np.zeros(n, dtype=bool)
    CH = 1 << 20
    qi, pi = [], []

    def flush():
        if not qi:
            return
        q = np.concatenate(qi)
        p = np.concatenate(pi)
        qi.clear()
        pi.clear()
        qs, ps = [s[int(k)] for k in q], [s[int(k)] for k in p]
        cp = collapse_pairs(qs, ps, min_overlap=max(int(min_overlap), 1), device=device)
        cand = np.flatnonzero((cp[:, 2] >= min_overlap) & (cp[:, 1] <= 5 * cp[:, 2]))
        if cand.size:
            cq, cpar = [qs[int(k)] for k in cand], [ps[int(k)] for k in cand]
            ev = nweval(cq, cpar, band=-1, device=device).reshape(-1, 3)
            l1 = np.array([len(x) for x in cq])
            l2 = np.array([len(x) for x in cpar])
            ok = (ev[:, 0] < l1) & (ev[:, 0] < l2) & (ev[:, 0] >= min_overlap) & (ev[:, 1] == 0) & (ev[:, 2] == 0)
            shift[q[cand[ok]]] = True

    pending = 0
    for j in range(n):
        k = int(npar[j])
        at = 0
        while at < k:
            take = min(k - at, CH - pending)
            qi.append(np.full(take, j, dtype=np.int64))
            pi.append(order[at:at + take].astype(np.int64))
            at += take
            pending += take
            if pending == CH:
                flush()
                pending = 0
    flush()
    if s_in == s:
        return shift
    flagged = {x for x, b in zip(s, shift) if b}
    return np.array([x in flagged for x in s_in], dtype=bool)


def merge_pairs(dadaF: DadaResult, derepF: Derep, dadaR: DadaResult, derepR: Derep, min_overlap=12, max_mismatch=0,
                return_rejects=False, just_concatenate=False, trim_overhang=False, device: int = 0):
    """mergePairs() for one sample (R/paired.R:92-201) through dada2hip_merge_pairs: a list of dict rows (sequence,
    abundance, forward, reverse, nmatch, nmismatch, nindel, prefer, accept) in the reference's order."""
    L = _lib.lib()
    NA = np.iinfo(np.int32).min
    mF, mR = np.asarray(derepF.map, dtype=np.int64), np.asarray(derepR.map, dtype=np.int64)
    # paired.R:115-119: the maps must be as long as each other and their largest entry (1-based there, 0-based here) must
    # name the LAST unique of the dada-class object - equality, not just "in range"
    def _max_ok(m, n):
        ok = m[m >= 0]
        return ok.size > 0 and int(ok.max()) + 1 == n
    if len(mF) != len(mR) or not _max_ok(mF, len(dadaF.map)) or not _max_ok(mR, len(dadaR.map)):
        raise _lib.Dada2HipError(1, "Non-corresponding derep-class and dada-class objects.")
    def denoised(dmap, rmap):
        dm = np.asarray(dmap, dtype=np.int64)
        out = np.full(len(rmap), NA, dtype=np.int32)
        ok = rmap >= 0
        v = dm[rmap[ok]]
        out[ok] = np.where(v > 0, v, NA)
        return out
    fwd, rev = denoised(dadaF.map, mF), denoised(dadaR.map, mR)
    sF, sR = list(dadaF.clustering["sequence"]), list(dadaR.clustering["sequence"])
    aF = (C.c_char_p * max(1, len(sF)))(*[x.encode() for x in sF])
    aR = (C.c_char_p * max(1, len(sR)))(*[x.encode() for x in sR])
    n0F = np.ascontiguousarray(dadaF.clustering["n0"], dtype=np.int32)
    n0R = np.ascontiguousarray(dadaR.clustering["n0"], dtype=np.int32)
    eb = C.create_string_buffer(_EB)
    h = C.c_void_p()
    _lib.check(L.dada2hip_merge_pairs(len(fwd), fwd.ctypes.data, rev.ctypes.data, len(sF), aF, n0F.ctypes.data, len(sR), aR,
                                      n0R.ctypes.data, int(min_overlap), int(max_mismatch), int(trim_overhang),
                                      int(just_concatenate), device, C.byref(h), eb, _EB), eb)
    try:
        n = L.dada2hip_mergers_nrow(h)
        col = {k: np.ctypeslib.as_array(getattr(L, "dada2hip_mergers_" + k)(h), (n,)).copy() if n else np.zeros(0, np.int32)
               for k in ("abundance", "forward", "reverse", "nmatch", "nmismatch", "nindel", "prefer", "accept")}
        rows = []
        for i in range(n):
            rows.append({"sequence": L.dada2hip_mergers_sequence(h, i).decode("ascii"), "abundance": int(col["abundance"][i]),
                         "forward": int(col["forward"][i]), "reverse": int(col["reverse"][i]), "nmatch": int(col["nmatch"][i]),
                         "nmismatch": int(col["nmismatch"][i]), "nindel": int(col["nindel"][i]),
                         "prefer": None if col["prefer"][i] == NA else int(col["prefer"][i]), "accept": bool(col["accept"][i])})
    finally:
        L.dada2hip_mergers_free(h)
    return rows if return_rejects else [r for r in rows if r["accept"]]


def _charpp(strs):
    return (C.c_char_p * max(len(strs), 1))(*[s.encode("ascii") for s in strs])


def _vectorize(s1, s2):
    """R's Vectorize over the two sequence arguments: scalars are accepted, a scalar is recycled against a list."""
    scalar = isinstance(s1, str) and isinstance(s2, str)
    a = [s1] if isinstance(s1, str) else list(s1)
    b = [s2] if isinstance(s2, str) else list(s2)
    if len(a) != len(b):
        if len(a) == 1:
            a = a * len(b)
        elif len(b) == 1:
            b = b * len(a)
        else:
            raise ValueError("Character vectors to be aligned must be of equal length.")
    return a, b, scalar


def nweval(s1, s2, match=5, mismatch=-4, gap=-8, homo_gap=None, band=-1, endsfree=True, vec=False, device: int = 0):
    """nweval (R/misc.R:222-225): C_eval_pair of nwalign(s1, s2, ...) - int32 [n, 3] = match, mismatch, indel, end gaps not
    counted (one row of three for two scalars).  ``vec`` chooses C_nwvec over C_nwalign as in nwalign (R/misc.R:179)."""
    a, b, scalar = _vectorize(s1, s2)
    n = len(a)
    out = np.zeros((n, 3), dtype=np.int32)
    eb = C.create_string_buffer(_EB)
    _lib.check(_lib.lib().dada2hip_nweval(n, _charpp(a), _charpp(b), match, mismatch, gap, gap if homo_gap is None else homo_gap,
                                          int(band), int(endsfree), int(bool(vec)), device, out.ctypes.data, eb, _EB), eb)
    return out[0] if scalar else out


def nwhamming(s1, s2, **kw):
    """nwhamming (R/misc.R:216-220): mismatches + indels of the alignment, end gaps excluded; an int for two scalars."""
    ev = nweval(s1, s2, **kw)
    return int(ev[1] + ev[2]) if ev.ndim == 1 else (ev[:, 1] + ev[:, 2]).astype(np.int32)


def collapse_pairs(queries, refs, min_overlap=20, match=5, mismatch=-4, device: int = 0):
    """What collapse_no_mismatch's scan kernel computes per (query, ref) pair: int32 [n, 4] = screen (bit 0: the first
    ``min_overlap`` bases of the query occur in the ref, bit 1: the reverse), G (best score of a gapless diagonal), m_max (longest
    diagonal without a mismatch), decision (0 screened out, 1 rejected by G > match * m_max, 2 needs the alignment)."""
    n = len(queries)
    if n != len(refs):
        raise ValueError("queries and refs must have the same length")
    out = np.zeros((n, 4), dtype=np.int32)
    eb = C.create_string_buffer(_EB)
    _lib.check(_lib.lib().dada2hip_collapse_pairs(n, _charpp(queries), _charpp(refs), int(min_overlap), match, mismatch, device,
                                                  out.ctypes.data, eb, _EB), eb)
    return out


def _sample_uniques(sample):
    """getUniques (R/misc.R:33-62) of one sample -> [(sequence, abundance)]: duplicates summed and then, as tapply leaves them,
    in ascending byte order of the sequences (:53-56)."""
    if isinstance(sample, DadaResult):
        pairs = list(zip(sample.clustering["sequence"], sample.clustering["abundance"]))
    elif isinstance(sample, Derep):
        pairs = list(zip(sample.seqs, sample.abundances))
    elif isinstance(sample, dict):
        pairs = list(sample.items())
    elif isinstance(sample, (list, tuple)) and all(isinstance(r, dict) and "sequence" in r and "abundance" in r for r in sample):
        pairs = [(r["sequence"], r["abundance"]) for r in sample if r.get("accept", True)]   # merge_pairs rows: the accepted ones
    else:
        raise ValueError("Unrecognized format: Requires a DadaResult, a Derep, a {sequence: abundance} mapping or merge_pairs rows.")
    pairs = [(str(s), int(a)) for s, a in pairs]
    if len({s for s, _ in pairs}) == len(pairs):
        return pairs
    summed = {}
    for s, a in pairs:
        summed[s] = summed.get(s, 0) + a
    return [(s, summed[s]) for s in sorted(summed, key=lambda x: x.encode("ascii"))]


def _order_columns(mat, order_by):
    """order(colSums(.), decreasing=TRUE) / order(colSums(. > 0), ...) (R/multiSample.R:46-52, :148-154): a stable order."""
    if order_by is None:
        return np.arange(mat.shape[1])
    if order_by == "abundance":
        key = mat.sum(axis=0, dtype=np.int64)
    elif order_by == "nsamples":
        key = (mat > 0).sum(axis=0)
    else:
        raise ValueError('order_by must be "abundance", "nsamples" or None')
    return np.argsort(-key, kind="stable")


def make_sequence_table(samples, order_by="abundance"):
    """makeSequenceTable (R/multiSample.R:31-55): (mat int32 [samples, sequences], seqs).  ``samples``: a list (or one) of
    DadaResult, Derep, {sequence: abundance} mappings or merge_pairs row lists.  Columns in order of first appearance across the
    samples, then stably ordered by ``order_by`` ("abundance", "nsamples" or None)."""
    if isinstance(samples, (DadaResult, Derep, dict)) or (isinstance(samples, list) and samples and isinstance(samples[0], dict)
                                                            and "sequence" in samples[0]):
        samples = [samples]
    if not isinstance(samples, (list, tuple)):
        raise ValueError("Requires a list of samples.")
    unqs = [_sample_uniques(s) for s in samples]
    col = {}
    for u in unqs:
        for s, _ in u:
            col.setdefault(s, len(col))
    mat = np.zeros((len(unqs), len(col)), dtype=np.int64)
    for i, u in enumerate(unqs):
        for s, a in u:
            mat[i, col[s]] = a
    if mat.size and mat.max() > np.iinfo(np.int32).max:
        raise _lib.Dada2HipError(1, "dada2hip: an abundance of the sequence table exceeds the integer range.")
    mat = mat.astype(np.int32)
    seqs = list(col)
    o = _order_columns(mat, order_by)
    return np.ascontiguousarray(mat[:, o]), [seqs[int(k)] for k in o]


def collapse_no_mismatch(mat, seqs, min_overlap=20, order_by="abundance", identical_only=False, vec=True, band=-1, verbose=False,
                         device: int = 0, match=5, mismatch=-4, gap=-8, stats: dict = None):
    """collapseNoMismatch (R/multiSample.R:104-160) through dada2hip_collapse_nomismatch: ``mat`` is the [samples, sequences] table,
    ``seqs`` its column names; returns (mat, seqs) of the collapsed table.  ``vec`` is accepted for signature parity: both values
    run the same device aligner, which follows nwalign_endsfree.  The library decides which column each
    column is added to; the sums, the ``order_by`` ordering and the reference's final, unconditional ordering by total abundance
    (:156, stable - so "nsamples" only breaks abundance ties) are done here.  With ``identical_only`` the de-duplicated table comes
    back in input order (:115).  ``stats`` (a dict) receives the library's counters (_lib.COLLAPSE_STATS)."""
    del vec
    m = np.asarray(mat)
    if m.ndim != 2 or m.shape[1] != len(seqs):
        raise ValueError("The sequence table must have one column per sequence.")
    if m.size and (m.max() > np.iinfo(np.int32).max or m.min() < np.iinfo(np.int32).min):
        raise _lib.Dada2HipError(1, "dada2hip: an abundance of the sequence table exceeds the integer range.")
    mf = np.asfortranarray(m.astype(np.int32))
    nrow, ncol = mf.shape
    into = np.zeros(ncol, dtype=np.int32)
    st = np.zeros(_lib.COLLAPSE_NSTATS, dtype=np.int64)
    eb = C.create_string_buffer(_EB)
    _lib.check(_lib.lib().dada2hip_collapse_nomismatch(nrow, ncol, mf.ctypes.data, _charpp(seqs), int(min_overlap), int(bool(identical_only)),
                                                       int(band), match, mismatch, gap, device, into.ctypes.data, st.ctypes.data, eb, _EB), eb)
    if stats is not None:
        stats.update({k: int(st[i]) for i, k in enumerate(_lib.COLLAPSE_STATS)})
        stats["into"] = into.copy()
    out = np.zeros((nrow, ncol), dtype=np.int64)
    np.add.at(out, (slice(None), into), mf.astype(np.int64))
    kept = np.flatnonzero(into == np.arange(ncol))               # input order, modulo the removed columns (:145)
    out = out[:, kept].astype(np.int32)
    names = [seqs[int(k)] for k in kept]
    if not identical_only:
        for ob in (order_by, "abundance"):
            o = _order_columns(out, ob)
            out, names = out[:, o], [names[int(k)] for k in o]
        if verbose:
            print("Output %d collapsed sequences out of %d input sequences." % (len(names), int(st[0])))
    return np.ascontiguousarray(out), names


# ---- assignTaxonomy (R/taxonomy.R:65-160 on C_assign_taxonomy2, src/taxonomy.cpp) -----------------------------------------------
TAX_LEVELS = ("Kingdom", "Phylum", "Class", "Order", "Family", "Genus", "Species")
_TAX_UNSPECIFIED = "_DADA2_UNSPECIFIED"


def read_fasta(path):
    """(ids, sequences) of a plain or gzip FASTA file, as ShortRead::readFasta gives them: the whole header line behind '>' and
    the record's lines joined, in upper case (a DNAStringSet holds upper case)."""
    import gzip
    with open(path, "rb") as fh:
        magic = fh.read(2)
    opener = gzip.open if magic == b"\x1f\x8b" else open
    ids, seqs, cur = [], [], None
    with opener(path, "rt") as fh:
        for line in fh:
            line = line.rstrip("\r\n")
            if line.startswith(">"):
                if cur is not None:
                    seqs.append("".join(cur))
                ids.append(line[1:])
                cur = []
            elif cur is not None:
                cur.append(line.strip().upper())
    if cur is not None:
        seqs.append("".join(cur))
    return ids, seqs


def _r_strsplit(s, sep=";"):
    """strsplit(s, sep)[[1]]: a trailing empty piece is dropped, and "" gives no piece."""
    parts = s.split(sep)
    if parts and parts[-1] == "":
        parts.pop()
    return parts


def taxonomy_reference(refs, ids):
    """The reference side of assignTaxonomy (R/taxonomy.R:76-122) from sequences and their id lines: references under 20 nt are
    dropped, id whitespace trimmed, UNITE ids rewritten, the format checked, every taxonomy padded with ``_DADA2_UNSPECIFIED;`` to
    the deepest one.  Returns (refs, genus_unq, ref_to_genus, genusmat): the kept references, the distinct taxonomy strings in
    order of first occurrence, the 0-based genus of every kept reference and the int32 [ngenus, depth] level codes (per level the
    distinct names numbered in order of first occurrence: the C code only tests them for equality)."""
    import re
    import warnings
    if len(refs) != len(ids):
        raise ValueError("One taxonomy per reference sequence is required.")
    keep = [i for i, r in enumerate(refs) if len(r) >= 20]                      # MIN_REF_LEN
    if len(keep) < len(refs):
        warnings.warn("Some reference sequences were too short (<20nts) and were excluded.")
    refs = [refs[i] for i in keep]
    tax = [ids[i].strip() for i in keep]
    if not tax:
        raise ValueError("No reference sequences.")
    if len(tax) >= 10 and all(re.search(r"FU\|re[pf]s", t) for t in tax[:10]):  # UNITE
        def unite(t):
            f = t.split("|")
            t = f[4] if len(f) > 4 else ""
            t = re.sub(r"[pcofg]__unidentified;", _TAX_UNSPECIFIED + ";", t)
            t = re.sub(r";s__(\w+)_", ";s__", t, flags=re.ASCII)
            return re.sub(r";s__sp$", ";" + _TAX_UNSPECIFIED, t)
        tax = [unite(t) for t in tax]
    if ";" not in tax[0]:
        if len(tax[0].split()) == 3:
            raise ValueError("Incorrect reference file format for assignTaxonomy (this looks like a file formatted for assignSpecies).")
        raise ValueError("Incorrect reference file format for assignTaxonomy.")
    depth = [len(_r_strsplit(t)) for t in tax]
    td = max(depth)
    tax = [t + (_TAX_UNSPECIFIED + ";") * (td - d) for t, d in zip(tax, depth)]
    genus_unq = list(dict.fromkeys(tax))
    pos = {g: k for k, g in enumerate(genus_unq)}
    ref_to_genus = np.array([pos[t] for t in tax], dtype=np.int32)
    rows = [_r_strsplit(g) for g in genus_unq]
    if any(len(r) != td for r in rows):
        raise ValueError("Incorrect reference file format for assignTaxonomy: a taxonomy does not end in ';'.")
    genusmat = np.zeros((len(rows), td), dtype=np.int32)
    for lvl in range(td):
        code = {}
        for g, r in enumerate(rows):
            genusmat[g, lvl] = code.setdefault(r[lvl], len(code))
    return refs, genus_unq, ref_to_genus, genusmat


class TaxonomyModel:
    """The trained classifier, resident on ``device``: ``TaxonomyModel(ref_fasta)`` or ``TaxonomyModel((refs, taxonomies))`` with
    taxonomies the id lines ("Kingdom;Phylum;...;").  Train once, pass to assign_taxonomy as often as needed."""

    def __init__(self, ref, device: int = 0):
        if isinstance(ref, (str, bytes)) or hasattr(ref, "__fspath__"):
            ids, seqs = read_fasta(ref)
        else:
            seqs, ids = ref
            seqs, ids = [str(x).upper() for x in seqs], [str(x) for x in ids]
        self._train(*taxonomy_reference(seqs, ids), device)

    @classmethod
    def from_parsed(cls, refs, genus_unq, ref_to_genus, genusmat, device: int = 0):
        """A model from what taxonomy_reference returns (or an equivalent the caller built)."""
        m = cls.__new__(cls)
        m._train(list(refs), list(genus_unq), np.ascontiguousarray(ref_to_genus, dtype=np.int32), np.ascontiguousarray(genusmat, dtype=np.int32),
                 device)
        return m

    def _train(self, refs, genus_unq, ref_to_genus, genusmat, device):
        self.refs, self.genus_unq, self.ref_to_genus, self.genusmat = refs, genus_unq, ref_to_genus, genusmat
        self.device = device
        self.depth = int(self.genusmat.shape[1])
        self._h = C.c_void_p()
        st = np.zeros(_lib.TAXONOMY_NSTATS, dtype=np.int64)
        gm = np.ascontiguousarray(self.genusmat)
        eb = C.create_string_buffer(_EB)
        _lib.check(_lib.lib().dada2hip_taxonomy_train(len(self.refs), _charpp(self.refs), self.ref_to_genus.ctypes.data, gm.shape[0], gm.shape[1],
                                                      gm.ctypes.data, device, C.byref(self._h), st.ctypes.data, eb, _EB), eb)
        self.stats = {k: int(st[i]) for i, k in enumerate(_lib.TAXONOMY_TRAIN_STATS)}

    @property
    def ngenus(self):
        return len(self.genus_unq)

    def table(self):
        """The log-probability table read back from the device: float32 [ngenus, 65536] (diagnostic)."""
        out = np.zeros((self.ngenus, 65536), dtype=np.float32)
        eb = C.create_string_buffer(_EB)
        _lib.check(_lib.lib().dada2hip_taxonomy_table(self._h, out.ctypes.data, eb, _EB), eb)
        return out

    def close(self):
        if getattr(self, "_h", None):
            _lib.lib().dada2hip_taxonomy_free(self._h)
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def taxonomy_unifs(seed, n):
    """The n uniforms the library draws from ``seed`` when it is given none (include/dada2hip.h: splitmix64 of the position)."""
    with np.errstate(over="ignore"):
        z = np.uint64(seed & 0xFFFFFFFFFFFFFFFF) + (np.arange(n, dtype=np.uint64) + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z ^= z >> np.uint64(31)
    return (z >> np.uint64(11)).astype(np.float64) * (1.0 / 9007199254740992.0)


def assign_taxonomy_raw(seqs, model: TaxonomyModel, try_rc=False, seed=0, unifs=None, stats: dict = None):
    """dada2hip_taxonomy_assign: {"tax" [n], "boot" [n, depth], "boot_tax" [n, 100], "ntie" [n, 101]}, 0-based genus indices
    (-1: the query is shorter than 50 nt).  ``unifs``: nseq * 100 * ((max length - 7) // 8) doubles in [0, 1), laid out as the
    reference's runif buffer; None: drawn from ``seed``."""
    seqs = [seqs] if isinstance(seqs, str) else list(seqs)
    n = len(seqs)
    tax = np.zeros(n, dtype=np.int32)
    boot = np.zeros((n, model.depth), dtype=np.int32)
    boot_tax = np.zeros((n, 100), dtype=np.int32)
    ntie = np.zeros((n, 101), dtype=np.int32)
    st = np.zeros(_lib.TAXONOMY_NSTATS, dtype=np.int64)
    u = None
    if unifs is not None:
        u = np.ascontiguousarray(unifs, dtype=np.float64).ravel()
        need = n * 100 * (max(max((len(s) for s in seqs), default=0) - 7, 0) // 8)
        if u.size < need:
            raise ValueError("unifs holds %d values, the call needs %d." % (u.size, need))
    eb = C.create_string_buffer(_EB)
    _lib.check(_lib.lib().dada2hip_taxonomy_assign(model._h, n, _charpp(seqs), int(bool(try_rc)), None if u is None else u.ctypes.data,
                                                   int(seed) & 0xFFFFFFFFFFFFFFFF, tax.ctypes.data, boot.ctypes.data, boot_tax.ctypes.data,
                                                   ntie.ctypes.data, st.ctypes.data, eb, _EB), eb)
    if stats is not None:
        stats.update({k: int(st[i]) for i, k in enumerate(_lib.TAXONOMY_STATS)})
    return {"tax": tax, "boot": boot, "boot_tax": boot_tax, "ntie": ntie}


def taxonomy_table_out(genus_unq, tax, boot, min_boot=50):
    """R/taxonomy.R:137-150: the [n, depth] object array of level names - per query the levels of its genus whose bootstrap
    count reaches ``min_boot``, ``_DADA2_UNSPECIFIED`` and everything else None."""
    td = boot.shape[1]
    out = np.full((len(tax), td), None, dtype=object)
    for i, g in enumerate(tax):
        if g < 0:
            continue
        names = [x for x, b in zip(_r_strsplit(genus_unq[int(g)]), boot[i]) if b >= min_boot]
        for l, x in enumerate(names):
            out[i, l] = None if x == _TAX_UNSPECIFIED else x
    return out


def assign_taxonomy(seqs, ref, min_boot=50, try_rc=False, output_bootstraps=False, tax_levels=TAX_LEVELS, seed=0, unifs=None,
                    device: int = 0):
    """assignTaxonomy (R/taxonomy.R:65-160).  ``ref``: a reference FASTA (plain or gzip), (refs, taxonomies) or a TaxonomyModel.
    Returns the [n, depth] object array of level names (None = NA), or with ``output_bootstraps`` {"tax", "boot", "levels"}.  The
    bootstrap draws come from ``seed`` (or ``unifs``, see assign_taxonomy_raw) where the reference asks R's generator."""
    import warnings
    seqs = [seqs] if isinstance(seqs, str) else list(seqs)
    if seqs and min(len(s) for s in seqs) < 50:
        warnings.warn("Some sequences were shorter than 50 nts and will not receive a taxonomic classification.")
    own = not isinstance(ref, TaxonomyModel)
    model = TaxonomyModel(ref, device=device) if own else ref
    try:
        raw = assign_taxonomy_raw(seqs, model, try_rc=try_rc, seed=seed, unifs=unifs)
        out = taxonomy_table_out(model.genus_unq, raw["tax"], raw["boot"], min_boot)
        levels = list(tax_levels[: model.depth])
    finally:
        if own:
            model.close()
    if output_bootstraps:
        return {"tax": out, "boot": raw["boot"], "levels": levels}
    return out


# ---- assignSpecies / addSpecies (R/taxonomy.R:162-360; the matching itself is dada2hip_species_match) --------------------------
def _r_strsplit_ws(s):
    """strsplit(s, "\\s")[[1]]: one separator per whitespace character (two blanks leave an empty piece between them), a trailing
    empty piece dropped, "" gives no piece."""
    import re
    parts = re.split(r"\s", s, flags=re.ASCII)
    if parts and parts[-1] == "":
        parts.pop()
    return parts


def species_reference(ids):
    """R/taxonomy.R:255-263 on the id lines of a species reference (">SeqID genus species"): the format check on the FIRST id, then
    (genus, species) = tokens 2 and 3 of every id, None where an id has fewer tokens."""
    ids = [str(x) for x in ids]
    if not ids:
        raise ValueError("No reference sequences.")
    if not len(_r_strsplit_ws(ids[0])) >= 3:
        if ids[0].count(";") >= 3:
            raise ValueError("Incorrect reference file format for assignSpecies (this looks like a file formatted for assignTaxonomy).")
        raise ValueError("Incorrect reference file format for assignSpecies.")
    toks = [_r_strsplit_ws(i) for i in ids]
    return [t[1] if len(t) > 1 else None for t in toks], [t[2] if len(t) > 2 else None for t in toks]


class SpeciesModel:
    """The references of assignSpecies, resident on ``device``: ``SpeciesModel(ref_fasta)`` or ``SpeciesModel((refs, ids))``.  Open
    once, pass to species_hits / assign_species / add_species as often as needed.  A FASTA file is read as ShortRead reads it
    (upper case); sequences handed over directly are taken as they are, and only upper-case A/C/G/T can be matched."""

    def __init__(self, ref, device: int = 0):
        if isinstance(ref, (str, bytes)) or hasattr(ref, "__fspath__"):
            ids, seqs = read_fasta(ref)
        else:
            seqs, ids = ref
            seqs, ids = [str(x) for x in seqs], [str(x) for x in ids]
        if len(seqs) != len(ids):
            raise ValueError("One id per reference sequence is required.")
        self.genus, self.species = species_reference(ids)
        self.refs, self.ids, self.device = seqs, ids, device
        self._h = C.c_void_p()
        st = np.zeros(_lib.SPECIES_NSTATS, dtype=np.int64)
        eb = C.create_string_buffer(_EB)
        _lib.check(_lib.lib().dada2hip_species_open(len(seqs), _charpp(seqs), device, C.byref(self._h), st.ctypes.data, eb, _EB), eb)
        self.stats = {k: int(st[i]) for i, k in enumerate(_lib.SPECIES_STATS)}

    @property
    def nref(self):
        return len(self.refs)

    def close(self):
        if getattr(self, "_h", None):
            _lib.lib().dada2hip_species_free(self._h)
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _check_species_queries(seqs):
    """taxonomy.R:254 (C_isACGT), and an empty query, which a PDict does not take."""
    for s in seqs:
        if not s:
            raise ValueError("An empty query sequence.")
        if s.strip("ACGT"):
            raise ValueError("Non-ACGT characters present in the query sequences.")


def species_hits(seqs, model: SpeciesModel, try_rc=False, stats: dict = None):
    """dada2hip_species_match: per query the int32 array of the 0-based references it occurs in (with ``try_rc``: it or its
    reverse complement), ascending, each reference once."""
    seqs = [seqs] if isinstance(seqs, str) else [str(s) for s in seqs]
    _check_species_queries(seqs)
    L = _lib.lib()
    h = C.c_void_p()
    st = np.zeros(_lib.SPECIES_NSTATS, dtype=np.int64)
    eb = C.create_string_buffer(_EB)
    _lib.check(L.dada2hip_species_match(model._h, len(seqs), _charpp(seqs), int(bool(try_rc)), C.byref(h), st.ctypes.data, eb, _EB), eb)
    try:
        off = np.ctypeslib.as_array(L.dada2hip_species_hits_offsets(h), shape=(len(seqs) + 1,)).copy()
        refs = np.ctypeslib.as_array(L.dada2hip_species_hits_refs(h), shape=(int(off[-1]),)).copy() if off[-1] else np.zeros(0, dtype=np.int32)
    finally:
        L.dada2hip_species_hits_free(h)
    if stats is not None:
        stats.update({k: int(st[i]) for i, k in enumerate(_lib.SPECIES_STATS)})
    return [refs[off[j]: off[j + 1]] for j in range(len(seqs))]


def _map_hits(idx, names, keep):
    """mapHits (R/taxonomy.R:163-171) on the reference indices of one query."""
    hits = [names[int(i)] for i in idx]
    hits = ["Escherichia/Shigella" if h is not None and ("Escherichia" in h or "Shigella" in h) else h for h in hits]
    unq = set(hits)
    if len(unq) > keep:
        return None
    named = sorted(h for h in unq if h is not None)              # (sort() drops NA; by code point here)
    return "/".join(named) if named else None


def species_table_out(hits, genus, species, keep):
    """R/taxonomy.R:282-283: the [n, 2] object array (Genus, Species; None = NA) from per-query reference indices.  ``keep``: the
    most distinct species names a query may have (math.inf for all); the genus column always allows one."""
    out = np.full((len(hits), 2), None, dtype=object)
    for i, idx in enumerate(hits):
        out[i, 0] = _map_hits(idx, genus, 1)
        out[i, 1] = _map_hits(idx, species, keep)
    return out


def assign_species(seqs, ref, allow_multiple=False, try_rc=False, n=2000, verbose=False, device: int = 0):
    """assignSpecies (R/taxonomy.R:240-289).  ``ref``: a species FASTA (plain or gzip), (refs, ids) or a SpeciesModel.  Returns the
    [n, 2] object array (Genus, Species; None = NA).  ``allow_multiple``: False, True or the largest number of species to join.
    ``n`` (the reference's chunk of queries per PDict) is accepted and changes nothing here."""
    import math
    keep = (math.inf if allow_multiple else 1) if isinstance(allow_multiple, (bool, np.bool_)) else int(allow_multiple)
    seqs = [seqs] if isinstance(seqs, str) else [str(s) for s in seqs]
    own = not isinstance(ref, SpeciesModel)
    if own and (isinstance(ref, (str, bytes)) or hasattr(ref, "__fspath__")):
        ids, refs = read_fasta(ref)                              # (the reference reads the file, then checks the queries, then the ids)
        ref = (refs, ids)
    _check_species_queries(seqs)
    model = SpeciesModel(ref, device=device) if own else ref
    try:
        out = species_table_out(species_hits(seqs, model, try_rc=try_rc), model.genus, model.species, keep)
    finally:
        if own:
            model.close()
    if verbose:
        print(sum(1 for x in out[:, 1] if x is not None), "out of", len(seqs), "were assigned to the species level.")
    return out


def match_genera(gen_tax, gen_binom, split_glyph="/"):
    """matchGenera (R/taxonomy.R:175-185): does the curated genus name agree with the binomial's genus - equal, or the binomial's
    genus followed by a blank, "_" or the glyph at the start of the curated name (Clostridium groups), or behind the glyph at its
    end (split genera).  ``gen_binom`` goes into the regular expressions unescaped, as in the reference."""
    import re
    if gen_tax is None or gen_binom is None or len(gen_tax) == 0 or len(gen_binom) == 0:
        return False
    return bool(gen_tax == gen_binom or re.search("^" + gen_binom + "[ _" + split_glyph + "]", gen_tax)
                or re.search(split_glyph + gen_binom + "$", gen_tax))


def add_species(taxtab, seqs, ref, colnames=None, allow_multiple=False, try_rc=False, n=2000, verbose=False, device: int = 0):
    """addSpecies (R/taxonomy.R:347-360): ``taxtab`` [n, ncol] (the output of assign_taxonomy for ``seqs``, the reference's row
    names) with a Species column appended - the species of assign_species where its genus agrees (match_genera) with the table's
    genus column, the one ``colnames`` calls "Genus", else the last; None elsewhere."""
    taxtab = np.asarray(taxtab, dtype=object)
    if taxtab.ndim != 2 or taxtab.shape[0] != len(seqs):
        raise ValueError("One row of the taxonomic table per sequence is required.")
    binom = assign_species(seqs, ref, allow_multiple=allow_multiple, try_rc=try_rc, n=n, verbose=verbose, device=device)
    gcol = list(colnames).index("Genus") if colnames is not None and "Genus" in list(colnames) else taxtab.shape[1] - 1
    out = np.full((taxtab.shape[0], taxtab.shape[1] + 1), None, dtype=object)
    out[:, :-1] = taxtab
    for i in range(taxtab.shape[0]):
        if match_genera(taxtab[i, gcol], binom[i, 0]):
            out[i, -1] = binom[i, 1]
    if verbose:
        print("Of which", sum(1 for x in out[:, -1] if x is not None), "had genera consistent with the input table.")
    return out


# ---- filterAndTrim (R/filter.R:402-1120, :1180-1275; src/filter.cpp) ----

_FILTER_DEFAULTS = dict(trunc_q=2, trunc_len=0, trim_left=0, trim_right=0, max_len=float("inf"), min_len=20, max_n=0, min_q=0,
                        max_ee=float("inf"), rm_lowcomplex=0)
_FILTER_REFUSED = {"orient_fwd": "orient.fwd (it reorders the reads of a chunk, so its output depends on n)",
                   "match_ids": "matchIDs", "id_sep": "id.sep", "id_field": "id.field", "window": "seqComplexity's window"}


def _refuse_filter_args(kw):
    for k, v in kw.items():
        if k not in _FILTER_REFUSED:
            raise TypeError(f"unexpected argument {k!r}")
        if v is not None and v is not False:
            raise NotImplementedError(f"{_FILTER_REFUSED[k]} is not supported by this library.")


def filter_params(which=0, *, trunc_q=2, trunc_len=0, trim_left=0, trim_right=0, max_len=float("inf"), min_len=20, max_n=0, min_q=0,
                  max_ee=float("inf"), rm_phix=False, rm_lowcomplex=0, min_matches=2, non_overlapping=True, kmer_size=0,
                  quality_type=0):
    """A dada2hip_filter_params.  The nine trimming arguments and rm_lowcomplex may be pairs (forward, reverse), as in
    fastqPairedFilter (R/filter.R:890-906); ``which`` picks the direction.  max_len inf is "no limit"."""
    def pick(v, name):
        if isinstance(v, (list, tuple, np.ndarray)):
            if len(v) not in (1, 2):
                raise ValueError(f"Input variable {name} must be length 1 or 2 (Forward, Reverse).")
            v = v[which if len(v) == 2 else 0]
        return v
    import math
    ml = pick(max_len, "maxLen")
    p = _lib.CFilterParams()
    p.trunc_q, p.trunc_len = int(pick(trunc_q, "truncQ")), int(pick(trunc_len, "truncLen"))
    p.trim_left, p.trim_right = int(pick(trim_left, "trimLeft")), int(pick(trim_right, "trimRight"))
    p.max_len = 0 if (ml is None or math.isinf(ml)) else max(int(ml), 1) if ml >= 1 else -1
    if p.max_len < 0:
        raise ValueError("maxLen must be at least 1.")
    p.min_len, p.max_n, p.min_q = int(pick(min_len, "minLen")), int(pick(max_n, "maxN")), int(pick(min_q, "minQ"))
    p.max_ee = float(pick(max_ee, "maxEE"))
    p.rm_lowcomplex = float(pick(rm_lowcomplex, "rm.lowcomplex"))
    p.rm_phix, p.min_matches, p.non_overlapping = int(bool(rm_phix)), int(min_matches), int(bool(non_overlapping))
    p.kmer_size, p.qual_offset = int(kmer_size), int(quality_type)
    return p


def _screen_sequence(phix):
    """The screen's reference: a sequence of A/C/G/T, or the path of a FASTA file whose first record is taken."""
    if phix is None or phix is False:
        return None
    if hasattr(phix, "__fspath__"):
        phix = phix.__fspath__()
    import os
    phix = phix.decode() if isinstance(phix, bytes) else str(phix)
    if not os.path.exists(phix):
        if phix.isalpha():
            return phix                                                    # (the library checks the letters)
        raise FileNotFoundError(phix)
    _, seqs = read_fasta(phix)
    if not seqs:
        raise ValueError("No sequence in the screen's reference file.")
    return seqs[0]


class FilterContext:
    """The state of filterAndTrim that stays on ``device`` across files: the word table of the phiX screen (``phix``: the genome as
    a string or the path of a FASTA file; the library ships none; None: no screen) and the expected-error tables."""

    def __init__(self, phix=None, word_size: int = 16, device: int = 0):
        self.ref = _screen_sequence(phix)
        self.word_size, self.device = int(word_size), device
        self._h = C.c_void_p()
        st = np.zeros(_lib.FILTER_NSTATS, dtype=np.int64)
        eb = C.create_string_buffer(_EB)
        _lib.check(_lib.lib().dada2hip_filter_open(self.ref.encode() if self.ref is not None else None, self.word_size, device,
                                                   C.byref(self._h), st.ctypes.data, eb, _EB), eb)
        self.stats = {k: int(st[i]) for i, k in enumerate(_lib.FILTER_STATS)}

    def close(self):
        if getattr(self, "_h", None):
            _lib.lib().dada2hip_filter_free(self._h)
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _blob(strs):
    bs = [s if isinstance(s, bytes) else str(s).encode() for s in strs]
    off = np.zeros(len(bs) + 1, dtype=np.int64)
    if bs:
        np.cumsum([len(b) for b in bs], out=off[1:])
    return b"".join(bs), off


def filter_reads(seqs, quals, ctx: FilterContext, params=None, *, kmers=False, stats: dict = None, **kw):
    """dada2hip_filter_reads on reads in memory (``quals``: the quality strings as in the FASTQ file).  Returns a dict: ``code``
    (0 kept, else the first stage failed, an index into _lib.FILTER_STAGES), ``window`` (n, 2: offset and length kept), ``ee``,
    ``hits`` (n, 2: the screen's counts against the reference and its reverse complement) and, with ``kmers``, ``kmer_counts``
    (n, 4^k) and ``complexity``.  ``params``: a filter_params(), or its keywords."""
    p = params if params is not None else filter_params(**kw)
    sb, off = _blob(seqs)
    qb, qoff = _blob(quals)
    if not np.array_equal(off, qoff):
        raise ValueError("Every read needs as many quality characters as bases.")
    n = len(off) - 1
    k = p.kmer_size or 2
    out = {"code": np.zeros(n, dtype=np.int32), "window": np.zeros((n, 2), dtype=np.int32), "ee": np.zeros(n, dtype=np.float64),
           "hits": np.zeros((n, 2), dtype=np.int32)}
    if kmers:
        out["kmer_counts"] = np.zeros((n, 4 ** k), dtype=np.int32)
        out["complexity"] = np.zeros(n, dtype=np.float64)
    st = np.zeros(_lib.FILTER_NSTATS, dtype=np.int64)
    eb = C.create_string_buffer(_EB)
    _lib.check(_lib.lib().dada2hip_filter_reads(ctx._h, n, sb, qb, off.ctypes.data, C.byref(p), out["code"].ctypes.data,
                                                out["window"].ctypes.data, out["ee"].ctypes.data, out["hits"].ctypes.data,
                                                out["kmer_counts"].ctypes.data if kmers else None,
                                                out["complexity"].ctypes.data if kmers else None, st.ctypes.data, eb, _EB), eb)
    if stats is not None:
        stats.update({k_: int(st[i]) for i, k_ in enumerate(_lib.FILTER_STATS)})
    return out


def _whole_read_params(**kw):
    """Parameters under which every non-empty read is kept whole (the quality characters handed over are 'I')."""
    return filter_params(trunc_q=-1, min_len=0, max_n=2 ** 31 - 1, quality_type=33, **kw)


def match_ref(seqs, ref, word_size=16, non_overlapping=True, device: int = 0):
    """C_matchRef (src/filter.cpp:7-32): per sequence the number of its windows of ``word_size`` that are words of the circular
    ``ref``, counted greedily when ``non_overlapping`` (a hit at j makes j + word_size + 1 the next window tested)."""
    seqs = [seqs] if isinstance(seqs, str) else [str(s) for s in seqs]
    with FilterContext(ref, word_size, device) as ctx:
        got = filter_reads(seqs, ["I" * len(s) for s in seqs], ctx, _whole_read_params(non_overlapping=non_overlapping))
    return got["hits"][:, 0].copy()


def is_phix(seqs, phix, word_size=16, min_matches=2, non_overlapping=True, device: int = 0):
    """isPhiX (R/filter.R:1180-1187) against the genome ``phix`` (a string, a FASTA path or an open FilterContext): True where the
    count against the genome or the count against its reverse complement reaches ``min_matches``."""
    seqs = [seqs] if isinstance(seqs, str) else [str(s) for s in seqs]
    ctx = phix if isinstance(phix, FilterContext) else FilterContext(phix, word_size, device)
    try:
        got = filter_reads(seqs, ["I" * len(s) for s in seqs], ctx, _whole_read_params(non_overlapping=non_overlapping))
    finally:
        if ctx is not phix:
            ctx.close()
    return (got["hits"] >= int(min_matches)).any(axis=1)


def seq_complexity(seqs, kmer_size=2, window=None, device: int = 0):
    """seqComplexity (R/filter.R:1248-1275) with window = NULL: the Shannon richness of the k-mers that are A/C/G/T only; NaN for
    a sequence without one."""
    if window is not None:
        raise NotImplementedError("seqComplexity's window is not supported by this library.")
    seqs = [seqs] if isinstance(seqs, str) else [str(s) for s in seqs]
    with FilterContext(None, 16, device) as ctx:
        got = filter_reads(seqs, ["I" * len(s) for s in seqs], ctx, _whole_read_params(kmer_size=kmer_size), kmers=True)
    return got["complexity"]


def _filter_ctx(rm_phix, ctx, device):
    if ctx is not None:
        return ctx, False
    if rm_phix is True:
        raise ValueError("rm_phix needs the genome (a sequence or the path of a FASTA file): the library ships no copy of it.")
    return FilterContext(rm_phix if rm_phix else None, 16, device), True


def fastq_filter(fn, fout, *, compress=True, n=10**6, quality_type=0, verbose=False, rm_phix=False, ctx: FilterContext = None,
                 device: int = 0, stats: dict = None, min_matches=2, non_overlapping=True, kmer_size=0, **kw):
    """fastqFilter (R/filter.R:613-730): (reads_in, reads_out).  ``rm_phix``: the genome (sequence or FASTA path), or True with a
    ``ctx`` that holds it, or False."""
    _refuse_filter_args({k: kw.pop(k) for k in list(kw) if k in _FILTER_REFUSED})
    for k, v in kw.items():
        if k not in _FILTER_DEFAULTS:
            raise TypeError(f"unexpected argument {k!r}")
        if isinstance(v, (list, tuple, np.ndarray)) and len(v) > 1:
            raise ValueError("Filtering and trimming arguments should be of length 1 when processing single-end (rather than paired-end) data.")
    c, own = _filter_ctx(rm_phix, ctx, device)
    try:
        p = filter_params(rm_phix=bool(rm_phix), min_matches=min_matches, non_overlapping=non_overlapping, kmer_size=kmer_size,
                          quality_type=quality_type, **kw)
        rin, rout = C.c_int64(), C.c_int64()
        st = np.zeros(_lib.FILTER_NSTATS, dtype=np.int64)
        eb = C.create_string_buffer(_EB)
        _lib.check(_lib.lib().dada2hip_filter_fastq(c._h, str(fn).encode(), str(fout).encode(), C.byref(p), int(bool(compress)), int(n),
                                                    C.byref(rin), C.byref(rout), st.ctypes.data, eb, _EB), eb)
    finally:
        if own:
            c.close()
    if stats is not None:
        stats.update({k_: int(st[i]) for i, k_ in enumerate(_lib.FILTER_STATS)})
    if verbose:
        print(f"Read in {rin.value}, output {rout.value} ({round(rout.value * 100 / max(rin.value, 1), 1)}%) filtered sequences.")
    if rout.value == 0 and verbose:
        print(f"The filter removed all reads: {fout} not written.")
    return rin.value, rout.value


def fastq_paired_filter(fn, fout, *, compress=True, n=10**6, quality_type=0, verbose=False, rm_phix=False, ctx: FilterContext = None,
                        device: int = 0, stats: dict = None, min_matches=2, non_overlapping=True, kmer_size=0, **kw):
    """fastqPairedFilter (R/filter.R:878-1140): ``fn`` and ``fout`` are (forward, reverse); a pair is kept when both reads pass;
    every trimming argument may be a pair."""
    _refuse_filter_args({k: kw.pop(k) for k in list(kw) if k in _FILTER_REFUSED})
    if isinstance(fn, str) or len(fn) != 2:
        raise ValueError("Two paired input file names required.")
    if isinstance(fout, str) or len(fout) != 2:
        raise ValueError("Two paired output file names required.")
    for k in kw:
        if k not in _FILTER_DEFAULTS:
            raise TypeError(f"unexpected argument {k!r}")
    c, own = _filter_ctx(rm_phix, ctx, device)
    try:
        ps = [filter_params(w, rm_phix=bool(rm_phix), min_matches=min_matches, non_overlapping=non_overlapping, kmer_size=kmer_size,
                            quality_type=quality_type, **kw) for w in (0, 1)]
        rin, rout = C.c_int64(), C.c_int64()
        st = np.zeros(_lib.FILTER_NSTATS, dtype=np.int64)
        eb = C.create_string_buffer(_EB)
        _lib.check(_lib.lib().dada2hip_filter_fastq_paired(c._h, str(fn[0]).encode(), str(fn[1]).encode(), str(fout[0]).encode(),
                                                           str(fout[1]).encode(), C.byref(ps[0]), C.byref(ps[1]), int(bool(compress)),
                                                           int(n), C.byref(rin), C.byref(rout), st.ctypes.data, eb, _EB), eb)
    finally:
        if own:
            c.close()
    if stats is not None:
        stats.update({k_: int(st[i]) for i, k_ in enumerate(_lib.FILTER_STATS)})
    if verbose:
        print(f"Read in {rin.value} paired-sequences, output {rout.value} ({round(rout.value * 100 / max(rin.value, 1), 1)}%) filtered paired-sequences.")
    return rin.value, rout.value


def filter_and_trim(fwd, filt, rev=None, filt_rev=None, *, compress=True, trunc_q=2, trunc_len=0, trim_left=0, trim_right=0,
                    max_len=float("inf"), min_len=20, max_n=0, min_q=0, max_ee=float("inf"), rm_phix=False, rm_lowcomplex=0, n=10**5,
                    quality_type=0, device: int = 0, verbose=False, ctx: FilterContext = None, _per_file=None, **kw):
    """filterAndTrim (R/filter.R:402-497) over one file or lists of files: returns (an (nfiles, 2) int64 array of reads.in /
    reads.out, the row names basename(fwd)).  ``rm_phix``: the phiX genome as a sequence or the path of a FASTA file (the library
    ships no copy), or False.  Output directories are created; duplicate output paths and outputs equal to an input are
    refused; a file from which nothing passes is not written.  ``_per_file``: the (single-end, paired) functions run per file, for
    modules that wrap this one; by default fastq_filter and fastq_paired_filter."""
    import os
    _refuse_filter_args(kw)
    single, pair = _per_file or (fastq_filter, fastq_paired_filter)
    aslist = lambda x: [os.fspath(x)] if (isinstance(x, (str, bytes)) or hasattr(x, "__fspath__")) else [os.fspath(y) for y in x]   # noqa: E731
    fwd, filt = aslist(fwd), aslist(filt)
    if not all(os.path.exists(f) for f in fwd):
        raise ValueError("Some input files do not exist.")
    if len(filt) == 1 and len(fwd) > 1:
        filt = [os.path.join(filt[0], os.path.basename(f)) for f in fwd]
    if len(fwd) != len(filt):
        raise ValueError("Every input file must have a corresponding output file.")
    paired = rev is not None
    if paired:
        if filt_rev is None:
            raise ValueError("Output files for the reverse reads are required.")
        rev, filt_rev = aslist(rev), aslist(filt_rev)
        if not all(os.path.exists(f) for f in rev):
            raise ValueError("Some input files (rev) do not exist.")
        if len(rev) != len(fwd):
            raise ValueError("Paired forward and reverse input files must correspond.")
        if len(filt_rev) == 1 and len(rev) > 1:
            filt_rev = [os.path.join(filt_rev[0], os.path.basename(f)) for f in rev]
        if len(rev) != len(filt_rev):
            raise ValueError("Every input file (rev) must have a corresponding output file (filt.rev).")
    outs = [os.path.abspath(f) for f in filt + (filt_rev if paired else [])]
    ins = [os.path.realpath(f) for f in fwd + (rev if paired else [])]
    for o in outs:
        if os.path.dirname(o):
            os.makedirs(os.path.dirname(o), exist_ok=True)
    outs = [os.path.realpath(o) for o in outs]
    if len(set(outs)) != len(outs):
        raise ValueError("All output files must be distinct.")
    if set(outs) & set(ins):
        raise ValueError("Output files must be distinct from the input files.")
    args = dict(trunc_q=trunc_q, trunc_len=trunc_len, trim_left=trim_left, trim_right=trim_right, max_len=max_len, min_len=min_len,
                max_n=max_n, min_q=min_q, max_ee=max_ee, rm_lowcomplex=rm_lowcomplex)
    c, own = _filter_ctx(rm_phix, ctx, device)
    rval = np.zeros((len(fwd), 2), dtype=np.int64)
    try:
        for i in range(len(fwd)):
            if paired:
                rval[i] = pair((fwd[i], rev[i]), (filt[i], filt_rev[i]), compress=compress, n=n, quality_type=quality_type,
                               verbose=verbose, rm_phix=bool(rm_phix), ctx=c, **args)
            else:
                rval[i] = single(fwd[i], filt[i], compress=compress, n=n, quality_type=quality_type, verbose=verbose,
                                 rm_phix=bool(rm_phix), ctx=c, **args)
    finally:
        if own:
            c.close()
    if len(fwd) and (rval[:, 1] == 0).all():
        import warnings
        warnings.warn("No reads passed the filter. Please revisit your filtering parameters.")
    return rval, [os.path.basename(f) for f in fwd]


def calc_pA_device(reads, E, prior, device: int = 0):
    """calc_pA (src/pval.cpp:44-64) evaluated by the device kernel."""
    L = _lib.lib()
    r = np.ascontiguousarray(reads, dtype=np.int32)
    e = np.ascontiguousarray(E, dtype=np.float64)
    p = np.ascontiguousarray(prior, dtype=np.uint8)
    out = np.zeros(r.size)
    eb = C.create_string_buffer(_EB)
    _lib.check(L.dada2hip_calc_pA(r.size, r.ctypes.data, e.ctypes.data, p.ctypes.data, device, out.ctypes.data, eb, _EB), eb)
    return out


# --------------------------------------------------------------------------------------------------
def accumulate_trans(trans_list):
    """R/errorModels.R:462-471."""
    maxcol = max(t.shape[1] for t in trans_list)
    out = np.zeros((16, maxcol), dtype=np.int64)
    for t in trans_list:
        out[:, : t.shape[1]] += t
    return out


def noqual_errfun(trans, pseudocount=1):
    """R/errorModels.R:222-249 (noqualErrfun): one rate per transition, aggregated over quality."""
    trans = np.asarray(trans, dtype=np.float64)
    obs = trans.sum(axis=1) + pseudocount
    err = np.zeros_like(trans)
    for i in range(4):
        tot = obs[4 * i: 4 * i + 4].sum()
        rates = obs[4 * i: 4 * i + 4] / tot
        for j in range(4):
            if i != j:
                err[4 * i + j, :] = rates[j]
        err[5 * i, :] = 1.0 - sum(rates[j] for j in range(4) if j != i)
    return err


def pseudo_priors_of(results, opts: DadaOpts):
    """R/dada.R:399-400: the columns of makeSequenceTable over a pass's clusterings found in at least ``PSEUDO_PREVALENCE`` samples
    or with at least ``PSEUDO_ABUNDANCE`` reads in all."""
    mat, seqs = make_sequence_table(list(results))
    hit = ((mat > 0).sum(axis=0) >= opts.PSEUDO_PREVALENCE) | (mat.sum(axis=0, dtype=np.int64) >= opts.PSEUDO_ABUNDANCE)
    return [s for s, h in zip(seqs, hit) if h]


def split_pooled(res: DadaResult, abundances, unique_to_pool) -> DadaResult:
    """One input sample's share of a pooled result (R/dada.R:451-472).  ``unique_to_pool``: the 0-based pooled row of each of the
    sample's uniques, ``abundances`` theirs.  The clusters some unique of the sample maps to are kept (NA is ignored) and
    renumbered by ``cumsum(keep)``; clustering rows, clusterquals columns and the birth_subs rows of kept clusters are pruned,
    ``birth_subs["clust"]`` and the map renumbered (NA kept), and ``clustering["abundance"]`` becomes the per-cluster sums of THIS
    sample's abundances.  Everything else stays the pooled run's, exactly as in R: n0, n1, nunq, pval, the birth_* columns
    (``birth_from`` still counts POOLED clusters), subqual and the per-unique pval vector (one entry per POOLED unique); the
    quality columns are "not the qualities for this sample alone" (:462)."""
    m = np.asarray(res.map, dtype=np.int64)[np.asarray(unique_to_pool, dtype=np.int64)]
    ok = m != NA_INTEGER
    nclust = res.nclust
    keep = np.zeros(nclust, dtype=bool)
    keep[m[ok] - 1] = True
    new_bi = np.cumsum(keep)
    clustering = {}
    for c, v in res.clustering.items():
        clustering[c] = [s for s, k in zip(v, keep) if k] if c == "sequence" else np.asarray(v)[keep].copy()
    new_map = np.full(m.shape, NA_INTEGER, dtype=np.int32)
    new_map[ok] = new_bi[m[ok] - 1]
    sums = np.zeros(int(keep.sum()), dtype=np.int64)
    np.add.at(sums, new_map[ok].astype(np.int64) - 1, np.asarray(abundances, dtype=np.int64)[ok])   # tapply(uniques, map, sum), :470
    clustering["abundance"] = sums.astype(np.int32)
    bc = np.asarray(res.birth_subs["clust"], dtype=np.int64)
    bkeep = keep[bc - 1] if bc.size else np.zeros(0, dtype=bool)
    birth_subs = {}
    for c, v in res.birth_subs.items():
        birth_subs[c] = [x for x, k in zip(v, bkeep) if k] if c in ("ref", "sub") else np.asarray(v)[bkeep].copy()
    birth_subs["clust"] = new_bi[bc[bkeep] - 1].astype(np.int32)
    return DadaResult(clustering, birth_subs, np.array(res.subqual, copy=True), np.asarray(res.clusterquals)[:, keep].copy(), new_map,
                      np.array(res.pval, copy=True), dict(res.stats))


def dada(dereps, err=None, *, self_consist=False, err_fun=noqual_errfun, opts: DadaOpts = None, priors=None,
         device: int = 0, verbose=False, samples=None, timings: list = None, host_input=None, on_pass=None, pool=False,
         prior_seqs=None):
    """The sample loop and selfConsist loop of R/dada.R:256-405 over resident samples.

    ``err_fun`` maps the accumulated 16 x Q transition counts to a new error matrix; the
    reference's default is ``loessErrfun`` (stats::loess, third-party, not available here) so the
    deterministic ``noqualErrfun`` stands in.  Returns (list[DadaResult], err_out,
    list of err matrices tried).  ``on_pass(k, errs_used, max_clust, results)`` is called after every pass with the
    error matrix each sample was run with (the all-ones start of R/dada.R:298 included) - the parity tests check every
    pass of the loop through it, not just the last.

    ``dereps``: a ``Derep`` or a list of them; a ``NativeDerep`` (the library's own object, from ``NativeDerep(path)``) stands wherever a
    ``Derep`` does and is made resident without a host copy (``Sample.from_native``) - the pooled object of ``pool=True`` is one.

    ``prior_seqs``: R's ``priors`` argument, a list of sequences (:149, :183, :335); they are matched against each resident
    sample on the device (``Sample.set_prior_seqs``) and OR-ed with the per-unique flags ``priors[i]`` where both are given.

    ``pool`` (:185-196): ``True`` combines the dereps (``combine_dereps``), runs the pass loop on ONE resident sample of the pooled
    object and splits the result back (``split_pooled``, which says what stays the pooled run's): one DadaResult per INPUT
    sample; per-sample ``priors`` flags, ``samples=`` and ``host_input=`` make no sense there and are a ValueError; ``on_pass``
    sees the pooled sample.  With one derep it is ``False`` (:187).  ``"pseudo"`` keeps the samples separate: after every pass
    with nconsist >= 1 the sequences found in ``PSEUDO_PREVALENCE`` samples or with ``PSEUDO_ABUNDANCE`` reads become priors of
    the next pass, and the loop may end only at nconsist >= 2 (:391-404) - so without ``self_consist`` the second pass runs with
    the matrix ``err_fun`` estimated from the first (:264, :300, :374), not with the caller's, and ``err_fun=None`` is a
    ValueError."""
    o = (opts or DadaOpts()).normalised()
    single = isinstance(dereps, (Derep, NativeDerep))
    if single:
        dereps = [dereps]
    pseudo = False
    if len(dereps) <= 1:                                           # :187
        pool = False
    if isinstance(pool, (bool, np.bool_)):
        pool = bool(pool)
    elif isinstance(pool, str) and pool == "pseudo":               # :193-195
        pool, pseudo = False, True
    else:
        raise ValueError("Invalid pool argument.")
    if pseudo and err_fun is None:
        raise ValueError('pool="pseudo" runs its second pass with the error matrix err_fun estimates from the first: err_fun is required.')
    prior_seqs = None if prior_seqs is None else [str(s) for s in prior_seqs]
    if pool:
        if priors is not None or samples is not None or host_input is not None:
            raise ValueError("pool=True runs one pooled sample: per-sample priors, samples= and host_input= do not apply (use prior_seqs).")
        import time
        inputs = list(dereps)
        t_create = time.perf_counter()
        pooled, u2p = _combine_native(inputs)
        try:
            smp = Sample.from_native(pooled, None, device)
            inner = None if timings is None else []
            try:
                res, err_out, errs = dada([pooled], err, self_consist=self_consist, err_fun=err_fun, opts=opts, device=device, verbose=verbose,
                                          samples=[smp], timings=inner, on_pass=on_pass, prior_seqs=prior_seqs)
            finally:
                if timings is not None:                             # [0] = the combine and the upload of the pooled sample
                    timings.extend([(time.perf_counter() - t_create) * 1e3 - sum(inner)] + inner[1:])
                smp.close()
        finally:
            pooled.close()

        def ab(d):
            if isinstance(d, NativeDerep):
                return np.ctypeslib.as_array(_lib.lib().dada2hip_derep_abundances(d._h), (d.nuniques,)).copy()
            return d.abundances
        return [split_pooled(res[0], ab(d), u) for d, u in zip(inputs, u2p)], err_out, errs
    import time
    own = samples is None
    t_create = time.perf_counter()
    if own:
        if host_input is not None and single:          # inputs already marshalled (bench.py): one resident sample from them
            samples = [Sample(host_input, None, None, None, device)]
        else:
            samples = [Sample.from_native(d, None if priors is None else priors[i], device) if isinstance(d, NativeDerep) else
                       Sample.from_derep(d, None if priors is None else priors[i], device) for i, d in enumerate(dereps)]
    if timings is not None:
        timings.append((time.perf_counter() - t_create) * 1e3)   # [0] = making the samples resident (upload), then one entry per pass
    initialize = self_consist and err is None
    nconsist = 0 if initialize else 1
    errs = []
    # the largest rounded quality of each sample (R/dada.R:297-313 extends err to it): a property of the sample, taken ONCE - as a
    # statement inside the pass loop it re-read the whole maxlen x nraw double matrix every pass (2 GB at 10^6 uniques: 70 ms of
    # every selfConsist pass, profiles/r09a_selfconsist_passes.txt)
    qmaxes = [d.qmax() for d in dereps]

    def flag_by_sequence(seqs):                                     # names(uniques) %in% c(priors, pseudo_priors), :335
        for i, smp in enumerate(samples):
            smp.set_prior_seqs(seqs, or_flags=None if priors is None else priors[i])
    try:
        if prior_seqs is not None:
            flag_by_sequence(prior_seqs)
        while True:
            if nconsist > 0:
                errs.append(np.array(err, copy=True))
            results, used = [], []
            t_pass = time.perf_counter()
            for d, smp, qmax in zip(dereps, samples, qmaxes):
                erri = np.ones((16, max(41, qmax + 1))) if initialize else extend_err(err, qmax)   # R/dada.R:297-313
                results.append(smp.run(erri, o, max_clust=1 if initialize else None, verbose=verbose))
                used.append(erri)
            if timings is not None:
                timings.append((time.perf_counter() - t_pass) * 1e3)
            if on_pass is not None:
                on_pass(len(errs) if not initialize else 0, used, 1 if initialize else None, results)
            cur = accumulate_trans([r.subqual for r in results])
            new_err = err_fun(cur) if err_fun is not None else None
            if initialize:
                initialize = False
                new_err[[0, 5, 10, 15], :] = 1.0                                                   # R/dada.R:385-388
            err = new_err
            if (not self_consist) or any(np.array_equal(e, err) for e in errs) or nconsist >= o.MAX_CONSIST:
                if not pseudo or nconsist >= 2:                     # :392: a pseudo-pooled run needs one full pass for its priors
                    break
            if pseudo and nconsist >= 1:                            # :398-402
                flag_by_sequence((prior_seqs or []) + pseudo_priors_of(results, o))
            nconsist += 1
    finally:
        if own:
            for smp in samples:
                smp.close()
    return (results[0] if single else results), err, errs
