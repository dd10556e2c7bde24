"""learnErrors and the error-estimation functions that need no loess (R/errorModels.R).

``learn_errors`` is R's ``learnErrors`` (:333-363): dereplicate samples until ``nbases`` is passed, make them resident and run the
selfConsist loop of ``api.dada`` over them.  The device work is dereplication and that loop; the fits are host work, 12 regressions
over at most 94 points per pass.  ``dada2_amd.api`` neither imports nor re-exports this module.

An error-estimation function maps a 16 x Q matrix of transition counts (rows ``A2A, A2C, ..., T2T``, column k = quality k) to a
16 x Q float64 matrix of rates:

* ``make_binned_qual_errfun(binned_q)`` - ``makeBinnedQualErrfun`` (:96-156) line for line, the reference's own function for
  binned qualities.  The only one here that claims the reference's bits.
* ``loess_direct_errfun`` - ``loessErrfun``'s frame (:28-67) around the DIRECT local-quadratic fit.  R's default ``loess``
  evaluates an interpolated surface (kd-tree vertices, blended); this is the fit that surface approximates, evaluated at every
  quality.  Not bit-comparable to R, and how far the two are apart has not been measured by anyone: there is no R to run.
* ``make_pacbio_errfun(base)`` - ``PacBioErrfun`` (:183-196): ``base`` below Q93, the maximum-likelihood column at Q93.
* ``noqual_errfun`` - ``api.noqual_errfun``, the same object.

``get_errors`` is ``getErrors`` (:390-423); ``errors_frame`` is the data frame ``plotErrors`` draws from
(R/plot-methods.R:61-113), as a dict of numpy columns.  Nothing is drawn."""
from __future__ import annotations

import dataclasses
import os
import re
import sys
import time
import warnings

import numpy as np

from . import _lib, api
from .io import Derep
from .opts import DadaOpts, DadaResult

noqual_errfun = api.noqual_errfun

TRANSITIONS = tuple(a + "2" + b for a in "ACGT" for b in "ACGT")
MAX_ERROR_RATE = 0.25
MIN_ERROR_RATE = 1e-7
_OFF = tuple(r for r in range(16) if r % 5)               # the 12 rows of ``est``, in R's rbind order


def _counts(trans):
    t = np.asarray(trans, dtype=np.float64)
    if t.ndim != 2 or t.shape[0] != 16:
        raise ValueError("A transition matrix must have 16 rows (A2A, A2C, ...).")
    return t


def expand_err(est12):
    """The tail the reference's functions share (:52-66, :140-154): the 12 off-diagonal rows clamped to [1e-7, 0.25], each
    self-transition row ``1 - colSums(its three rates)``.  R's ``colSums`` accumulates in ``LDOUBLE`` and rounds once, so the sum
    is taken in ``np.longdouble`` in row order and rounded once to float64 (``api.noqual_errfun`` sums in double: R's
    ``noqualErrfun`` goes through the same ``colSums``, and the two can differ in the last bit)."""
    est = np.array(est12, dtype=np.float64)
    if est.ndim != 2 or est.shape[0] != 12:
        raise ValueError("expand_err takes the 12 off-diagonal rows (A2C, A2G, A2T, C2A, ...).")
    est[est > MAX_ERROR_RATE] = MAX_ERROR_RATE
    est[est < MIN_ERROR_RATE] = MIN_ERROR_RATE
    err = np.empty((16, est.shape[1]), dtype=np.float64)
    err[list(_OFF)] = est
    for i in range(4):
        s = np.zeros(est.shape[1], dtype=np.longdouble)
        for r in range(3 * i, 3 * i + 3):
            s = s + est[r].astype(np.longdouble)
        err[5 * i] = 1.0 - s.astype(np.float64)
    return err


def _carry_edges(pred):
    """:43-46, :131-134: columns past the last prediction take it, columns before the first take it."""
    have = np.flatnonzero(~np.isnan(pred))
    pred[have[-1] + 1:] = pred[have[-1]]
    pred[: have[0]] = pred[have[0]]
    return pred


def make_binned_qual_errfun(binned_q):
    """``makeBinnedQualErrfun(binnedQ)`` (:96-156): piecewise linear between the observed rates at consecutive binned qualities.
    ``seq(loP, hiP, length.out = n)`` is restated as R's ``seq.default`` computes it: ``loP``, ``loP + k * ((hiP - loP) / (n - 1))``
    for k = 1 .. n - 2, ``hiP``; ``rep(loP, n)`` where the two are equal.  R's ``stop``s are ``ValueError``s with R's texts, its
    ``warning``s go through ``warnings.warn``."""
    if binned_q is None:
        raise ValueError("The quality scores used in your data must be provided.")
    binned = [int(q) for q in binned_q]

    def binned_qual_errfun(trans, binned_quals=binned):
        t = _counts(trans)
        nq = t.shape[1]
        qq = np.arange(nq)
        seen = qq[t.sum(axis=0) > 0]
        qmax = seen.max() if seen.size else -np.inf
        qmin = seen.min() if seen.size else np.inf
        if qmax > max(binned_quals):
            raise ValueError("Input data contains a higher quality score than the provided binned values.")
        if qmin < min(binned_quals):
            raise ValueError("Input data contains a lower quality score than the provided binned values.")
        if qmax not in binned_quals:
            warnings.warn("Maximum observed quality score is not in the provided binned values.")
        if qmin not in binned_quals:
            warnings.warn("Minimum observed quality score is not in the provided binned values.")
        est = np.empty((12, nq), dtype=np.float64)
        for k, row in enumerate(_OFF):
            i = row // 4
            errs = t[row]
            tot = t[4 * i: 4 * i + 4].sum(axis=0)
            with np.errstate(divide="ignore", invalid="ignore"):
                p = errs / tot                                     # NaN where tot == 0
            pred = np.full(nq, np.nan)
            for lo, hi in zip(binned_quals[:-1], binned_quals[1:]):
                if hi < lo:
                    raise ValueError("The binned quality scores must be increasing (R's seq() fails on a negative length.out).")
                if lo < 0 or hi >= nq:                             # df$p[hiQ + 1] past the last row is NA
                    continue
                lo_p, hi_p = p[lo], p[hi]
                if np.isnan(lo_p) or np.isnan(hi_p):
                    continue
                n = hi - lo + 1
                if n > 2 and lo_p != hi_p:
                    pred[lo + 1: hi] = lo_p + np.arange(1, n - 1, dtype=np.float64) * ((hi_p - lo_p) / (n - 1))
                else:
                    pred[lo: hi + 1] = lo_p
                pred[lo], pred[hi] = lo_p, hi_p
            if np.isnan(pred).all():                               # R: max(integer(0)) is -Inf, and pred[[-Inf]] fails
                raise ValueError("No two consecutive binned quality scores were observed for %s: error rates cannot be interpolated."
                                 % TRANSITIONS[row])
            est[k] = _carry_edges(pred)
        return expand_err(est)

    return binned_qual_errfun


def _local_quadratic(x, y, w, x0, q):
    """The intercept at ``x0`` of the tricube-weighted least-squares quadratic over the ``q`` nearest points."""
    d = np.abs(x - x0)
    h = np.sort(d)[q - 1]
    with np.errstate(divide="ignore", invalid="ignore"):
        v = np.where(d < h, w * (1.0 - (d / h) ** 3) ** 3, 0.0)
    sv = np.sqrt(v)
    dx = x - x0
    design = np.stack([np.ones_like(dx), dx, dx * dx], axis=1) * sv[:, None]
    coef = np.linalg.lstsq(design, sv * y, rcond=None)[0]
    return coef[0]


def loess_direct_errfun(trans, span=0.75):
    """``loessErrfun``'s frame (:28-67) around the direct local-quadratic fit - NOT R's default ``loess`` surface.

    Per transition: ``rlogp = log10((errs + 1) / tot)`` with prior weights ``tot``; columns with ``tot == 0`` are dropped.  With n
    kept columns, ``q = min(n, floor(n * span + 1e-5))`` (fewer than 3 is a ``ValueError``).  At every integer ``x0`` from the
    smallest to the largest kept quality, h is the q-th smallest ``|x_i - x0|``, ``v_i = tot_i * (1 - (|x_i - x0| / h)^3)^3`` where
    ``|x_i - x0| < h`` and 0 elsewhere, and the prediction is the intercept of the minimum-norm weighted least-squares quadratic in
    ``x_i - x0`` (``numpy.linalg.lstsq`` on the ``sqrt(v)``-scaled design).  Columns outside the kept range carry the edge values
    (R's surface is NA there and :43-46 carries the edges), then ``10^pred`` and ``expand_err``.

    This is the direct surface.  R's default (``surface = "interpolate"``) fits at the vertices of a kd-tree and blends between
    them; the difference between the two has not been measured by anyone, since there is no R to run beside this code.  Only
    ``make_binned_qual_errfun`` claims the reference's bits."""
    t = _counts(trans)
    nq = t.shape[1]
    est = np.empty((12, nq), dtype=np.float64)
    for k, row in enumerate(_OFF):
        i = row // 4
        tot = t[4 * i: 4 * i + 4].sum(axis=0)
        keep = np.flatnonzero(tot > 0)
        n = keep.size
        q = min(n, int(np.floor(n * span + 1e-5)))
        if q < 3:
            raise ValueError("Too few quality scores with observations for a local quadratic fit of %s (%d, span %g)."
                             % (TRANSITIONS[row], n, span))
        x = keep.astype(np.float64)
        w = tot[keep]
        y = np.log10((t[row][keep] + 1.0) / w)
        pred = np.full(nq, np.nan)
        for x0 in range(int(keep[0]), int(keep[-1]) + 1):
            pred[x0] = _local_quadratic(x, y, w, float(x0), q)
        est[k] = 10.0 ** _carry_edges(pred)
    return expand_err(est)


def make_pacbio_errfun(base=loess_direct_errfun):
    """``PacBioErrfun`` (:183-196) over ``base`` where R has ``loessErrfun``: with a column for Q93, ``base`` on columns 0..92 and
    ``(trans[, 93] + 1) / (tot93 + 4)`` for Q93, ``tot93`` per source nucleotide; without one, R's message and ``base(trans)``."""
    def pacbio_errfun(trans):
        t = _counts(trans)
        if t.shape[1] >= 94:
            if t.shape[1] != 94:
                raise ValueError("Max qual score of 93 not the last column as expected.")
            err = base(t[:, :93])
            tot93 = np.repeat(t[:, 93].reshape(4, 4).sum(axis=1), 4)
            return np.concatenate([err, ((t[:, 93] + 1.0) / (tot93 + 4.0))[:, None]], axis=1)
        print("The max qual score of 93 was not detected. Using standard error fitting.", file=sys.stderr)
        return base(t)

    return pacbio_errfun


# ---- getErrors (:390-423) and the frame of plotErrors (R/plot-methods.R:61-113) ------------------------------------------------------
def _is_matrix(obj):
    return isinstance(obj, np.ndarray) and obj.ndim == 2 and obj.dtype.kind in "biuf"


def _as_dada(obj):
    """What ``api.dada`` returns, ``(result(s), err_out[, err_in])``, as R's dada-class fields; None if ``obj`` is not that."""
    if not isinstance(obj, tuple) or len(obj) not in (2, 3):
        return None
    res = obj[0]
    if isinstance(res, DadaResult):
        res = [res]
    if not (isinstance(res, list) and res and all(isinstance(r, DadaResult) for r in res)):
        return None
    return dict(err_out=obj[1], err_in=obj[2] if len(obj) == 3 else None, trans=api.accumulate_trans([r.subqual for r in res]))


def get_errors(obj, detailed=False, enforce=True):
    """``getErrors`` (:390-423).  ``obj``: an error matrix; a dict with ``err_out``, ``err_in`` and ``trans`` (what ``learn_errors``
    returns); what ``api.dada`` returns - ``(DadaResult or list of them, err_out[, err_in])``, R's dada-class object(s); or a list
    of those, which must share one ``err_out`` and whose counts are accumulated.  Returns ``err_out``, or with ``detailed`` the
    dict of the three (entries may be None).  ``enforce`` checks ``err_out`` with R's errors and R's warning for a zero."""
    rval = dict(err_out=None, err_in=None, trans=None)
    one = _as_dada(obj)
    if _is_matrix(obj):
        rval["err_out"] = obj
    elif one is not None:
        rval = one
    elif isinstance(obj, list) and obj and all(_as_dada(x) is not None for x in obj):
        each = [_as_dada(x) for x in obj]
        first = each[0]["err_out"]
        for e in each:
            same = (e["err_out"] is None and first is None) or (e["err_out"] is not None and first is not None
                                                                  and np.array_equal(e["err_out"], first, equal_nan=True))
            if not same:
                raise ValueError("If list of dada-class objects provided, all must have the same output error rates.")
        rval = dict(err_out=first, err_in=each[0]["err_in"], trans=api.accumulate_trans([e["trans"] for e in each]))
    elif isinstance(obj, dict) and all(k in obj for k in ("err_out", "err_in", "trans")):
        rval = obj
    if enforce:
        e = rval["err_out"]
        if e is None:
            raise ValueError("Error matrix is NULL.")
        if not (isinstance(e, np.ndarray) and e.dtype.kind in "biuf"):
            raise ValueError("Error matrix must be numeric.")
        if not (e.ndim == 2 and e.shape[0] == 16):
            raise ValueError("Error matrix must have 16 rows (A2A, A2C, ...).")
        if not np.all(e >= 0):
            raise ValueError("All error matrix entries must be >= 0.")
        if not np.all(e <= 1):
            raise ValueError("All error matrix entries must be <=1.")
        if np.any(e == 0):
            warnings.warn("Zero in error matrix.")
    return rval if detailed else rval["err_out"]


def errors_frame(obj, nominal_q=False):
    """The data frame ``plotErrors`` draws from (R/plot-methods.R:61-113) as a dict of numpy columns, one row per (quality,
    transition) in ``melt``'s order (transitions fastest): ``Transition, Qual, count, from, to, tot, Observed, Estimated, Input,
    Nominal``.  ``Input`` is the first matrix of ``err_in``.  The self-transition rows of count, tot, Observed, Estimated and
    Input are NaN, those of Nominal only under ``nominal_q``, as R blanks them.  Without counts the frame is built from
    ``err_out`` (R's column ``est``) and count, tot and Observed are NaN throughout."""
    one_col = "plotErrors only supported when using quality scores in the error model (i.e. USE_QUALS=TRUE)."
    dq = get_errors(obj, detailed=True, enforce=False)
    trans, err_out, err_in = dq["trans"], dq["err_out"], dq["err_in"]
    df = {}
    if trans is not None:
        trans = np.asarray(trans)
        if trans.shape[1] <= 1:
            raise ValueError(one_col)
        nq = trans.shape[1]
    elif err_out is not None:
        err_out = np.asarray(err_out)
        if err_out.shape[1] <= 1:
            raise ValueError(one_col)
        nq = err_out.shape[1]
    else:
        raise ValueError("Non-null observed and/or estimated error rates (dq$trans or dq$err_out) must be provided.")
    n = 16 * nq
    df["Transition"] = np.tile(np.array(TRANSITIONS), nq)
    df["Qual"] = np.repeat(np.arange(nq), 16)
    df["from"] = np.array([s[0] for s in df["Transition"]])
    df["to"] = np.array([s[2] for s in df["Transition"]])

    def lookup(mat):                                                # mapply(function(x, y) mat[x, y], Transition, Qual)
        mat = np.asarray(mat, dtype=np.float64)
        if mat.shape[0] != 16 or mat.shape[1] < nq:
            raise IndexError("subscript out of bounds")
        return mat[:, :nq].T.reshape(n).copy()

    if trans is not None:
        df["count"] = trans.astype(np.float64).T.reshape(n).copy()
        tot = trans.astype(np.float64).reshape(4, 4, nq).sum(axis=1)       # tapply(count, list(from, Qual), sum)
        df["tot"] = np.repeat(tot, 4, axis=0).T.reshape(n).copy()
        with np.errstate(divide="ignore", invalid="ignore"):
            df["Observed"] = df["count"] / df["tot"]
    else:
        df["est"] = lookup(err_out)
        df["count"] = np.full(n, np.nan)
        df["tot"] = np.full(n, np.nan)
        df["Observed"] = np.full(n, np.nan)
    df["Estimated"] = lookup(err_out) if err_out is not None else np.full(n, np.nan)
    if err_in is not None:
        df["Input"] = lookup(err_in[0] if isinstance(err_in, (list, tuple)) else err_in)
    else:
        df["Input"] = np.full(n, np.nan)
    is_self = df["from"] == df["to"]
    qual = df["Qual"].astype(np.float64)
    df["Nominal"] = (1.0 / 3.0) * 10.0 ** -(qual / 10.0)
    df["Nominal"][is_self] = 1.0 - 10.0 ** -(qual[is_self] / 10.0)
    for c in ("count", "tot", "Observed", "Estimated", "Input") + (("Nominal",) if nominal_q else ()):
        df[c][is_self] = np.nan
    order = ["Transition", "Qual", "count", "from", "to", "tot", "Observed", "Estimated", "Input", "Nominal"]
    return {c: df[c] for c in order + [c for c in df if c not in order]}


# ---- learnErrors (:333-363) ----------------------------------------------------------------------------------------------------------------
_FASTQ_PATTERNS = (".fastq.gz$", ".fastq.bz2$", ".fastq$")


def parse_fastq_directory(path, pattern=_FASTQ_PATTERNS):
    """``parseFastqDirectory`` (R/sequenceIO.R:332-360): the files of the first pattern (regular expressions, as ``list.files``
    takes them) that any file name matches, sorted; files of a later pattern are left out with R's warning."""
    if not os.path.isdir(path):
        raise ValueError("Provided path is not an existing directory.")
    names = sorted(os.listdir(path))
    fn, multi_ext = [], False
    for pat in pattern:
        foo = [f for f in names if re.search(pat, f)]
        if foo:
            if not fn:
                fn = foo
            else:
                multi_ext = True
    if not fn:
        raise ValueError("No files found in this directory with the expected extension(s): " + ", ".join(pattern))
    if multi_ext:
        warnings.warn("Multiple fastq-type file extensions detected in this directory. Only those with extensions appearing earliest "
                      "in the search list were kept: " + ", ".join(pattern))
    return [os.path.join(path, f) for f in fn]


class _FileDerep(api.NativeDerep):
    """``api.NativeDerep(path)`` as ``learn_errors`` makes it.  The library marks the positions past a read's end with R's NA, a
    signalling NaN, and ``numpy.nanmax`` takes that for a number on some hosts and answers NaN; here the largest quality is taken
    over the entries ``isnan`` leaves, a block of rows at a time."""

    def qmax(self) -> int:
        q = np.ctypeslib.as_array(_lib.lib().dada2hip_derep_quals(self._h), (self.nuniques, self.maxlen))
        best = -np.inf
        for r in range(0, self.nuniques, 4096):
            blk = q[r: r + 4096]
            ok = ~np.isnan(blk)
            if ok.any():
                best = max(best, float(blk[ok].max()))
        return int(np.ceil(best))


def _reads_and_bases(d):
    """``sum(uniques)`` and ``sum(uniques * nchar(names(uniques)))`` (:350-351)."""
    if isinstance(d, api.NativeDerep):
        L = _lib.lib()
        ab = np.ctypeslib.as_array(L.dada2hip_derep_abundances(d._h), (d.nuniques,)).astype(np.int64)
        sp = L.dada2hip_derep_seqs(d._h)
        lens = np.fromiter((len(sp[i]) for i in range(d.nuniques)), dtype=np.int64, count=d.nuniques)
    else:
        ab = np.asarray(d.abundances, dtype=np.int64)
        lens = np.fromiter((len(s) for s in d.seqs), dtype=np.int64, count=len(d.seqs))
    return int(ab.sum()), int((ab * lens).sum())


def learn_errors(fls, nbases=1e8, *, err_fun, nreads=None, randomize=False, MAX_CONSIST=10, OMEGA_C=0, qual_offset=0, opts=None,
                 verbose=False, device=0, keep_samples=False):
    """``learnErrors`` (:333-363) over resident samples.

    ``err_fun`` is required: R's default ``loessErrfun`` cannot be offered, and a silent substitute would be wrong.  ``fls``: a
    path, a list of paths, a directory (``parse_fastq_directory``), a ``Derep`` / ``NativeDerep`` or a list of them.  Paths are
    dereplicated one at a time with ``api.NativeDerep(path, qual_offset=qual_offset)``; objects are used as given.  After each
    sample its reads and bases are added, and the loop stops after the sample that makes the bases exceed ``nbases`` (strictly;
    that sample is used, later files are never opened).  ``nreads`` switches the test to reads and gives R's deprecation warning.

    ``randomize``: False keeps the order, True draws a permutation from a fresh ``numpy.random.default_rng()``, an int is its seed,
    a sequence is the permutation itself.  R's ``sample()`` stream cannot be reproduced, so no seed gives R's order.

    The options are ``dataclasses.replace(opts or DadaOpts(), MAX_CONSIST=MAX_CONSIST, OMEGA_C=OMEGA_C)``: the named arguments
    win.  The samples are made resident here and ``api.dada(dereps, None, self_consist=True, err_fun=err_fun, ...)`` runs on them.
    With ``keep_samples=False`` the samples, and the dereps made here from paths, are closed, also when the loop raises; with
    ``keep_samples=True`` they come back in ``info`` so that ``api.dada(info["dereps"], err_out, samples=info["samples"])`` does not
    upload again (the caller closes them).

    Returns ``{"err_out", "err_in", "trans", "info"}``: ``err_in`` the list of matrices tried (R's ``$err_in`` under selfConsist),
    ``trans`` the accumulated counts of the last pass, ``info`` with ``nbases, nreads, nsamples, passes, converged`` (false when
    the loop ended on ``MAX_CONSIST``, as R reports it), ``timings_ms`` and, when kept, ``dereps`` and ``samples``.  ``verbose``
    prints R's lines; 2 and above also turns on the library's own."""
    if err_fun is None or not callable(err_fun):
        raise TypeError("learn_errors needs err_fun: R's default loessErrfun is stats::loess and is not offered here; pass "
                        "make_binned_qual_errfun(...), loess_direct_errfun, make_pacbio_errfun() or noqual_errfun.")
    if nreads is not None:
        warnings.warn("The nreads parameter is DEPRECATED. Please update your code with the nbases parameter.")
    if isinstance(fls, (Derep, api.NativeDerep)):
        fls = [fls]
    elif isinstance(fls, (str, os.PathLike)):
        fls = [fls]
    else:
        fls = list(fls)
    if len(fls) == 1 and isinstance(fls[0], (str, os.PathLike)) and os.path.isdir(fls[0]):
        fls = parse_fastq_directory(os.fspath(fls[0]))
    if not fls:
        raise ValueError("learn_errors needs at least one sample.")
    if isinstance(randomize, (bool, np.bool_)):
        perm = np.random.default_rng().permutation(len(fls)) if randomize else None
    elif isinstance(randomize, (int, np.integer)):
        perm = np.random.default_rng(int(randomize)).permutation(len(fls))
    else:
        perm = np.asarray(list(randomize), dtype=np.int64)
        if not np.array_equal(np.sort(perm), np.arange(len(fls))):
            raise ValueError("randomize, given as a sequence, must be a permutation of range(len(fls)).")
    if perm is not None:
        fls = [fls[int(k)] for k in perm]
    o = dataclasses.replace(opts or DadaOpts(), MAX_CONSIST=MAX_CONSIST, OMEGA_C=OMEGA_C)

    dereps, made, samples = [], [], []
    done = False
    try:
        NBASES = NREADS = 0
        t0 = time.perf_counter()
        for f in fls:
            if isinstance(f, (Derep, api.NativeDerep)):
                d = f
            else:
                d = _FileDerep(os.fspath(f), qual_offset=qual_offset)
                made.append(d)
            dereps.append(d)
            r, b = _reads_and_bases(d)
            NREADS += r
            NBASES += b
            if (NBASES > nbases) if nreads is None else (NREADS > nreads):
                break
        if verbose:
            print(NBASES, "total bases in", NREADS, "reads from", len(dereps), "samples will be used for learning the error rates.")
        t1 = time.perf_counter()
        for d in dereps:
            samples.append(api.Sample.from_native(d, None, device) if isinstance(d, api.NativeDerep) else
                           api.Sample.from_derep(d, None, device))
        t2 = time.perf_counter()
        timings = []
        results, err_out, errs = api.dada(dereps, None, self_consist=True, err_fun=err_fun, opts=o, samples=samples, device=device,
                                          verbose=int(verbose) >= 2, timings=timings)
        passes = len(errs)                                          # R's nconsist where the loop ends (R/dada.R:391)
        converged = passes < o.MAX_CONSIST                          # R/dada.R:409
        if verbose:
            if converged:
                print("Convergence after ", passes, " rounds.")
            else:
                print("Self-consistency loop terminated before convergence.", file=sys.stderr)
        info = dict(nbases=NBASES, nreads=NREADS, nsamples=len(dereps), passes=passes, converged=converged,
                    timings_ms=dict(derep=(t1 - t0) * 1e3, upload=(t2 - t1) * 1e3, passes=timings[1:]))
        if keep_samples:
            info["dereps"], info["samples"] = dereps, samples
        done = True
        return dict(err_out=err_out, err_in=errs, trans=api.accumulate_trans([r.subqual for r in results]), info=info)
    finally:
        if not (done and keep_samples):
            for s in samples:
                s.close()
            for d in made:
                d.close()
