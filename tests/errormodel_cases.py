"""learnErrors and the error-estimation functions (dada2_amd/errormodels.py; R/errorModels.R): restatements and the cases the
module is held to.  tests/test_errormodels.py runs the fits on the CPU; tests/test_gpu_learn_errors.py runs the loop on the device.

The restatements are written apart from the module, from the R text, in plain Python loops over doubles: ``restate_binned`` is
``makeBinnedQualErrfun`` (:96-156) with ``seq.default`` spelled out, ``exact_binned`` the same interpolation over
``fractions.Fraction``, ``mp_loess_log10`` the stated local-quadratic problem of ``loess_direct_errfun`` in 50-digit ``mpmath``.

The three runs: the golden pair sam1F / sam2F with every quality replaced by the largest of (7, 17, 27, 37) not above it and the
binned function; the same pair as it is with ``loess_direct_errfun``; samPB with ``make_pacbio_errfun()`` and ``BAND_SIZE=32``.
The transition counts the reference's loop (``pool_cases.restate_dada`` over ``oracle.ref.dada_uniques``) ends with in each are
recorded in tests/golden/errormodel_trans.npz (tests/golden/make_errormodel_golden.py), so the CPU tests need no reference; the
GPU tests run the loop itself against the live reference and check the recording on the way."""
import gzip
import os
from fractions import Fraction

import numpy as np

from helpers import GOLDEN, _same_float

BINS = (7, 17, 27, 37)
OFF = [r for r in range(16) if r % 5]
RUNS = ("binned", "loess", "pacbio")

# loess_direct_errfun against the 50-digit evaluation, largest |difference| of log10 rate over the three recorded matrices and the
# exactly quadratic one, as measured where the recording was made (numpy 2.2 on OpenBLAS); the tolerance is ten times that, the
# margin for another host's LAPACK (DESIGN.md §8k has both numbers).
LOESS_MEASURED = 2.7e-14
LOESS_TOL = 10 * LOESS_MEASURED


def recorded_trans(name):
    z = np.load(os.path.join(GOLDEN, "errormodel_trans.npz"))
    return z[name].astype(np.int64)


# ---- the binned files ------------------------------------------------------------------------------------------------------------------
def write_binned_copy(src, dst, bins=BINS, offset=33):
    """A gzip FASTQ copy of ``src`` with every quality replaced by the largest bin not above it."""
    table = bytearray(range(256))
    for c in range(offset, 256):
        below = [b for b in bins if b <= c - offset]
        assert below or c - offset < min(bins)
        if below:
            table[c] = max(below) + offset
    with gzip.open(src, "rb") as f:
        lines = f.read().split(b"\n")
    for i in range(3, len(lines), 4):
        assert min(lines[i]) - offset >= min(bins), "a quality below the lowest bin"
        lines[i] = lines[i].translate(bytes(table))
    with gzip.open(dst, "wb", compresslevel=1) as f:
        f.write(b"\n".join(lines))
    return dst


def binned_pair(tmp_dir):
    return [write_binned_copy(os.path.join(GOLDEN, n + ".fastq.gz"), os.path.join(str(tmp_dir), n + ".binned.fastq.gz"))
            for n in ("sam1F", "sam2F")]


def golden_paths(*names):
    return [os.path.join(GOLDEN, n + ".fastq.gz") for n in names]


def oracle_dereps(api, paths):
    """The files dereplicated by the library, as numpy Dereps for ``pool_cases.restate_dada``.  The library marks the positions
    past a read's end with R's NA, a signalling NaN, which ``numpy.nanmax`` (restate_dada's qmax) takes for a number on some hosts
    and answers NaN: here every NaN becomes the quiet one, nothing else changes."""
    from dada2_amd.io import Derep
    out = []
    for p in paths:
        d = api.derep_fastq(p)
        with np.errstate(invalid="ignore"):
            out.append(Derep(d.seqs, d.abundances, np.where(np.isnan(d.quals), np.nan, d.quals), d.map))
    return out


# ---- expand_err and makeBinnedQualErrfun, scalar ------------------------------------------------------------------------------------------
def restate_expand(est12):
    """R/errorModels.R:140-150 entry by entry; the column sum in np.longdouble (colSums' LDOUBLE), rounded once."""
    nq = len(est12[0])
    est = [[float(v) for v in row] for row in est12]
    for row in est:
        for k in range(nq):
            if row[k] > 0.25:
                row[k] = 0.25
            if row[k] < 1e-7:
                row[k] = 1e-7
    err = [[0.0] * nq for _ in range(16)]
    for i in range(4):
        mine = est[3 * i: 3 * i + 3]
        others = [j for j in range(4) if j != i]
        for k in range(nq):
            s = np.longdouble(0.0)
            for row in mine:
                s = s + np.longdouble(row[k])
            err[5 * i][k] = 1.0 - float(s)
            for j, row in zip(others, mine):
                err[4 * i + j][k] = row[k]
    return np.array(err, dtype=np.float64)


def r_seq(lo, hi, n):
    """seq.default(from, to, length.out = n): c(from, from + seq_len(n - 2) * ((to - from) / (n - 1)), to); rep(from, n) if equal."""
    if n <= 2:
        return [lo, hi][:n]
    if lo == hi:
        return [lo] * n
    by = (hi - lo) / (n - 1)
    return [lo] + [lo + k * by for k in range(1, n - 1)] + [hi]


def binned_segments(trans, bins, row):
    """[(loQ, hiQ, loP, hiP)] of the segments :120-129 uses for this transition; P as (errs, tot) integer pairs."""
    i = row // 4
    nq = len(trans[0])
    tot = [sum(int(trans[4 * i + j][k]) for j in range(4)) for k in range(nq)]
    out = []
    for lo, hi in zip(bins[:-1], bins[1:]):
        if hi < nq and tot[lo] > 0 and tot[hi] > 0:
            out.append((lo, hi, (int(trans[row][lo]), tot[lo]), (int(trans[row][hi]), tot[hi])))
    return out


def restate_binned_est(trans, bins):
    """The 12 x Q matrix ``est`` of :109-138, before the clamps."""
    nq = len(trans[0])
    est = []
    for row in OFF:
        pred = [None] * nq
        for lo, hi, (le, lt), (he, ht) in binned_segments(trans, bins, row):
            vals = r_seq(le / lt, he / ht, hi - lo + 1)
            for k, v in enumerate(vals):
                pred[lo + k] = v
        have = [k for k in range(nq) if pred[k] is not None]
        for k in range(nq):
            if k > have[-1]:
                pred[k] = pred[have[-1]]
            if k < have[0]:
                pred[k] = pred[have[0]]
        est.append(pred)
    return est


def restate_binned(trans, bins):
    return restate_expand(restate_binned_est(trans, bins))


def exact_binned(trans, bins, row):
    """{quality: (exact Fraction of the interpolation, Fraction of the larger endpoint as a double, is_endpoint)} inside segments."""
    out = {}
    for lo, hi, (le, lt), (he, ht) in binned_segments(trans, bins, row):
        a, b = Fraction(le / lt), Fraction(he / ht)            # the endpoints as the doubles R holds
        n = hi - lo + 1
        for k in range(n):
            out[lo + k] = (a + (b - a) * Fraction(k, n - 1) if n > 1 else a, max(a, b), k in (0, n - 1))
    return out


def ulp_of(x):
    return float(np.spacing(np.float64(x)))


# ---- matrices made for an edge ------------------------------------------------------------------------------------------------------------
def skipped_segment_matrix(seed=3):
    """16 x 41, qualities 7..37 seen at the bins only, but nothing read as a true G at Q27: for G the segments (17, 27) and
    (27, 37) are skipped, 18..41 carry the value at 17 - and for every transition columns 0..6 and 38..40 carry an edge."""
    rng = np.random.default_rng(seed)
    t = np.zeros((16, 41), dtype=np.int64)
    for q, scale in zip(BINS, (3000, 900, 200, 20)):
        for i in range(4):
            t[5 * i, q] = 400000 + int(rng.integers(0, 9999))
            for j in range(4):
                if j != i:
                    t[4 * i + j, q] = int(rng.integers(scale // 2, scale))
    t[8:12, 27] = 0
    return t


def clamped_matrix():
    """Rates above 0.25 at Q7 and below 1e-7 (zero errors among 10^8) at Q37, ordinary in between: both clamps, and interior
    points on either side of each."""
    t = np.zeros((16, 41), dtype=np.int64)
    for q, (self_n, err_n) in zip(BINS, ((10, 30), (100000, 300), (1000000, 40), (100000000, 0))):
        for i in range(4):
            t[5 * i, q] = self_n
            for j in range(4):
                if j != i:
                    t[4 * i + j, q] = err_n + j
    t[1, 37] = 0
    t[2, 37] = 0
    t[3, 37] = 0
    return t


def quadratic_log10(q, n):
    return -1.0 - 0.09 * q - 0.0005 * q * q + 0.1 * n


def quadratic_matrix():
    """16 x 41 real-valued "counts", qualities 5..38, whose rlogp = log10((errs + 1) / tot) is ``quadratic_log10(q, n)`` for the n-th
    rate of each nucleotide, up to the roundings of a product, a sum, a division and a logarithm (under 1e-15 in all): tot = 2^30
    in every seen column, errs + 1 = tot * 10^f(q).  A local quadratic fit reproduces a quadratic, whatever the weights."""
    t = np.zeros((16, 41), dtype=np.float64)
    tot = float(2 ** 30)
    for i in range(4):
        others = [j for j in range(4) if j != i]
        for q in range(5, 39):
            errs = [tot * 10.0 ** quadratic_log10(q, n) - 1.0 for n in range(3)]
            for j, e in zip(others, errs):
                t[4 * i + j, q] = e
            t[5 * i, q] = tot - sum(errs)
    return t


# ---- loess_direct_errfun's stated problem in mpmath ---------------------------------------------------------------------------------------
def _solve_fractions(G, y):
    """G c = y over Fractions, G square and non-singular (Gauss-Jordan with the first non-zero pivot)."""
    m = len(G)
    A = [list(G[r]) + [y[r]] for r in range(m)]
    for c in range(m):
        piv = next(r for r in range(c, m) if A[r][c] != 0)
        A[c], A[piv] = A[piv], A[c]
        A[c] = [v / A[c][c] for v in A[c]]
        for r in range(m):
            if r != c and A[r][c] != 0:
                A[r] = [v - A[r][c] * w for v, w in zip(A[r], A[c])]
    return [A[r][m] for r in range(m)]


def mp_loess_log10(trans, span=0.75, row=None):
    """{row: [log10 prediction per column, a Fraction]} of the problem ``loess_direct_errfun`` states, edges carried; before 10^
    and the clamps.  ``rlogp`` is taken from mpmath at 60 digits and held as a rational with 55 decimals; everything after it is
    rational - the tricube weight over h is (h^3 - d^3)^3 / h^9, and the common h^9 drops out of a weighted fit - so the
    intercept is exact in ``rlogp``: Cramer's rule on the 3 x 3 weighted normal equations, or, with fewer than three points
    under positive weight, the minimum-norm interpolant X^T (X X^T)^-1 y."""
    import mpmath as mp
    mp.mp.dps = 60
    scale = 10 ** 55
    nq = len(trans[0])
    out = {}
    for r in (OFF if row is None else [row]):
        i = r // 4
        tot = [sum(int(trans[4 * i + j][k]) for j in range(4)) for k in range(nq)]
        keep = [k for k in range(nq) if tot[k] > 0]
        n = len(keep)
        q = min(n, int(Fraction(n) * Fraction(span) + Fraction(1, 100000)))
        assert q >= 3
        y = [int(mp.floor(mp.log10(mp.mpf(int(trans[r][k]) + 1) / tot[k]) * scale)) for k in keep]
        pred = [None] * nq
        for x0 in range(keep[0], keep[-1] + 1):
            d = [abs(k - x0) for k in keep]
            h = sorted(d)[q - 1]
            pts = [(k - x0, yy, tot[k] * (h ** 3 - dd ** 3) ** 3) for k, yy, dd in zip(keep, y, d) if dd < h]
            if len(pts) >= 3:
                S = [sum(v * dx ** p for dx, _, v in pts) for p in range(5)]
                T = [sum(v * dx ** p * yy for dx, yy, v in pts) for p in range(3)]
                det = (S[0] * (S[2] * S[4] - S[3] * S[3]) - S[1] * (S[1] * S[4] - S[3] * S[2]) + S[2] * (S[1] * S[3] - S[2] * S[2]))
                num = (T[0] * (S[2] * S[4] - S[3] * S[3]) - S[1] * (T[1] * S[4] - S[3] * T[2]) + S[2] * (T[1] * S[3] - S[2] * T[2]))
                c0 = Fraction(num, det)
            else:
                X = [[Fraction(1), Fraction(dx), Fraction(dx * dx)] for dx, _, _ in pts]
                G = [[sum(a * b for a, b in zip(u, w)) for w in X] for u in X]
                lam = _solve_fractions(G, [Fraction(yy) for _, yy, _ in pts])
                c0 = sum(lam)                                     # the first column of X is ones
            pred[x0] = c0 / scale
        for k in range(nq):
            if k > keep[-1]:
                pred[k] = pred[keep[-1]]
            if k < keep[0]:
                pred[k] = pred[keep[0]]
        out[r] = pred
    return out


def loess_log10_difference(errfun, trans, span=0.75):
    """Largest |log10(rate of errfun) - (prediction of mp_loess_log10, clamped as the rate is)| over the 12 transitions and every
    column."""
    import mpmath as mp
    mp.mp.dps = 60
    got = errfun(np.array(trans), span)
    want = mp_loess_log10(trans, span)
    lo, hi = mp.log10(mp.mpf(1e-7)), mp.log10(mp.mpf(0.25))
    worst = 0.0
    for r in OFF:
        for k, p in enumerate(want[r]):
            p = min(max(mp.mpf(p.numerator) / p.denominator, lo), hi)
            worst = max(worst, float(abs(mp.log10(mp.mpf(float(got[r, k]))) - p)))
    return worst


# ---- the loop against the reference's ------------------------------------------------------------------------------------------------------
_REF = {}


def reference_loop(key, dereps, err_fun, opts):
    """``pool_cases.restate_dada(dereps, None, True, err_fun, opts)`` once per key: (results, err_out, errs, trans, passes, converged)."""
    if key not in _REF:
        import pool_cases as pc
        from dada2_amd import api
        res, err, errs = pc.restate_dada(dereps, None, True, err_fun, opts)
        for a in [err] + errs:
            a.setflags(write=False)
        _REF[key] = dict(results=res, err_out=err, err_in=errs, trans=api.accumulate_trans([r.subqual for r in res]),
                         passes=len(errs), converged=len(errs) < opts.MAX_CONSIST)
    return _REF[key]


def assert_learned_equals(got, want):
    """A ``learn_errors`` result against ``reference_loop``'s, bit for bit."""
    _same_float(got["err_out"], want["err_out"], 0)
    assert len(got["err_in"]) == len(want["err_in"])
    for a, b in zip(got["err_in"], want["err_in"]):
        _same_float(a, b, 0)
    assert np.array_equal(got["trans"], want["trans"])
    assert got["info"]["passes"] == want["passes"]
    assert got["info"]["converged"] == want["converged"]
