"""The error-estimation functions, get_errors and errors_frame of dada2_amd/errormodels.py on the CPU, against the restatements of
tests/errormodel_cases.py (plain loops over doubles, exact rationals, 50-digit mpmath).  No GPU, no reference at run time: the
transition counts of the three reference runs are the recording tests/golden/errormodel_trans.npz."""
import warnings
from fractions import Fraction

import numpy as np
import pytest

import errormodel_cases as ec
from dada2_amd import api, errormodels as em
from dada2_amd.opts import DadaResult
from helpers import _same_float


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


BINNED_MATRICES = {"run": lambda: ec.recorded_trans("binned"), "skipped": ec.skipped_segment_matrix, "clamped": ec.clamped_matrix}


# ---- the binned function -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(BINNED_MATRICES))
def test_binned_function_equals_the_scalar_restatement_bit_for_bit(name):
    t = BINNED_MATRICES[name]()
    got = em.make_binned_qual_errfun(ec.BINS)(t)
    want = ec.restate_binned(t.tolist(), list(ec.BINS))
    assert got.shape == want.shape == (16, t.shape[1]) and got.dtype == np.float64
    assert np.array_equal(_bits(got), _bits(want))
    est = np.array(ec.restate_binned_est(t.tolist(), list(ec.BINS)))
    if name == "skipped":                                          # G: both segments at Q27 skipped, 18.. carry the value at 17
        for k in (6, 7, 8):
            assert np.all(got[ec.OFF[k], 17:] == got[ec.OFF[k], 17]) and got[ec.OFF[k], 16] != got[ec.OFF[k], 17]
        assert np.all(got[1, :7] == got[1, 7]) and np.all(got[1, 38:] == got[1, 37]) and got[1, 36] != got[1, 37]
    if name == "clamped":
        assert (est > 0.25).any() and (est < 1e-7).any()
        assert (got[ec.OFF] == 0.25).any() and (got[ec.OFF] == 1e-7).any()
        assert got[ec.OFF].max() == 0.25 and got[ec.OFF].min() == 1e-7


@pytest.mark.parametrize("name", list(BINNED_MATRICES))
def test_binned_function_against_exact_rationals(name):
    """Endpoints exact; an unclamped interior value within 4 ulp of the exact interpolation, the ulp taken at the larger endpoint:
    the subtraction, the division, the product and the sum each round by at most half an ulp of a quantity no larger than that
    endpoint - 2 ulp, doubled as margin."""
    t = BINNED_MATRICES[name]()
    got = em.make_binned_qual_errfun(ec.BINS)(t)
    interior = 0
    for row in ec.OFF:
        for q, (exact, larger, is_end) in ec.exact_binned(t.tolist(), list(ec.BINS), row).items():
            if not (Fraction(1e-7) <= exact <= Fraction(0.25)):
                continue
            v = float(got[row, q])
            if is_end:
                if 1e-7 <= float(exact) <= 0.25:
                    assert Fraction(v) == exact, (row, q)
            elif 1e-7 < v < 0.25:
                interior += 1
                ulp = ec.ulp_of(float(larger))
                off = abs(Fraction(v) - exact) / Fraction(ulp)
                assert off <= 4, (row, q, float(off))
    assert interior > 100


def test_binned_function_errors_and_warnings():
    with pytest.raises(ValueError, match="The quality scores used in your data must be provided."):
        em.make_binned_qual_errfun(None)
    t = ec.recorded_trans("binned")
    with pytest.raises(ValueError, match="Input data contains a higher quality score than the provided binned values."):
        em.make_binned_qual_errfun((7, 17, 27))(t)
    with pytest.raises(ValueError, match="Input data contains a lower quality score than the provided binned values."):
        em.make_binned_qual_errfun((17, 27, 37))(t)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        em.make_binned_qual_errfun(ec.BINS)(t)                     # consistent data: silent
    with pytest.warns(UserWarning, match="Maximum observed quality score is not in the provided binned values."):
        em.make_binned_qual_errfun((7, 17, 27, 36, 40))(t)
    with pytest.warns(UserWarning, match="Minimum observed quality score is not in the provided binned values."):
        em.make_binned_qual_errfun((2, 8, 17, 27, 37))(t)
    lone = np.zeros((16, 41), dtype=np.int64)
    lone[:, 17] = 5                                                # one observed bin: no segment has both ends
    with pytest.raises(ValueError, match="error rates cannot be interpolated"):
        em.make_binned_qual_errfun(ec.BINS)(lone)


# ---- expand_err --------------------------------------------------------------------------------------------------------------------------
def _triple_where_the_sums_differ():
    """(a, b, c) in [1e-7, 0.25] with float64(longdouble a + b + c) != (a + b) + c in double, found by a seeded search."""
    rng = np.random.default_rng(11)
    for _ in range(10000):
        a, b, c = (float(x) for x in rng.uniform(1e-7, 0.25, size=3))
        wide = float(np.longdouble(a) + np.longdouble(b) + np.longdouble(c))
        if wide != (a + b) + c:
            return a, b, c, wide
    raise AssertionError("no such triple among 10 000 draws")


def test_expand_err_sums_in_long_double_and_clamps():
    rng = np.random.default_rng(2)
    est = rng.uniform(0.0, 0.3, size=(12, 50))
    est[:, :5] = rng.uniform(0.0, 2e-7, size=(12, 5))
    got = em.expand_err(est)
    assert np.array_equal(_bits(got), _bits(ec.restate_expand(est.tolist())))
    cl = np.clip(est, 1e-7, 0.25)
    assert np.array_equal(got[ec.OFF], cl)
    for i in range(4):
        wide = (cl[3 * i].astype(np.longdouble) + cl[3 * i + 1].astype(np.longdouble)) + cl[3 * i + 2].astype(np.longdouble)
        assert np.array_equal(got[5 * i], 1.0 - wide.astype(np.float64))
    assert est.max() > 0.25 and est.min() < 1e-7                   # and the input was left alone
    with pytest.raises(ValueError):
        em.expand_err(np.zeros((16, 3)))


def test_expand_err_differs_from_the_double_sum_by_an_ulp_where_it_should():
    if np.finfo(np.longdouble).nmant <= np.finfo(np.float64).nmant:
        pytest.skip("this host's long double is no wider than double: the sums cannot differ")
    a, b, c, wide = _triple_where_the_sums_differ()
    est = np.full((12, 1), 0.01)
    est[0:3, 0] = (a, b, c)
    got = em.expand_err(est)
    narrow = (a + b) + c
    assert abs(wide - narrow) == ec.ulp_of(min(wide, narrow))
    assert got[0, 0] == 1.0 - wide
    assert wide != narrow


def test_noqual_errfun_is_the_api_object():
    assert em.noqual_errfun is api.noqual_errfun


# ---- the direct local-quadratic fit ------------------------------------------------------------------------------------------------------
def test_loess_direct_errfun_against_mpmath_at_50_digits(capsys):
    """The tolerance is ten times the difference measured where the recording was made (errormodel_cases.LOESS_MEASURED), the
    margin for another host's LAPACK; the figure of THIS host is printed before it is judged."""
    pytest.importorskip("mpmath")
    worst = {}
    for run in ec.RUNS:
        t = ec.recorded_trans(run)
        worst[run] = ec.loess_log10_difference(em.loess_direct_errfun, t[:, :93].tolist() if run == "pacbio" else t.tolist())
    with capsys.disabled():
        print("\nloess_direct_errfun vs mpmath, largest |d log10 rate|:", {k: "%.3g" % v for k, v in worst.items()},
              "tolerance %.3g" % ec.LOESS_TOL)
    assert max(worst.values()) <= ec.LOESS_TOL, worst


def test_loess_direct_errfun_reproduces_a_quadratic():
    t = ec.quadratic_matrix()
    got = em.loess_direct_errfun(t)
    for i in range(4):
        others = [j for j in range(4) if j != i]
        for n, j in enumerate(others):
            want = np.array([ec.quadratic_log10(q, n) for q in range(5, 39)])
            assert np.max(np.abs(np.log10(got[4 * i + j, 5:39]) - want)) <= ec.LOESS_TOL
            assert np.all(got[4 * i + j, :5] == got[4 * i + j, 5]) and np.all(got[4 * i + j, 39:] == got[4 * i + j, 38])


def test_loess_direct_errfun_edges_gaps_and_too_few_points():
    t = ec.recorded_trans("loess").copy()
    seen = np.flatnonzero(t.sum(axis=0) > 0)
    lo, hi = int(seen[0]), int(seen[-1])
    assert lo > 0 and hi < t.shape[1] - 1
    gap = (lo + hi) // 2
    t[:, gap] = 0                                                  # a column without observations inside the range
    got = em.loess_direct_errfun(t)
    assert got.shape == t.shape and np.isfinite(got).all()
    want = ec.mp_loess_log10(t.tolist(), row=1)[1]
    assert abs(np.log10(got[1, gap]) - float(want[gap])) <= ec.LOESS_TOL      # predicted, not carried
    assert got[1, gap] != got[1, gap - 1] and got[1, gap] != got[1, gap + 1]
    for r in ec.OFF:
        assert np.all(got[r, :lo] == got[r, lo]) and np.all(got[r, hi + 1:] == got[r, hi])
    few = np.zeros((16, 41), dtype=np.int64)
    few[:, [10, 20, 30]] = 7                                       # n = 3: q = floor(2.25) = 2
    with pytest.raises(ValueError, match="Too few quality scores"):
        em.loess_direct_errfun(few)
    few[:, 35] = 7                                                 # n = 4: q = 3, local fits over two or three points
    assert np.isfinite(em.loess_direct_errfun(few)).all()
    worst = ec.loess_log10_difference(em.loess_direct_errfun, few.tolist())
    assert worst <= ec.LOESS_TOL, worst


# ---- PacBio -------------------------------------------------------------------------------------------------------------------------------
def test_pacbio_errfun_q93_column_and_fall_through(capsys):
    t = ec.recorded_trans("pacbio")
    assert t.shape == (16, 94) and t[:, 93].sum() > 0
    calls = []

    def base(m):
        calls.append(np.array(m))
        return em.noqual_errfun(m)

    got = em.make_pacbio_errfun(base)(t)
    assert got.shape == (16, 94) and len(calls) == 1 and np.array_equal(calls[0], t[:, :93])
    assert np.array_equal(got[:, :93], em.noqual_errfun(t[:, :93]))
    for r in range(16):
        tot = sum(int(t[4 * (r // 4) + j, 93]) for j in range(4))
        assert got[r, 93] == (int(t[r, 93]) + 1) / (tot + 4)
    _same_float(em.make_pacbio_errfun()(t)[:, :93], em.loess_direct_errfun(t[:, :93]), 0)      # the default base
    with pytest.raises(ValueError, match="Max qual score of 93 not the last column as expected."):
        em.make_pacbio_errfun(base)(np.concatenate([t, t[:, :1]], axis=1))
    capsys.readouterr()
    short = ec.recorded_trans("loess")
    assert np.array_equal(em.make_pacbio_errfun(base)(short), em.noqual_errfun(short))
    assert "The max qual score of 93 was not detected. Using standard error fitting." in capsys.readouterr().err


# ---- get_errors / errors_frame -------------------------------------------------------------------------------------------------------------
def _result(subqual):
    return DadaResult({"sequence": []}, {}, np.asarray(subqual), np.zeros((0, 0)), np.zeros(0, np.int32), np.zeros(0))


def test_get_errors_accepts_what_r_accepts():
    err = em.noqual_errfun(ec.recorded_trans("loess"))
    assert em.get_errors(err) is err
    t1, t2 = ec.recorded_trans("loess"), ec.recorded_trans("pacbio")
    learned = dict(err_out=err, err_in=[err, err], trans=t1, info={})
    assert em.get_errors(learned) is err and em.get_errors(learned, detailed=True) is learned
    one = em.get_errors((_result(t1), err, [err * 1.0]), detailed=True)
    assert one["err_out"] is err and np.array_equal(one["trans"], t1) and len(one["err_in"]) == 1
    pair = em.get_errors(([_result(t1), _result(t2)], err), detailed=True)          # what api.dada returns for two samples
    assert pair["err_in"] is None and np.array_equal(pair["trans"], api.accumulate_trans([t1, t2]))
    both = em.get_errors([(_result(t1), err), (_result(t2), err.copy())], detailed=True)
    assert np.array_equal(both["trans"], pair["trans"]) and both["err_out"] is err
    with pytest.raises(ValueError, match="If list of dada-class objects provided, all must have the same output error rates."):
        em.get_errors([(_result(t1), err), (_result(t2), err * 0.5)])
    assert em.get_errors("nothing R knows", enforce=False) is None


def test_get_errors_validity_errors_and_the_zero_warning():
    ok = np.full((16, 3), 0.25)
    for bad, text in ((None, "Error matrix is NULL."), (np.array([["a"] * 3] * 16), "Error matrix must be numeric."),
                      (np.full((12, 3), 0.25), r"Error matrix must have 16 rows \(A2A, A2C, ...\)."),
                      (ok - 0.3, "All error matrix entries must be >= 0."), (ok + 0.8, "All error matrix entries must be <=1.")):
        with pytest.raises(ValueError, match=text):
            em.get_errors(dict(err_out=bad, err_in=None, trans=None))
        assert em.get_errors(dict(err_out=bad, err_in=None, trans=None), enforce=False) is bad
    zero = ok.copy()
    zero[3, 1] = 0.0
    with pytest.warns(UserWarning, match="Zero in error matrix."):
        assert em.get_errors(zero) is zero
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        em.get_errors(ok)


def test_errors_frame_on_a_hand_written_example():
    #                 Q0   Q1   Q2
    trans = np.array([[90, 180, 0],      # A2A
                      [5, 10, 0],        # A2C
                      [3, 6, 0],         # A2G
                      [2, 4, 0],         # A2T
                      [1, 0, 0],         # C2A
                      [97, 50, 0],       # C2C
                      [1, 0, 0],         # C2G
                      [1, 0, 0],         # C2T
                      [4, 4, 4],         # G2A
                      [4, 4, 4],         # G2C
                      [88, 88, 88],      # G2G
                      [4, 4, 4],         # G2T
                      [0, 7, 1],         # T2A
                      [0, 7, 1],         # T2C
                      [0, 7, 1],         # T2G
                      [0, 79, 7]])       # T2T
    err_out = np.arange(48, dtype=np.float64).reshape(16, 3) / 100.0
    err_first, err_second = err_out + 0.25, err_out + 0.5
    df = em.errors_frame(dict(err_out=err_out, err_in=[err_first, err_second], trans=trans))
    assert list(df) == ["Transition", "Qual", "count", "from", "to", "tot", "Observed", "Estimated", "Input", "Nominal"]
    assert all(len(v) == 48 for v in df.values())
    assert list(df["Transition"][:3]) == ["A2A", "A2C", "A2G"] and list(df["Qual"][:17]) == [0] * 16 + [1]
    tots = {"A": (100, 200, 0), "C": (100, 50, 0), "G": (100, 100, 100), "T": (0, 100, 10)}
    for r in range(48):
        t, q = r % 16, r // 16
        name = em.TRANSITIONS[t]
        assert df["Transition"][r] == name and df["Qual"][r] == q and df["from"][r] == name[0] and df["to"][r] == name[2]
        if name[0] == name[2]:
            for c in ("count", "tot", "Observed", "Estimated", "Input"):
                assert np.isnan(df[c][r]), (c, r)
            assert df["Nominal"][r] == 1 - 10 ** -(q / 10)
        else:
            tot = tots[name[0]][q]
            assert df["count"][r] == trans[t, q] and df["tot"][r] == tot
            if tot:
                assert df["Observed"][r] == trans[t, q] / tot
            else:
                assert np.isnan(df["Observed"][r])
            assert df["Estimated"][r] == err_out[t, q] and df["Input"][r] == err_first[t, q]
            assert df["Nominal"][r] == (1 / 3) * 10 ** -(q / 10)
    assert df["Observed"][1] == 0.05 and df["Observed"][16 + 12] == 0.07 and df["Observed"][32 + 12] == 0.1
    blank = em.errors_frame(dict(err_out=err_out, err_in=None, trans=trans), nominal_q=True)
    assert np.isnan(blank["Nominal"][[0, 5, 10, 15]]).all() and not np.isnan(blank["Nominal"][1])
    assert np.isnan(blank["Input"]).all()
    only = em.errors_frame(err_out)                                # a bare matrix: R's column est, nothing observed
    assert np.isnan(only["count"]).all() and np.isnan(only["Observed"]).all() and only["est"][1] == err_out[1, 0]
    assert only["Estimated"][1] == err_out[1, 0] and np.isnan(only["Estimated"][0])
    text = r"plotErrors only supported when using quality scores in the error model \(i.e. USE_QUALS=TRUE\)."
    with pytest.raises(ValueError, match=text):
        em.errors_frame(dict(err_out=err_out, err_in=None, trans=trans[:, :1]))
    with pytest.raises(ValueError, match=text):
        em.errors_frame(err_out[:, :1])
    with pytest.raises(ValueError, match="Non-null observed and/or estimated error rates"):
        em.errors_frame(dict(err_out=None, err_in=None, trans=None))


# ---- the parts of learn_errors that run before any device work ------------------------------------------------------------------------------
def test_parse_fastq_directory_follows_the_reference(tmp_path):
    with pytest.raises(ValueError, match="Provided path is not an existing directory."):
        em.parse_fastq_directory(str(tmp_path / "missing"))
    with pytest.raises(ValueError, match="No files found in this directory with the expected extension"):
        em.parse_fastq_directory(str(tmp_path))
    for n in ("b.fastq", "a.fastq", "notes.txt"):
        (tmp_path / n).write_text("")
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert em.parse_fastq_directory(str(tmp_path)) == [str(tmp_path / "a.fastq"), str(tmp_path / "b.fastq")]
    (tmp_path / "c.fastq.gz").write_text("")
    with pytest.warns(UserWarning, match="Multiple fastq-type file extensions detected in this directory."):
        assert em.parse_fastq_directory(str(tmp_path)) == [str(tmp_path / "c.fastq.gz")]


def test_learn_errors_refuses_a_missing_err_fun_and_a_bad_permutation():
    with pytest.raises(TypeError):
        em.learn_errors(["a.fastq"])
    with pytest.raises(TypeError, match="err_fun"):
        em.learn_errors(["a.fastq"], err_fun=None)
    with pytest.raises(ValueError, match="permutation"):
        em.learn_errors(["a.fastq", "b.fastq"], err_fun=em.noqual_errfun, randomize=[0, 0])
