"""The case table of tests/regime_cases.py itself (CPU): every case is seeded and reproducible, stays inside R's integer range,
and its facts hold on the oracle - i.e. the sample reaches the regime it is named after (more than 1 024 partitions with movers
into table-overflow partitions; tie lists of the intended length, born in scan order; E and reads in every arm of pgamma_lower,
candidates at OMEGA_A, the 32-bit wraps).  The -m gpu module and the emulated runs assert the same facts before comparing."""
import numpy as np
import pytest

import regime_cases as R
from helpers import derep_sha256


@pytest.mark.parametrize("name", list(R.CASES))
def test_case_is_seeded_reproducible_and_within_r_integer_range(name):
    fn, kw = R.CASES[name]
    a, b = fn(**kw), fn(**kw)
    assert derep_sha256(a[0]) == derep_sha256(b[0])
    assert (a[1] is None) == (b[1] is None) and (a[1] is None or np.array_equal(a[1], b[1])) and a[2] == b[2]
    d = a[0]
    assert int(d.abundances.astype(np.int64).sum()) <= R.INT_MAX and int(d.abundances.min()) >= 1
    assert len(set(d.seqs)) == d.nraw
    if "permuted" not in name:
        assert (np.diff(d.abundances.astype(np.int64)) <= 0).all()      # abundance order, as derepFastq leaves it


@pytest.mark.parametrize("name", [n for n in R.CASES if n not in R.GPU_ONLY])
def test_case_facts_hold_on_the_oracle(oracle_c, name):
    """(crowd_large - half a minute of oracle - has its facts asserted where it runs, in tests/test_gpu_regimes.py.)"""
    res = R.check_facts(name)
    d, pri, opts, facts = R.build(name)
    if name.startswith("crowd"):
        assert res.nclust > R.TAB and d.nraw < 2 * 4096
    if name.startswith("tied"):
        want = {"tied_65": (43, 65), "tied_300": (262, 300), "tied_4096": (4074, 4096), "tied_4100": (4078, 4100), "tied_4200": (4178, 4200), "tied_5000": (4994, 5000),
                "tied_two_groups_movers": (2, 300), "tied_4200_permuted": (4178, 4200), "tied_300_permuted": (262, 300)}[name]
        lens = facts["tie_lens"]
        assert min(n for n in lens if n > 1) == want[0] and max(lens) == want[1], (min(lens), max(lens))
    if name.startswith("deep"):
        assert facts["arms"] == [1, 2, 3, 4]


def test_the_tie_tiers_are_all_reached():
    """<= BUD_TIES inline, <= TIES_FULL full records on the device, beyond: index list + host rebuild (driver.cpp decide_bud) -
    and tied_4100 crosses from the third tier into the second inside one run."""
    tiers = set()
    for name in ("tied_65", "tied_300", "tied_4096", "tied_4100", "tied_4200", "tied_two_groups_movers"):
        d, pri, opts, facts = R.build(name)
        facts["tie_list_lengths"](None, None)
        t = {0 if n <= R.BUD_TIES else 1 if n <= R.TIES_FULL else 2 for n in facts["tie_lens"] if n > 1}
        tiers |= {(name, x) for x in t}
    assert {("tied_65", 1), ("tied_65", 0), ("tied_300", 1), ("tied_4096", 1), ("tied_4100", 2), ("tied_4100", 1), ("tied_4200", 2),
            ("tied_two_groups_movers", 0), ("tied_two_groups_movers", 1)} <= tiers
    assert ("tied_4200", 1) not in tiers and ("tied_4096", 2) not in tiers


def test_pgamma_arm_classifier_follows_ppois_h():
    """regime_cases.pgamma_arm restates the arm conditions of pgamma_lower (csrc/ppois.h, R's pgamma_raw) - spot values on each
    side of every boundary."""
    arm = R.pgamma_arm
    assert [arm(0.999, 5), arm(1.0, 5), arm(4.0, 5), arm(4.5, 5)] == [1, 2, 2, 3]
    assert [arm(840.0, 1000), arm(839.9, 1000), arm(999.0, 1000), arm(999.5, 1000), arm(1200.0, 1000), arm(1201.0, 1000)] == [4, 2, 4, 4, 4, 3]
    assert arm(0.0, 3) == 0
