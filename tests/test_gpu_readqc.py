"""The read diagnostics on the MI355X (-m gpu): dada2hip_qprofile_* / dada2hip_complexity_* and dada2_amd.readqc against the
restatements of tests/readqc_cases.py (held to an independent count and to the R code's quirks in tests/test_readqc.py).  The
quality tables are compared cell by cell as integers, the statistics exactly; the windowed complexities have identical NaN
positions and differ from the restatement by at most 1e-12 relatively (at most 256 positive terms of at most 1/e summed in double
where R sums in long double: about 3e-14 on H <= ln 256, so about 2e-13 on exp(H)); window = None is api.seq_complexity bit for
bit.  The same cases run under the emulator (tests/test_emu_readqc.py).  The 70 000 reads run here only."""
import pytest

import readqc_cases as rc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rq():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from dada2_amd import readqc
    return readqc


@pytest.mark.parametrize("name", rc.CASE_NAMES)
def test_case_equals_the_restatement(rq, name):
    rc.CASES[name](rq)


def test_more_reads_than_one_blocks_slice(rq):
    rc.check_strided_table(rq)


def test_api_has_gained_nothing(rq):
    from dada2_amd import api
    assert not hasattr(api, "plot_complexity") and not hasattr(api, "quality_profile") and hasattr(rq, "complexity_profile")
