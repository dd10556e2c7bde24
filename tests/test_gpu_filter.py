"""filterAndTrim on the MI355X (-m gpu): dada2hip_filter_open / _reads / _fastq / _fastq_paired against the restatement of
tests/filter_cases.py (pinned to the reference's C_matchRef and C_matrixEE on the CPU, in tests/test_filter.py).  Every case
compares every read: the stage code, the kept window, the two counts of the screen and the k-mer counts as integers, EE as
bit-equal doubles, written files as bytes; the complexity value at relative 1e-12.  The same cases run under the emulator
(tests/test_emu_filter.py).  The batch of 131 073 reads runs here only: three pieces of a call, and in each more reads than
k_filter_scan has waves (8 192) and k_filter_kmers blocks (16 384)."""
import pytest

import filter_cases as fc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def api():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from dada2_amd import api as a
    return a


@pytest.mark.parametrize("name", fc.CASE_NAMES)
def test_case_equals_the_restatement(api, name):
    fc.CASES[name](api)


@pytest.mark.parametrize("which", ("phix", "global"))
def test_batch_past_one_piece_and_one_sweep_of_the_grids(api, which):
    """The word table in LDS (the genome) and in global memory (a 9 000-nt random reference)."""
    fc.check_strided_batch(api, which)


def test_file_past_one_piece_and_one_sweep_of_the_grids(api, tmp_path):
    fc.check_strided_file(api, str(tmp_path))
