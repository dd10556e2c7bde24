"""removePrimers on the MI355X (-m gpu): dada2hip_primers_reads / _fastq and dada2_amd.primers against the restatement of
tests/primer_cases.py (pinned to the reference's example file in tests/test_primers.py).  Every case compares every read: the
code, the flip, first and last, the four hit counts and the eight starts as integers; written files as bytes.  The same cases run
under the emulator (tests/test_emu_primers.py).  The batch of 69 633 reads runs here only: two pieces of a call, and in each more
reads than k_primers has blocks (4 096)."""
import pytest

import primer_cases as pc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pr():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from dada2_amd import primers
    return primers


@pytest.mark.parametrize("name", pc.CASE_NAMES)
def test_case_equals_the_restatement(pr, name):
    pc.CASES[name](pr)


def test_batch_past_one_piece_and_one_sweep_of_the_grid(pr):
    pc.check_strided_batch(pr)


def test_api_does_not_export_it(pr):
    from dada2_amd import api
    assert not hasattr(api, "remove_primers") and hasattr(pr, "remove_primers")
