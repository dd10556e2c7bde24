"""orient.fwd, matchIDs, id.sep and id.field on the MI355X (-m gpu): dada2hip_filter_reads_oriented, dada2hip_filter_fastq_oriented
and dada2hip_filter_fastq_paired_ex against the restatement of tests/filter_orient_cases.py (pinned to hand-worked examples on the
CPU, in tests/test_filter_orient.py).  Every case compares every read: the stage code, the orientation, the kept window, the two
counts of the screen and the k-mer counts as integers, EE as bit-equal doubles, written files as bytes.  The same cases run under
the emulator (tests/test_emu_filter_orient.py); the batch of 131 073 reads runs here only: three pieces of a call, and in each
more reads than k_filter_orient and k_filter_scan have waves, so a wave takes several reads of different orientation."""
import pytest

import filter_orient_cases as oc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def flt():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return oc.flt()


@pytest.mark.parametrize("name", oc.CASE_NAMES)
def test_case_equals_the_restatement(flt, name):
    oc.CASES[name](flt)


def test_batch_past_one_piece_and_one_sweep_of_the_grids(flt):
    oc.check_big_batch(flt)
