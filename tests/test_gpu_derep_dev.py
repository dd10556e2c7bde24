"""The device dereplicator on the MI355X (-m gpu): dada2hip_derep_reads and the fused dada2hip_filter_derep_fastq / _paired through
dada2_amd.dereplicate, against oracle.derep.derep_from_reads and the host's dada2hip_derep_fastq (tests/derep_dev_cases.py: the
comparison is exact in every field, the quality matrix bit for bit).  Cases 1-9 also run under the emulator
(tests/test_emu_derep_dev.py); the 70 000 reads and the files through the filter run here only."""
import pytest

import derep_dev_cases as dc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dd():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from dada2_amd import dereplicate
    return dereplicate


@pytest.mark.parametrize("name", dc.CASE_NAMES)
def test_reads_in_memory_equal_the_oracle_and_the_host(dd, name):
    dc.CASES[name](dd)


def test_more_than_one_default_piece(dd):
    dc.check_two_default_pieces(dd)


@pytest.mark.parametrize("name", dc.FUSED_NAMES)
def test_filter_and_derep_equals_the_two_steps(dd, name):
    dc.FUSED_CASES[name](dd)


def test_api_has_gained_nothing(dd):
    from dada2_amd import api
    assert not hasattr(api, "derep_reads") and not hasattr(api, "filter_and_derep") and hasattr(dd, "filter_and_derep")
