"""The resident form of the device dereplicator on the MI355X (-m gpu): dada2hip_derep_reads_resident and the fused
dada2hip_filter_derep_fastq_resident / _paired_resident through dada2_amd.dereplicate, against the route the library already
has - derep_reads / filter_and_derep -> Sample.from_native (tests/derep_resident_cases.py): the derep objects' fields, the
resident rows byte for byte with their padding, the runs field for field, the errors' class and text, the traffic condition.
The cases in memory also run under the emulator (tests/test_emu_derep_resident.py); the files through the filter run here only."""
import pytest

import derep_resident_cases as rc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dd():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from dada2_amd import dereplicate
    return dereplicate


@pytest.mark.parametrize("name", rc.CASE_NAMES)
def test_both_routes_leave_the_same_resident_sample(dd, name):
    rc.CASES[name](dd)


@pytest.mark.parametrize("byte", (0xFF, 0x5A))
def test_every_pad_byte_is_written_on_poisoned_memory(dd, byte):
    rc.run_poisoned(dd, byte)


@pytest.mark.parametrize("name", rc.FUSED_NAMES)
def test_filter_and_sample_equals_filter_and_derep_made_resident(dd, name):
    rc.FUSED_CASES[name](dd)
