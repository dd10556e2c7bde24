"""mergeSequenceTables on the MI355X (-m gpu): dada2hip_seqtab_merge through dada2_amd.seqtables against the specification of
tests/seqtab_cases.py - the whole result (matrix, sequences, sample names) and the column map, exactly.  The cases also run under
the emulator in their lighter form (tests/test_emu_seqtables.py); the 40 tables of 5 000 columns run here only."""
import pytest

import seqtab_cases as sc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def st():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from dada2_amd import seqtables
    return seqtables


@pytest.mark.parametrize("name", sc.CASE_NAMES)
def test_merge_equals_the_specification(st, name):
    sc.CASES[name](st)


def test_forty_tables_of_five_thousand_columns(st):
    sc.check_large(st)
