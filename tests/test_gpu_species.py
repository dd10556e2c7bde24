"""assignSpecies / addSpecies on the MI355X (-m gpu): dada2hip_species_open / _match against the restatement of
tests/species_cases.py (pinned to the reference's example data on the CPU, in tests/test_species.py).  Every case is exact
equality of the per-query lists of reference indices; the same cases run under the emulator (tests/test_emu_species.py).  One
more runs here only: 8 200 references, past the 8 192 that one sweep of k_species_seed's grid takes."""
import pytest

import species_cases as sc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def api():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from dada2_amd import api as a
    return a


@pytest.mark.parametrize("name", sc.CASE_NAMES)
def test_case_equals_the_restatement(api, name):
    sc.CASES[name](api)


def test_more_references_than_one_sweep_of_the_seed_grid(api):
    sc.check_strided(api)
