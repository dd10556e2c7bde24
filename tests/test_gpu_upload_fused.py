"""The boundary call's fused upload on the device (tests/upload_fused_cases.py): one pass over the rows with the chunks' copies
queued from inside it on two streams, input errors raised behind the pass, and no host wait between create and run; each case
with a chunk of 512 rows and with the automatic chunk, against the plain-C restatement."""
import pytest

import upload_fused_cases as uc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", sorted(uc.SHAPES))
def test_upload_shapes_match_the_restatement_on_the_device(name):
    assert uc.run_shape(name).startswith("ok ")


@pytest.mark.parametrize("name", sorted(uc.ERRORS))
def test_input_errors_keep_their_message_and_order_on_the_device(name):
    assert uc.run_error(name).startswith("ok ")


def test_boundary_call_equals_the_resident_sample_on_the_device():
    assert uc.run_boundary_equals_resident().startswith("ok ")


def test_two_samples_in_flight_equal_their_single_calls_on_the_device():
    assert uc.run_multi_equals_single().startswith("ok ")


def test_chunks_and_kmer_launches_are_what_the_rows_allow_on_the_device(capfd):
    """The knob makes the chunks it says, and a chunk with a row outside the stated geometry gets no k-mer launch, nor does any
    chunk behind it (the library's DADA2HIP_V2_SUMMARY line of every upload, read from stderr)."""
    capfd.readouterr()
    assert uc.run_chunk_cases().startswith("ok ")
    err = capfd.readouterr().err
    assert uc.upload_lines(err) == uc.EXPECTED_UPLOAD_LINES, err[-4000:]


@pytest.mark.parametrize("name", sorted(uc.WORKLIST_CASES))
def test_final_worklist_is_built_on_the_device(name):
    assert uc.run_worklist(name).startswith("ok ")
