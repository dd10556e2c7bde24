"""One resident sample across changing options, errors and aborts on the MI355X (-m gpu), against tests/resident_cases.py.

dada2hip_sample_create once, then any number of runs, set_priors / set_prior_seqs calls and compares: the Run object, the round
engines' buffers, the aligner rings and the uploaded error matrix stay on the handle from one call to the next, and
every other parity test takes a fresh sample per case.  Here one handle walks through 22 option steps (forward, reversed - a buffer
that shrinks keeps the previous run's tail - and in one seeded shuffle), through the band steps on the two aligners that keep a
scratch ring, through error matrices of 41 and 94 columns, a learned one and a refused one, through prior flags set by flag and by
sequence, through compares between runs, through an abort at the 1st, 3rd and 8th round and through the device-raised "Bad
lambda." of round 0 and of a later round on every engine; two handles run interleaved, and a sample is built from the memory a
larger one has freed.  After every step the result is the oracle's on a fresh computation, work counters included; that the
steps of a walk differ from one another, that the flags change the reference's result and that the error inputs fail where they
must is asserted from the oracle alone before the library is asked."""
import pytest

import resident_cases as rc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def api(oracle_c):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from dada2_amd import api as a
    return a


@pytest.mark.parametrize("how", ["forward", "reversed", "shuffled"])
def test_option_walk_on_one_sample_equals_the_oracle_at_every_step(api, how):
    assert rc.case_option_walk(api, how) == len(rc.WALK) == 22


@pytest.mark.parametrize("how", ["forward", "reversed"])
@pytest.mark.parametrize("kernel", ["lane", "wide"])
def test_band_walk_resizes_the_scratch_rings_of_the_lane_and_wide_aligners(api, kernel, how):
    rc.case_band_walk(api, kernel, how)


def test_err_walk_41_columns_94_columns_inflated_learned_and_refused(api):
    rc.case_err_walk(api)


def test_priors_walk_by_flag_and_by_sequence_each_call_replaces_the_last(api, oracle_ref):
    rc.case_priors_walk(api)


def test_compare_between_runs_leaves_the_runs_alone(api):
    rc.case_compare_between_runs(api)


@pytest.mark.parametrize("env", rc.ENGINE_ENVS, ids=rc.ENGINE_IDS)
def test_aborted_sample_runs_again_with_other_options_and_with_defaults(api, env):
    rc.case_abort_then_run(api, env)


@pytest.mark.parametrize("env", rc.ENGINE_ENVS, ids=rc.ENGINE_IDS)
def test_bad_lambda_from_the_device_then_a_run_on_the_same_sample(api, env):
    """DADA2HIP_ERR_RUNTIME with the reference's own text (compute_lambda_ts, pval.cpp:194), from round 0 and from a later round."""
    rc.case_device_error_then_run(api, env)


def test_two_samples_alive_at_once_run_interleaved(api):
    rc.case_two_samples_interleaved(api)


@pytest.mark.parametrize("trim", [False, True], ids=["from-the-cache", "cache-trimmed"])
def test_sample_built_from_the_memory_a_larger_one_freed(api, trim):
    rc.case_memory_handed_on(api, trim)
