"""The two host ends of the boundary call on the device (tests/host_ends_cases.py): marshalling in front, the final pass with its
pinned staging, single wait and pooled assembly behind the rounds; each case against the plain-C restatement and the goldens."""
import os

import pytest

import host_ends_cases as hc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", sorted(hc.CASES))
def test_host_ends_match_the_restatement_on_the_device(name):
    assert hc.run_case(name).startswith("ok ")


def test_host_ends_with_two_samples_in_flight_on_the_device():
    assert hc.run_multi().startswith("ok ")


@pytest.mark.parametrize("label", [k for k, _, _ in hc.INVALID])
def test_invalid_base_is_refused_on_the_device(label):
    assert hc.run_invalid(label).startswith("ok ")


# nw_kernel_launches of synth3000_default as the build BEFORE the final pass was re-queued reports it, measured on the device
# (profiles/r12c_profile_knob_launches.txt: four runs each way, alternating with this build on one box): 7 when every launch is
# event-timed - round 0, the batch compares and the final pass's one big aligner launch - and 2 when the times are sampled
# (n_round_launches + 1).  The two are NOT "equal, or one apart": the fully timed count includes the compares.  Both stayed put
# while the timing-dependent number of prefetch compares moved between 2 and 3.  The final pass records the same events as
# before, so this build must report the same two values.
PARENT_LAUNCHES_EVENT_TIMED = 7
PARENT_LAUNCHES_SAMPLED = 2


def test_fully_event_timed_run_still_times_every_launch_of_the_final_pass():
    from helpers import assert_results_equal, case_inputs
    from dada2_amd import api
    d, err, pri, opts, exp, meta = case_inputs("synth3000_default")
    plain = api.dada_uniques(d.seqs, d.abundances, pri, err, d.quals, opts)
    old = os.environ.get("DADA2HIP_PROFILE")
    os.environ["DADA2HIP_PROFILE"] = "1"
    try:
        prof = api.dada_uniques(d.seqs, d.abundances, pri, err, d.quals, opts)
    finally:
        if old is None:
            del os.environ["DADA2HIP_PROFILE"]
        else:
            os.environ["DADA2HIP_PROFILE"] = old
    assert_results_equal(prof, exp)
    assert_results_equal(plain, exp)
    ps, qs = prof.stats, plain.stats
    print("nw_kernel_launches", ps["nw_kernel_launches"], qs["nw_kernel_launches"], "dev_ms_final", ps["dev_ms_final"])
    assert set(ps) == set(qs)
    assert ps["kernel_times_sampled"] == 0 and qs["kernel_times_sampled"] == 1
    assert ps["dev_ms_final"] > 0 and ps["dev_ms_nw"] > 0 and ps["nw_kernel_ms"] > 0
    for k in ("nnw", "ngapless", "nshroud", "rounds", "ncompare"):
        assert ps[k] == qs[k], k
    assert int(ps["nw_kernel_launches"]) == PARENT_LAUNCHES_EVENT_TIMED, ps["nw_kernel_launches"]
    assert int(qs["nw_kernel_launches"]) == PARENT_LAUNCHES_SAMPLED, qs["nw_kernel_launches"]
