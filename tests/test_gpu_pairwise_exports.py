"""The pairwise alignment exports on the MI355X, per kernel instance (-m gpu): dada2hip_nwvec and dada2hip_nwalign (and with
them what dada2hip_merge_pairs aligns with) run the PAIR form of the lane kernels - k_nw<33|65|129|193|257, pair> and
k_nw_gen<pair>: a centre per work item, 64 unrelated pairs to a wave, the alignment handed back as a move string per pair that
the host turns into the two gapped strings.  The aligner sweep of tests/test_gpu_aligner_instances.py never names these six
and never looks at a move string.

Each test drives one of them on purpose with a batch of tests/pair_cases.py (W either side of every class boundary; 1, 63, 64,
65 and 257 pairs; ends-free, global and homopolymer-gap aligners; four score sets; strings of 2-5 nt; letters outside ACGT),
compares both strings of every pair with the plain-C oracle, checks what needs no oracle (equal lengths, no gap-gap column, the
degapped outputs are the inputs), aligns eight pairs of the batch alone as well, and asks the launch ledger which instance ran;
the last test names any of the six that never did.  Nothing here reads the reference tree."""
import pytest

import pair_cases as P

pytestmark = pytest.mark.gpu

_SEEN = {"mask": 0, "tests": 0}          # the pair instances the tests of this module asserted and ran, and how many tests did
VEC_CASES = P.vec_cases()
ALIGN_CASES = P.align_cases()


@pytest.fixture(scope="module")
def api():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from dada2_amd import api as a
    return a


@pytest.mark.parametrize("case", [c for c in VEC_CASES if not c.letters], ids=[c.name for c in VEC_CASES if not c.letters])
def test_nwvec_batches_per_pair_instance(api, oracle_c, case):
    """api.nwvec on the whole batch against cport.C_nwalign, pair by pair and string by string; the ledger shows the case's pair
    instance and nothing else; eight pairs of the batch alone through api.nwalign give what the batch gave."""
    ran = P.run_vec_case(api, oracle_c, case)
    _SEEN["mask"] |= ran
    _SEEN["tests"] += 1


@pytest.mark.parametrize("case", [c for c in VEC_CASES if c.letters], ids=[c.name for c in VEC_CASES if c.letters])
def test_nwvec_two_plane_letters_wider_than_a_wave(api, oracle_c, oracle_ref, case):
    """130 pairs with N and IUPAC codes (two 2-bit planes per string) against the reference's own C_nwvec call on raw bytes
    (the prebuilt oracle/_ref); always k_nw_gen<pair>."""
    ran = P.run_vec_case(api, oracle_c, case, ref=oracle_ref)
    _SEEN["mask"] |= ran


@pytest.mark.parametrize("case", ALIGN_CASES, ids=[c.name for c in ALIGN_CASES])
def test_nwalign_homopolymer_gaps_per_pair_instance(api, oracle_c, case):
    """api.nwalign with homopolymer gap penalties -1 and 0, one pair per call whose own W sits on a class boundary."""
    ran = P.run_align_case(api, oracle_c, case)
    _SEEN["mask"] |= ran
    _SEEN["tests"] += 1


RING_CASES = P.ring_vec_cases()


@pytest.mark.parametrize("case", RING_CASES, ids=[c.name for c in RING_CASES])
def test_nwvec_wraps_the_scratch_ring_per_pair_instance(api, oracle_c, case, request):
    """600 pairs under DADA2HIP_NW_RING=4 (256 pairs per trip: every wave of the launch goes back to the slot it has used, two
    of them twice, the last chunk ragged) against the oracle string by string, per pair instance, ends free and global, and
    the two-plane letters batch against the reference's own C_nwvec; dada2hip_nw_ring_trips shows three trips, and the same call
    with the knob unset gives the same strings in one."""
    ref = request.getfixturevalue("oracle_ref") if case.letters else None
    assert P.run_ring_vec_case(api, oracle_c, case, ref=ref) == case.expect


def test_nwvec_wraps_the_automatic_ring_on_unbanded_pairs_of_1500_nt(api, oracle_c):
    """No knob: 4 200 unbanded pairs of 1 400-1 500 nt (the full-length 16S sequence table).  ensure_scratch sizes the ring to 64
    waves there (4.6 GB of pointers), so waves 0 and 1 align a second chunk over their first; every item against the oracle's
    alignment of its pool pair (24 distinct pairs, items 4 096 apart differ), dada2hip_nw_ring_trips says 2.
    Measured once on the MI355X: 2.4 s the call, 2.6 s the test (k_nw_gen<pair> on 64 waves, every DP row through global scratch)."""
    trips, dt = P.run_long_batch(api, oracle_c)
    print("nwvec, %d unbanded pairs of 1 400-1 500 nt: %d trips, %.2f s" % (P.LONG_N, trips, dt))
    assert trips == 2


def test_every_pair_instance_ran_on_this_gpu():
    """Reads what the tests above recorded - each of them asserted the instance it names before recording it.  It needs the
    module run as a whole, in file order: the message says how many of those tests ran."""
    from aligner_cases import instance_names
    names = instance_names()
    ntests = len([c for c in VEC_CASES if not c.letters]) + len(ALIGN_CASES)
    missing = [names[b] for b in P.pair_instances() if not _SEEN["mask"] & b]
    assert not missing, "%d of the module's %d instance tests ran before this one; never ran on this GPU: %s" % (
        _SEEN["tests"], ntests, ", ".join(missing))
