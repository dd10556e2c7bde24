"""Alignment-level parity of EVERY compiled aligner instance on the MI355X (-m gpu).

The aligner is some fifty separately compiled kernels chosen at launch from the sample's geometry and options (k_nw_ad by lanes
per alignment / EDGE / score mode / FAST, its bimera mode, k_nw_adw, the k_nw<WMAX> classes, k_nw_gen).  Each test here drives
one of them on purpose, checks every pair against the plain-C oracle (lambda bit-equal, hamming equal, whole results by
assert_results_equal) and asks the library's launch ledger (dada2hip_launch_ledger) which instance actually ran; the last test
fails naming any instance that never did.  The cases are tests/aligner_cases.py; nothing here reads the reference tree."""
import numpy as np
import pytest

import aligner_cases as A
from helpers import assert_results_equal, tperr1
from dada2_amd.io import Derep
from dada2_amd.opts import DadaOpts

pytestmark = pytest.mark.gpu

_SEEN = {"mask": 0, "tests": 0}          # the aligner instances the tests of this module asserted and ran, and how many tests did
CASES = A.aligner_cases()


@pytest.fixture(scope="module")
def api():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from dada2_amd import api as a
    return a


# ---- 1. the aligner sweep ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_aligner_sweep(api, oracle_c, case, monkeypatch):
    """Every unique of the case's sample against each of its centres, all of them through the aligner (the asserted nnw == N -
    skipped is what keeps this from silently testing the gapless path), pair by pair against the oracle; the ledger shows the
    expected instance and nothing else of the aligner families."""
    monkeypatch.delenv("DADA2HIP_NW_KERNEL", raising=False)
    npairs, got = A.run_case(api, oracle_c, case)
    assert npairs > 0
    _SEEN["mask"] |= got
    _SEEN["tests"] += 1


# ---- 2. the screen sweep ------------------------------------------------------------------------------------------------------------
SCREEN_SAMPLES = A.screen_samples()


@pytest.mark.parametrize("kw,cutoff", A.SCREEN_OPTIONS, ids=["-".join("%s=%s" % kv for kv in kw.items()) + "-cut%g" % c for kw, c in A.SCREEN_OPTIONS])
@pytest.mark.parametrize("sample", SCREEN_SAMPLES, ids=[s.name for s in SCREEN_SAMPLES])
def test_screen_sweep(api, oracle_c, sample, kw, cutoff, monkeypatch):
    """Samples of the table (plus reads at every k-mer distance), reads of 6-20 nt and low-complexity reads in which one 5-mer occurs
    more than 63 and more than 255 times, under every screen option: class by raw_align's rule from the oracle's kdist / kodist,
    lambda and hamming of every unique, the class counters of the stats."""
    monkeypatch.delenv("DADA2HIP_NW_KERNEL", raising=False)
    counts, at_cutoff = A.run_screen(api, oracle_c, sample, kw, cutoff)
    assert sum(counts) == len(sample.seqs) * len(sample.centres)
    # every class the option set is meant to produce occurred in this sample, and the exact cutoffs were hit exactly
    o = DadaOpts(**dict(dict(BAND_SIZE=sample.band), **kw)).normalised()
    want = [True, o.USE_KMERS, o.BAND_SIZE == 0 or (o.GAPLESS and o.USE_KMERS), o.BAND_SIZE != 0]
    assert [c > 0 for c in counts] == want, (sample.name, kw, cutoff, "skipped / shrouded / gapless / NW", counts)
    if o.USE_KMERS and cutoff in (0.5, 0.25):
        assert at_cutoff > 0, (sample.name, kw, cutoff, "no pair at a k-mer distance equal to the cutoff")


# ---- 3. the batch path: FAST and the per-partition-centre layout exist only inside a run -----------------------------------------------
BATCH_ROWS = [   # (band, maxlen - minlen, GL, EDGE)
    (16, 0, 21, 0), (19, 0, 21, 1), (24, 0, 32, 0), (30, 0, 32, 1), (32, 0, 64, 0), (62, 0, 64, 1), (32, 60, 64, 1)]


def batch_sample(band, diff, n=2500, L=150):
    """A seeded sample of a few thousand uniques with indels (both sides of the pointer-free pass), its length range pinned to
    [L - diff, L] by explicit uniques of the extreme lengths."""
    from dada2_amd.synth import make_sample
    seed = 7000 + 100 * band + diff
    d = make_sample(tperr1(), n, L=L, G=8, seed=seed, Lmin=(L - diff) if diff else None, indel_rate=1.5e-3 if diff else 0.0, chunk=4000)
    seqs, ab, quals = list(d.seqs), list(d.abundances), d.quals
    rng = np.random.default_rng(seed)
    extra = []
    if diff == 0:
        # equal lengths: reads with a deletion early and a base appended (the pass hands them over), a few per variant
        for k in range(60):
            s = seqs[k % 8]
            p = 5 + int(rng.integers(0, L - 20))
            extra.append(s[:p] + s[p + 1:] + "ACGT"[int(rng.integers(0, 4))])
    else:
        full = max(seqs, key=len)
        full = full + "".join("ACGT"[int(x)] for x in rng.integers(0, 4, size=L - len(full)))
        extra += [full, full[diff:], full[: L - diff], seqs[1][: L - diff]]
    extra = [s for s in dict.fromkeys(extra) if s not in set(seqs)]
    q = np.full((len(seqs) + len(extra), L), np.nan)
    q[: len(seqs), : quals.shape[1]] = quals
    for i, s in enumerate(extra):
        q[len(seqs) + i, : len(s)] = rng.integers(20, 41, size=len(s))
    seqs += extra
    ab += [1] * len(extra)
    lens = [len(s) for s in seqs]
    assert max(lens) == L and min(lens) == L - diff, (min(lens), max(lens))
    return Derep(seqs, np.array(ab, dtype=np.int32), q, np.zeros(0, dtype=np.int32))


@pytest.mark.parametrize("band,diff,gl,edge", BATCH_ROWS, ids=["b%d_d%d" % r[:2] for r in BATCH_ROWS])
def test_batch_path_fast_pass_and_full_kernel(api, oracle_c, band, diff, gl, edge, monkeypatch):
    monkeypatch.delenv("DADA2HIP_NW_KERNEL", raising=False)
    d = batch_sample(band, diff)
    o = DadaOpts(BAND_SIZE=band)
    A.read_ledger()
    got = api.dada_uniques(d.seqs, d.abundances, None, tperr1(), d.quals, o)
    ran = A.read_ledger() & ~A.GAPLESS_BITS
    want = oracle_c.dada_uniques(d.seqs, d.abundances, None, tperr1(), d.quals, o)
    assert_results_equal(got, want)
    assert ran == A.bit_ad(gl, edge, "fast") | A.bit_ad(gl, edge, "default"), A.describe(ran)
    assert got.stats["nnw_fast"] > 0 and got.stats["nnw_retry"] > 0, (got.stats["nnw_fast"], got.stats["nnw_retry"])
    _SEEN["mask"] |= ran
    _SEEN["tests"] += 1


# ---- 4. bimera mode ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_shift,diff,bit_default,bit_generic", A.LR_ROWS, ids=["ms%d_d%d" % r[:2] for r in A.LR_ROWS])
def test_bimera_mode_instances(api, oracle_c, max_shift, diff, bit_default, bit_generic, monkeypatch):
    """api.bimera_pairs on pair sets built to every window row of the aligner sweep (band = max_shift), default and user scores,
    one-off on / off, against the oracle: the LR instance of the row, or the lane kernel of class 129 past the kernel's last window."""
    monkeypatch.delenv("DADA2HIP_NW_KERNEL", raising=False)
    qs, ps = A.bimera_pair_set(max_shift, diff, seed=max_shift * 100 + diff)
    for sc in A.LR_SCORES:
        for one_off in (False, True):
            A.read_ledger()
            got = api.bimera_pairs(qs, ps, one_off, *sc, max_shift)
            ran = A.read_ledger() & ~A.GAPLESS_BITS
            want = oracle_c.bimera_pairs(qs, ps, one_off, *sc, max_shift)
            bad = np.nonzero((got != want).any(axis=1))[0]
            assert bad.size == 0, (sc, one_off, A.describe(ran), [(qs[i], ps[i], got[i].tolist(), want[i].tolist()) for i in bad[:3]])
            assert ran == (bit_default if sc == (5, -4, -8) else bit_generic), A.describe(ran)
            _SEEN["mask"] |= ran
    _SEEN["tests"] += 1


# ---- 4b. the lane aligners' scratch ring: a wave's second and third chunk in the slot it has used ------------------------------------
RING_CASES = A.ring_cases()


@pytest.mark.parametrize("case", RING_CASES, ids=[c.name for c in RING_CASES])
def test_lane_aligners_wrap_their_scratch_ring(api, oracle_c, case):
    """The lane case's sample grown past 512 uniques under DADA2HIP_NW_RING=4 (256 alignments per trip, the last chunk ragged):
    every unique against each centre, pair by pair against the oracle as the sweep does, three trips by
    dada2hip_nw_ring_trips, and bit for bit what the same compare gives with the knob unset.  What this covers is a reused slot's
    stale contents and the index of a later trip's results: dada2hip_sample_compare has ONE centre per launch and passes neither
    chunk_centre nor a view, so a per-chunk centre is not exercised here (the bimera test below and
    test_whole_path_on_the_lane_kernels_wraps_the_scratch_ring of tests/test_gpu_parity.py do that)."""
    npairs, got = A.run_ring_case(api, oracle_c, case)
    assert npairs > 2 * A.RING_MIN_WORK and got == case.expect


def test_bimera_pairs_on_the_lane_route_wrap_the_scratch_ring(api, oracle_c):
    """k_nw + k_bimera_lr under DADA2HIP_NW_KERNEL=lane and a ring of four waves: 600 pairs, each a chunk of its own with its
    own query (chunk_centre is read per chunk, a wave's 150 chunks land at their own slots), against the oracle as
    test_bimera_pair_quantities_match_the_reference[lane] does, and equal to the call with the knob unset; then
    api.table_bimera2 on a table whose chimeras have up to a hundred candidate parents (chunks of 64 live lanes that share the
    query chunk_centre names) against the oracle's flags.  These launches keep move strings and pass NO view: view_by_chunk is
    not reached here (k_bimera_lr reads the moves by work index) - tests/test_gpu_parity.py's ring test covers it."""
    assert A.run_ring_bimera(api, oracle_c) == 600


# ---- 5. completeness ----------------------------------------------------------------------------------------------------------------
def expected_instances():
    """Every instance the build holds and the dispatcher can reach, written out."""
    out = []
    for gl in (21, 32, 64):
        for edge in (0, 1):
            for mode in ("default", "generic", "homo", "fast"):
                out.append(A.bit_ad(gl, edge, mode))
            for generic in (0, 1):
                out.append(A.bit_lr(gl, edge, generic))
        for generic in (0, 1):
            out.append(A.bit_adw(gl, generic))
    for w in (33, 65, 129, 193, 257):
        out += [A.bit_nw(w, "plain"), A.bit_nw(w, "nonplain")]
    out.append(A.bit_gen())
    assert len(out) == 24 + 12 + 6 + 10 + 1
    return out


def test_every_aligner_instance_ran_on_this_gpu():
    """Reads what the aligner sweep, the batch-path and the bimera tests recorded - each of them asserted the instance it names
    before recording it.  It needs the module run as a whole, in file order: the message says how many of those tests ran."""
    names = A.instance_names()
    ntests = len(CASES) + len(BATCH_ROWS) + len(A.LR_ROWS)
    missing = [names[b] for b in expected_instances() if not _SEEN["mask"] & b]
    assert not missing, "%d of the module's %d instance tests ran before this one; never ran on this GPU: %s" % (
        _SEEN["tests"], ntests, ", ".join(missing))
