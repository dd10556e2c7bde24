"""Two of BASELINE.json's workloads at the depth bench.py times them, every output against a recording of the reference
(tests/golden/depth_*.expected.npz, written by tests/golden/make_depth_goldens.py on the host where oracle/_ref is built; the
reference never runs here):

  configs[4]  bench.py --config 5: 200 000 uniques of 1 450-1 510 nt, BAND_SIZE 32, no MAX_CLUST - all 128 partitions.  The
              indel-heavy long reads switch the aligner's pointer-free first pass off early in the run.  With whole batches
              aligned ahead, prefetch compares run on the second stream meanwhile: the regime in which a switch read
              separately by each launch of a compare could leave pairs unaligned.  Run with the default knobs and with engine
              variants that interleave the compares differently.
  configs[2]  bench.py --selfconsist: the learnErrors loop on the 1 000 000-unique headline sample, every pass (the all-ones
              MAX_CLUST 1 start, the half-converged passes with store growth), the pass count, convergence and err_out.

The inputs are drawn as bench.py draws them, through its input cache (at_size._inputs); a recording names the sha256 of the
input it was made from, so a generator drift fails as such and not as a parity failure."""
import numpy as np
import pytest

from helpers import assert_matches_recording, derep_sha256, load_recording
from dada2_amd.opts import DadaOpts

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def api():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from dada2_amd import api as a
    return a


def _drawn(case, rec):
    import at_size
    dereps, err = at_size._inputs(case)
    d = dereps[0]
    assert derep_sha256(d) == rec["meta"]["input_sha256"], \
        f"the sample bench.py draws for {case} is not the one recorded: the generator changed, rerun make_depth_goldens.py"
    return d, err


@pytest.fixture(scope="module")
def long_reads():
    rec = load_recording("cfg5")
    d, err = _drawn("cfg5", rec)
    assert np.array_equal(err, rec["passes"][0]["err"])
    return d, err, rec


# (knobs, pointer-free pass expected on, prefetch compares expected).  By default long reads are aligned at their round's
# commit, and then no compare runs on the second stream (driver.cpp v3_setup); aligning whole batches ahead puts prefetch
# compares beside the main stream's: alone, with the fewest batch buffers the overlap takes (main-stream misses beside
# prefetches) and with prefetches planned at the newest batch position.  Then the pass off from the start, and the compares on
# one stream only.
LONG_READ_VARIANTS = [
    ({}, True, False),
    ({"DADA2HIP_V2_ALIGN": "batch"}, True, True),
    ({"DADA2HIP_V2_ALIGN": "batch", "DADA2HIP_V2_NBUF": "4"}, True, True),
    ({"DADA2HIP_V2_ALIGN": "batch", "DADA2HIP_V3_PF_EARLY": "0"}, True, True),
    ({"DADA2HIP_V2_ALIGN": "batch", "DADA2HIP_AD_FAST": "0"}, False, True),
    ({"DADA2HIP_V2_ALIGN": "batch", "DADA2HIP_V3_OVERLAP": "0"}, True, False),
]


@pytest.mark.parametrize("env,fast,prefetch", LONG_READ_VARIANTS,
                         ids=["default", "align_batch", "align_batch_nbuf4", "align_batch_pf_early0", "align_batch_ad_fast0",
                              "align_batch_overlap0"])
def test_long_reads_200k_all_partitions_match_recording(api, long_reads, monkeypatch, env, fast, prefetch):
    d, err, rec = long_reads
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    o = DadaOpts(**rec["meta"]["opts"])
    assert o.BAND_SIZE == 32 and o.MAX_CLUST == 0
    got = api.dada_uniques(d.seqs, d.abundances, None, err, d.quals, o)
    st = got.stats
    print("stats", {k: int(st[k]) for k in ("nnw", "nnw_fast", "nnw_retry", "pf_compares", "pf_hits", "batch_compares")})
    assert got.nclust == rec["passes"][0]["nclust"] == 128
    assert_matches_recording(got, rec["passes"][0])
    # the regime did occur: the pointer-free pass switched itself off (more than a quarter of its pairs retried) ...
    if fast:
        assert st["nnw_fast"] >= 2048 and 4 * st["nnw_retry"] > st["nnw_fast"], (st["nnw_fast"], st["nnw_retry"])
    else:
        assert st["nnw_fast"] == 0 and st["nnw_retry"] == 0
    # ... while compares ran on the second stream (or none did)
    assert (st["pf_compares"] > 0) == prefetch, st["pf_compares"]


def test_selfconsist_1M_every_pass_matches_recording(api):
    rec = load_recording("sc1M")
    d, _ = _drawn("cfg3", rec)
    o = DadaOpts(**rec["meta"]["opts"])
    seen = []

    def on_pass(k, used, max_clust, results):     # checked as the loop goes (what a pass used is what the recording used)
        i = len(seen)
        assert i < len(rec["passes"]), "more passes than recorded"
        want = rec["passes"][i]
        assert np.array_equal(used[0], want["err"]), f"err used by pass {i}"
        assert max_clust == want["max_clust"], (i, max_clust, want["max_clust"])
        assert_matches_recording(results[0], want)
        seen.append((k, results[0].nclust))

    res, err_out, errs = api.dada(d, None, self_consist=True, opts=o, on_pass=on_pass)
    assert len(seen) == rec["meta"]["npasses"] == len(errs) + 1
    assert seen[0][1] == 1 and max(n for _, n in seen) > 500
    assert any(np.array_equal(e, err_out) for e in errs) == rec["meta"]["converged"]
    assert np.array_equal(err_out, rec["err_out"])
    assert_matches_recording(res, rec["passes"][-1])
