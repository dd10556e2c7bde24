"""The run-level mergePairs on the MI355X (-m gpu): dada2_amd.paired.merge_pairs - dada2hip_merge_run: k_mp_tally, k_mp_compact,
k_nw_gen<pair>, k_mp_eval, k_mp_consensus - against the specification of tests/paired_cases.py, row for row on every key, rejects
included.  The cases also run under the emulator in their lighter form (tests/test_emu_paired.py).  The whole path: the reference's
own example, sam1F / sam1R as tests/test_merge.py builds it, beside sam2F / sam2R from the FASTQ fixtures through api.derep_fastq
and api.dada_uniques with the committed error matrix (the two files pair: 1 500 reads each) - the run against the per-sample oracle
and against a loop of the unchanged api.merge_pairs."""
import os

import numpy as np
import pytest

import paired_cases as pc
from helpers import GOLDEN, case_inputs, tperr1

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def P():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from dada2_amd import paired
    return paired


@pytest.mark.parametrize("name", pc.CASE_NAMES)
def test_run_equals_the_specification(P, name):
    pc.CASES[name](P)


def test_whole_path_two_samples(P):
    from dada2_amd import api
    from dada2_amd.io import Derep, extend_err
    from dada2_amd.opts import DadaOpts
    maps = np.load(os.path.join(GOLDEN, "sam1_maps.npz"))
    res, dereps = {}, {}
    for fq, case in (("sam1F", "sam1F_default"), ("sam1R", "sam1R_default")):
        d, err, pri, opts, exp, meta = case_inputs(case)
        res[fq] = api.dada_uniques(d.seqs, d.abundances, pri, err, d.quals, opts, device=0)
        dereps[fq] = Derep(d.seqs, d.abundances, d.quals, maps[fq])
    for fq in ("sam2F", "sam2R"):
        d = api.derep_fastq(os.path.join(GOLDEN, fq + ".fastq.gz"))
        res[fq] = api.dada_uniques(d.seqs, d.abundances, None, extend_err(tperr1(), int(np.ceil(np.nanmax(d.quals)))), d.quals, DadaOpts(), device=0)
        dereps[fq] = d
    samples = [(res[s + "F"], dereps[s + "F"], res[s + "R"], dereps[s + "R"]) for s in ("sam1", "sam2")]

    def fact(want):
        assert all(sum(r["abundance"] for r in w if r["accept"]) > 1000 for w in want)     # most of the 1 500 read pairs of either fixture merge
        assert all(any(not r["accept"] for r in w) for w in want)
    got = pc.check(P, samples, "whole path", fact, names=["sam1", "sam2"])
    loop = [api.merge_pairs(*s, return_rejects=True) for s in samples]
    for g, w in zip(got, loop):
        pc.same_rows(g, w, "against the loop of api.merge_pairs")
    ok = P.merge_pairs([s[0] for s in samples], [s[1] for s in samples], [s[2] for s in samples], [s[3] for s in samples])
    assert ok == [[r for r in g if r["accept"]] for g in got]
