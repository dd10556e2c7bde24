"""Pooled and pseudo-pooled dada() and priors by sequence on the MI355X (-m gpu), against tests/pool_cases.py.

The match kernel: first_match and the flags of dada2hip_sample_set_prior_seqs against Python's list.index / in on one sample of about
700 uniques (lengths 15 to 250; pairs that share their first 32 bases and differ in the last base, or in the last base of a full
word; a proper prefix of another) for eight prior lists (duplicates, an N, an entry longer than any unique, many entries under one
key, the empty list, a list of one, or_flags on uniques that match nothing), every list through LDS, through global memory
(DADA2HIP_PRIORS_LDS_KEYS=4), with one block that strides (DADA2HIP_PRIORS_GRID=1) and with two that stride over keys in global
memory; after EVERY call one Sample.run with OMEGA_P loosened, against the reference run with the same flags - the host mirror
and the device array agree, flag by flag; where a flag is set the reference's result differs from its result without flags.

pool=True and pool="pseudo" on sam1F + sam2F with tperr1, without and with self_consist (MAX_CONSIST=3), pool=True also with
prior_seqs: every per-sample DadaResult and every error matrix against the restated pipeline on the reference's dada_uniques, bit for
bit, p-values within helpers.P_RTOL.  The pseudo-pooled cases are ones where the reference's pseudo-pooled result differs from its
independent result, asserted here from the reference alone."""
import numpy as np
import pytest

import pool_cases as pc
from dada2_amd.opts import DadaOpts
from helpers import assert_results_equal

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def api(oracle_ref):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from dada2_amd import api as a
    return a


@pytest.mark.parametrize("path", list(pc.MATCH_PATHS))
def test_prior_sequences_match_as_list_index_says(api, path):
    """Every prior list through this path, each call followed by the loosened-OMEGA_P run against the reference with the same flags."""
    pc.case_match_path(api, path, run=True)


@pytest.mark.parametrize("self_consist", [False, True])
def test_pooled_run_equals_the_restated_pipeline(api, self_consist):
    dereps, err = pc.golden_pair()
    got, _ = pc.check_dada(api, dereps, err, self_consist, DadaOpts(MAX_CONSIST=3), True)
    assert sum(int(g.clustering["abundance"].sum()) for g in got) <= 3000 and got[0].nclust >= 2


def test_pooled_run_with_prior_sequences(api):
    dereps, err = pc.golden_pair()
    # singletons and doubletons of either sample: OMEGA_P decides about them where OMEGA_A would not
    priors = [s for d in dereps for s, a in zip(d.seqs, d.abundances) if a <= 2][::9] + ["ACGTN", dereps[0].seqs[0]]
    o = DadaOpts(OMEGA_P=1e-2)
    got, want = pc.check_dada(api, dereps, err, False, o, True, prior_seqs=priors)
    plain, _, _ = pc.restate_dada(dereps, err, False, api.noqual_errfun, o, True)
    assert any(w.clustering["sequence"] != p.clustering["sequence"] for w, p in zip(want, plain))   # the priors did something


@pytest.mark.parametrize("self_consist", [False, True])
def test_pseudo_pooled_run_equals_the_restated_pipeline(api, self_consist):
    dereps, err = pc.golden_pair()
    o = DadaOpts(MAX_CONSIST=3)
    assert pc.pseudo_differs(dereps, err, self_consist, o)
    pc.check_dada(api, dereps, err, self_consist, o, "pseudo")


def test_prior_sequences_without_pooling_are_ored_with_the_flags(api):
    dereps, err = pc.golden_pair()
    flags = [(np.arange(d.nraw) % 97 == 5).astype(np.uint8) for d in dereps]
    priors = [dereps[0].seqs[-1], dereps[1].seqs[-3], dereps[0].seqs[400]]
    pc.check_dada(api, dereps, err, False, DadaOpts(OMEGA_P=1e-2), False, prior_seqs=priors, flags=flags)


def test_pool_with_one_derep_is_the_unpooled_call(api):
    dereps, err = pc.golden_pair()
    a, ea, _ = api.dada([dereps[0]], err, pool=True)
    b, eb, _ = api.dada([dereps[0]], err)
    assert len(a) == len(b) == 1 and np.array_equal(ea, eb)
    assert_results_equal(a[0], b[0], exact_float=True)
    c, _, _ = api.dada(dereps[0], err, pool=True)                 # a bare derep: a bare result
    assert_results_equal(c, b[0], exact_float=True)


def test_native_dereps_stand_where_dereps_do(api):
    """A list of NativeDerep objects, unpooled and pooled, gives what the same samples give as numpy Dereps."""
    import os
    paths = [os.path.join(pc.GOLDEN, n + ".fastq.gz") for n in ("sam1F", "sam2F")]
    nds = [api.NativeDerep(p) for p in paths]
    try:
        ds = [nd.to_derep() for nd in nds]
        err = pc.golden_pair()[1]
        for kw in ({}, {"pool": True}):
            a, ea, _ = api.dada(nds, err, **kw)
            b, eb, _ = api.dada(ds, err, **kw)
            assert len(a) == len(b) == 2 and np.array_equal(ea, eb)
            for x, y in zip(a, b):
                assert_results_equal(x, y, exact_float=True)
        one, _, _ = api.dada(nds[0], err)                         # a bare NativeDerep: a bare result
        assert_results_equal(one, api.dada(ds[0], err)[0], exact_float=True)
    finally:
        for nd in nds:
            nd.close()
