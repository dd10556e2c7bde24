"""Cases for the two host ends of the boundary call - the marshalling in front (packing, quality conversion, chunked upload)
and the final pass behind the rounds (work lists, staging, the one wait, the assembly of the outputs on the pool) - shared by
tests/test_emu_host_ends.py (the product's code under the emulator) and tests/test_gpu_host_ends.py (the device).  Every case
is one boundary call compared field by field with the plain-C restatement (oracle/cport), and with the committed golden
where the case is one."""
import dataclasses

import numpy as np

from helpers import assert_results_equal, case_inputs

# name -> (golden case, option overrides, prefix of the uniques or None, set priors, compare with the golden too)
CASES = {
    "sam1F_default": ("sam1F_default", {}, None, False, True),
    "samPB_band32": ("samPB_band32", {}, None, False, True),        # the wide final path, mixed lengths
    "sam1F_max_clust_1": ("sam1F_default", dict(MAX_CLUST=1), None, False, False),   # C = 1: no birth pairs
    "sam1F_max_clust_2": ("sam1F_default", dict(MAX_CLUST=2), None, False, False),
    "sam1F_band0": ("sam1F_default", dict(BAND_SIZE=0), None, False, False),         # gapless final alignments
    "sam1F_priors": ("sam1F_default", {}, None, True, False),
    "sam1F_prefix_1": ("sam1F_default", {}, 1, False, False),
    "sam1F_prefix_65": ("sam1F_default", {}, 65, False, False),
}
MULTI = "two_in_flight"                                             # dada_uniques_multi: the pool shared by two final passes

# (label, position or "last", replacement byte)
INVALID = [("first", 0, b"N"), ("p15", 15, b"N"), ("p16", 16, b"N"), ("last", "last", b"N"), ("lower", 40, b"a"), ("x80", 33, b"\x80")]
INVALID_MESSAGE = "Sequences must be made up only of A/C/G/T"


def _inputs(name):
    golden, over, prefix, priors, with_golden = CASES[name]
    d, err, pri, opts, exp, meta = case_inputs(golden)
    opts = dataclasses.replace(opts, **over)
    seqs, ab, quals = d.seqs, d.abundances, d.quals
    if prefix is not None:
        seqs, ab = seqs[:prefix], ab[:prefix]
        quals = np.ascontiguousarray(quals[:prefix, : max(len(s) for s in seqs)])
    if priors:
        pri = (np.arange(len(seqs)) % 97 == 3).astype(np.uint8)
    return seqs, ab, quals, pri, err, opts, (exp if with_golden else None)


def run_case(name, device=0):
    """One boundary call of the case on the library that dada2_amd._lib points at; returns a line for the log."""
    from dada2_amd import api
    from oracle import cport
    seqs, ab, quals, pri, err, opts, exp = _inputs(name)
    got = api.dada_uniques(seqs, ab, pri, err, quals, opts, device=device)
    want = cport.dada_uniques(seqs, ab, pri, err, quals, opts)
    assert_results_equal(got, want)
    if exp is not None:
        assert_results_equal(got, exp)
    return "ok %s %d partitions" % (name, got.nclust)


def run_multi(device=0):
    """Four samples (sam1F and three prefixes of it) through dada_uniques_multi with two in flight on one device, each against
    the restatement: the final passes of two samples use the host pool at the same time."""
    from dada2_amd import api
    from dada2_amd.io import Derep
    from oracle import cport
    d, err, pri, opts, exp, meta = case_inputs("sam1F_default")
    sizes = [d.nraw, 65, max(2, d.nraw // 2), 130]
    dereps = [Derep(d.seqs[:n], d.abundances[:n], np.ascontiguousarray(d.quals[:n, : max(len(s) for s in d.seqs[:n])]),
                    np.zeros(0, dtype=np.int32)) for n in sizes]
    got = api.dada_uniques_multi(dereps, err, opts, devices=(device, device))
    assert len(got) == len(dereps)
    for g, x in zip(got, dereps):
        assert_results_equal(g, cport.dada_uniques(x.seqs, x.abundances, None, err, x.quals, opts))
    assert_results_equal(got[0], exp)
    return "ok %s %s partitions" % (MULTI, [g.nclust for g in got])


def run_invalid(label, device=0):
    """A byte other than A C G T in one sequence: the call fails with the reference's message."""
    from dada2_amd import _lib, api
    pos, byte = {k: (p, b) for k, p, b in INVALID}[label]
    d, err, pri, opts, exp, meta = case_inputs("sam1F_default")
    n = 70
    seqs = [s.encode("ascii") for s in d.seqs[:n]]
    victim = 37
    p = len(seqs[victim]) - 1 if pos == "last" else pos
    seqs[victim] = seqs[victim][:p] + byte + seqs[victim][p + 1:]
    quals = np.ascontiguousarray(d.quals[:n, : max(len(s) for s in seqs)])
    try:
        api.dada_uniques(seqs, d.abundances[:n], None, err, quals, opts, device=device)
    except _lib.Dada2HipError as ex:
        assert INVALID_MESSAGE in str(ex), str(ex)
        return "ok invalid %s" % label
    raise AssertionError("an invalid base (%s) was accepted" % label)
