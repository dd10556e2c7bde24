"""Every stage's lightest cases with the allocation cache handing out DIRTY memory (DADA2HIP_ALLOC_POISON, csrc/hostpar.h) - shared
by tests/test_emu_poisoned_memory.py (the product's code under the emulator, EMU_GUARD=1) and tests/test_gpu_poisoned_memory.py.

Device and pinned buffers come from one per-process cache, and a freed block goes to the next request of its size class as the
last user left it: what a kernel finds in a buffer it has not written depends on which stage ran before it in the process.  The
knob makes that a case: every block handed out, fresh or recycled, is filled with one byte over its whole size class, the class
slack and the 64 bytes behind the last element included.  Nothing is restated here - a stage's callable runs that stage's own
``light`` cases, each of which compares with its own oracle; this module only arranges the memory they run in.

run_stage(stage, byte), in one process:
  1. the stage's cases under the knob.  The library's fill counters (dada2hip_alloc_poison_stats) must have grown, device blocks
     and bytes for every stage, pinned blocks too for the stages that stage their input through pinned memory: a knob that was
     not read fails here, it does not pass quietly;
  2. the same cases again with the knob unset: the recycled-dirty run.  Its blocks are what run 1 left in the cache - the poison
     byte wherever run 1 wrote nothing, run 1's own tables, counters and lists everywhere else - and it must hold as well.  The
     counters must NOT move (the knob is read at every boundary call, not once per process).

Two bytes, because one byte alone hides the initialisation that happens to write it:
  0xFF  is -1 as an integer, ~0 as a key, a NaN as a double and above every read index - exactly the "empty" fill of the stages'
        tables and lists, so it hides a missing 0xFF fill, and shows a missing zero (a count that starts at -1 / 4 294 967 295).
  0x5A  is no stage's sentinel: 0x5A5A5A5A = 1 515 870 810 as an int32 (a large positive index: under EMU_GUARD an address made
        from it stops at once), 0x5A5A5A5A5A5A5A5A as a key, finite and about 2.7e131 as a double.  It shows a missing 0xFF fill
        and a missing zero alike.
  (0x00, roughly what a fresh hipMalloc in a young process reads as today, hides every missing zero: that is the gap.)
Every missing initialisation is wrong under at least one of the two.  The sentinels checked against them: the dereplicator's
DD_EMPTY (-1), DD_PENDING (-2) and DD_SKIP (-1) and the pair table's MP_EMPTY (~0 as uint64; all in csrc/engine.h), the final
work list's -1 behind a partition's members (kernels.hip), and NA_INTEGER (0x80000000): none of them is 0x5A5A5A5A; DD_EMPTY,
DD_SKIP, MP_EMPTY and the work list's -1 are 0xFF bytes throughout, DD_PENDING and NA_INTEGER are neither byte repeated.

Seconds: one run_stage (poisoned + recycled, byte 0x5A) under the guarded emulator with the jobs side by side on 8 host cores
(`emu_s`), the same two runs with the knob never set (`emu_plain_s`: measured while three emulator builds ran beside them, hence
the slower of the two - the fills are memsets and cost nothing that shows), and on the MI355X (`gpu_s`: the test's call under byte
0xFF / 0x5A; regimes' first number includes the oracle's runs, which the second reuses); measured once, when the table was written.
primers took 6.7 / 6.2 s on the device, 3.1 s each of its poisoned and its recycled half, and is therefore cut in two there
(GPU_PARTS: 3.5 + 3.2 / 3.1 + 3.0 s).  Every emulator job fits the 900 s of its subprocess as it is; none is cut.
"""
import os
import time

KNOB = "DADA2HIP_ALLOC_POISON"
BYTES = (0xFF, 0x5A)


def _filter(names=None):
    import filter_cases as F
    return F.emu_run(names)


def _filter_orient(names=None):
    import filter_orient_cases as F
    return F.emu_run(names)


def _primers(names=None):
    import primer_cases as P
    return P.emu_run(names)


def _readqc(names=None):
    import readqc_cases as Q
    return Q.emu_run(names)


def _derep(names=None):
    import derep_dev_cases as D
    return D.emu_run(names)


UPLOAD_RUNS = ("n513", "n1537", "boundary_equals_resident", "multi_equals_single")


def _upload(names=None):
    import upload_fused_cases as U
    for n in names or UPLOAD_RUNS:
        if n == "boundary_equals_resident":
            U.run_boundary_equals_resident()
        elif n == "multi_equals_single":
            U.run_multi_equals_single()
        else:
            U.run_shape(n)


WORKLIST_RUNS = ("band16", "band16_lane")


def _worklist(names=None):
    import upload_fused_cases as U
    for n in names or WORKLIST_RUNS:
        U.run_worklist(n)


RESIDENT_RUNS = ("memory_handed_on", "option_walk")


def _resident(names=None):
    import resident_cases as R
    from dada2_amd import api
    for n in names or RESIDENT_RUNS:
        if n == "memory_handed_on":
            R.case_memory_handed_on(api, trim=False)
        else:
            assert n == "option_walk", n
            R.case_option_walk(api, "forward", small=True)


def _regimes(names=None):
    import regime_cases as R
    import regime_runner
    regime_runner.run_cases("single", list(names or R.EMU_CASES))


def _pool(names=None):
    import pool_cases as P
    return P.emu_run()


def _paired(names=None):
    import paired_cases as P
    return P.emu_run(names or tuple(n for n in P.EMU_NAMES if n != "interface"))   # (interface: files, no buffers of its own)


def _seqtab(names=None):
    import seqtab_cases as S
    return S.emu_run(names)


def _bimera(names=None):
    import bimera_denovo_cases as B
    return B.emu_run()


def _collapse(names=None):
    import collapse_cases as C
    return C.emu_run()


def _taxonomy(names=None):
    import taxonomy_cases as T
    return T.emu_run()


def _species(names=None):
    import species_cases as S
    return S.emu_run()


# stage -> its callable; pinned: the stage stages its input through pinned memory (the pinned counters must grow as well);
# names: the cases a job is cut to (None = the callable's whole light list); emu_ff: the emulator module runs 0xFF too (hash
# tables, -1-filled lists); the seconds as the docstring says
STAGES = {
    "filter":        dict(run=_filter, pinned=True, names=None, emu_ff=False, emu_s=19.7, emu_plain_s=28.6, gpu_s=(3.1, 2.9)),
    "filter_orient": dict(run=_filter_orient, pinned=False, names=None, emu_ff=False, emu_s=7.6, emu_plain_s=12.7, gpu_s=(1.1, 1.1)),
    "primers":       dict(run=_primers, pinned=True, names=None, emu_ff=False, emu_s=18.8, emu_plain_s=24.9, gpu_s=(6.7, 6.2)),
    "readqc":        dict(run=_readqc, pinned=True, names=None, emu_ff=False, emu_s=4.1, emu_plain_s=6.2, gpu_s=(0.6, 0.6)),
    "derep":         dict(run=_derep, pinned=True, names=None, emu_ff=True, emu_s=1.9, emu_plain_s=2.8, gpu_s=(0.5, 0.5)),
    "upload":        dict(run=_upload, pinned=True, names=None, emu_ff=True, emu_s=49.1, emu_plain_s=62.0, gpu_s=(2.3, 2.1)),
    "worklist":      dict(run=_worklist, pinned=False, names=None, emu_ff=True, emu_s=3.4, emu_plain_s=4.8, gpu_s=(0.3, 0.3)),
    "resident":      dict(run=_resident, pinned=False, names=None, emu_ff=False, emu_s=19.5, emu_plain_s=25.7, gpu_s=(0.5, 0.4)),
    "regimes":       dict(run=_regimes, pinned=False, names=None, emu_ff=False, emu_s=313.6, emu_plain_s=330.1, gpu_s=(4.4, 1.4)),
    "pool":          dict(run=_pool, pinned=False, names=None, emu_ff=False, emu_s=5.3, emu_plain_s=7.1, gpu_s=(0.4, 0.5)),
    "paired":        dict(run=_paired, pinned=False, names=None, emu_ff=True, emu_s=1.0, emu_plain_s=1.9, gpu_s=(3.5, 3.4)),
    "seqtab":        dict(run=_seqtab, pinned=False, names=None, emu_ff=True, emu_s=1.2, emu_plain_s=1.7, gpu_s=(0.3, 0.3)),
    "bimera":        dict(run=_bimera, pinned=False, names=None, emu_ff=False, emu_s=2.1, emu_plain_s=3.3, gpu_s=(0.2, 0.1)),
    "collapse":      dict(run=_collapse, pinned=False, names=None, emu_ff=False, emu_s=0.4, emu_plain_s=0.6, gpu_s=(0.3, 0.3)),
    "taxonomy":      dict(run=_taxonomy, pinned=False, names=None, emu_ff=False, emu_s=15.6, emu_plain_s=18.4, gpu_s=(2.5, 1.5)),
    "species":       dict(run=_species, pinned=False, names=None, emu_ff=False, emu_s=0.9, emu_plain_s=1.1, gpu_s=(0.1, 0.1)),
}
STAGE_NAMES = tuple(STAGES)
EMU_JOBS = [(s, b) for s in STAGE_NAMES for b in ((0x5A, 0xFF) if STAGES[s]["emu_ff"] else (0x5A,))]
# On the device a stage whose light list takes more than a few seconds is cut by case name into parts (every case stays, and keeps
# its comparisons): the parts of a stage together are its whole list (tests/test_emu_poisoned_memory.py checks that they are).
GPU_PARTS = {
    "primers": (("lengths", "chunk_boundaries", "letters", "orientation", "tiles_and_pieces", "example_file", "refusals"),
                ("batches", "mismatch_budget", "multiple_hits", "window", "random_sweep", "file_rules")),
}
GPU_JOBS = [(s, b, part) for s in STAGE_NAMES for b in BYTES for part in GPU_PARTS.get(s, (None,))]


def gpu_job_id(job):
    s, b, part = job
    return "%s-0x%02X" % (s, b) if part is None else "%s-part%d-0x%02X" % (s, GPU_PARTS[s].index(part) + 1, b)


def poison_stats():
    """dada2hip_alloc_poison_stats: device blocks, device bytes, pinned blocks, pinned bytes filled since the process started."""
    import ctypes as C
    from dada2_amd import _lib
    out = (C.c_int64 * 4)()
    _lib.lib().dada2hip_alloc_poison_stats(out)
    return tuple(int(v) for v in out)


def _with_knob(value, f):
    old = os.environ.get(KNOB)
    if value is None:
        os.environ.pop(KNOB, None)
    else:
        os.environ[KNOB] = str(value)
    try:
        return f()
    finally:
        if old is None:
            os.environ.pop(KNOB, None)
        else:
            os.environ[KNOB] = old


def run_stage(stage, byte, names=None):
    """The stage's cases poisoned with ``byte`` (None: the knob never set - the timing baseline, no counter asserted), then once
    more on what that run left behind.  Returns a line "ok <stage> ..." with the seconds of both runs and the fills counted."""
    st = STAGES[stage]
    names = names or st["names"]
    s0 = poison_stats()
    t0 = time.time()
    _with_knob(byte, lambda: st["run"](names))
    t1 = time.time()
    s1 = poison_stats()
    if byte is not None:
        grew = [b - a for a, b in zip(s0, s1)]
        assert grew[0] > 0 and grew[1] >= 256 * grew[0], (stage, "no device block was filled: %s ignored?" % KNOB, s0, s1)
        if st["pinned"]:
            assert grew[2] > 0 and grew[3] >= 256 * grew[2], (stage, "no pinned block was filled", s0, s1)
    else:
        assert s1 == s0, (stage, "fills counted with the knob unset", s0, s1)
    _with_knob(None, lambda: st["run"](names))                        # the recycled-dirty run
    t2 = time.time()
    s2 = poison_stats()
    assert s2 == s1, (stage, "fills counted with the knob unset: read once per process?", s1, s2)
    return "ok %s byte %s poisoned %.1fs recycled %.1fs fills %s" % (stage, "-" if byte is None else "0x%02X" % byte, t1 - t0, t2 - t1,
                                                                    [b - a for a, b in zip(s0, s1)])
