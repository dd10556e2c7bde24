"""Runs cases of tests/regime_cases.py through the library in a process of its own (the engine knobs, DADA2HIP_*, are read once
per process) and compares every output with the oracle.  Used by tests/test_emu.py (the emulated library), by
tests/test_gpu_regimes.py (the real one, under each engine setting) and by hand.

usage: python regime_runner.py <emu | hip> <single | multi> <case>[,<case>...]
       python regime_runner.py oracle <c | ref> <case>[,<case>...]      (only fills REGIME_ORACLE_CACHE)

single  api.dada_uniques per case.
multi   all cases in ONE dada2hip_run_multi call, two host threads on device 0 (the cases must share their options).

Per case: the facts of the case hold on the oracle's result (regime_cases.check_facts: the sample reaches its regime), then
assert_results_equal against the plain-C oracle - p-values at P_RTOL, everything else bit-exact - and against the reference
itself where oracle/_ref is present and REGIME_WITH_REF=1.  Prints "ok <case> <json of the run's stats>" per case.  The oracle
results are kept in the directory REGIME_ORACLE_CACHE names, if any: they do not depend on the engine setting."""
import json
import os
import pickle
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

STAT_KEYS = ("rounds", "tail_launches", "tail_blocks", "tail_mirror", "tail_threads", "tail_pauses", "tail_fallbacks",
             "tail_xcd_barrier", "overlap_on", "pf_compares", "nshuffle", "nmoves", "batch_compares")


def cached_oracle(name, which="c"):
    """The oracle's (which = "c") or the reference's ("ref") result of a case: from REGIME_ORACLE_CACHE if it is there."""
    import regime_cases as R
    cache = os.environ.get("REGIME_ORACLE_CACHE")
    path = os.path.join(cache, "%s.%s.pkl" % (name, which)) if cache else None
    if path and os.path.exists(path):
        with open(path, "rb") as f:
            res = pickle.load(f)
        R._ORACLE[(name, "oracle.cport" if which == "c" else "oracle.ref", which == "ref")] = res
        return res
    if which == "c":
        res = R.oracle_result(name)
    else:
        from oracle import ref
        ref.set_threads(min(16, os.cpu_count() or 1))
        try:
            res = R.oracle_result(name, ref, multithread=True)
        finally:
            ref.set_threads(1)
    if path:
        tmp = "%s.%d.tmp" % (path, os.getpid())
        with open(tmp, "wb") as f:
            pickle.dump(res, f)
        os.replace(tmp, path)
    return res


def main(which, mode, names):
    if which == "hip":
        import torch  # noqa: F401  (before the library: tests/conftest.py's note on the two HIP runtimes)
    from dada2_amd import _lib
    if which == "emu":   # the functional emulator of tests/emu: the real kernels and driver on the CPU (test infrastructure)
        sys.path.insert(0, os.path.join(ROOT, "tests", "emu"))
        import build as emu_build
        _lib.LIB_PATH = emu_build.build()
    run_cases(mode, names)


def run_cases(mode, names):
    """The cases through whatever library dada2_amd._lib points at (main, and tests/poison_cases.py in a process that has chosen it)."""
    import regime_cases as R
    from helpers import P_RTOL, assert_results_equal, tperr1
    from dada2_amd import api
    from oracle import ref
    with_ref = os.environ.get("REGIME_WITH_REF") == "1" and ref.available()
    built = [R.build(n) for n in names]
    wants = [R.check_facts(n, cached_oracle(n)) for n in names]
    if mode == "multi":
        assert all(b[2] == built[0][2] for b in built), "the cases of one run_multi call share their options"
        inputs = [api.HostInput.from_derep(d, pri) for d, pri, o, f in built]
        gots = api.dada_uniques_multi(inputs, tperr1(), built[0][2], devices=(0, 0))
    else:
        gots = [api.dada_uniques(d.seqs, d.abundances, pri, tperr1(), d.quals, o) for d, pri, o, f in built]
    for n, (d, pri, o, f), got, want in zip(names, built, gots, wants):
        assert_results_equal(got, want, p_rtol=P_RTOL, check_birth_from=pri is None)
        if with_ref:
            assert_results_equal(got, cached_oracle(n, "ref"), p_rtol=P_RTOL, check_birth_from=pri is None)
        st = {k: (float(got.stats[k]) if isinstance(got.stats[k], float) else int(got.stats[k])) for k in STAT_KEYS if k in got.stats}
        st.update(nclust=int(got.nclust), nraw=int(d.nraw), ref=bool(with_ref))
        print("ok", n, json.dumps(st), flush=True)


if __name__ == "__main__":
    if sys.argv[1] == "oracle":
        for n in sys.argv[3].split(","):
            cached_oracle(n, sys.argv[2])
            print("ok", n, flush=True)
    else:
        main(sys.argv[1], sys.argv[2], sys.argv[3].split(","))
