"""GPU parity (-m gpu) in the three regimes of tests/regime_cases.py: more than 1 024 partitions (the round tail's per-partition
LDS tables overflow into their global-memory arms, the per-cluster arrays grow 1 024 -> 2 048), tie lists of 65 ... 4 200 exactly
tied bud candidates (past the 64 inline records, past the 4 096 full records the device keeps), abundances up to the top of R's
integer range (every arm of pgamma_lower inside a whole run, candidates at OMEGA_A, the 32-bit wraps of $subqual and
$clusterquals).  Every case against the plain-C oracle through assert_results_equal - p-values at P_RTOL, everything else
bit-exact - and against the reference itself where oracle/_ref is present, under a representative set of engine settings, each
in a process of its own (tests/regime_runner.py: the knobs are read once per process), through dada2hip_run_multi with two
samples in flight and through the two-rank sharded run.  The runner asserts each case's facts on the oracle's result before it
compares (a sample that stops reaching its regime fails the test), and the stats name the engine that ran.

The oracle is the slow side (half a minute for the large crowd): its results are computed once, side by side, into a
directory all runs of the session share."""
import json
import os
import subprocess
import sys

import pytest

import regime_cases as R
from test_shard import run_group

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RUNNER = os.path.join(ROOT, "tests", "regime_runner.py")

CROWD = ("crowd_large", "crowd_small_priors")
TIED = ("tied_65", "tied_300", "tied_4096", "tied_4100", "tied_4200", "tied_5000", "tied_two_groups_movers")
PLAIN = ("tied_4200_permuted", "tied_300_permuted")
DEEP = tuple(n for n in R.CASES if n.startswith("deep"))
HEAVY = ("crowd_large", "crowd_small", "crowd_small_priors", "crowd_small_nogreedy")


@pytest.fixture(scope="module")
def oracle_cache(tmp_path_factory):
    """REGIME_ORACLE_CACHE for the runs of this module, filled for the slow cases side by side up front."""
    from oracle import ref
    path = str(tmp_path_factory.mktemp("regime_oracle"))
    env = dict(os.environ, REGIME_ORACLE_CACHE=path)
    jobs = [("c", n) for n in HEAVY] + ([("ref", n) for n in HEAVY] if ref.available() else [])
    jobs += [("c", ",".join(TIED + PLAIN + DEEP))] + ([("ref", ",".join(TIED + PLAIN + DEEP))] if ref.available() else [])
    procs = [subprocess.Popen([sys.executable, RUNNER, "oracle", which, names], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                              text=True) for which, names in jobs]
    for (which, names), p in zip(jobs, procs):
        out, _ = p.communicate(timeout=1200)
        assert p.returncode == 0, (which, names, out[-3000:])
    return path


def _run(oracle_cache, mode, names, env_extra, timeout=900):
    env = dict(os.environ, REGIME_ORACLE_CACHE=oracle_cache, REGIME_WITH_REF="1", **env_extra)
    out = subprocess.run([sys.executable, RUNNER, "hip", mode, ",".join(names)], env=env, capture_output=True, text=True, timeout=timeout)
    assert out.returncode == 0 and out.stdout.count("ok ") == len(names), out.stdout[-2000:] + out.stderr[-4000:]
    stats = {}
    for line in out.stdout.splitlines():
        if line.startswith("ok "):
            _, name, js = line.split(" ", 2)
            stats[name] = json.loads(js)
    from oracle import ref
    assert all(st["ref"] == ref.available() for st in stats.values())      # (the reference was compared with wherever it is there)
    return stats


def _persistent(st):
    return st["tail_launches"] > 0 and st["tail_fallbacks"] == 0


# (settings, what the stats must show of the engine that ran: a predicate over one run's stats and its case name)
ENGINES = {
    "default": ({}, lambda n, st: _persistent(st) and st["tail_mirror"] == 1 and st["overlap_on"] == 1),
    "chains": ({"DADA2HIP_V2_TAIL": "chain"}, lambda n, st: st["tail_launches"] == 0 and st["batch_compares"] > 0),
    # the block caps of k2_shuffle / k2_pupdate (2 048 / 1 024 blocks of 256 threads: a thread strides only past 524 288 / 262 144
    # uniques) forced down: one block each - the 8 192 and more uniques of crowd_large are 32 and more visits per thread, under
    # the 1 000 the 16-bit per-thread counts of the shuffle pass allow - and 3 / 2 blocks, an uneven stride, with blocking waits
    # (ACCEPTED GAP: the stats carry neither the grids launched nor sh_filter, so the predicates of these four rows are the plain
    #  chains / tail ones and an ignored DADA2HIP_V2_GRID_* or _FILTER would leave them green - unlike DADA2HIP_NW_RING, which has
    #  its diagnostic.  That the rows bite is shown by the break experiments of DESIGN section 12 only: a sweep cut to its first
    #  visit turns the capped rows red and no other.)
    "chains-grid1": ({"DADA2HIP_V2_TAIL": "chain", "DADA2HIP_V2_GRID_SHUFFLE": "1", "DADA2HIP_V2_GRID_PUPDATE": "1"},
                     lambda n, st: st["tail_launches"] == 0 and st["batch_compares"] > 0),
    "chains-grid3-2-blocking-waits": ({"DADA2HIP_V2_TAIL": "chain", "DADA2HIP_V2_GRID_SHUFFLE": "3", "DADA2HIP_V2_GRID_PUPDATE": "2",
                                       "DADA2HIP_WAIT": "block"}, lambda n, st: st["tail_launches"] == 0 and st["batch_compares"] > 0),
    # the unfiltered shuffle (every later call of a round visits every unique) the filtered default must agree with: on the
    # chains and in the persistent tail, which runs the same shuffle_body and reads Eng2::sh_filter too
    "chains-unfiltered-shuffle": ({"DADA2HIP_V2_TAIL": "chain", "DADA2HIP_V2_FILTER": "0"},
                                  lambda n, st: st["tail_launches"] == 0 and st["batch_compares"] > 0),
    "tail-unfiltered-shuffle": ({"DADA2HIP_V2_FILTER": "0"}, lambda n, st: _persistent(st) and st["tail_mirror"] == 1),
    "classic-engine": ({"DADA2HIP_ENGINE": "classic"}, lambda n, st: st["tail_launches"] == 0 and st["batch_compares"] == 0),
    # (a crowd variant takes six neighbours along when it is born: with four movers inline every such round pauses)
    "mirror-checked-grid5-pauses": ({"DADA2HIP_V3_MIRROR": "2", "DADA2HIP_V3_GRID": "5", "DADA2HIP_V2_MOV_INLINE": "4"},
                                    lambda n, st: _persistent(st) and st["tail_mirror"] == 1 and st["tail_blocks"] == 5
                                    and (n != "crowd_large" or st["tail_pauses"] > 0)),
    "tail-serial": ({"DADA2HIP_V3_OVERLAP": "0"}, lambda n, st: _persistent(st) and st["overlap_on"] == 0 and st["pf_compares"] == 0),
    "nbuf1": ({"DADA2HIP_V2_NBUF": "1"}, lambda n, st: _persistent(st) and st["overlap_on"] == 0),   # (the overlap needs four buffers)
    "xcd-barrier-grid9": ({"DADA2HIP_V3_XBAR": "1", "DADA2HIP_V3_GRID": "9"},
                          lambda n, st: _persistent(st) and st["tail_xcd_barrier"] == 1 and st["tail_blocks"] == 9),
    # (every decision on the host - the path ties and prior births always take; it runs on the classic round loop)
    "host-applied-births": ({"DADA2HIP_NO_AUTOBIRTH": "1"}, lambda n, st: st["tail_launches"] == 0 and st["tail_fallbacks"] == 0),
}
CLASSIC_LOOP = ("classic-engine", "host-applied-births")     # the settings whose rounds the host drives one by one


@pytest.mark.parametrize("engine", list(ENGINES))
def test_regimes_match_the_oracle_under_each_engine(oracle_cache, engine):
    env, ran = ENGINES[engine]
    stats = _run(oracle_cache, "single", CROWD + TIED + PLAIN + DEEP, env)
    for name, st in stats.items():
        if name in PLAIN:         # input that is not abundance-sorted: plain mode, whatever the engine setting
            assert st["tail_launches"] == 0, (name, st)
        else:
            assert ran(name, st), (engine, name, st)
    big = stats["crowd_large"]
    assert big["nraw"] >= 2 * 4096 and big["nclust"] > 1024 + 200, big
    # (nmoves is the device-driven round loop's count of the moves its host mirror replayed: the classic loop keeps none)
    assert big["nmoves"] > 4096 if engine not in CLASSIC_LOOP else big["nmoves"] == 0, big
    if engine == "default":
        assert big["tail_blocks"] >= 3, big                       # the tail's tables are per block: three blocks and more
    for name in ("tied_4100", "tied_4200", "tied_5000"):
        assert stats[name]["nraw"] > R.TIES_FULL and stats[name]["nclust"] == R.CASES[name][1].get("max_clust", 24), stats[name]


def test_non_greedy_crowd_with_a_comparison_store_that_has_to_grow(oracle_cache):
    """GREEDY = FALSE on the crowd: every unique is compared with every centre, more than a thousand stored comparisons in some
    chains - with the store's first allocation forced down (DADA2HIP_NODE_CAP=1) it grows through H2_CAPACITY on the way."""
    for env in ({"DADA2HIP_NODE_CAP": "1"}, {"DADA2HIP_NODE_CAP": "1", "DADA2HIP_V2_TAIL": "chain"}):
        st = _run(oracle_cache, "single", ("crowd_small_nogreedy",), env)["crowd_small_nogreedy"]
        assert (st["tail_launches"] > 0) == ("DADA2HIP_V2_TAIL" not in env) and st["nclust"] > 1024, st


@pytest.mark.parametrize("names", [("crowd_large", "crowd_small"), ("tied_4200", "tied_4100", "tied_4096", "tied_65"),
                                   ("tied_4200_permuted", "tied_4200")], ids=["crowds", "ties", "ties-plain-and-not"])
def test_regimes_through_run_multi_two_in_flight_on_one_device(oracle_cache, names):
    """dada2hip_run_multi, two host threads on the one device: the second sample in flight runs on the launch chains."""
    stats = _run(oracle_cache, "multi", names, {})
    assert len(stats) == len(names)


@pytest.mark.parametrize("case", ["crowd_large", "tied_4200", "tied_300", "tied_two_groups_movers"])
def test_regimes_sharded_over_two_ranks_on_one_gpu(oracle_cache, case, monkeypatch):
    """Two gloo ranks share the GPU (tests/shard_worker.py): each rank lists the ties of ITS best key and the union decides;
    the sharded result equals the unsharded one bit for bit and the oracle's."""
    monkeypatch.setenv("REGIME_ORACLE_CACHE", oracle_cache)
    run_group("hip", "gloo", "regime:" + case, 2)
