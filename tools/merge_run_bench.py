#!/usr/bin/env python3
"""mergePairs over a run at a study-like size: S samples of K = ceil(sqrt(P)) forward and K reverse
denoised sequences of 250 nt (amplicons of 440 nt: forward i and reverse i overlap by 60), P unique (forward, reverse) pairs - the
K that belong together, which merge, and P - K mispairings, which do not - and N read pairs each, nine in ten of them on the true
pairs, 2 % unassigned on either side.  Times dada2_amd.paired.merge_pairs on all samples in one call against a loop of
dada2_amd.api.merge_pairs over the same objects - both paths in one process, their rows compared for equality first - and prints,
as one JSON line, both wall times and the stats words of the run-level call.
Usage: merge_run_bench.py [samples=96] [unique pairs=3000] [reads=100000] [out.json]"""
import contextlib
import io
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
S = int(sys.argv[1]) if len(sys.argv) > 1 else 96
P = int(sys.argv[2]) if len(sys.argv) > 2 else 3000
N = int(sys.argv[3]) if len(sys.argv) > 3 else 100000
OUT = sys.argv[4] if len(sys.argv) > 4 else None

from dada2_amd import api, paired  # noqa: E402
from dada2_amd.io import Derep  # noqa: E402
from dada2_amd.opts import DadaResult  # noqa: E402

rng = np.random.default_rng(813)
letters = np.frombuffer(b"ACGT", dtype=np.uint8)
comp = bytes.maketrans(b"ACGT", b"TGCA")
NA = np.iinfo(np.int32).min


def note(*a):
    print(*a, file=sys.stderr, flush=True)


def dada_of(seqs, n0):
    n = len(seqs)
    return DadaResult({"sequence": seqs, "abundance": np.ones(n, np.int32), "n0": n0}, {}, np.zeros((16, 1), np.int32), np.zeros((1, n)),
                      np.arange(1, n + 1, dtype=np.int32), np.zeros(n))


def sample():
    K = int(np.ceil(np.sqrt(P)))
    amps = letters[rng.integers(0, 4, size=(K, 440))]
    seqsF = [a[:250].tobytes().decode() for a in amps]
    seqsR = [a[190:].tobytes().translate(comp)[::-1].decode() for a in amps]
    wrong = rng.choice(K * K - K, size=P - K, replace=False)         # mispairings: (i, j) with j != i
    wf, wr = wrong // (K - 1), wrong % (K - 1)
    wr = wr + (wr >= wf)
    pf, pr = np.concatenate([np.arange(K), wf]), np.concatenate([np.arange(K), wr])
    pick = np.concatenate([rng.permutation(P),                       # every unique pair once, then reads by weight
                           np.where(rng.random(N - P) < 0.9, rng.choice(K, size=N - P, p=rng.dirichlet(np.full(K, 0.3))), rng.integers(0, P, size=N - P))])
    f, r = pf[pick].astype(np.int32), pr[pick].astype(np.int32)
    f[rng.random(N) < 0.02] = -1
    r[rng.random(N) < 0.02] = -1
    f[-1], r[-1] = K - 1, K - 1                                      # (the last unique of either map is named)
    dereps = [Derep(["A"] * K, np.ones(K, np.int32), np.zeros((K, 1)), m) for m in (f, r)]
    return dada_of(seqsF, rng.integers(1, 200, K).astype(np.int32)), dereps[0], dada_of(seqsR, rng.integers(1, 200, K).astype(np.int32)), dereps[1]


t0 = time.perf_counter()
samples = [sample() for _ in range(S)]
cols = [[s[i] for s in samples] for i in range(4)]
out = {"samples": S, "unique_pairs": P, "reads": N, "generate_s": round(time.perf_counter() - t0, 3), "cores": os.cpu_count()}
note("generated", out["generate_s"], "s")
quiet = contextlib.redirect_stdout(io.StringIO())                   # ("Duplicate sequences in merged output.": the rejects' empty sequences)
with quiet:
    paired.merge_pairs(*[c[:2] for c in cols], return_rejects=True)  # (the library and the device, once, outside the clocks)
    api.merge_pairs(*samples[0], return_rejects=True)

run_walls, loop_walls, best = [], [], None
for rep in range(2):
    st = {}
    t0 = time.perf_counter()
    with quiet:
        got = paired.merge_pairs(*cols, return_rejects=True, stats=st)
    run_walls.append(round(time.perf_counter() - t0, 3))
    note("run-level", run_walls[-1], "s", st)
    if best is None or st["total_us"] < best["total_us"]:
        best = st
    t0 = time.perf_counter()
    loop = [api.merge_pairs(*s, return_rejects=True) for s in samples]
    loop_walls.append(round(time.perf_counter() - t0, 3))
    note("loop of api.merge_pairs", loop_walls[-1], "s")
    if rep == 0:
        if S == 1:
            got = [got]
        assert got == loop, "the two paths give different rows"
        out["rows_equal"] = True
        out["rows"] = sum(len(g) for g in got)
        out["accepted_reads"] = sum(r["abundance"] for g in got for r in g if r["accept"])
out["run_level_wall_s"] = run_walls
out["loop_wall_s"] = loop_walls
out["stats"] = best
chunks = max(best["chunks"], 1)
out["download_bytes_per_chunk"] = best["download_bytes"] // chunks
out["old_path_move_bytes_per_chunk"] = (best["unique_pairs"] // chunks) * (2 * 250 + 2)
line = json.dumps(out)
print(line)
if OUT:
    with open(OUT, "w") as fh:
        fh.write(line + "\n")
