#!/usr/bin/env python3
"""mergeSequenceTables at a study-like size: T tables of C columns of 250-420 nt and R rows each, a third of
every table's sequences shared by all tables, half of the tables in the other orientation, try_rc on.  Times three calls of
dada2_amd.seqtables.merge_sequence_tables and prints, as one JSON line, the stats words of the best, the wall time of a host
np.add.at with the same row and column maps (what k_st_accumulate does), and - where the host has the memory for its 64-bit
matrix - the wall time of the dict-based specification of tests/seqtab_cases.py, whose result the device's must then equal.
The column sums of the result are always checked against the inputs' through the column map.
Usage: seqtab_bench.py [tables=64] [columns=20000] [rows=48] [out.json]"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
T = int(sys.argv[1]) if len(sys.argv) > 1 else 64
NCOL = int(sys.argv[2]) if len(sys.argv) > 2 else 20000
NROW = int(sys.argv[3]) if len(sys.argv) > 3 else 48
OUT = sys.argv[4] if len(sys.argv) > 4 else None

from dada2_amd import seqtables as st  # noqa: E402

rng = np.random.default_rng(812)


def note(*a):
    print(*a, file=sys.stderr, flush=True)


letters = np.frombuffer(b"ACGT", dtype=np.uint8)


def sequences(n):
    lens = rng.integers(250, 421, size=n)
    text = letters[rng.integers(0, 4, size=int(lens.sum()))].tobytes().decode("ascii")
    ends = np.cumsum(lens).tolist()
    return [text[e - k:e] for e, k in zip(ends, lens.tolist())]


t0 = time.perf_counter()
shared = sequences(NCOL // 3)
tables = []
for t in range(T):
    cols = shared + sequences(NCOL - len(shared))
    cols = [cols[i] for i in rng.permutation(len(cols)).tolist()]
    if t % 2:
        cols = [st.rc(s) for s in cols]
    cells = rng.integers(1, 5000, size=(NROW, NCOL), dtype=np.int32) * (rng.random((NROW, NCOL)) < 0.3)
    tables.append((np.ascontiguousarray(cells, dtype=np.int32), cols, ["run%d_s%d" % (t, i) for i in range(NROW)]))
out = {"tables": T, "columns": NCOL, "rows": NROW, "generate_s": round(time.perf_counter() - t0, 3), "cores": os.cpu_count()}

note("generated", out["generate_s"], "s")
best, calls = None, []
for _ in range(3):
    s = {}
    t0 = time.perf_counter()
    mat, seqs, names = st.merge_sequence_tables(tables, try_rc=True, stats=s)
    wall = time.perf_counter() - t0
    calls.append(round(wall, 3))
    note("call", wall, "s", {k: v for k, v in s.items() if k != "col_map"})
    if best is None or s["total_us"] < best["total_us"]:
        best = dict(s)
        best["python_wall_s"] = round(wall, 3)
col_map = best.pop("col_map")
out["calls_wall_s"] = calls
out["best"] = best

# the column sums through the column map
want = np.zeros(len(seqs), dtype=np.int64)
np.add.at(want, col_map, np.concatenate([m.sum(axis=0, dtype=np.int64) for m, _, _ in tables]))
got = mat.sum(axis=0, dtype=np.int64)
assert np.array_equal(got, want), "column sums"
assert np.all(got[:-1] >= got[1:]), "not ordered by decreasing sum"
out["column_sums_checked"] = True

# the host's np.add.at with the same maps
t0 = time.perf_counter()
host = np.zeros(mat.shape, dtype=np.int32)
c0 = 0
for t, (m, cols, rows) in enumerate(tables):
    np.add.at(host, (np.arange(t * NROW, (t + 1) * NROW)[:, None], col_map[c0:c0 + len(cols)][None, :]), m)
    c0 += len(cols)
out["host_add_at_s"] = round(time.perf_counter() - t0, 3)
note("host np.add.at", out["host_add_at_s"], "s")
assert np.array_equal(host, mat), "the host's adds give another matrix"
out["cells_checked"] = True
del host

avail = 0
with open("/proc/meminfo") as fh:
    for line in fh:
        if line.startswith("MemAvailable:"):
            avail = int(line.split()[1]) * 1024
if avail > 16 * mat.size + (8 << 30):
    import seqtab_cases as sc
    t0 = time.perf_counter()
    spec = sc.spec_merge_fast(tables, try_rc=True)
    out["spec_merge_fast_s"] = round(time.perf_counter() - t0, 3)
    sc.same((mat, seqs, names, col_map), spec, "the specification")
    out["equals_specification"] = True
else:
    out["spec_merge_fast_s"] = None
line = json.dumps(out)
print(line)
if OUT:
    with open(OUT, "w") as fh:
        fh.write(line + "\n")
