#!/usr/bin/env python3
"""Timing of isBimeraDenovo on a pooled uniques vector: dada2hip_bimera_denovo (parents as a prefix of the ranking, windows of ranks,
the fold on the device) against the only route the library had to the same flags before it - a one-row dada2hip_table_bimera2 with
min_abund = minParentAbundance + 1 -, same vector, flags compared.  The vector is the column sums of bench_bimera.make_table.
Usage: bench_bimera_denovo.py [nseq] [L] [repeats]        prints one JSON line
Environment: BIMERA_NO_TABLE=1 leaves the one-row table call out; BIMERA_REF_NSEQ=n also runs the reference's loop (oracle/_ref,
C_is_bimera on 16 threads) on n sequences of the vector taken at equal steps, where oracle/_ref has been built."""
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools")]


def make_vector(nseq=8000, L=250, nsam=8, seed=7):
    """(sequences, int32 abundances): the column sums of bench_bimera.make_table, columns without a count left out."""
    from bench_bimera import make_table
    mat, seqs = make_table(nseq, nsam, L, seed)
    ab = mat.sum(axis=0, dtype=np.int64)
    keep = ab > 0
    return [s for s, k in zip(seqs, keep) if k], ab[keep].astype(np.int32)


def _timed(fn, repeats):
    ts, out = [], None
    for _ in range(repeats):
        t0 = time.perf_counter()
        out = fn()
        ts.append(time.perf_counter() - t0)
    return out, {"median_s": statistics.median(ts), "min_s": min(ts), "max_s": max(ts), "all_s": ts}


def reference_loop(seqs, ab, threads=16):
    """The loop of R/chimeras.R:124-148 over the reference's C_is_bimera, `threads` queries at a time."""
    from concurrent.futures import ThreadPoolExecutor
    from oracle import ref
    ref.lib()

    def one(i):
        pars = [seqs[k] for k in range(len(seqs)) if ab[k] > 2 * ab[i] and ab[k] > 8]
        return False if len(pars) < 2 else bool(ref.is_bimera(seqs[i], pars))
    with ThreadPoolExecutor(threads) as ex:
        return list(ex.map(one, range(len(seqs))))


def record(api, nseq=8000, L=250, repeats=5, device=0, table=True, ref_nseq=0):
    seqs, ab = make_vector(nseq, L)
    api.is_bimera_denovo((seqs[:64], ab[:64]), device=device)             # warm-up (context, allocation cache)
    st = {}
    flags, t_new = _timed(lambda: api.is_bimera_denovo((seqs, ab), device=device, stats=st), repeats)
    out = {"what": "isBimeraDenovo (R/chimeras.R:105) on a pooled uniques vector", "nseq": len(seqs), "L": L, "repeats": repeats,
           "bimera_denovo": t_new, "flagged": int(flags.sum()), "stats": st,
           "aligned_over_possible": st["pairs_aligned"] / max(1, st["pairs_possible"])}
    if table:
        m = ab.reshape(1, -1)
        api.table_bimera2(m[:, :64], seqs[:64], min_fold=2, min_abund=9, device=device)
        (nflag, _), t_tab = _timed(lambda: api.table_bimera2(m, seqs, min_fold=2, min_abund=9, device=device), repeats)
        out["one_row_table_bimera2"] = t_tab
        out["flags_equal"] = bool(np.array_equal(nflag > 0, flags))
        out["speedup_median"] = t_tab["median_s"] / t_new["median_s"]
    if ref_nseq:
        from oracle import ref
        if ref.available():
            step = max(1, len(seqs) // ref_nseq)
            s2, a2 = seqs[::step][:ref_nseq], ab[::step][:ref_nseq]
            t0 = time.perf_counter()
            want = reference_loop(s2, a2)
            out["reference_16_threads"] = {"nseq": len(s2), "s": time.perf_counter() - t0}
            got, t_sub = _timed(lambda: api.is_bimera_denovo((s2, a2), device=device), 1)
            out["reference_16_threads"].update(bimera_denovo_s=t_sub["median_s"], equal=bool(got.tolist() == want), flagged=int(sum(want)))
    return out


if __name__ == "__main__":
    nseq = int(sys.argv[1]) if len(sys.argv) > 1 else 8000
    L = int(sys.argv[2]) if len(sys.argv) > 2 else 250
    repeats = int(sys.argv[3]) if len(sys.argv) > 3 else 5
    from dada2_amd import api
    print(json.dumps(record(api, nseq, L, repeats, table=not os.environ.get("BIMERA_NO_TABLE"),
                            ref_nseq=int(os.environ.get("BIMERA_REF_NSEQ", "0")))))
