#!/usr/bin/env python3
"""tools/species_bench.py - assignSpecies at size (not bench.py's workload): --families families x --variants references of
--reflen nt (a family's members are copies of one ancestor with 1 % substitutions, so near-misses exist; 0.1 % of the letters are
N) and --queries queries of --qlen nt: a third cut from references, a third cut and changed at one base, a third random.

    python tools/species_bench.py

prints one JSON line: the time to open the references, the match call with try_rc off and on (best of --repeats after a warm-up
call) with its split from the call's stats, the share of windows that passed the presence bitmap, the seed kernel's rate against
the resident blob, and the restatement of tests/species_cases.py (``q in r`` on Python strings, ONE host thread) on the first
--prefix queries with equal results asserted.  One thread against one GPU: not a like-for-like ratio, and not the reference's
R + Biostrings, which this tool cannot run."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def synth(families, variants, reflen, queries, qlen, seed):
    rng = np.random.RandomState(seed)
    letters = np.frombuffer(b"ACGTN", dtype=np.uint8)
    anc = rng.randint(0, 4, (families, reflen)).astype(np.uint8)
    ref = np.repeat(anc, variants, axis=0)
    sub = rng.random_sample(ref.shape) < 0.01
    ref = np.where(sub, rng.randint(0, 4, ref.shape).astype(np.uint8), ref)
    ref[rng.random_sample(ref.shape) < 0.001] = 4
    pick = rng.randint(0, ref.shape[0], queries)
    off = rng.randint(0, reflen - qlen + 1, queries)
    q = np.stack([ref[p, o: o + qlen] for p, o in zip(pick, off)])
    q = np.where(q == 4, rng.randint(0, 4, q.shape).astype(np.uint8), q)           # (a query holds A/C/G/T only)
    kind = np.arange(queries) % 3                                                  # 0 cut, 1 cut and changed at one base, 2 random
    for j in np.nonzero(kind == 1)[0]:
        i = rng.randint(qlen)
        q[j, i] = (q[j, i] + 1 + rng.randint(3)) % 4
    q[kind == 2] = rng.randint(0, 4, (int((kind == 2).sum()), qlen)).astype(np.uint8)
    to_s = lambda m: [letters[row].tobytes().decode() for row in m]   # noqa: E731
    return to_s(ref), to_s(q)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--families", type=int, default=10000)
    ap.add_argument("--variants", type=int, default=10)
    ap.add_argument("--reflen", type=int, default=1400)
    ap.add_argument("--queries", type=int, default=5000)
    ap.add_argument("--qlen", type=int, default=250)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--prefix", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    from dada2_amd import api
    import species_cases as sc
    refs, qs = synth(a.families, a.variants, a.reflen, a.queries, a.qlen, a.seed)
    rec = {"tool": "species_bench", "references": len(refs), "reflen": a.reflen, "queries": a.queries, "qlen": a.qlen, "seed": a.seed}
    t0 = time.perf_counter()
    m = api.SpeciesModel((refs, ["r%d Genus%d species%d" % (i, i // a.variants, i) for i in range(len(refs))]))
    rec.update(open_s=round(time.perf_counter() - t0, 4), open_library_s=m.stats["total_us"] / 1e6, resident_bytes=m.stats["resident_bytes"])
    runs, results = {}, {}
    for label, t in (("try_rc_off", False), ("try_rc_on", True)):
        best = None
        for _ in range(1 + a.repeats):                           # (the first call warms the allocation cache)
            st = {}
            t0 = time.perf_counter()
            hits = api.species_hits(qs, m, try_rc=t, stats=st)
            wall = time.perf_counter() - t0
            if best is None or wall < best[0]:
                best = (wall, st)
        wall, st = best
        results[t] = hits
        seed_s = st["seed_device_us"] / 1e6
        runs[label] = dict(match_s=round(wall, 4), library_s=st["total_us"] / 1e6, seed_host_s=st["seed_host_us"] / 1e6, seed_device_s=seed_s,
                           verify_host_s=st["verify_host_us"] / 1e6, verify_device_s=st["verify_device_us"] / 1e6, launches=st["launches"],
                           windows=st["windows"], windows_past_bitmap=st["windows_past_bitmap"],
                           share_past_bitmap=round(st["windows_past_bitmap"] / max(st["windows"], 1), 5), candidates=st["candidates"],
                           candidate_reruns=st["candidate_reruns"], hits=st["hits"],
                           queries_with_a_hit=int(sum(1 for h in hits if len(h))),
                           seed_blob_GBps=round(m.stats["resident_bytes"] / max(seed_s, 1e-9) / 1e9, 2),
                           seed_Gwindows_per_s=round(st["windows"] / max(seed_s, 1e-9) / 1e9, 3))
    m.close()
    sub = qs[: a.prefix]
    t0 = time.perf_counter()
    want = sc.restate_hits(sub, refs, try_rc=True)
    t_host = time.perf_counter() - t0
    assert [[int(x) for x in h] for h in results[True][: len(sub)]] == want, "the library and the restatement differ"
    assert [[int(x) for x in h] for h in results[False][: len(sub)]] == sc.restate_hits(sub, refs, try_rc=False)
    rec.update(runs=runs, restatement=dict(threads=1, prefix=len(sub), try_rc=True, prefix_s=round(t_host, 3),
                                           ms_per_query=round(t_host / max(len(sub), 1) * 1e3, 2),
                                           all_queries_s_extrapolated=round(t_host / max(len(sub), 1) * a.queries, 1), equal=True))
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
