#!/usr/bin/env python3
"""tools/taxonomy_bench.py - assignTaxonomy at size (not bench.py's workload): a synthetic model of --genera genera x --refs
references of --reflen nt and --queries queries of --qlen nt, cut from the references with 3 % substitutions.

    python tools/taxonomy_bench.py device                 train / upload / assign times of the library, and the share of the assign
                                                          call in each kernel instance; a second assign under DADA2HIP_TAX_SLAB=0
                                                          (every query through the gather instance) for the slab / gather comparison
    python tools/taxonomy_bench.py reference --prefix N   the reference's own src/taxonomy.cpp, compiled by the recipe of
                                                          tests/golden/make_taxonomy_golden.py, on the first N queries on this
                                                          machine's CPU, --threads threads (the recipe's default is one)
Each prints one JSON line.  The two modes build the same model and queries from --seed."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def synth(genera, refs_per, reflen, queries, qlen, seed):
    rng = np.random.RandomState(seed)
    letters = np.frombuffer(b"ACGT", dtype=np.uint8)

    def mutate(a, rate):
        hit = rng.random_sample(a.shape) < rate
        return np.where(hit, rng.randint(0, 4, a.shape).astype(np.uint8), a)
    anc = rng.randint(0, 4, (genera, reflen)).astype(np.uint8)
    ref = mutate(np.repeat(anc, refs_per, axis=0), 0.02)
    r2g = np.repeat(np.arange(genera, dtype=np.int32), refs_per)
    pick = rng.randint(0, ref.shape[0], queries)
    off = rng.randint(0, reflen - qlen + 1, queries)
    q = mutate(np.stack([ref[p, o: o + qlen] for p, o in zip(pick, off)]), 0.03)
    to_s = lambda m: [letters[row].tobytes().decode() for row in m]   # noqa: E731
    genusmat = np.stack([np.zeros(genera, np.int32), np.arange(genera, dtype=np.int32) % 7, np.arange(genera, dtype=np.int32) % 91,
                         np.arange(genera, dtype=np.int32)], axis=1).astype(np.int32)
    return to_s(ref), r2g, genusmat, to_s(q), r2g[pick]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=("device", "reference"))
    ap.add_argument("--genera", type=int, default=2000)
    ap.add_argument("--refs", type=int, default=10)
    ap.add_argument("--reflen", type=int, default=1400)
    ap.add_argument("--queries", type=int, default=5000)
    ap.add_argument("--qlen", type=int, default=250)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--prefix", type=int, default=100)
    ap.add_argument("--threads", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    refs, r2g, gm, qs, truth = synth(a.genera, a.refs, a.reflen, a.queries, a.qlen, a.seed)
    rec = {"tool": "taxonomy_bench", "mode": a.mode, "genera": a.genera, "refs_per_genus": a.refs, "reflen": a.reflen, "queries": a.queries,
           "qlen": a.qlen, "seed": a.seed}
    if a.mode == "reference":
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
        import make_taxonomy_golden as mk
        import taxonomy_cases as tc
        sub = qs[: a.prefix]
        unifs = tc.unif_buffer(a.seed, tc.n_unifs(sub))
        with tempfile.TemporaryDirectory() as tmp:
            L = mk.build_ref(tmp)
            t0 = time.perf_counter()
            one = mk.run_ref(L, refs, r2g, gm, sub[:1], tc.unif_buffer(a.seed, tc.n_unifs(sub[:1])), nthreads=a.threads)   # (the model + one query)
            t_model = time.perf_counter() - t0
            t0 = time.perf_counter()
            res = mk.run_ref(L, refs, r2g, gm, sub, unifs, nthreads=a.threads)
            t_all = time.perf_counter() - t0
        del one
        per_query = (t_all - t_model) / max(len(sub) - 1, 1)
        rec.update(threads=a.threads, prefix=len(sub), model_and_one_query_s=round(t_model, 3), prefix_call_s=round(t_all, 3),
                   assign_ms_per_query=round(per_query * 1e3, 3), assign_s_extrapolated=round(per_query * a.queries, 1),
                   genus_correct=float((res["tax"] == truth[: len(sub)]).mean()))
    else:
        from dada2_amd import api
        t0 = time.perf_counter()
        m = api.TaxonomyModel.from_parsed(refs, ["g%d;" % g for g in range(a.genera)], r2g, gm)
        t_train = time.perf_counter() - t0
        rec.update(train_s=round(t_train, 3), train_build_s=m.stats["build_us"] / 1e6, train_upload_s=m.stats["upload_us"] / 1e6,
                   table_bytes=m.stats["table_bytes"])
        runs = {}
        for label, env in (("default", {}), ("gather_only", {"DADA2HIP_TAX_SLAB": "0"})):
            os.environ.pop("DADA2HIP_TAX_SLAB", None)
            os.environ.update(env)
            best = None
            for _ in range(1 + a.repeats):                       # (the first call warms the allocation cache)
                st = {}
                t0 = time.perf_counter()
                raw = api.assign_taxonomy_raw(qs, m, seed=a.seed, stats=st)
                wall = time.perf_counter() - t0
                if best is None or wall < best[0]:
                    best = (wall, st)
            wall, st = best
            runs[label] = dict(assign_s=round(wall, 4), prepare_s=st["prepare_us"] / 1e6, slab_queries=st["slab_queries"],
                               gather_queries=st["gather_queries"], slab_device_s=st["slab_device_us"] / 1e6,
                               gather_device_s=st["gather_device_us"] / 1e6,
                               share_slab=round(st["slab_device_us"] / 1e6 / wall, 3), share_gather=round(st["gather_device_us"] / 1e6 / wall, 3),
                               genus_correct=float((raw["tax"] == truth).mean()), tied_entries=float((raw["ntie"] > 1).mean()))
        os.environ.pop("DADA2HIP_TAX_SLAB", None)
        m.close()
        rec.update(runs=runs, slab_not_slower=bool(runs["default"]["slab_device_s"] <= runs["gather_only"]["gather_device_s"]))
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
