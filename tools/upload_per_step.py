"""tools/upload_per_step.py <tag> [steps=40]: single boundary calls on bench.py's headline sample (1M uniques x 250 nt) after five
warm-up calls; prints one JSON line with the library's clocks of every call (ms_upload, ms_final, ms_total, ms_bookkeep, ms_setup,
ms_round0) and the call's wall time as its caller sees it: median, range, share of calls above 1.5 x median, every value.  Run it
once per build on one box to compare two builds (profiles/r25a_upload_per_step.jsonl)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

import bench  # noqa: E402


def main():
    tag, steps = sys.argv[1], int(sys.argv[2]) if len(sys.argv) > 2 else 40
    args = argparse.Namespace(uniques=0, length=0, variants=0, deep=False, shard=False)
    dereps, his, err, mine, c = bench.make_inputs(3, args, 0)
    from dada2_amd import api
    from dada2_amd.opts import DadaOpts
    opts = DadaOpts(BAND_SIZE=16)
    keys = ("ms_upload", "ms_final", "ms_total", "ms_bookkeep", "ms_setup", "ms_round0")
    rec = {k: [] for k in keys}
    rec["ms_wall"] = []
    for i in range(5 + steps):
        t0 = time.perf_counter()
        r = api.dada_uniques(his[0], None, None, err, None, opts)
        w = (time.perf_counter() - t0) * 1e3
        if i < 5:
            continue
        for k in keys:
            rec[k].append(round(float(r.stats.get(k, float("nan"))), 3))
        rec["ms_wall"].append(round(w, 3))
    out = {"tag": tag, "steps": steps, "partitions": int(r.nclust)}
    for k, v in rec.items():
        a = np.asarray(v)
        med = float(np.median(a))
        out[k] = {"median": round(med, 3), "min": float(a.min()), "max": float(a.max()),
                  "share_above_1.5x_median": float((a > 1.5 * med).mean()), "all": v}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
