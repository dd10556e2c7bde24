#!/usr/bin/env python3
"""Timing of collapseNoMismatch (R/multiSample.R:104-160) on a synthetic sequence table of 250-nt amplicons: families of true
variants (dada2_amd.synth.true_variants: roots at 3-25 % from one ancestor, seven variants at Hamming 1-7 each) and, for every
one of them, a copy trimmed or extended at either end - the columns that collapse.

    collapse_bench.py [--compare N] [--device-only M] [--out FILE]

--compare N      dada2hip_collapse_nomismatch on N columns against the restatement of the reference's loop
                 (tests/collapse_cases.py) over the reference compiled in place (oracle/_ref) where it is there, else over the
                 plain-C oracle; the results must be equal, both are timed (default 2 000)
--device-only M  the device path alone on M columns (default 20 000)
One JSON line (with --out: written to FILE, added to the line a previous run left there): the library's counters and its host
clocks per stage (join, scan, align, resolve) of both runs, and the totals."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def make_table(ncol, nsam=4, L=250, seed=11):
    from dada2_amd.synth import true_variants
    rng = np.random.default_rng(seed)
    G = (ncol + 1) // 2
    codes, _ = true_variants(rng, (G + 7) // 8 * 8, L)
    full = list(dict.fromkeys("".join("ACGT"[int(x)] for x in row) for row in codes))[:G]
    seqs = list(full)
    seen = set(seqs)
    k = 0
    while len(seqs) < ncol:
        s = full[k % len(full)]
        k += 1
        a, b = int(rng.integers(0, 12)), int(rng.integers(0, 12))
        kind = int(rng.integers(0, 3))
        v = s[a: L - b] if kind == 0 else ("".join("ACGT"[int(x)] for x in rng.integers(0, 4, size=a)) + s[: L - b] if kind == 1
                                         else s[a:] + "".join("ACGT"[int(x)] for x in rng.integers(0, 4, size=b)))
        if v not in seen:
            seen.add(v)
            seqs.append(v)
    order = rng.permutation(len(seqs))
    seqs = [seqs[int(i)] for i in order]
    mat = (rng.zipf(1.6, size=(nsam, len(seqs))) % 5000) * (rng.random((nsam, len(seqs))) < 0.6)
    mat[0, mat.sum(axis=0) == 0] = 1
    return mat.astype(np.int32), seqs


def device_run(api, mat, seqs, device=0):
    st = {}
    t0 = time.perf_counter()
    out = api.collapse_no_mismatch(mat, seqs, stats=st, device=device)
    wall = (time.perf_counter() - t0) * 1e3
    st.pop("into")
    rec = {k: v for k, v in st.items() if not k.endswith("_us")}
    rec.update({"ms_" + k[:-3]: round(v / 1e3, 3) for k, v in st.items() if k.endswith("_us")})
    rec.update(columns=len(seqs), kept=len(out[1]), ms_call=round(wall, 3))
    return out, rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--compare", type=int, default=2000)
    ap.add_argument("--device-only", type=int, default=20000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from dada2_amd import api
    import collapse_cases as cc
    from oracle import cport, ref
    rec = {"what": "collapseNoMismatch (R/multiSample.R:104-160) on synthetic 250-nt sequence tables, 4 samples, minOverlap 20"}
    warm = make_table(64)
    api.collapse_no_mismatch(*warm)                                  # context, allocation cache
    if a.compare > 0:
        mat, seqs = make_table(a.compare)
        got, r = device_run(api, mat, seqs)
        checker = cc.checker_for(cport, ref)
        t0 = time.perf_counter()
        want = cc.restate(mat, seqs, checker)
        r["ms_restatement"] = round((time.perf_counter() - t0) * 1e3, 1)
        r["restatement_over"] = "oracle/_ref (C_nwvec)" if checker is ref else "plain-C oracle"
        cc.assert_same_table(got, want, "collapse_bench --compare")
        r["equal"] = True
        rec["compare"] = r
    if a.device_only > 0:
        mat, seqs = make_table(a.device_only)
        _, rec["device_only"] = device_run(api, mat, seqs)
    if a.out and os.path.exists(a.out):                             # (the two runs as two commands: the second adds to the first's line)
        with open(a.out) as fh:
            prev = json.loads(fh.read() or "{}")
        prev.update(rec)
        rec = prev
    line = json.dumps(rec)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
