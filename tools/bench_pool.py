#!/usr/bin/env python3
"""tools/bench_pool.py - pooled dada() at size (not bench.py's workload): the eight synthetic samples of BASELINE.json configs[3]
(8 x 250 000 uniques x 250 nt, half of each sample's true variants shared; dada2_amd.synth.make_shared_truth_samples).

    python tools/bench_pool.py [--uniques n] [--host-marshal PATH]

prints one JSON line:
  combine   dada2hip_derep_combine alone (the views are built before the clock starts), best of --repeats: wall time, the bytes of
            quality doubles it read and the rate; beside it, with --host-marshal (the program built from tools/host_marshal.cpp), the
            plain vector sum over a matrix of as many rows on --threads threads: the host's read bound for the same bytes
  match     dada2hip_sample_set_prior_seqs against the pooled resident sample for 10^3 and 10^5 prior sequences (half of them pooled
            uniques, half random), best of --repeats after a warm-up call, under DADA2HIP_PROFILE=1: the host's packing, the kernel by
            device events, the host's wall time from the first upload to the end of the copy back (the kernel inside it) and the call
  dada      one api.dada(..., pool=True) end to end (combine, upload, the pass, the split) beside api.dada(...) on the eight samples
            one after the other, both without selfConsist, same process
Records, not thresholds."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--uniques", type=int, default=0, help="uniques per sample (default: configs[3]'s 250 000)")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--host-marshal", default=None, help="path of the program built from tools/host_marshal.cpp")
    ap.add_argument("--priors", default="1000,100000", help="sizes of the prior lists")
    ap.add_argument("--no-dada", action="store_true")
    a = ap.parse_args()
    os.environ["DADA2HIP_PROFILE"] = "1"
    from dada2_amd import _lib, api
    from dada2_amd.io import extend_err
    from dada2_amd.synth import make_shared_truth_samples
    cfg = {"length": 250}
    err = extend_err(np.load(os.path.join(ROOT, "tests", "golden", "tperr1.npy")), 40)
    t0 = time.perf_counter()
    dereps = make_shared_truth_samples(err, a.uniques or 250_000, L=cfg["length"])
    out = {"what": "pooled dada() on BASELINE.json configs[3]'s inputs", "samples": len(dereps), "uniques_per_sample": dereps[0].nraw,
           "length": cfg["length"], "draw_s": round(time.perf_counter() - t0, 1)}
    L = _lib.lib()

    def note(msg):
        print("[bench_pool] " + msg, file=sys.stderr, flush=True)
    note("inputs drawn in %.0f s" % out["draw_s"])

    # ---- the combine ----
    keep = []
    views = (_lib.CDerepView * len(dereps))(*[api._derep_view(d, keep) for d in dereps])
    u2p = np.zeros(sum(d.nraw for d in dereps), dtype=np.int32)
    eb = C.create_string_buffer(2048)
    best, pooled = None, None
    for _ in range(a.repeats):
        h = C.c_void_p()
        t = time.perf_counter()
        _lib.check(L.dada2hip_derep_combine(len(dereps), views, C.byref(h), u2p.ctypes.data, eb, 2048), eb)
        ms = (time.perf_counter() - t) * 1e3
        best = ms if best is None else min(best, ms)
        if pooled is not None:
            pooled.close()
        pooled = api.NativeDerep._from_handle(h)
    qbytes = sum(8 * d.nraw * d.quals.shape[1] for d in dereps)
    out["combine"] = {"pooled_uniques": pooled.nuniques, "reads": int(pooled.nreads), "ms": round(best, 2), "quality_bytes_read": qbytes,
                      "quality_bytes_written": 8 * pooled.nuniques * pooled.maxlen, "read_GBps": round(qbytes / best / 1e6, 1),
                      "host_threads": "the library's pool (hostpar.h: from the CPU quota)"}
    if a.host_marshal:
        rows = sum(d.nraw for d in dereps)
        txt = subprocess.run([a.host_marshal, "--threads", str(a.threads), "--rows", str(rows), "--len", str(cfg["length"]), "--reps", "3"],
                             capture_output=True, text=True, timeout=600).stdout
        for line in txt.splitlines():
            f = line.split()
            if f and f[0] == "sum":
                out["combine"]["vector_sum"] = {"rows": rows, "threads": a.threads, "ms": float(f[1]), "read_GBps": float(f[2])}
                out["combine"]["combine_over_vector_sum"] = round(best / float(f[1]), 2)

    note("combine %.1f ms" % best)
    # ---- the match ----
    smp = api.Sample.from_native(pooled, None, 0)
    rng = np.random.default_rng(7)
    sp = L.dada2hip_derep_seqs(pooled._h)
    out["match"] = []
    for n in [int(x) for x in a.priors.split(",")]:
        pick = rng.choice(pooled.nuniques, size=min(n // 2, pooled.nuniques), replace=False)
        pri = [sp[int(i)].decode() for i in pick] + ["".join("ACGT"[int(x)] for x in rng.integers(0, 4, size=cfg["length"])) for _ in range(n - pick.size)]
        smp.set_prior_seqs(pri)
        rec = None
        for _ in range(a.repeats):
            t = time.perf_counter()
            nset = smp.set_prior_seqs(pri)
            py_ms = (time.perf_counter() - t) * 1e3
            st = smp.prior_seqs_stats()
            if rec is None or st["total_us"] < rec["call_us"]:
                rec = {"priors": n, "flags_set": nset, "keys": st["keys"], "keys_in_lds": st["keys_in_lds"], "blocks": st["blocks"],
                       "pack_us": st["pack_us"], "kernel_device_us": st["kernel_device_us"], "uploads_kernel_copy_back_us": st["device_us"],
                       "call_us": st["total_us"], "python_call_ms": round(py_ms, 2)}
        assert rec["flags_set"] == pick.size, rec
        out["match"].append(rec)
        note("match %d: %s" % (n, rec))
    smp.close()
    pooled.close()

    # ---- dada(pool=True) beside the eight independent calls ----
    if not a.no_dada:
        recs = {}
        for name, kw in (("independent", {}), ("pooled", {"pool": True}), ("independent_again", {}), ("pooled_again", {"pool": True})):
            tm = []
            t = time.perf_counter()
            res, _, _ = api.dada(dereps, err, timings=tm, **kw)
            recs[name] = {"ms": round((time.perf_counter() - t) * 1e3, 1), "upload_ms": round(tm[0], 1), "pass_ms": round(tm[1], 1),
                          "partitions": [r.nclust for r in res]}
            note("dada %s: %.0f ms" % (name, recs[name]["ms"]))
        out["dada"] = recs
    print(json.dumps(out))


if __name__ == "__main__":
    main()
