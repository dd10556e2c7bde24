#!/usr/bin/env python3
"""tools/resident_bench.py - from a file of reads to a sample that is ready to run, both ways (not bench.py's workload).

    python tools/resident_bench.py file      # DESIGN 8j's input: --reads reads x --len nt, a plain file, trunc_len 240, max_ee 2, filt=None
    python tools/resident_bench.py samples   # DESIGN 8g's inputs: --samples samples of --uniques uniques, fed as reads in memory

The parent's route - dereplicate.filter_and_derep (derep_reads) + Sample.from_native - and the resident route -
dereplicate.filter_and_sample (derep_reads_resident) - alternate in one process, --repeats times each; per route the best wall
time, every wall time (the spread), and the stats words of the best run, the resident route's resident_* words among them.
One JSON document on stdout.  `file` draws its reads as DESIGN 8j says: variants from dada2_amd.synth, 0.09 % substitutions,
qualities that decay along the read (tools/filter_bench.py's model).  `samples` takes synth.make_shared_truth_samples' uniques
and writes every unique out `abundance` times with its rounded mean qualities as the characters."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def file_reads(n, ln, seed):
    from dada2_amd import synth
    rng = np.random.default_rng(seed)
    codes, _ = synth.true_variants(rng, 256, ln)
    which = np.minimum(rng.zipf(1.3, size=n) - 1, 255)
    seq = np.asarray(codes, dtype=np.uint8)[which]
    sub = rng.random((n, ln)) < 0.0009
    seq = np.where(sub, (seq + rng.integers(1, 4, (n, ln), dtype=np.uint8)) & 3, seq)
    seq = np.frombuffer(b"ACGT", dtype=np.uint8)[seq]
    pos = np.arange(ln) / ln
    level = rng.uniform(0.3, 1.6, (n, 1))
    q = 38 - 22 * level * pos[None, :] ** 2 + rng.normal(0, 3, (n, ln))
    return seq, (np.clip(np.rint(q), 3, 40) + 33).astype(np.uint8)


def alternate(repeats, routes):
    """routes: {name: callable -> (stats dict, closer)}; the routes alternate, each --repeats times."""
    out = {k: dict(wall_ms=[]) for k in routes}
    for _ in range(repeats):
        for name, f in routes.items():
            t0 = time.perf_counter()
            st, close = f()
            ms = (time.perf_counter() - t0) * 1e3
            close()
            if not out[name]["wall_ms"] or ms < min(out[name]["wall_ms"]):
                out[name]["stats"] = st
            out[name]["wall_ms"].append(round(ms, 2))
    for v in out.values():
        v["best_ms"] = min(v["wall_ms"])
    return out


def mode_file(a):
    from filter_bench import write_fastq
    from dada2_amd import api, dereplicate as dd
    seq, qual = file_reads(a.reads, a.len, a.seed)
    args = dict(trunc_len=240, max_ee=2, n=a.n)
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "reads.fastq")
        write_fastq(path, seq, qual)
        ctx = api.FilterContext(None)

        def parent():
            st = {}
            _, nd = dd.filter_and_derep(path, None, stats=st, ctx=ctx, **args)
            t = time.perf_counter()
            smp = api.Sample.from_native(nd)
            st["sample_from_native_ms"] = round((time.perf_counter() - t) * 1e3, 2)
            return st, lambda: (smp.close(), nd.close())

        def resident():
            st = {}
            _, rd = dd.filter_and_sample(path, None, stats=st, ctx=ctx, **args)
            return st, rd.close
        parent()[1]()                                             # (the first call of a process: allocations, module load)
        res = alternate(a.repeats, {"parent_route": parent, "resident_route": resident})
        ctx.close()
    return dict(mode="file", reads=a.reads, length=a.len, filter=dict(trunc_len=240, max_ee=2), chunk_reads=a.n, routes=res)


def derep_blob(resident, sb, qb, off, st):
    """dada2hip_derep_reads / _resident on reads that already lie in one buffer (dereplicate.derep_reads joins a list first)."""
    import ctypes as C
    from dada2_amd import _lib, api, dereplicate as dd
    h, hs, eb = C.c_void_p(), C.c_void_p(), C.create_string_buffer(2048)
    ds = np.zeros(_lib.DEREP_NSTATS, dtype=np.int64)
    rs = np.zeros(_lib.RESIDENT_NSTATS, dtype=np.int64)
    L = _lib.lib()
    if resident:
        _lib.check(L.dada2hip_derep_reads_resident(len(off) - 1, sb, qb, off.ctypes.data, 10 ** 6, 33, 0, C.byref(h), C.byref(hs), ds.ctypes.data,
                                                   rs.ctypes.data, eb, 2048), eb)
        for i, k in enumerate(dd.RESIDENT_STATS):
            st["resident_" + k] = st.get("resident_" + k, 0) + int(rs[i])
    else:
        _lib.check(L.dada2hip_derep_reads(len(off) - 1, sb, qb, off.ctypes.data, 10 ** 6, 33, 0, C.byref(h), ds.ctypes.data, eb, 2048), eb)
    for i, k in enumerate(dd.STATS):
        st[k] = st.get(k, 0) + int(ds[i])
    return dd.ResidentDerep._from_handles(h, hs, 0) if resident else api.NativeDerep._from_handle(h)


def mode_samples(a):
    from dada2_amd import api, synth
    err = np.load(os.path.join(ROOT, "tests", "golden", "tperr1.npy"))
    inputs = []
    for d in synth.make_shared_truth_samples(err, n_uniques=a.uniques, nsamples=a.samples, L=a.len):
        ab = np.asarray(d.abundances, dtype=np.int64)
        seqs = np.frombuffer("".join(d.seqs).encode(), dtype=np.uint8).reshape(len(d.seqs), -1)
        q = (np.rint(np.asarray(d.quals)) + 33).astype(np.uint8)
        rows = np.repeat(np.arange(len(ab)), ab)
        np.random.default_rng(a.seed).shuffle(rows)
        inputs.append((seqs[rows].tobytes(), q[rows].tobytes(), np.arange(len(rows) + 1, dtype=np.int64) * seqs.shape[1]))

    def parent():
        st = {}
        nds = [derep_blob(False, sb, qb, off, st) for sb, qb, off in inputs]
        t = time.perf_counter()
        smps = [api.Sample.from_native(nd) for nd in nds]
        st["sample_from_native_ms"] = round((time.perf_counter() - t) * 1e3, 2)
        return st, lambda: [o.close() for o in smps + nds]

    def resident():
        st = {}
        rds = [derep_blob(True, sb, qb, off, st) for sb, qb, off in inputs]
        return st, lambda: [o.close() for o in rds]
    parent()[1]()
    res = alternate(a.repeats, {"parent_route": parent, "resident_route": resident})
    return dict(mode="samples", samples=a.samples, uniques=a.uniques, length=a.len, reads=[len(i[2]) - 1 for i in inputs], routes=res)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=("file", "samples"))
    ap.add_argument("--reads", type=int, default=10 ** 6)
    ap.add_argument("--len", type=int, default=250)
    ap.add_argument("--n", type=int, default=10 ** 5)
    ap.add_argument("--samples", type=int, default=8)
    ap.add_argument("--uniques", type=int, default=250000)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    print(json.dumps(mode_file(a) if a.mode == "file" else mode_samples(a), indent=1, sort_keys=True))


if __name__ == "__main__":
    main()
