#!/usr/bin/env python3
"""tools/readqc_bench.py - the read diagnostics at size (not bench.py's workload): a synthetic FASTQ of --reads reads of --length
nt, A/C/G/T with a low-complexity stretch in one read of ten, qualities that fall off towards the end of the read.

    python tools/readqc_bench.py        # on the GPU

prints one JSON line:
  table       dada2hip_qprofile_reads on the quality strings in memory (best of --repeats by the library's clock): library time,
              the kernel's device time from its events, the quality bytes per second of kernel time beside the memory's rate;
  window      dada2hip_complexity_reads with window 25, by 5 likewise, with the windows per second of kernel time;
  files       dada2hip_qprofile_fastq and dada2hip_complexity_fastq from plain and from gzip input, each with the library's clocks
              and the share of the wall time that parsing, inflate and the kernels are (the parser runs under the chunk before
              it, so the shares need not add up to one);
  restatement tests/readqc_cases.py's numpy restatements over the first --prefix reads: equal tables, and the largest relative
              difference of a windowed complexity."""
import argparse
import gzip
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

HBM_GBS = 6300.0              # HBM3E, achievable (a float4 copy)


def synth(n, length, seed):
    """(seqs, quals): lists of bytes."""
    rng = np.random.RandomState(seed)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    mat = acgt[rng.randint(0, 4, (n, length))]
    low = np.flatnonzero(rng.random_sample(n) < 0.1)
    start = rng.randint(0, max(1, length - 60), len(low))
    for i, s in zip(low, start):
        mat[i, s:s + 60] = acgt[rng.randint(2, 4, 60)]
    mean = np.linspace(38, 22, length)
    pool = np.clip(np.rint(rng.normal(mean, 4, (min(n, 50000), length))), 2, 41).astype(np.uint8) + 33   # (50 000 distinct quality strings)
    return [r.tobytes() for r in mat], [pool[i % len(pool)].tobytes() for i in range(n)]


def best_of(repeats, call, key="total_us"):
    best = None
    for _ in range(repeats):
        st = {}
        t0 = time.perf_counter()
        got = call(st)
        wall = time.perf_counter() - t0
        if best is None or st[key] < best[1][key]:
            best = (wall, st, got)
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=10**6)
    ap.add_argument("--file-reads", type=int, default=250000, help="the first of the reads that go into the files")
    ap.add_argument("--length", type=int, default=250)
    ap.add_argument("--window", type=int, default=25)
    ap.add_argument("--by", type=int, default=5)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--prefix", type=int, default=2000)
    a = ap.parse_args()
    import readqc_cases as rc
    from dada2_amd import readqc as rq
    seqs, quals = synth(a.reads, a.length, a.seed)
    nbytes = a.reads * a.length
    keys = ("open_inflate_us", "parse_us", "upload_us", "kernel_device_us", "download_us", "total_us", "upload_bytes", "pieces", "cycles")
    rec = {"tool": "readqc_bench", "reads": a.reads, "length": a.length, "bases": nbytes, "seed": a.seed, "params": {"window": a.window, "by": a.by}}

    rq.quality_table(quals[:1000])                                 # (the runtime and the code object are up)
    rq.seq_complexity(seqs[:1000], window=a.window, by=a.by)
    wall, st, tab = best_of(a.repeats, lambda st: rq.quality_table(quals, stats=st))
    lib_s, dev_s = st["total_us"] / 1e6, st["kernel_device_us"] / 1e6
    rec["table"] = dict(python_wall_s=round(wall, 4), library_s=lib_s, kernel_s=dev_s, reads_per_s_library=round(a.reads / lib_s),
                        gb_per_s_kernel=round(nbytes / max(dev_s, 1e-9) / 1e9, 2), hbm_gb_per_s_achievable=HBM_GBS,
                        share_of_hbm=round(nbytes / max(dev_s, 1e-9) / 1e9 / HBM_GBS, 4), **{k: st[k] for k in keys})
    wall, st, cx = best_of(a.repeats, lambda st: rq.seq_complexity(seqs, window=a.window, by=a.by, stats=st))
    lib_s, dev_s = st["total_us"] / 1e6, st["kernel_device_us"] / 1e6
    windows = a.reads * len(range(0, a.length - a.window + 1, a.by))
    rec["window"] = dict(python_wall_s=round(wall, 4), library_s=lib_s, kernel_s=dev_s, reads_per_s_library=round(a.reads / lib_s),
                         windows=windows, windows_per_s_kernel=round(windows / max(dev_s, 1e-9)),
                         gb_per_s_kernel=round(nbytes / max(dev_s, 1e-9) / 1e9, 2), below_8=int((cx < 8).sum()), **{k: st[k] for k in keys})

    with tempfile.TemporaryDirectory() as tmp:
        plain, gz = os.path.join(tmp, "in.fastq"), os.path.join(tmp, "in.fastq.gz")
        fr = min(a.file_reads, a.reads)
        tab, cx = rq.quality_table(quals[:fr]), rq.seq_complexity(seqs[:fr], window=a.window, by=a.by)
        with open(plain, "wb") as fh:
            fh.write(b"".join(b"@r%09d\n%s\n+\n%s\n" % (i, s, q) for i, (s, q) in enumerate(zip(seqs[:fr], quals[:fr]))))
        with open(plain, "rb") as fi, gzip.open(gz, "wb", compresslevel=6) as fo:
            fo.write(fi.read())
        rec["input_bytes"] = {"reads": fr, "plain": os.path.getsize(plain), "gzip": os.path.getsize(gz)}
        runs = {}
        for name, src in (("plain", plain), ("gzip", gz)):
            for what, call in (("table", lambda st: rq.quality_table_fastq(src, stats=st)),
                               ("window", lambda st: rq.complexity_fastq(src, window=a.window, by=a.by, n=None, stats=st))):
                best = None
                for _ in range(a.repeats):
                    st = {}
                    t0 = time.perf_counter()
                    got = call(st)
                    wall = time.perf_counter() - t0
                    if best is None or wall < best[0]:
                        best = (wall, st, got)
                wall, st, got = best
                same = bool(np.array_equal(got["counts"], tab)) if what == "table" else bool(got.tobytes() == cx.tobytes())
                runs[what + "_from_" + name] = dict(wall_s=round(wall, 4), reads_per_s=round(fr / wall), equal_to_in_memory=same,
                                                    share_parse=round(st["parse_us"] / 1e6 / wall, 3),
                                                    share_inflate=round(st["open_inflate_us"] / 1e6 / wall, 3),
                                                    share_kernel=round(st["kernel_device_us"] / 1e6 / wall, 3), **{k: st[k] for k in keys})
        rec["files"] = runs

    n = min(a.prefix, a.reads)
    t0 = time.perf_counter()
    want_tab = rc.restate_table([q.decode() for q in quals[:n]])
    want_cx = rc.restate_complexity([s.decode() for s in seqs[:n]], window=a.window, by=a.by)
    t_restate = time.perf_counter() - t0
    got_tab = rq.quality_table(quals[:n])
    got_cx = rq.seq_complexity(seqs[:n], window=a.window, by=a.by)
    rel = float(np.max(np.abs(got_cx - want_cx) / want_cx))
    equal = bool(np.array_equal(got_tab, want_tab)) and rel <= rc.CX_RTOL and all(r["equal_to_in_memory"] for r in rec["files"].values())
    rec["restatement"] = dict(what="tests/readqc_cases.py, numpy on one host thread: NOT a like-for-like figure for the reference", prefix=n,
                              seconds=round(t_restate, 3), table_equal=bool(np.array_equal(got_tab, want_tab)), complexity_max_rel=rel, equal=equal)
    print(json.dumps(rec))
    return 0 if equal else 1


if __name__ == "__main__":
    sys.exit(main())
