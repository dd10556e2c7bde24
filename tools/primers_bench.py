#!/usr/bin/env python3
"""tools/primers_bench.py - removePrimers at size (not bench.py's workload): a synthetic FASTQ of --reads reads of 1 450 to 1 550
nt, both primers of the reference's documented call (27F and the reverse complement of 1492R) planted with 0 to 3 mismatches
each, half of the reads reverse-complemented, --bare of them without a primer.

    python tools/primers_bench.py        # on the GPU

prints one JSON line:
  in_memory   dada2hip_primers_reads on the reads in memory (best of --repeats by the library's clock): library time, the
              kernel's device time from its events, (start positions x primer letters x patterns) per second of kernel time,
              and the bytes that cross the host link per second of library time beside the link's and the memory's rates;
  files       dada2hip_primers_fastq plain -> plain, plain -> gzip and gzip -> plain, each with the library's clocks and the
              share of the wall time that parsing, inflate and deflate are (the parser runs under the chunk before it, so the
              shares need not add up to one);
  restatement tests/primer_cases.py's restate_read over the first --prefix reads on ONE host thread, in Python: it shows that the
              results are equal, and its time is NOT a like-for-like figure for the reference (R and Biostrings are not here)."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

HOST_LINK_GBS = 63.0          # PCIe Gen5 x16, specified
HBM_GBS = 6300.0              # HBM3E, achievable (a float4 copy)


def synth(n, bare_share, seed):
    """(seqs, quals): lists of bytes."""
    import primer_cases as pc
    rng = np.random.RandomState(seed)
    fwd, rev = pc.F27, pc.rc(pc.R1492)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    comp = np.zeros(256, dtype=np.uint8)
    for a, b in zip(b"ACGT", b"TGCA"):
        comp[a] = b
    lens = rng.randint(1450, 1551, n)
    mat = acgt[rng.randint(0, 4, (n, 1550))]

    def words(primer):
        w = np.empty((n, len(primer)), dtype=np.uint8)
        for i, c in enumerate(primer):
            s = np.frombuffer(pc.SETS[c].encode(), dtype=np.uint8)
            w[:, i] = s[rng.randint(0, len(s), n)]
            k = rng.randint(0, 4, n)                           # 0 to 3 mismatches: letter i is one with probability k / L
            hit = rng.random_sample(n) < k / len(primer)
            o = np.frombuffer("".join(b for b in "ACGT" if b not in pc.SETS[c]).encode(), dtype=np.uint8)
            w[hit, i] = o[rng.randint(0, len(o), int(hit.sum()))]
        return w
    wf, wr = words(fwd), words(rev)
    lead, tail = rng.randint(0, 30, n), rng.randint(0, 30, n)
    bare = rng.random_sample(n) < bare_share
    flip = rng.random_sample(n) < 0.5
    seqs = []
    for i in range(n):
        r = mat[i, : lens[i]]
        if not bare[i]:
            r[lead[i]: lead[i] + len(fwd)] = wf[i]
            e = lens[i] - tail[i]
            r[e - len(rev): e] = wr[i]
        seqs.append((comp[r[::-1]] if flip[i] else r).tobytes())
    qual = (np.clip(np.rint(rng.normal(60, 12, 1550)), 3, 93) + 33).astype(np.uint8).tobytes()
    return seqs, [qual[: len(s)] for s in seqs]


def write_fastq(path, seqs, quals):
    with open(path, "wb") as fh:
        fh.write(b"".join(b"@r%09d\n%s\n+\n%s\n" % (i, s, q) for i, (s, q) in enumerate(zip(seqs, quals))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=100000)
    ap.add_argument("--bare", type=float, default=0.03)
    ap.add_argument("--n", type=int, default=10**5)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--prefix", type=int, default=1000)
    a = ap.parse_args()
    os.environ.setdefault("DADA2HIP_PROFILE", "1")
    import primer_cases as pc
    from dada2_amd import primers as pr
    fwd, rev, mm = pc.F27, pc.rc(pc.R1492), 2
    seqs, quals = synth(a.reads, a.bare, a.seed)
    nbytes = sum(len(s) for s in seqs)
    rec = {"tool": "primers_bench", "reads": a.reads, "bases": nbytes, "bare_share": a.bare, "seed": a.seed,
           "params": {"primer_fwd": fwd, "primer_rev": rev, "max_mismatch": mm, "orient": True, "n": a.n}}
    keys = ("open_inflate_us", "parse_us", "upload_us", "kernel_device_us", "download_us", "deflate_us", "write_us", "total_us", "upload_bytes",
            "pieces", "tiles")

    pr.primer_hits(seqs[:1000], fwd, rev, max_mismatch=mm)                     # (the runtime and the code object are up)
    best = None
    for _ in range(a.repeats):
        st = {}
        t0 = time.perf_counter()
        got = pr.primer_hits(seqs, fwd, rev, max_mismatch=mm, stats=st)
        wall = time.perf_counter() - t0
        if best is None or st["total_us"] < best[1]["total_us"]:
            best = (wall, st)
    wall, st = best
    cells = sum((len(s) - L + 2 * mm + 1) * L for s in seqs for L in (len(fwd), len(rev))) * 2
    lib_s, dev_s = st["total_us"] / 1e6, st["kernel_device_us"] / 1e6
    moved = st["upload_bytes"] + 64 * a.reads                                  # (32 B of verdict and 32 B of starts per read come back)
    rec["in_memory"] = dict(python_wall_s=round(wall, 4), library_s=lib_s, kernel_s=dev_s, reads_per_s_library=round(a.reads / lib_s),
                            cells=cells, cells_per_s_kernel=round(cells / max(dev_s, 1e-9)), bytes_moved=moved,
                            gb_per_s_library=round(moved / lib_s / 1e9, 3), gb_per_s_kernel=round(nbytes / max(dev_s, 1e-9) / 1e9, 3),
                            host_link_gb_per_s_spec=HOST_LINK_GBS, hbm_gb_per_s_achievable=HBM_GBS, kept=int((got["code"] == 0).sum()),
                            flipped=int(got["flip"].sum()), **{k: st[k] for k in keys})

    with tempfile.TemporaryDirectory() as tmp:
        plain, gz = os.path.join(tmp, "in.fastq"), os.path.join(tmp, "in.fastq.gz")
        write_fastq(plain, seqs, quals)
        import gzip
        with open(plain, "rb") as fi, gzip.open(gz, "wb", compresslevel=6) as fo:
            fo.write(fi.read())
        rec["input_bytes"] = {"plain": os.path.getsize(plain), "gzip": os.path.getsize(gz)}
        runs = {}
        for name, src, compress in (("plain_to_plain", plain, False), ("plain_to_gzip", plain, True), ("gzip_to_plain", gz, False)):
            out = os.path.join(tmp, "out.fastq" + (".gz" if compress else ""))
            best = None
            for _ in range(a.repeats):
                st = {}
                t0 = time.perf_counter()
                counts = pr.primers_fastq(src, out, fwd, rev, max_mismatch=mm, compress=compress, n=a.n, stats=st)
                wall = time.perf_counter() - t0
                if best is None or wall < best[0]:
                    best = (wall, st, counts)
            wall, st, counts = best
            runs[name] = dict(wall_s=round(wall, 4), reads_per_s=round(a.reads / wall), reads_in=counts[0], reads_out=counts[1],
                              share_parse=round(st["parse_us"] / 1e6 / wall, 3), share_inflate=round(st["open_inflate_us"] / 1e6 / wall, 3),
                              share_deflate=round(st["deflate_us"] / 1e6 / wall, 3), share_kernel=round(st["kernel_device_us"] / 1e6 / wall, 3),
                              **{k: st[k] for k in keys})
        rec["files"] = runs

    n = min(a.prefix, a.reads)
    t0 = time.perf_counter()
    want = [pc.restate_read(s.decode(), fwd, rev, max_mismatch=mm) for s in seqs[:n]]
    t_restate = time.perf_counter() - t0
    equal = all((int(got["code"][i]), int(got["flip"][i]), int(got["first"][i]), int(got["last"][i]), tuple(got["hits"][i].tolist()),
                 tuple(got["starts"][i].reshape(-1).tolist())) == (w["code"], w["flip"], w["first"], w["last"], w["hits"], w["starts"])
                for i, w in enumerate(want))
    rec["restatement"] = dict(what="tests/primer_cases.py restate_read, Python, one host thread: NOT like for like", prefix=n,
                              seconds=round(t_restate, 3), reads_per_s=round(n / t_restate), equal=bool(equal))
    print(json.dumps(rec))
    return 0 if equal else 1


if __name__ == "__main__":
    sys.exit(main())
