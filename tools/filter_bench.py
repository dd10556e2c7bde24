#!/usr/bin/env python3
"""tools/filter_bench.py - filterAndTrim at size (not bench.py's workload): a synthetic FASTQ of --reads reads x --len nt, --phix
of them cut from the phiX genome (tests/golden/phix_genome.fa), qualities that decay along the read, filtered with
truncLen 240, maxEE 2 and the phiX screen.

    python tools/filter_bench.py device       # on the GPU
    python tools/filter_bench.py reference    # where the reference's sources are (DADA2_REFERENCE)
    python tools/filter_bench.py oriented     # on the GPU: orient.fwd and matchIDs (dada2_amd.filtering)

`device` prints one JSON line: reads/s for plain and gzip input and plain and gzip output (best of --repeats), each with the
library's own clocks (parse, upload, the three kernels, download, deflate, write), and dada2hip_filter_reads on the same reads
in memory.  `reference` compiles tests/golden/filter_ref_wrap.cpp by the golden generator's recipe and times C_matchRef (both
strands) + C_matrixEE on a --prefix of the same reads, cut to 240, on ONE thread: the reference's COMPUTE only - not ShortRead's
parsing, trimming and writing, which this tool cannot run - so the two lines are not a like-for-like ratio.  `oriented`: every
read starts with a 20-nt barcode and half of them are stored as their reverse complement; the same reads go through
dada2hip_filter_reads and dada2hip_filter_reads_oriented in memory and through the plain-to-plain file run both ways, with the
device time of the orientation kernel and of the scan; then a pair of files that differ in 1 % of their records through
dada2hip_filter_fastq_paired_ex with match_ids, with the id join's share of the call."""
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
PHIX_FA = os.path.join(ROOT, "tests", "golden", "phix_genome.fa")


def synth(n, ln, phix_share, seed):
    """(seq, qual): n x ln uint8 matrices of letters and Phred+33 quality characters."""
    from dada2_amd import api
    rng = np.random.RandomState(seed)
    g = np.frombuffer(api.read_fasta(PHIX_FA)[1][0].encode(), dtype=np.uint8)
    seq = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.randint(0, 4, (n, ln))]
    rows = rng.choice(n, int(n * phix_share), replace=False)
    gg = np.concatenate([g, g[:ln]])
    for r, o in zip(rows, rng.randint(0, len(g), len(rows))):
        seq[r] = gg[o: o + ln]
    pos = np.arange(ln) / ln
    level = rng.uniform(0.3, 1.6, (n, 1))                                      # per-read decay: some reads pass maxEE 2, some do not
    q = 38 - 22 * level * pos[None, :] ** 2 + rng.normal(0, 3, (n, ln))
    qual = (np.clip(np.rint(q), 3, 40) + 33).astype(np.uint8)
    return seq, qual


def write_fastq(path, seq, qual):
    n, ln = seq.shape
    ids = np.frombuffer(b"".join(b"@r%09d\n" % i for i in range(n)), dtype=np.uint8).reshape(n, 12)
    rec = np.empty((n, 12 + ln + 3 + ln + 1), dtype=np.uint8)
    rec[:, :12] = ids
    rec[:, 12: 12 + ln] = seq
    rec[:, 12 + ln: 15 + ln] = np.frombuffer(b"\n+\n", dtype=np.uint8)
    rec[:, 15 + ln: 15 + 2 * ln] = qual
    rec[:, -1] = 10
    rec.tofile(path)


def device(a):
    from dada2_amd import api
    seq, qual = synth(a.reads, a.len, a.phix, a.seed)
    rec = {"tool": "filter_bench", "mode": "device", "reads": a.reads, "len": a.len, "phix_share": a.phix, "seed": a.seed,
           "params": {"trunc_len": 240, "max_ee": 2, "rm_phix": True, "n": a.n}}
    kw = dict(trunc_len=240, max_ee=2)
    keys = ("open_inflate_us", "parse_us", "upload_us", "scan_device_us", "ee_device_us", "kmers_device_us", "download_us", "deflate_us", "write_us", "total_us",
            "upload_bytes")
    with tempfile.TemporaryDirectory() as tmp, api.FilterContext(PHIX_FA) as ctx:
        plain, gz = os.path.join(tmp, "in.fastq"), os.path.join(tmp, "in.fastq.gz")
        write_fastq(plain, seq, qual)
        api.fastq_filter(plain, gz, compress=True, trunc_q=-1, min_len=0, max_n=10**6, ctx=ctx)   # (the library's own writer makes the .gz)
        rec["input_bytes"] = {"plain": os.path.getsize(plain), "gzip": os.path.getsize(gz)}
        rec["table"] = {k: ctx.stats[k] for k in ("table_keys", "table_in_lds")}
        runs = {}
        for src_name, src in (("plain", plain), ("gzip", gz)):
            for out_name, compress in (("plain", False), ("gzip", True)):
                out = os.path.join(tmp, "out.fastq" + (".gz" if compress else ""))
                best = None
                for _ in range(a.repeats):
                    st = {}
                    t0 = time.perf_counter()
                    counts = api.fastq_filter(src, out, compress=compress, n=a.n, rm_phix=True, ctx=ctx, stats=st, **kw)
                    wall = time.perf_counter() - t0
                    if best is None or wall < best[0]:
                        best = (wall, st, counts)
                wall, st, counts = best
                runs["%s_to_%s" % (src_name, out_name)] = dict(wall_s=round(wall, 4), reads_per_s=round(a.reads / wall), reads_in=counts[0],
                                                               reads_out=counts[1], dropped_max_ee=st["dropped_max_ee"],
                                                               dropped_rm_phix=st["dropped_rm_phix"], **{k: st[k] for k in keys})
        rec["files"] = runs
        seqs = [r.tobytes() for r in seq]
        quals = [r.tobytes() for r in qual]
        best = None
        for _ in range(a.repeats):
            st = {}
            t0 = time.perf_counter()
            got = api.filter_reads(seqs, quals, ctx, rm_phix=True, stats=st, **kw)
            wall = time.perf_counter() - t0
            if best is None or st["total_us"] < best[1]["total_us"]:
                best = (wall, st)
        wall, st = best
        dev_s = (st["scan_device_us"] + st["ee_device_us"]) / 1e6
        rec["in_memory"] = dict(python_wall_s=round(wall, 4), library_s=st["total_us"] / 1e6, reads_per_s_library=round(a.reads / (st["total_us"] / 1e6)),
                                kernels_s=dev_s, reads_per_s_kernels=round(a.reads / max(dev_s, 1e-9)), kept=int((got["code"] == 0).sum()),
                                **{k: st[k] for k in keys})
    print(json.dumps(rec))


BARCODE = b"ACGTTGCAAGGCTCATGCTA"
_COMP = bytes.maketrans(b"ACGT", b"TGCA")


def write_fastq_ids(path, ids, seq, qual):
    with open(path, "wb") as fh:
        fh.write(b"".join(b"%s\n%s\n+\n%s\n" % (i, s.tobytes(), q.tobytes()) for i, s, q in zip(ids, seq, qual)))


def best_of(repeats, f, key=lambda r: r[0]):
    best = None
    for _ in range(repeats):
        t0 = time.perf_counter()
        got = f()
        r = (time.perf_counter() - t0, got)
        if best is None or key(r) < key(best):
            best = r
    return best


def oriented(a):
    from dada2_amd import api, filtering
    seq, qual = synth(a.reads, a.len, a.phix, a.seed)
    seq[:, :len(BARCODE)] = np.frombuffer(BARCODE, dtype=np.uint8)
    rng = np.random.RandomState(a.seed + 1)
    rows = rng.choice(a.reads, a.reads // 2, replace=False)                     # stored as the reverse complement
    seq[rows] = np.frombuffer(seq[rows].tobytes().translate(_COMP), dtype=np.uint8).reshape(len(rows), a.len)[:, ::-1]
    qual[rows] = qual[rows][:, ::-1]
    bar = BARCODE.decode()
    kw = dict(trunc_len=240, max_ee=2)
    rec = {"tool": "filter_bench", "mode": "oriented", "reads": a.reads, "len": a.len, "phix_share": a.phix, "seed": a.seed, "barcode": bar,
           "flipped_share": 0.5, "params": {"trunc_len": 240, "max_ee": 2, "rm_phix": True, "n": a.n}}
    keys = ("parse_us", "upload_us", "orient_device_us", "scan_device_us", "ee_device_us", "download_us", "write_us", "id_join_us", "total_us")
    with tempfile.TemporaryDirectory() as tmp, api.FilterContext(PHIX_FA) as ctx:
        seqs, quals = [r.tobytes() for r in seq], [r.tobytes() for r in qual]
        mem = {}
        for name, extra in (("plain", {}), ("oriented", {"orient_fwd": bar})):
            def call():
                st = {}
                got = filtering.filter_reads(seqs, quals, ctx, rm_phix=True, stats=st, **kw, **extra)
                return st, got
            wall, (st, got) = best_of(a.repeats, call, key=lambda r: r[1][0]["total_us"])
            mem[name] = dict(python_wall_s=round(wall, 4), library_s=st["total_us"] / 1e6, kept=int((got["code"] == 0).sum()),
                             flipped=st.get("flipped", 0), **{k: st.get(k, 0) for k in keys})
        rec["in_memory"] = mem
        plain, out = os.path.join(tmp, "in.fastq"), os.path.join(tmp, "out.fastq")
        write_fastq(plain, seq, qual)
        files = {}
        for name, extra in (("plain", {}), ("oriented", {"orient_fwd": bar})):
            def call():
                st = {}
                counts = filtering.fastq_filter(plain, out, compress=False, n=a.n, rm_phix=True, ctx=ctx, stats=st, **kw, **extra)
                return st, counts
            wall, (st, counts) = best_of(a.repeats, call)
            files[name] = dict(wall_s=round(wall, 4), reads_per_s=round(a.reads / wall), reads_in=counts[0], reads_out=counts[1],
                               **{k: st.get(k, 0) for k in keys})
        rec["plain_to_plain"] = files
        # ---- a pair of files that differ in 1 % of their records, matched by id ----
        ids_f = [b"@M01:7:FC:1:%d:%d:%d 1:N:0:ACGT" % (1101 + i // 10**5, i % 10**5, 3 * i) for i in range(a.reads)]
        ids_r = [i[:-10] + b"2:N:0:ACGT" for i in ids_f]
        keep_f, keep_r = rng.rand(a.reads) >= 0.005, rng.rand(a.reads) >= 0.005
        inf, inr, of, orv = (os.path.join(tmp, x) for x in ("F.fastq", "R.fastq", "oF.fastq", "oR.fastq"))
        write_fastq_ids(inf, [i for i, k in zip(ids_f, keep_f) if k], seq[keep_f], qual[keep_f])
        write_fastq_ids(inr, [i for i, k in zip(ids_r, keep_r) if k], seq[keep_r], qual[keep_r])

        def pair():
            st = {}
            counts = filtering.fastq_paired_filter((inf, inr), (of, orv), compress=False, n=a.n, rm_phix=True, ctx=ctx, stats=st, match_ids=True, **kw)
            return st, counts
        wall, (st, counts) = best_of(a.repeats, pair)
        rec["paired_match_ids"] = dict(wall_s=round(wall, 4), pairs_per_s=round(counts[0] / wall), reads_in=counts[0], reads_out=counts[1],
                                       records_forward=int(keep_f.sum()), records_reverse=int(keep_r.sum()), dropped_ids=st["dropped_ids"],
                                       id_join_share_of_call=round(st["id_join_us"] / max(st["total_us"], 1), 4), **{k: st.get(k, 0) for k in keys})
    print(json.dumps(rec))


def reference(a):
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import make_filter_golden as mg
    import filter_cases as fc
    seq, qual = synth(a.reads, a.len, a.phix, a.seed)
    n = min(a.prefix, a.reads)
    seqs = [r[:240].tobytes().decode() for r in seq[:n]]
    qrows = [(r[:240].astype(np.int32) - 33).tolist() for r in qual[:n]]
    g = fc.phix()
    with tempfile.TemporaryDirectory() as tmp:
        L = mg.build_ref(tmp)
        t0 = time.perf_counter()
        hf, hr = mg.ref_match(L, seqs, g, 16, True), mg.ref_match(L, seqs, fc.rc(g), 16, True)
        t_match = time.perf_counter() - t0
        t0 = time.perf_counter()
        _, ee = mg.ref_ee(L, qrows)
        t_ee = time.perf_counter() - t0
    print(json.dumps({"tool": "filter_bench", "mode": "reference", "what": "C_matchRef (both strands) + C_matrixEE on reads cut to 240, compute only",
                      "threads": 1, "prefix": n, "match_s": round(t_match, 4), "ee_s": round(t_ee, 4),
                      "reads_per_s": round(n / (t_match + t_ee)), "all_reads_s_extrapolated": round((t_match + t_ee) / n * a.reads, 1),
                      "flagged": int(((hf >= 2) | (hr >= 2)).sum()), "ee_over_2": int((ee > 2).sum())}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=("device", "reference", "oriented"))
    ap.add_argument("--reads", type=int, default=10**6)
    ap.add_argument("--len", type=int, default=250)
    ap.add_argument("--phix", type=float, default=0.01)
    ap.add_argument("--n", type=int, default=10**5)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--prefix", type=int, default=20000)
    a = ap.parse_args()
    {"device": device, "reference": reference, "oriented": oriented}[a.mode](a)


if __name__ == "__main__":
    main()
