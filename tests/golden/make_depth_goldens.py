#!/usr/bin/env python3
"""Record the reference's results at the depth bench.py times (tests/golden/depth_*.expected.npz).

    make -C oracle && python tests/golden/make_depth_goldens.py

Runs only where oracle/_ref is built.  Each input is drawn exactly as bench.py draws it (bench.make_inputs through
tests/at_size.py:_inputs, same seeds, same input cache), the reference's O2 build (the parity target) runs on it, and the
recording is written with fixed zip timestamps, so a rerun rewrites both files byte for byte.

  depth_cfg5.expected.npz             configs[4] (bench.py --config 5): 200 000 uniques of 1 450-1 510 nt, BAND_SIZE 32,
                                      no MAX_CLUST: all 128 partitions
  depth_selfconsist_1M.expected.npz   configs[2] (bench.py --selfconsist): the learnErrors loop on the 1 000 000-unique
                                      headline sample, driven as dada2_amd.api.dada drives it: pass 0 from an all-ones err
                                      with MAX_CLUST 1, then accumulate_trans -> noqual_errfun -> the R/dada.R:385-388
                                      diagonal fix after pass 0 -> extend_err, until convergence or MAX_CONSIST

Measured reference time on an 8-core host, the two recordings in two processes at once, 4 threads each (--threads 4):
  depth_cfg5             1 491 s (one call, 128 partitions)
  depth_selfconsist_1M   1 094 s (6 passes: 34 / 113 / 278 / 208 / 212 / 246 s; 1, 412, 687, 647, 647, 647 partitions;
                         converged)
Drawing the inputs adds 15-30 s each (bench.py's input cache keeps them).

Per recording: sha256 of the drawn input, the whole clustering table / birth_subs / subqual / err of every pass, and a
sha256 of map and clusterquals.  Per-unique p-values are kept for every unique with abundance > 1 plus a fixed-seed sample of
the others (most are singletons at exactly 1.0) - for as many passes as the 1 MB budget of a file allows: the last pass first,
then the passes with the most partitions -, then map and clusterquals themselves where they still fit (pack()).
``--raw DIR`` keeps the reference's raw results in DIR and reuses them, so the packing can be redone without rerunning the
reference.
"""
import argparse
import io
import json
import os
import pickle
import sys
import time
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, "..", ".."))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

from dada2_amd.opts import DadaOpts  # noqa: E402
from helpers import DEPTH_RECORDINGS as FILES, canon_sha256, derep_sha256  # noqa: E402

RECORDINGS = ("cfg5", "sc1M")
FILE_BUDGET = 1_000_000          # bytes per recording
PVAL_SAMPLE = 16_384             # singletons whose p-value is kept besides every unique with abundance > 1
PVAL_SEED = 20261016


def opts(name):
    """The options bench.py runs each workload with."""
    import bench
    if name == "cfg5":
        return DadaOpts(BAND_SIZE=bench.CONFIGS[5]["band"])
    return DadaOpts(BAND_SIZE=bench.CONFIGS[3]["band"])


def draw(name):
    """(derep, err) exactly as bench.py draws them."""
    import at_size
    dereps, err = at_size._inputs("cfg5" if name == "cfg5" else "cfg3")
    return dereps[0], err


def pval_rows(abundances):
    """Indices of the uniques whose p-value a recording keeps: all with abundance > 1, plus a seeded sample of the rest."""
    ab = np.asarray(abundances)
    multi = np.flatnonzero(ab > 1)
    single = np.flatnonzero(ab <= 1)
    rng = np.random.default_rng(PVAL_SEED)
    pick = np.sort(rng.choice(single, size=min(PVAL_SAMPLE, single.size), replace=False)) if single.size else single
    return np.union1d(multi, pick).astype(np.int64)


def run_loop(ref, d, o, log=print):
    """The selfConsist loop of dada2_amd.api.dada with the reference in place of the GPU.  Returns (passes, err_out,
    converged); passes = [(err used, max_clust or None, result)]."""
    from dada2_amd.api import accumulate_trans, noqual_errfun
    from dada2_amd.io import extend_err
    o = o.normalised()
    qmax = d.qmax()
    errs, passes = [], []
    err, initialize, nconsist = None, True, 0
    while True:
        if nconsist > 0:
            errs.append(np.array(err, copy=True))
        erri = np.ones((16, max(41, qmax + 1))) if initialize else extend_err(err, qmax)
        mc = 1 if initialize else None
        t0 = time.time()
        r = ref.dada_uniques(d.seqs, d.abundances, None, erri, d.quals, o, max_clust=mc, multithread=True)
        log(f"  pass {len(passes)}: {r.nclust} partitions, {time.time() - t0:.1f} s")
        passes.append((erri, mc, r))
        new_err = noqual_errfun(accumulate_trans([r.subqual]))
        if initialize:
            initialize = False
            new_err[[0, 5, 10, 15], :] = 1.0                     # R/dada.R:385-388
        err = new_err
        converged = any(np.array_equal(e, err) for e in errs)
        if converged or nconsist >= o.MAX_CONSIST:
            break
        nconsist += 1
    return passes, err, converged


def compute(name, threads, raw_dir=None, log=print):
    """The reference's raw results for one recording (cached under raw_dir when given)."""
    path = os.path.join(raw_dir, f"{name}.pkl") if raw_dir else None
    if path and os.path.exists(path):
        with open(path, "rb") as fh:
            return pickle.load(fh)
    from oracle import ref
    assert ref.available("O2"), "oracle/_ref not built: make -C oracle"
    t0 = time.time()
    d, err = draw(name)
    log(f"{name}: drew {d.nraw} uniques in {time.time() - t0:.1f} s")
    ref.set_threads(threads)
    o = opts(name)
    t0 = time.time()
    if name == "cfg5":
        r = ref.dada_uniques(d.seqs, d.abundances, None, err, d.quals, o, multithread=True)
        out = dict(passes=[(err, None, r)], err_out=None, converged=None)
    else:
        passes, err_out, converged = run_loop(ref, d, o, log)
        out = dict(passes=passes, err_out=err_out, converged=converged)
    out.update(input_sha256=derep_sha256(d), abundances=np.asarray(d.abundances), seconds=time.time() - t0, threads=threads)
    log(f"{name}: reference took {out['seconds']:.1f} s on {threads} threads")
    if path:
        os.makedirs(raw_dir, exist_ok=True)
        with open(path + ".tmp", "wb") as fh:
            pickle.dump(out, fh, protocol=pickle.HIGHEST_PROTOCOL)
        os.replace(path + ".tmp", path)
    return out


def _result_arrays(prefix, r):
    cl, bs = r.clustering, r.birth_subs
    a = {prefix + "cl_sequence": np.array(cl["sequence"], dtype="S"),
         prefix + "bs_ref": np.array(bs["ref"], dtype="S"), prefix + "bs_sub": np.array(bs["sub"], dtype="S"),
         prefix + "subqual": r.subqual}
    for c in ("abundance", "n0", "n1", "nunq", "pval", "birth_from", "birth_pval", "birth_fold", "birth_ham", "birth_qave"):
        a[prefix + "cl_" + c] = np.asarray(cl[c])
    for c in ("pos", "qual", "clust"):
        a[prefix + "bs_" + c] = np.asarray(bs[c])
    return a


def npz_bytes(arrays):
    """np.savez_compressed with fixed zip timestamps and member order: the same arrays give the same bytes."""
    buf = io.BytesIO()
    with zipfile.ZipFile(buf, "w", compression=zipfile.ZIP_DEFLATED) as zf:
        for k in sorted(arrays):
            b = io.BytesIO()
            np.lib.format.write_array(b, np.asanyarray(arrays[k]), allow_pickle=False)
            zi = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            zi.compress_type = zipfile.ZIP_DEFLATED
            zi.external_attr = 0o644 << 16
            zf.writestr(zi, b.getvalue(), compresslevel=9)
    return buf.getvalue()


def pack(name, raw):
    """The recording's arrays, meta included.  Always: every table of every pass (an array equal to the same array of an
    earlier pass is stored once: meta passes[k]["same_as"]), its err, the sha256 of map and clusterquals.  Then, while the
    file stays within FILE_BUDGET: the per-unique p-values of the kept rows - the last pass first, then the passes with the
    most partitions - and after them maps and cluster qualities, newest pass first."""
    passes = raw["passes"]
    rows = pval_rows(raw["abundances"])
    pmeta = [dict(max_clust=mc, nclust=int(r.nclust), map_sha256=canon_sha256(r.map),
                  clusterquals_sha256=canon_sha256(r.clusterquals), same_as={}) for _, mc, r in passes]
    arrays = {"pval_rows_delta": np.diff(rows, prepend=0).astype(np.int32)}
    for k, (err_used, _, r) in enumerate(passes):
        for key, val in dict(_result_arrays("", r), err=np.asarray(err_used, dtype=np.float64)).items():
            same = [j for j in range(k) if f"p{j}_{key}" in arrays and arrays[f"p{j}_{key}"].dtype == val.dtype
                    and np.array_equal(arrays[f"p{j}_{key}"], val)]
            if same:
                pmeta[k]["same_as"][key] = same[0]
            else:
                arrays[f"p{k}_{key}"] = val
    if raw["err_out"] is not None:
        arrays["err_out"] = np.asarray(raw["err_out"], dtype=np.float64)
    meta = dict(recording=name, opts=dict(vars(opts(name))), npasses=len(passes), converged=raw["converged"],
                input_sha256=raw["input_sha256"], nuniques=int(len(raw["abundances"])), pval_sample=PVAL_SAMPLE,
                pval_seed=PVAL_SEED, passes=pmeta)
    arrays["meta"] = np.array(json.dumps(meta, sort_keys=True))
    last = len(passes) - 1
    order = [last] + sorted((k for k in range(last)), key=lambda k: (-passes[k][2].nclust, -k))
    extras = [(f"p{k}_pval", passes[k][2].pval[rows]) for k in order]
    extras += [(f"p{k}_{what}", getattr(passes[k][2], what)) for k in reversed(range(len(passes))) for what in ("map", "clusterquals")]
    for key, val in extras:
        trial = dict(arrays, **{key: val})
        if len(npz_bytes(trial)) <= FILE_BUDGET:
            arrays = trial
    return arrays


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=RECORDINGS, action="append")
    ap.add_argument("--threads", type=int, default=os.cpu_count() or 1)
    ap.add_argument("--raw", default=None, help="keep / reuse the reference's raw results in this directory")
    a = ap.parse_args()
    for name in a.only or RECORDINGS:
        raw = compute(name, a.threads, a.raw)
        arrays = pack(name, raw)
        data = npz_bytes(arrays)
        path = os.path.join(HERE, FILES[name])
        with open(path + ".tmp", "wb") as fh:
            fh.write(data)
        os.replace(path + ".tmp", path)
        meta = json.loads(str(arrays["meta"]))
        kept = sorted(k for k in arrays if k.split("_", 1)[-1] in ("pval", "map", "clusterquals"))
        print(f"{FILES[name]}: {len(data)} bytes, {meta['npasses']} pass(es), nclust {[p['nclust'] for p in meta['passes']]}, "
              f"converged {meta['converged']}, reference {raw['seconds']:.0f} s on {raw['threads']} threads, kept {kept}", flush=True)


if __name__ == "__main__":
    main()
