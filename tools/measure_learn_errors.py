"""One measurement of learn_errors: 8 dada2_amd.synth samples of 20 000 uniques x 250 nt, qualities binned, the binned function, one run after a
one-sample warm-up; the wall split into counting / upload, the passes (api.dada's timings) and the fits.

    python tools/measure_learn_errors.py [record.json]        # needs an MI355X
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import torch  # noqa: E402,F401  (before the library, as tests/conftest.py does)

from dada2_amd import errormodels as em  # noqa: E402
from dada2_amd.io import Derep  # noqa: E402
from dada2_amd.synth import make_shared_truth_samples  # noqa: E402
from helpers import tperr1  # noqa: E402

BINS = (7, 17, 27, 37)
t0 = time.perf_counter()
raw = make_shared_truth_samples(tperr1(), n_uniques=20000, nsamples=8, L=250, G=64, seed=20261020)
edges = np.array(BINS)
samples = []
for d in raw:
    q = np.rint(d.quals)
    b = edges[np.clip(np.searchsorted(edges, q, side="right") - 1, 0, len(BINS) - 1)].astype(np.float64)
    samples.append(Derep(d.seqs, d.abundances, b, d.map))
t_synth = time.perf_counter() - t0
print("synth %.1f s" % t_synth, [int(d.abundances.sum()) for d in samples], flush=True)

fits = []
base = em.make_binned_qual_errfun(BINS)


def timed(trans):
    t = time.perf_counter()
    out = base(trans)
    fits.append((time.perf_counter() - t) * 1e3)
    return out


em.learn_errors(samples[0], err_fun=timed, MAX_CONSIST=1)         # warm-up: the runtime's start-up is not the subject
del fits[:]
t = time.perf_counter()
got = em.learn_errors(samples, nbases=1e12, err_fun=timed)
wall = (time.perf_counter() - t) * 1e3
info = got["info"]
rec = dict(what="learn_errors, one run after a one-sample warm-up; samples taken one after another",
           samples=8, uniques_per_sample=20000, read_length=250, bins=BINS, err_fun="make_binned_qual_errfun",
           nreads=info["nreads"], nbases=info["nbases"], passes=info["passes"], converged=info["converged"],
           wall_ms=wall, derep_ms=info["timings_ms"]["derep"], upload_ms=info["timings_ms"]["upload"],
           pass_ms=info["timings_ms"]["passes"], passes_total_ms=sum(info["timings_ms"]["passes"]),
           fit_ms=fits, fits_total_ms=sum(fits), synth_s=t_synth,
           note="dereps are given as objects (synth has no files), so derep_ms is the read and base count only; pass_ms[0] is "
                "the initialisation pass (all-ones matrix, MAX_CLUST = 1)")
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        json.dump(rec, f, indent=1)
print(json.dumps(rec))
