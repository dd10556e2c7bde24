"""Records tests/golden/errormodel_trans.npz: the transition counts the reference's selfConsist loop ends with in the three runs
of tests/errormodel_cases.py (pool_cases.restate_dada over oracle.ref.dada_uniques, OMEGA_C = 0).  Needs oracle/_ref; no GPU.

    python tests/golden/make_errormodel_golden.py
"""
import os
import sys
import tempfile
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import errormodel_cases as ec  # noqa: E402
from dada2_amd import api, errormodels as em  # noqa: E402
from dada2_amd.opts import DadaOpts  # noqa: E402


def main():
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        runs = {
            "binned": (ec.binned_pair(tmp), em.make_binned_qual_errfun(ec.BINS), DadaOpts(OMEGA_C=0)),
            "loess": (ec.golden_paths("sam1F", "sam2F"), em.loess_direct_errfun, DadaOpts(OMEGA_C=0)),
            "pacbio": (ec.golden_paths("samPB"), em.make_pacbio_errfun(), DadaOpts(OMEGA_C=0, BAND_SIZE=32)),
        }
        for name, (paths, fun, opts) in runs.items():
            dereps = ec.oracle_dereps(api, paths)
            t0 = time.perf_counter()
            ref = ec.reference_loop(name, dereps, fun, opts)
            print(name, [d.nraw for d in dereps], "uniques,", ref["passes"], "passes, converged", ref["converged"],
                  [r.nclust for r in ref["results"]], "clusters, %.1f s" % (time.perf_counter() - t0), ref["trans"].shape)
            out[name] = ref["trans"].astype(np.int32)
    np.savez_compressed(os.path.join(HERE, "errormodel_trans.npz"), **out)


if __name__ == "__main__":
    main()
