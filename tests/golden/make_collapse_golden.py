"""Golden vectors for the pair relation of collapseNoMismatch (R/multiSample.R:127-132), produced by the REFERENCE's own C code
(C_nwvec / C_nwalign / C_eval_pair compiled in place into oracle/_ref):
    python tests/golden/make_collapse_golden.py
writes tests/golden/collapse_pairs.npz = the pairs of collapse_cases.sweep_pairs() with, per pair, what a brute-force numpy scan
of the gapless diagonals gives (both screen bits, G, m_max; scores 5 / -4) and the reference's eval_pair triple of the unbanded
ends-free alignment by either aligner (ev_vec: nwvec_raw(band=-1), what nwhamming(vec=TRUE) sees; ev_plain: C_nwalign(band=-1))."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import collapse_cases as cc  # noqa: E402
from oracle import ref  # noqa: E402


def main():
    qs, rs, mo = cc.sweep_pairs()
    scan = np.array([cc.brute_pair(q, r, m) for q, r, m in zip(qs, rs, mo)], dtype=np.int32)
    ev_vec = np.array([cc.nweval(ref, q, r, vec=True) for q, r in zip(qs, rs)], dtype=np.int32)
    ev_plain = np.array([cc.nweval(ref, q, r, vec=False) for q, r in zip(qs, rs)], dtype=np.int32)
    np.savez_compressed(os.path.join(HERE, "collapse_pairs.npz"), queries=np.array(qs), refs=np.array(rs),
                        min_overlap=np.array(mo, dtype=np.int32), scan=scan, ev_vec=ev_vec, ev_plain=ev_plain)
    ham = ev_vec[:, 1] + ev_vec[:, 2]
    rejects = scan[:, 1] > cc.SCORES[0] * scan[:, 2]
    print("pairs", len(qs), "bound rejects", int(rejects.sum()), "of them with hamming 0:", int((rejects & (ham == 0)).sum()),
          "sent on", int((~rejects).sum()), "of them hamming 0:", int((~rejects & (ham == 0)).sum()),
          "aligners disagree on zero:", int(((ham == 0) != (ev_plain[:, 1] + ev_plain[:, 2] == 0)).sum()))


if __name__ == "__main__":
    main()
