"""Golden vectors for filterAndTrim, produced by the REFERENCE's own src/filter.cpp:
    python tests/golden/make_filter_golden.py
compiles tests/golden/filter_ref_wrap.cpp - which includes the reference file unmodified and in place, over oracle/shim - into a
temporary directory, runs C_matchRef and C_matrixEE on the cases below and writes tests/golden/filter.npz: the inputs, the counts
and the expected errors as doubles.  tests/test_filter.py holds the restatement of tests/filter_cases.py to this file.
tests/golden/phix_genome.fa beside this script is a copy of the reference's inst/extdata/phix_genome.fa (data)."""
import ctypes as C
import os
import random
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)

from make_taxonomy_golden import REF   # noqa: E402  (where the reference's sources are: DADA2_REFERENCE)
NA = -2 ** 31


def build_ref(outdir, opt="-O2"):
    """The wrapper + the reference's filter.cpp as outdir/libfilterref.so (oracle/Makefile's flags); returns the loaded library."""
    lib = os.path.join(outdir, "libfilterref.so")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", opt, "-ffp-contract=off", "-fPIC", "-w", "-I", os.path.join(ROOT, "oracle", "shim"),
                           "-I", os.path.join(REF, "src"), "-shared", "-o", lib, os.path.join(HERE, "filter_ref_wrap.cpp"), "-lm"])
    L = C.CDLL(lib)
    L.filter_ref_match.argtypes = [C.c_int, C.POINTER(C.c_char_p), C.c_char_p, C.c_uint, C.c_int, C.c_void_p, C.c_char_p, C.c_size_t]
    L.filter_ref_ee.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_char_p, C.c_size_t]
    return L


def ref_match(L, seqs, ref, word_size, non_overlapping):
    out = np.zeros(len(seqs), dtype=np.int32)
    eb = C.create_string_buffer(1024)
    arr = (C.c_char_p * max(len(seqs), 1))(*[s.encode("ascii") for s in seqs])
    if L.filter_ref_match(len(seqs), arr, ref.encode("ascii"), word_size, int(non_overlapping), out.ctypes.data, eb, 1024) != 0:
        raise RuntimeError(eb.value.decode())
    return out


def ref_ee(L, qrows):
    """qrows: lists of integer quality scores of any lengths (the matrix is padded with NA, as as(quality(fq), "matrix") pads)."""
    ncol = max([len(q) for q in qrows] + [1])
    m = np.full((len(qrows), ncol), NA, dtype=np.int32)
    for i, q in enumerate(qrows):
        m[i, :len(q)] = q
    out = np.zeros(len(qrows), dtype=np.float64)
    eb = C.create_string_buffer(1024)
    if L.filter_ref_ee(len(qrows), ncol, m.ctypes.data, out.ctypes.data, eb, 1024) != 0:
        raise RuntimeError(eb.value.decode())
    return m, out


def golden_cases():
    """The sequences of the screen's cases and random reads; the (word size, nonOverlapping) settings; quality rows."""
    import filter_cases as fc
    rng = random.Random(2024)
    seqs, _ = fc.screen_reads()
    more, quals = fc.mixed_reads(rng, 200, p_phix=0.5)
    seqs = seqs + more
    settings = [(16, True), (16, False), (8, True), (20, True), (20, False), (32, True), (1, True)]
    qrows = [[ord(c) - 33 for c in q] for q in quals]
    qrows += [[10] * 20, [20] * 200, [10] * 19, [10] * 21, [], [0], [2] * 300, [40] * 5000, [93] * 10]
    qrows += [[rng.randint(0, 41) for _ in range(rng.choice((1, 63, 64, 65, 250, 301)))] for _ in range(100)]
    return seqs, settings, qrows


def main():
    import filter_cases as fc
    seqs, settings, qrows = golden_cases()
    g = fc.phix()
    out = {"seqs": np.array(seqs), "settings": np.array([(w, int(n)) for w, n in settings], dtype=np.int32)}
    with tempfile.TemporaryDirectory() as tmp:
        L = build_ref(tmp)
        for w, n in settings:
            out["hits_%d_%d" % (w, int(n))] = np.stack([ref_match(L, seqs, g, w, n), ref_match(L, seqs, fc.rc(g), w, n)], axis=1)
        m, ee = ref_ee(L, qrows)
        out["quals"], out["ee"] = m, ee
    h = out["hits_16_1"]
    print("%d sequences, %d flagged by isPhiX's defaults; %d quality rows, EE %.3g .. %.3g; 20 x Q10 -> %r" % (
        len(seqs), int(((h >= 2).any(axis=1)).sum()), len(qrows), ee.min(), ee.max(), float(ee[200])))
    np.savez_compressed(os.path.join(HERE, "filter.npz"), **out)


if __name__ == "__main__":
    main()
