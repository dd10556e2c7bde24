"""Golden vectors for assignTaxonomy, produced by the REFERENCE's own src/taxonomy.cpp:
    python tests/golden/make_taxonomy_golden.py
compiles tests/golden/taxonomy_ref_wrap.cpp - which includes the reference file unmodified and in place, over oracle/shim - into
a temporary directory, runs every case of tests/taxonomy_cases.py through it TWICE (the reference breaks ties with a
std::random_device-seeded engine: two runs differ) and writes tests/golden/taxonomy.npz: per case the inputs, the seed of its
uniforms and the reference's tax / boot / boot_tax of both runs, 0-based and row-major.  Per case it prints the share of
(query, pass) entries whose maximum is tied, by the numpy restatement, checks that every reference pick lies in the
restatement's tie set, and refuses a case over the cap that is not about ties.  The example files beside this script are copies
of the reference's inst/extdata/example_train_set.fa.gz and example_seqs.fa (data)."""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

REF = os.environ.get("DADA2_REFERENCE", "/root/reference")


def build_ref(outdir, opt="-O2"):
    """The wrapper + the reference's taxonomy.cpp as outdir/libtaxref.so (oracle/Makefile's flags); returns the loaded library."""
    lib = os.path.join(outdir, "libtaxref.so")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", opt, "-ffp-contract=off", "-fPIC", "-w", "-I", os.path.join(ROOT, "oracle", "shim"),
                           "-I", os.path.join(REF, "src"), "-shared", "-o", lib, os.path.join(HERE, "taxonomy_ref_wrap.cpp"), "-lpthread", "-lm"])
    L = C.CDLL(lib)
    cpp = C.POINTER(C.c_char_p)
    L.taxonomy_ref_run.argtypes = [C.c_int, cpp, cpp, C.c_int, cpp, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_longlong,
                                   C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_char_p, C.c_size_t]
    return L


def run_ref(L, refs, ref_to_genus, genusmat, seqs, unifs, try_rc=False, nthreads=1):
    """One run of C_assign_taxonomy2: {"tax", "boot", "boot_tax"}."""
    import taxonomy_cases as tc

    def arr(strs):
        return (C.c_char_p * len(strs))(*[s.encode("ascii") for s in strs])
    n, gm = len(seqs), np.ascontiguousarray(genusmat, dtype=np.int32)
    r2g = np.ascontiguousarray(ref_to_genus, dtype=np.int32) + 1
    u = np.ascontiguousarray(unifs, dtype=np.float64)
    tax, boot, boot_tax = np.zeros(n, np.int32), np.zeros((n, gm.shape[1]), np.int32), np.zeros((n, 100), np.int32)
    eb = C.create_string_buffer(1024)
    rc = L.taxonomy_ref_run(n, arr(seqs), arr([tc.rc(s) for s in seqs]), len(refs), arr(refs), r2g.ctypes.data, gm.shape[0], gm.shape[1],
                            gm.ctypes.data, int(try_rc), u.ctypes.data, u.size, nthreads, tax.ctypes.data, boot.ctypes.data, boot_tax.ctypes.data, eb, 1024)
    if rc != 0:
        raise RuntimeError(eb.value.decode())
    return {"tax": tax, "boot": boot, "boot_tax": boot_tax}


def main():
    import taxonomy_cases as tc
    out = {}
    entries = ties = 0
    with tempfile.TemporaryDirectory() as tmp:
        L = build_ref(tmp)
        for name, c in tc.build_cases().items():
            unifs = tc.unif_buffer(c["seed"], tc.n_unifs(c["seqs"]))
            runs = [run_ref(L, c["refs"], c["ref_to_genus"], c["genusmat"], c["seqs"], unifs, c["try_rc"]) for _ in range(2)]
            table = tc.train_table(c["refs"], c["ref_to_genus"], c["genusmat"].shape[0])
            best, tied = tc.restate(table, c["seqs"], unifs, c["try_rc"])
            ran = tied.any(axis=2)
            nt = tied.sum(axis=2)
            for k, r in enumerate(runs):
                tc.assert_picks_in_tie_sets(tc.picks(r), tied, "%s run %d" % (name, k))
            differ = int((tc.picks(runs[0]) != tc.picks(runs[1])).sum())
            share = (nt > 1).sum() / max(int(ran.sum()), 1)
            print("%-12s genera %4d queries %2d entries %4d tied %4d (%.1f %%) the two reference runs differ in %d" % (
                name, table.shape[0], len(c["seqs"]), int(ran.sum()), int((nt > 1).sum()), 100 * share, differ))
            if name not in tc.TIES_ARE_THE_POINT:
                if share > tc.TIE_CAP:
                    raise SystemExit("case %s is over the cap of tied entries: choose another seed" % name)
                entries += int(ran.sum())
                ties += int((nt > 1).sum())
            out[name + "/refs"] = np.array(c["refs"])
            out[name + "/ref_to_genus"] = np.asarray(c["ref_to_genus"], dtype=np.int32)
            out[name + "/genusmat"] = np.asarray(c["genusmat"], dtype=np.int32)
            out[name + "/seqs"] = np.array(c["seqs"])
            out[name + "/try_rc"] = np.array(bool(c["try_rc"]))
            out[name + "/seed"] = np.array(c["seed"], dtype=np.int64)
            for k, r in enumerate(runs):
                for key, v in r.items():
                    out["%s/run%d_%s" % (name, k, key)] = v
    assert tuple(out[k].shape for k in out) and set(n.split("/")[0] for n in out) == set(tc.CASE_NAMES)
    np.savez_compressed(tc.GOLDEN, **out)
    print("compared entries %d, tied %d (%.1f %%); wrote %s (%d bytes)" % (entries, ties, 100.0 * ties / entries, tc.GOLDEN, os.path.getsize(tc.GOLDEN)))


if __name__ == "__main__":
    main()
