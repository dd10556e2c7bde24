"""removePrimers (R/filter.R:81-233) on the GPU: primer search on both strands, orientation and trimming.

The public entry point is ``dada2_amd.primers.remove_primers``.  It lives in this module, and ``dada2_amd.api`` neither imports nor
re-exports it: ``tests/filter_cases.py`` pins that ``dada2_amd.api`` has no attribute ``remove_primers``.

``primer_hits`` is dada2hip_primers_reads on reads in memory (per-read verdicts, no whole-file rule); ``remove_primers`` restates
the R wrapper around dada2hip_primers_fastq: the path checks, the output directories, the reads.in / reads.out matrix with its row
names, the messages under ``verbose`` and the warning when nothing passes.  Matching with indels (``allow.indels = TRUE``,
Biostrings' edit-distance matcher) is not supported."""
from __future__ import annotations

import ctypes as C
import os
import warnings

import numpy as np

from . import _lib

_EB = 2048
_COMPLEMENT = str.maketrans("ACGTMRWSYKVHDBN", "TGCAKYWSRMBDHVN")   # Biostrings' complement of the IUPAC codes


def rc(seq):
    """The reverse complement, with the IUPAC complement (A<->T C<->G M<->K R<->Y V<->B H<->D; W, S and N map to themselves)."""
    return str(seq).translate(_COMPLEMENT)[::-1]


def is_acgt(seq):
    """C_isACGT: True when the sequence is upper-case A/C/G/T only (the primer is then matched with fixed = TRUE)."""
    return all(c in "ACGT" for c in str(seq))


def _params(primer_fwd, primer_rev, max_mismatch, allow_indels, trim_fwd, trim_rev, orient):
    if allow_indels:
        raise NotImplementedError("removePrimers' allow.indels = TRUE is not supported by this library.")
    if not isinstance(primer_fwd, str) or not (primer_rev is None or isinstance(primer_rev, str)):
        raise ValueError("Primer sequences must be provided as base R strings.")
    return _lib.CPrimerParams(primer_fwd.encode(), None if primer_rev is None else primer_rev.encode(), int(max_mismatch),
                              int(bool(trim_fwd)), int(bool(trim_rev)), int(bool(orient)), 0, 0)


def primer_hits(seqs, primer_fwd, primer_rev=None, max_mismatch=2, orient=True, trim_fwd=True, trim_rev=True, device=0,
                stats: dict = None):
    """dada2hip_primers_reads on sequences in memory.  Returns a dict of per-read arrays: ``code`` (0 kept, else an index into
    _lib.PRIMER_CODES), ``flip``, ``first`` and ``last`` (the kept window, 1-based and inclusive, in the kept orientation),
    ``hits`` (n, 4: forward primer, reverse primer, forward primer on the reverse complement, reverse primer on it) and ``starts``
    (n, 4, 2: the first and the last start of each, 1-based on its strand; -2**31 without a match)."""
    p = _params(primer_fwd, primer_rev, max_mismatch, False, trim_fwd, trim_rev, orient)
    bs = [s if isinstance(s, bytes) else str(s).encode() for s in seqs]
    n = len(bs)
    off = np.zeros(n + 1, dtype=np.int64)
    if bs:
        np.cumsum([len(b) for b in bs], out=off[1:])
    out = {k: np.zeros(n, dtype=np.int32) for k in ("code", "flip", "first", "last")}
    out["hits"] = np.zeros((n, 4), dtype=np.int32)
    out["starts"] = np.zeros((n, 4, 2), dtype=np.int32)
    st = np.zeros(_lib.PRIMERS_NSTATS, dtype=np.int64)
    eb = C.create_string_buffer(_EB)
    rv = _lib.lib().dada2hip_primers_reads(n, b"".join(bs), off.ctypes.data, C.byref(p), int(device), out["code"].ctypes.data,
                                           out["flip"].ctypes.data, out["first"].ctypes.data, out["last"].ctypes.data,
                                           out["hits"].ctypes.data, out["starts"].ctypes.data, st.ctypes.data, eb, _EB)
    if stats is not None:
        stats.update({k: int(st[i]) for i, k in enumerate(_lib.PRIMERS_STATS)})
    _lib.check(rv, eb)
    return out


def primers_fastq(fn, fout, primer_fwd, primer_rev=None, max_mismatch=2, trim_fwd=True, trim_rev=True, orient=True, compress=True,
                  n=10**5, device=0, stats: dict = None):
    """dada2hip_primers_fastq on one file: (reads_in, reads_out).  ``n``: records per chunk."""
    p = _params(primer_fwd, primer_rev, max_mismatch, False, trim_fwd, trim_rev, orient)
    rin, rout = C.c_int64(), C.c_int64()
    st = np.zeros(_lib.PRIMERS_NSTATS, dtype=np.int64)
    eb = C.create_string_buffer(_EB)
    _lib.check(_lib.lib().dada2hip_primers_fastq(os.fspath(fn).encode(), os.fspath(fout).encode(), C.byref(p), int(bool(compress)), int(n),
                                                 int(device), C.byref(rin), C.byref(rout), st.ctypes.data, eb, _EB), eb)
    if stats is not None:
        stats.update({k: int(st[i]) for i, k in enumerate(_lib.PRIMERS_STATS)})
    return rin.value, rout.value


def remove_primers(fn, fout, primer_fwd, primer_rev=None, max_mismatch=2, allow_indels=False, trim_fwd=True, trim_rev=True,
                   orient=True, compress=True, verbose=False, device=0):
    """removePrimers over one file or lists of files: returns (an (nfiles, 2) int64 array of reads.in / reads.out, the row names
    basename(fn)).  Output directories are created; duplicate outputs and outputs equal to an input are refused; an existing
    output is removed first; a file from which nothing passes is not written."""
    aslist = lambda x: [os.fspath(x)] if (isinstance(x, (str, bytes)) or hasattr(x, "__fspath__")) else [os.fspath(y) for y in x]   # noqa: E731
    fn, fout = aslist(fn), aslist(fout)
    if len(fn) != len(fout):                                                                    # :87
        raise ValueError("Every input file must have a corresponding output file.")
    _params(primer_fwd, primer_rev, max_mismatch, allow_indels, trim_fwd, trim_rev, orient)   # (refusals before anything is created)
    for odir in sorted({os.path.dirname(f) for f in fout}):                                   # :91-97
        if odir and not os.path.isdir(odir):
            if verbose:
                print("Creating output directory:", odir)
            os.makedirs(odir, exist_ok=True)
    if not all(os.path.exists(f) for f in fn):                                                  # :98
        raise ValueError("Some input files do not exist.")
    ins, outs = [os.path.realpath(f) for f in fn], [os.path.realpath(f) for f in fout]
    if len(set(outs)) != len(outs):                                                             # :101
        raise ValueError("All output files must be distinct.")
    if set(outs) & set(ins):                                                                    # :102
        raise ValueError("Output files must be distinct from the input files.")
    rval = np.zeros((len(fn), 2), dtype=np.int64)
    multi_msg = True
    for i in range(len(fn)):
        st = {}
        if verbose and os.path.exists(outs[i]):
            print("Overwriting file:" + outs[i])                                                # :217
        rval[i] = primers_fastq(ins[i], outs[i], primer_fwd, primer_rev, max_mismatch, trim_fwd, trim_rev, orient, compress,
                                device=device, stats=st)
        if verbose:
            if st["multiple_matches"] and multi_msg:                                            # :160-163
                print("Multiple matches to the primer(s) in some sequences. Using the longest possible match.")
                multi_msg = False
            if st["flipped"] and rval[i, 1]:                                                    # :182
                print(st["flipped"], "sequences out of", int(rval[i, 0]), "are being reverse-complemented.")
            perc = round(int(rval[i, 1]) * 100 / int(rval[i, 0]), 1) if rval[i, 0] else float("nan")   # filt.print, :235-239
            print(f"Read in {int(rval[i, 0])}, output {int(rval[i, 1])} ({perc}%) filtered sequences.")
    if len(fn) and (rval[:, 1] == 0).all():                                                     # :227-231
        warnings.warn("No reads passed the primer detection.")
    elif verbose and (rval[:, 1] == 0).any():
        print("Some input samples had no reads pass the primer detection.")
    return rval, [os.path.basename(f) for f in fn]
