"""mergePairs over the samples of a run (R/paired.R:92-201), on the device.

``merge_pairs`` takes what the reference's mergePairs takes - one sample or many, dada-class and derep-class objects, file names,
a directory - and goes through dada2hip_merge_run once for all of them: a lane per read pair tallies the (forward, reverse)
pairs of every sample in a table of its own, the unique pairs of all samples are aligned chunk by chunk, and every alignment is
judged (C_eval_pair, prefer, accept) and merged (C_pair_consensus) where the aligner left its moves.  ``api.merge_pairs`` is the
one-sample entry and is unchanged; ``dada2_amd.api`` neither imports nor re-exports this module."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import _lib, api, errormodels
from .dereplicate import _bytes as _blob   # strings as bytes and their offsets
from .io import Derep
from .opts import DadaResult

_EB = 4096
STATS = _lib.MERGE_STATS                                   # the int64 words of dada2hip_merge_run's stats
COLUMNS = ("abundance", "forward", "reverse", "nmatch", "nmismatch", "nindel", "prefer", "accept")
_NA = np.iinfo(np.int32).min
_NOT_DADA = "dadaF and dadaR must be provided as dada-class objects or lists of dada-class objects."
_NOT_DEREP = "derepF and derepR must be provided as derep-class objects or as character vectors of filenames."
_LENGTHS = "The dadaF/derepF/dadaR/derepR arguments must be the same length."
_BAD_MAP = "Incorrect format of $map in derep-class arguments."
_NO_MATCH = "Non-corresponding derep-class and dada-class objects."


def _refuse(msg):
    return _lib.Dada2HipError(1, msg)


def _dadas(obj):
    """(list of DadaResult, names or None): :94-95, :100-102; the names of a dict are names(dadaF), :199."""
    names = None
    if isinstance(obj, DadaResult):
        obj = [obj]
    elif isinstance(obj, dict):
        names, obj = [str(k) for k in obj], list(obj.values())
    if not (isinstance(obj, (list, tuple)) and all(isinstance(d, DadaResult) for d in obj)):
        raise _refuse(_NOT_DADA)
    return list(obj), names


def _dereps(obj):
    """A list of Derep / NativeDerep / file names: :96-99, :103-106."""
    if isinstance(obj, (Derep, api.NativeDerep)):
        return [obj]
    if isinstance(obj, (str, os.PathLike)):
        path = os.fspath(obj)
        return errormodels.parse_fastq_directory(path) if os.path.isdir(path) else [path]
    if isinstance(obj, dict):
        obj = list(obj.values())
    if not (isinstance(obj, (list, tuple)) and all(isinstance(d, (Derep, api.NativeDerep, str, os.PathLike)) for d in obj)):
        raise _refuse(_NOT_DEREP)
    return list(obj)


def _read_map(d, keep):
    """The map of a derep-class object as int32, 0-based, negative for NA: a NativeDerep's in place, a file through the host
    dereplicator (getDerep, :112-113).  What the array looks into is appended to ``keep``."""
    if isinstance(d, (str, os.PathLike)):
        d = api.NativeDerep(os.fspath(d))
    keep.append(d)
    if isinstance(d, api.NativeDerep):
        if not d.nreads:
            return np.zeros(0, dtype=np.int32)
        return np.ctypeslib.as_array(_lib.lib().dada2hip_derep_map(d._h), (d.nreads,))
    m = np.asarray(d.map)
    if m.dtype.kind not in "iu" or m.ndim != 1:
        raise _refuse(_BAD_MAP)                                # (:114)
    if m.size and int(m.max()) > np.iinfo(np.int32).max:
        raise _refuse(_NO_MATCH)
    return np.ascontiguousarray(np.where(m < 0, -1, m), dtype=np.int32) if m.dtype != np.int32 else np.ascontiguousarray(m)


def _pointers(arrays):
    return (C.c_void_p * max(len(arrays), 1))(*[a.ctypes.data if a.size else None for a in arrays])


def _rows(L, h, s, dF, dR, propagate):
    n = L.dada2hip_merge_run_nrow(h, s)
    if not n:
        return []
    col = {k: np.ctypeslib.as_array(C.cast(L.dada2hip_merge_run_column(h, s, i), C.POINTER(C.c_int32)), (n,)).tolist()
           for i, k in enumerate(COLUMNS)}
    off_p = C.c_void_p()
    base = L.dada2hip_merge_run_sequences(h, s, C.byref(off_p))
    off = np.ctypeslib.as_array(C.cast(off_p, C.POINTER(C.c_int64)), (n + 1,)).tolist()
    text = C.string_at(base + off[0], off[-1] - off[0]).decode("ascii") if off[-1] > off[0] else ""
    extra = [(c, dF.clustering[c], dR.clustering[c]) for c in propagate]
    rows = []
    for i in range(n):
        row = {"sequence": text[off[i] - off[0]:off[i + 1] - off[0]]}
        row.update({k: col[k][i] for k in COLUMNS})
        row["prefer"] = None if row["prefer"] == _NA else row["prefer"]
        row["accept"] = bool(row["accept"])
        for c, cf, cr in extra:                                # (:180-183)
            f, r = cf[row["forward"] - 1], cr[row["reverse"] - 1]
            row["F." + c], row["R." + c] = getattr(f, "item", lambda f=f: f)(), getattr(r, "item", lambda r=r: r)()
        rows.append(row)
    return rows


def merge_pairs(dadaF, derepF, dadaR, derepR, min_overlap=12, max_mismatch=0, return_rejects=False, propagate_col=(),
                just_concatenate=False, trim_overhang=False, verbose=False, device: int = 0, stats: dict = None):
    """mergePairs: ``dadaF`` / ``dadaR`` are one DadaResult, a list of them or a dict ``{name: DadaResult}``; ``derepF`` /
    ``derepR`` a Derep, a NativeDerep (its map is read in place), a FASTQ file name, a list of those, or one directory of FASTQ
    files.  Returns one list of row dicts per sample - ``sequence, abundance, forward, reverse, nmatch, nmismatch, nindel,
    prefer, accept`` and ``F.<col>`` / ``R.<col>`` for every ``propagate_col`` that is a column of the clustering table - as a
    list, as a dict where ``dadaF`` had names, or alone where there is one sample (:199-200).  Rows stand in order of first
    appearance, stably by decreasing abundance; a sample with no pair left gives ``[]``; every sample's rows are what
    ``api.make_sequence_table`` takes.  ``stats`` (a dict) receives the library's counters (``STATS``)."""
    dF, names = _dadas(dadaF)
    dR, _ = _dadas(dadaR)
    eF, eR = _dereps(derepF), _dereps(derepR)
    if len({len(dF), len(eF), len(dR), len(eR)}) > 1:
        raise _refuse(_LENGTHS)                                # (:108-109)
    S = len(dF)
    keep = []
    mF, mR = [_read_map(d, keep) for d in eF], [_read_map(d, keep) for d in eR]
    for s in range(S):
        if mF[s].size != mR[s].size:                           # (:116)
            raise _refuse("%s (sample %s: %d forward and %d reverse reads)" % (_NO_MATCH, repr(names[s]) if names else s + 1, mF[s].size, mR[s].size))
    uF = [np.ascontiguousarray(d.map, dtype=np.int32) for d in dF]
    uR = [np.ascontiguousarray(d.map, dtype=np.int32) for d in dR]
    fb, foff = _blob([q for d in dF for q in d.clustering["sequence"]])
    rb, roff = _blob([q for d in dR for q in d.clustering["sequence"]])
    n0F = np.ascontiguousarray(np.concatenate([np.asarray(d.clustering["n0"]) for d in dF]) if S else [], dtype=np.int32)
    n0R = np.ascontiguousarray(np.concatenate([np.asarray(d.clustering["n0"]) for d in dR]) if S else [], dtype=np.int32)
    i32 = lambda v: np.array(v, dtype=np.int32)               # noqa: E731
    nreads = np.array([m.size for m in mF], dtype=np.int64)
    nuF, nuR, ncF, ncR = i32([u.size for u in uF]), i32([u.size for u in uR]), i32([d.nclust for d in dF]), i32([d.nclust for d in dR])
    pF, pR, pUF, pUR = _pointers(mF), _pointers(mR), _pointers(uF), _pointers(uR)
    st = np.zeros(_lib.MERGE_NSTATS, dtype=np.int64)
    eb = C.create_string_buffer(_EB)
    h = C.c_void_p()
    L = _lib.lib()
    _lib.check(L.dada2hip_merge_run(S, nreads.ctypes.data, C.cast(pF, C.c_void_p), C.cast(pR, C.c_void_p), nuF.ctypes.data, C.cast(pUF, C.c_void_p),
                                    nuR.ctypes.data, C.cast(pUR, C.c_void_p), ncF.ctypes.data, fb, foff.ctypes.data, n0F.ctypes.data,
                                    ncR.ctypes.data, rb, roff.ctypes.data, n0R.ctypes.data, int(min_overlap), int(max_mismatch),
                                    int(bool(trim_overhang)), int(bool(just_concatenate)), int(device), C.byref(h), st.ctypes.data, eb, _EB), eb)
    try:
        out = []
        for s in range(S):
            propagate = [c for c in propagate_col if c in dF[s].clustering]          # (:179) other names are dropped silently
            rows = _rows(L, h, s, dF[s], dR[s], propagate)
            if verbose:
                if not rows:                                   # (:134)
                    print("No paired-reads (in ZERO unique pairings) successfully merged out of %d pairings) input." % mF[s].size)
                else:                                          # (:188)
                    print("%d paired-reads (in %d unique pairings) successfully merged out of %d (in %d pairings) input."
                          % (sum(r["abundance"] for r in rows if r["accept"]), sum(r["accept"] for r in rows),
                             sum(r["abundance"] for r in rows), len(rows)))
            if not return_rejects:
                rows = [r for r in rows if r["accept"]]
            seqs = [r["sequence"] for r in rows]
            if len(set(seqs)) < len(seqs):                     # (:192-194)
                print("Duplicate sequences in merged output.")
            out.append(rows)
    finally:
        L.dada2hip_merge_run_free(h)
    if stats is not None:
        stats.update({k: int(st[i]) for i, k in enumerate(STATS)})
    if S == 1:
        return out[0]
    return dict(zip(names, out)) if names is not None else out
