"""mergeSequenceTables on the device (R/multiSample.R:290-364), and the two helpers getSequences (R/misc.R:101-128) and
uniquesToFasta (R/sequenceIO.R:226-237).

A sequence table here is a triple ``(mat, seqs, sample_names)``: ``(mat, seqs)`` is what ``api.make_sequence_table`` returns, an
integer array [samples, sequences] with its column names, and ``sample_names`` are the names of its rows.
``merge_sequence_tables`` goes through dada2hip_seqtab_merge: the column names of all tables are dereplicated on the device, with
``try_rc`` every distinct sequence's reverse complement is looked up in the same table, and the cells are added, keyed and reordered
there.  ``dada2_amd.api`` neither imports nor re-exports this module."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import _lib, api
from .dereplicate import _bytes as _blob   # names as latin-1 bytes and their offsets
from .primers import rc   # noqa: F401  (Biostrings' complement of the IUPAC letters, as tryRC takes it)

_EB = 4096
STATS = _lib.SEQTAB_STATS                                 # the int64 words of dada2hip_seqtab_merge's stats
_ORDER = {"abundance": 1, "nsamples": 2}
_I32 = np.iinfo(np.int32)


class _Result:
    """The library's handle, freed with the last array that looks into it."""

    def __init__(self, h):
        self.h = h

    def __del__(self):
        if self.h:
            _lib.lib().dada2hip_seqtab_free(self.h)
            self.h = None


def _names(fn, h, n):
    off_p = C.c_void_p()
    ptr = fn(h, C.byref(off_p))
    off = np.ctypeslib.as_array(C.cast(off_p, C.POINTER(C.c_int64)), shape=(n + 1,)).tolist() if n else [0]
    text = C.string_at(ptr, off[-1]).decode("latin-1") if off[-1] else ""
    return [text[off[i]:off[i + 1]] for i in range(n)]


def _tables(tables):
    """The checks that need the Python objects: ``(int32 matrices, all column names, all row names)``, table after table."""
    if not isinstance(tables, (list, tuple)) or len(tables) < 2:
        raise ValueError("At least two sequence tables are expected")
    mats, cols, rows = [], [], []
    for i, t in enumerate(tables):
        if not (isinstance(t, (list, tuple)) and len(t) == 3):
            raise ValueError(f"Sequence table {i + 1}: a (mat, seqs, sample_names) triple is expected.")
        m = np.asarray(t[0])
        if m.ndim != 2:
            raise ValueError(f"Not a matrix (sequence table {i + 1}).")
        seqs, names = list(t[1]), list(t[2])
        if m.shape != (len(names), len(seqs)):
            raise ValueError(f"Sequence table {i + 1}: {m.shape[0]} x {m.shape[1]} cells do not fit {len(names)} row (sample) names "
                             f"and {len(seqs)} column (sequence) names.")
        if m.dtype.kind not in "iub":
            raise ValueError(f"Sequence table {i + 1}: integer counts are expected.")
        if m.size and (int(m.max()) > _I32.max or int(m.min()) < _I32.min):
            raise _lib.Dada2HipError(1, "dada2hip: an abundance of the sequence table exceeds the integer range.")
        mats.append(np.ascontiguousarray(m, dtype=np.int32))
        cols += seqs
        rows += names
    return mats, cols, rows


def merge_sequence_tables(tables, repeats="error", order_by="abundance", try_rc=False, device: int = 0, stats: dict = None):
    """mergeSequenceTables: ``tables`` is a list of at least two ``(mat, seqs, sample_names)`` triples; returns
    ``(mat int32 [samples, sequences] C-contiguous, seqs, sample_names)``.

    Sample names are the tables' row names in order; a name in more than one table is an error with ``repeats="error"`` and one
    summed row, at its first place, with ``repeats="sum"``.  The sequences stand in order of first appearance and are then stably
    ordered by ``order_by`` ("abundance", "nsamples" or None).  With ``try_rc`` a sequence whose reverse complement appears earlier
    is added to that one (every letter must then be upper-case ACGT or an IUPAC code).  Refused, unlike in the reference, which
    warns: a table that holds a column name or a row name twice.  Also refused: an empty table, and a merged cell above the int32
    range (NA in the reference).  ``stats`` (a dict) receives the library's counters (``STATS``) and ``col_map``, the column of the
    result every input column went to, table after table."""
    if repeats not in ("error", "sum"):
        raise ValueError('repeats must be "error" or "sum"')
    if order_by is not None and not (isinstance(order_by, str) and order_by in _ORDER):
        raise ValueError('order_by must be "abundance", "nsamples" or None')
    mats, cols, rows = _tables(tables)
    n = len(mats)
    nrow = np.array([m.shape[0] for m in mats], dtype=np.int32)
    ncol = np.array([m.shape[1] for m in mats], dtype=np.int32)
    cells = (C.c_void_p * n)(*[m.ctypes.data for m in mats])
    cb, coff = _blob(cols)
    rb, roff = _blob(rows)
    col_map = np.zeros(len(cols), dtype=np.int32)
    st = np.zeros(_lib.SEQTAB_NSTATS, dtype=np.int64)
    eb = C.create_string_buffer(_EB)
    h = C.c_void_p()
    L = _lib.lib()
    _lib.check(L.dada2hip_seqtab_merge(n, nrow.ctypes.data, ncol.ctypes.data, C.cast(cells, C.c_void_p), cb, coff.ctypes.data, rb,
                                       roff.ctypes.data, int(repeats == "sum"), _ORDER.get(order_by, 0), int(bool(try_rc)), int(device),
                                       C.byref(h), col_map.ctypes.data, st.ctypes.data, eb, _EB), eb)
    res = _Result(h)
    nr, nc = L.dada2hip_seqtab_nrow(h), L.dada2hip_seqtab_ncol(h)
    if nr * nc:
        buf = (C.c_int32 * (nr * nc)).from_address(L.dada2hip_seqtab_cells(h))
        buf._owner = res                                   # the array's base keeps the buffer, the buffer the handle
        mat = np.frombuffer(buf, dtype=np.int32).reshape(nr, nc)
    else:
        mat = np.zeros((nr, nc), dtype=np.int32)
    out_seqs = _names(L.dada2hip_seqtab_sequences, h, nc)
    out_names = _names(L.dada2hip_seqtab_samples, h, nr)
    if stats is not None:
        stats.update({k: int(st[i]) for i, k in enumerate(STATS)})
        stats["col_map"] = col_map
    return mat, out_seqs, out_names


def _file_sequences(path):
    import gzip
    with open(path, "rb") as fh:
        gz = fh.read(2) == b"\x1f\x8b"
    with (gzip.open if gz else open)(path, "rb") as fh:
        head = fh.read(1)
    if head == b">":
        return api.read_fasta(path)[1]
    d = api.derep_fastq(path)                               # the FASTQ reader: every read is its unique's sequence
    return [d.seqs[int(m)].upper() if m >= 0 else "" for m in np.asarray(d.map)]


def get_sequences(obj, collapse=False):
    """getSequences: the sequences of ``obj``, in upper case.  ``obj``: a path to a FASTA or FASTQ file (every record's
    sequence); a sequence or a list of sequences; or what ``api.get_uniques`` takes - a {sequence: abundance} mapping, a
    (sequences, abundances) pair, a DadaResult, a Derep, a ``(mat, seqs)`` table.  ``collapse`` keeps the first of every
    duplicate of a list of sequences; of an object with abundances it gives ``api.get_uniques``' merged names, which stand in
    ascending byte order when something was merged (names(tapply(.)), R/misc.R:55)."""
    if isinstance(obj, (str, os.PathLike)):
        if os.path.isfile(os.fspath(obj)):
            return _file_sequences(os.fspath(obj))
        return [str(obj).upper()]
    if isinstance(obj, (list, tuple)) and all(isinstance(s, str) for s in obj):
        seqs = list(dict.fromkeys(obj)) if collapse else list(obj)
    elif collapse:
        seqs = api.get_uniques(obj)[0]
    else:
        seqs = api._input_uniques(obj)[0]
    return [s.upper() for s in seqs]


def uniques_to_fasta(unqs, fout, ids=None, mode="w", width=20000):
    """uniquesToFasta: ``unqs`` (what ``api.get_uniques`` takes) as FASTA records in input order, duplicates kept
    (getUniques(collapse=FALSE)).  ``ids``: one per sequence, by default ``sq<i>;size=<abundance>;``.  A record is ``>id`` and the
    sequence in lines of ``width`` letters; ``mode`` "w" writes the file anew, "a" appends."""
    if mode not in ("w", "a"):
        raise ValueError('mode must be "w" or "a"')
    if int(width) < 1:
        raise ValueError("width must be at least 1")
    width = int(width)
    seqs, abund = api._input_uniques(unqs)
    if ids is None:
        ids = ["sq%d;size=%d;" % (i + 1, int(a)) for i, a in enumerate(abund)]
    ids = [str(x) for x in ids]
    if len(ids) != len(seqs):
        raise ValueError("One id per sequence is required.")
    with open(fout, mode, newline="\n") as fh:
        for name, s in zip(ids, seqs):
            fh.write(">" + name + "\n")
            for i in range(0, len(s), width):
                fh.write(s[i:i + width] + "\n")
