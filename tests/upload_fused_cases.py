"""Cases for the boundary call's fused upload (sample_create's one pass over the rows: length, abundance, prior, 2-bit packing and
quality rounding of a row in one visit, the chunks' copies queued by the thread that finishes a chunk) and for the call that no
longer waits for the upload between create and run - shared by tests/test_emu_upload_fused.py (the product's code under the
emulator) and tests/test_gpu_upload_fused.py (the device).  Every result is compared field by field - clustering, birth_subs,
subqual, clusterquals, map, pval - with the plain-C restatement (oracle/cport) by helpers.assert_results_equal.

The samples are small on purpose: a piece of the pass is 512 rows and DADA2HIP_UPLOAD_CHUNK_ROWS=512 makes a chunk one piece, so
513 rows already cross a piece border and a chunk border, and 1 537 rows are four chunks with a last one of one row.  Each shape
runs with the knob and without it (one chunk).  Reads are 20-52 nt, ragged, the quality matrix NaN behind every read's end, and 52
is no multiple of 16 (the packed rows' and the quality rows' padding is live)."""
import re

import numpy as np

from helpers import assert_results_equal, tperr1
from species_cases import with_env

KNOB = "DADA2HIP_UPLOAD_CHUNK_ROWS"
ENVS = [{KNOB: "512"}, {}]

MSG_LONG = "Input sequences exceed the maximum allowed string length."
MSG_KMER = "Input sequences must all be longer than the kmer-size (5)."
MSG_STRIDE = "Sequence must have associated qualities for each nucleotide position."
MSG_ACGT = "Invalid derep$uniques vector. Sequences must be made up only of A/C/G/T."
MSG_QUAL = "Invalid derep$quals matrix. Quality values must be positive integers."

_BASE = {}


def base():
    """1 537 uniques of 20-52 nt (dada2_amd.synth), NaN behind each read's end."""
    if "d" not in _BASE:
        from dada2_amd.synth import make_sample
        d = make_sample(tperr1(), 1537, L=60, G=6, seed=5, Lmin=20, chunk=6200)
        lens = np.array([len(s) for s in d.seqs])
        q = np.asarray(d.quals, dtype=np.float64)
        assert q.shape == (1537, lens.max()) and lens.min() >= 20 and lens.max() % 16 != 0, (q.shape, lens.min(), lens.max())
        for i in (0, 1, 700, 1536):                                  # NaN exactly behind the read's end
            assert not np.isnan(q[i, : lens[i]]).any() and np.isnan(q[i, lens[i]:]).all()
        assert (lens < lens.max()).sum() > 100
        _BASE["d"] = (list(d.seqs), np.asarray(d.abundances, dtype=np.int32), q)
    return _BASE["d"]


def prefix(n):
    seqs, ab, q = base()
    seqs, ab = seqs[:n], ab[:n]
    return seqs, ab, np.ascontiguousarray(q[:n, : max(len(s) for s in seqs)])


def longest_at(n, row):
    """The first n uniques with ONE longest read, in ``row``: every other read as long loses its last base."""
    seqs, ab, q = prefix(n)
    seqs, q = list(seqs), q.copy()
    lens = [len(s) for s in seqs]
    m = max(lens)
    j = lens.index(m)
    seqs[j], seqs[row] = seqs[row], seqs[j]
    q[[j, row]] = q[[row, j]]
    ab = ab.copy()
    ab[[j, row]] = ab[[row, j]]
    for i, s in enumerate(seqs):
        if i != row and len(s) == m:
            seqs[i] = s[:-1]
            q[i, m - 1] = np.nan
    assert [i for i, s in enumerate(seqs) if len(s) == m] == [row]
    return seqs, ab, q


SHAPES = {
    "n1": lambda: prefix(1),
    "n511": lambda: prefix(511),
    "n512": lambda: prefix(512),
    "n513": lambda: prefix(513),
    "n1537": lambda: prefix(1537),
    "longest_last": lambda: longest_at(1100, 1099),
    "longest_first": lambda: longest_at(1100, 0),
    "longest_second_chunk": lambda: longest_at(1100, 700),
}


def _oracle(seqs, ab, q, opts=None):
    from oracle import cport
    from dada2_amd.opts import DadaOpts
    return cport.dada_uniques(seqs, ab, None, tperr1(), q, opts or DadaOpts())


def run_shape(name, device=0):
    """The shape through the boundary call with a chunk of 512 rows and with the automatic chunk, each against the restatement."""
    from dada2_amd import api
    seqs, ab, q = SHAPES[name]()
    want = _oracle(seqs, ab, q)
    for env in ENVS:
        got = with_env(env, lambda: api.dada_uniques(seqs, ab, None, tperr1(), q, device=device))
        assert_results_equal(got, want)
    return "ok %s %d uniques %d partitions" % (name, len(seqs), want.nclust)


# ---- input errors: today's message, the earliest of today's order, and a valid call afterwards --------------------------------------
def _bad_letter(seqs, ab, q):
    seqs = list(seqs)
    seqs[-1] = seqs[-1][:-1] + "N"                                   # the last base of the last row
    return seqs, ab, q


def _bad_quality(value):
    def f(seqs, ab, q):
        q = q.copy()
        r = len(seqs) - 3                                            # a row of the last chunk (1 537 rows: the chunk of one row is 1536)
        q[r, len(seqs[r]) // 2] = value
        return seqs, ab, q
    return f


def _stride(delta):
    def f(seqs, ab, q):
        if delta > 0:
            q = np.concatenate([q, np.full((q.shape[0], delta), np.nan)], axis=1)
        else:
            q = q[:, :delta]                                         # a row is longer than the stated stride
        return seqs, ab, np.ascontiguousarray(q)
    return f


def _short(n):
    def f(seqs, ab, q):
        seqs = list(seqs)
        seqs[len(seqs) // 2] = seqs[len(seqs) // 2][:n]
        return seqs, ab, q
    return f


def _letter_and_stride(seqs, ab, q):
    seqs, ab, q = _bad_letter(seqs, ab, q)
    return _stride(+1)(seqs, ab, q)


# name -> (rows, what is done to them, the message)
ERRORS = {
    "non_acgt_last_base_last_row": (1537, _bad_letter, MSG_ACGT),
    "quality_minus_one": (1537, _bad_quality(-1.0), MSG_QUAL),
    "quality_300": (1537, _bad_quality(300.0), MSG_QUAL),
    # 640 rows of stride 49..64: the pinned quality bytes (640 x 64 B) and packed rows (640 x 16 B) are whole allocation classes of
    # the library's cache, so under the emulator's guarded allocations the inaccessible page starts at their last byte
    "stride_one_above": (640, _stride(+1), MSG_STRIDE),
    "stride_one_below": (640, _stride(-1), MSG_STRIDE),
    "read_of_6": (600, _short(6), None),                            # 6 nt is legal: the k-mer-size rule is "longer than 5"
    "read_of_5": (600, _short(5), MSG_KMER),
    "letter_and_stride": (600, _letter_and_stride, MSG_STRIDE),     # two errors at once: the stride check comes first
}


def run_error(name, device=0):
    from dada2_amd import _lib, api
    n, make, message = ERRORS[name]
    good = prefix(n)
    seqs, ab, q = make(*good)
    for env in ENVS:
        if message is None:
            got = with_env(env, lambda: api.dada_uniques(seqs, ab, None, tperr1(), q, device=device))
            assert_results_equal(got, _oracle(seqs, ab, q))
        else:
            try:
                with_env(env, lambda: api.dada_uniques(seqs, ab, None, tperr1(), q, device=device))
            except _lib.Dada2HipError as ex:
                assert str(ex).endswith(message) or message in str(ex), str(ex)
                assert getattr(ex, "code", 1) == 1, ex.code            # DADA2HIP_ERR_INPUT
            else:
                raise AssertionError("%s was accepted" % name)
        # the process is as good as before: the same rows, valid, through the same call
        got = with_env(env, lambda: api.dada_uniques(*good[:2], None, tperr1(), good[2], device=device))
        assert_results_equal(got, _oracle(*good))
    return "ok error %s" % name


# ---- the boundary call against a resident sample, and two samples in flight ----------------------------------------------------------
def run_boundary_equals_resident(device=0):
    """dada_uniques (upload not waited for between create and run) and Sample(...).run (upload complete when create returns) on the
    same input: equal results, twice over on the resident sample."""
    from dada2_amd import api
    seqs, ab, q = prefix(1100)
    want = _oracle(seqs, ab, q)
    for env in ENVS:
        a = with_env(env, lambda: api.dada_uniques(seqs, ab, None, tperr1(), q, device=device))
        s = with_env(env, lambda: api.Sample(seqs, ab, None, q, device=device))
        try:
            b, c = s.run(tperr1()), s.run(tperr1())
        finally:
            s.close()
        for r in (a, b, c):
            assert_results_equal(r, want)
        assert_results_equal(a, b)
    return "ok boundary equals resident, %d partitions" % want.nclust


def run_multi_equals_single(device=0):
    """run_multi with two samples in flight on one device: each sample's result is its single call's."""
    from dada2_amd import api
    from dada2_amd.io import Derep
    ds = [Derep(*prefix(n), np.zeros(0, dtype=np.int32)) for n in (1100, 513, 700, 1)]
    for env in ENVS:
        got = with_env(env, lambda: api.dada_uniques_multi(ds, tperr1(), devices=(device, device)))
        assert len(got) == len(ds)
        for g, d in zip(got, ds):
            single = with_env(env, lambda: api.dada_uniques(d.seqs, d.abundances, None, tperr1(), d.quals, device=device))
            assert_results_equal(g, single)
            assert_results_equal(g, _oracle(d.seqs, d.abundances, d.quals))
    return "ok multi equals single"


# ---- what the pass did, from its DADA2HIP_V2_SUMMARY line: chunks made, k-mer launches given -----------------------------------------
UPLOAD_LINE = re.compile(r"\[upload\] rows (\d+)  chunk rows (\d+)  chunks (\d+)  k-mer launches (\d+)")
AUTO_CHUNK_ROWS = (16 << 20) // 64 // 512 * 512                     # 16 MB of quality rows of 64 bytes (reads of 49-64 nt)


def upload_lines(stderr_text):
    """(rows, chunk rows, chunks, k-mer launches) of every upload the library reported on stderr."""
    return [tuple(int(x) for x in m.groups()) for m in UPLOAD_LINE.finditer(stderr_text)]


def _short_row(row, n):
    def f(seqs, ab, q):
        seqs = list(seqs)
        seqs[row] = seqs[row][:n]
        return seqs, ab, q
    return f


def _one_column_short(seqs, ab, q):
    return seqs, ab, np.ascontiguousarray(q[:, :-1])


# (input, environment, expected line, expected message or None).  A chunk is 512 rows under the knob, so 1 100 rows are chunks of
# rows 0-511, 512-1023 and 1024-1099; the copies and launches go out in chunk order, whichever thread finishes a chunk.  The k-mer
# build is launched for a chunk only while every row so far fits the stated geometry (k-mer size < length <= quals_nrow): a misfit
# in chunk k leaves exactly k launches.  An input that fails for another reason has had all its launches, on rows that fit.
CHUNK_CASES = [
    ("n513_knob", lambda: prefix(513), ENVS[0], (513, 512, 2, 2), None),                    # the knob is read: two chunks, not one
    ("n1537_knob", lambda: prefix(1537), ENVS[0], (1537, 512, 4, 4), None),
    ("n1537_auto", lambda: prefix(1537), ENVS[1], (1537, AUTO_CHUNK_ROWS, 1, 1), None),
    ("read_of_5_in_chunk_1", lambda: _short_row(700, 5)(*prefix(1100)), ENVS[0], (1100, 512, 3, 1), MSG_KMER),
    ("read_of_5_in_chunk_0", lambda: _short_row(10, 5)(*prefix(1100)), ENVS[0], (1100, 512, 3, 0), MSG_KMER),
    ("row_past_the_stride_in_chunk_2", lambda: _one_column_short(*longest_at(1100, 1099)), ENVS[0], (1100, 512, 3, 2), MSG_STRIDE),
    ("row_past_the_stride_in_chunk_0", lambda: _one_column_short(*longest_at(1100, 0)), ENVS[0], (1100, 512, 3, 0), MSG_STRIDE),
    ("bad_letter", lambda: _bad_letter(*prefix(1100)), ENVS[0], (1100, 512, 3, 3), MSG_ACGT),
    ("stride_one_above", lambda: _stride(+1)(*prefix(1100)), ENVS[0], (1100, 512, 3, 3), MSG_STRIDE),
]
EXPECTED_UPLOAD_LINES = [c[3] for c in CHUNK_CASES]


def run_chunk_cases(device=0):
    """Every case of CHUNK_CASES in order with DADA2HIP_V2_SUMMARY set; the caller compares upload_lines(the process's stderr)
    with EXPECTED_UPLOAD_LINES."""
    from dada2_amd import _lib, api
    for name, make, env, line, message in CHUNK_CASES:
        seqs, ab, q = make()
        assert max(len(s) for s in seqs) > 48, name                 # (quality rows of 64 bytes: AUTO_CHUNK_ROWS)
        e = dict(env)
        e["DADA2HIP_V2_SUMMARY"] = "1"
        try:
            got = with_env(e, lambda: api.dada_uniques(seqs, ab, None, tperr1(), q, device=device))
        except _lib.Dada2HipError as ex:
            assert message is not None and message in str(ex), (name, str(ex))
        else:
            assert message is None, name
            assert_results_equal(got, _oracle(seqs, ab, q))
    return "ok chunk cases"


# ---- the final pass's work list, built on the device ---------------------------------------------------------------------------------
# (band, DADA2HIP_NW_KERNEL or None): BAND_SIZE 0 is the gapless final pass, `lane` makes a chunk 64 slots
WORKLIST_CASES = {"band0": (0, None), "band16": (16, None), "band32": (32, None), "band16_lane": (16, "lane")}
WL_LEN = 60


def _final_worklist(sample):
    """dada2hip_sample_final_worklist of a Sample that has been run: (work, chunk_centre, per, built_on_device)."""
    import ctypes as C
    from dada2_amd import _lib
    L = _lib.lib()
    info = np.zeros(4, dtype=np.int64)
    eb = C.create_string_buffer(1024)
    _lib.check(L.dada2hip_sample_final_worklist(sample._h, None, 0, None, 0, info.ctypes.data, eb, 1024), eb)
    work, cc = np.full(int(info[0]), -7, dtype=np.int32), np.full(int(info[1]), -7, dtype=np.int32)
    _lib.check(L.dada2hip_sample_final_worklist(sample._h, work.ctypes.data, work.size, cc.ctypes.data, cc.size, info.ctypes.data, eb, 1024), eb)
    return work, cc, int(info[2]), int(info[3])


def worklist_sample(per):
    """Groups of 60-nt reads far from each other: a centre with many reads and single-read uniques one substitution away from it,
    which stay with it (a single read never buds).  Group sizes per, per - 1, per + 1, 1 (a centre alone) and three of 150; where
    a chunk is ONE slot (the cooperative aligner at a wide band) there is no group of per - 1."""
    assert 1 <= per <= 150, per
    rng = np.random.default_rng(77)
    sizes = [m for m in (150, per, 1, per - 1, 150, per + 1, 150) if m > 0]
    seqs, ab = [], []
    for g, m in enumerate(sizes):
        centre = "".join("ACGT"[int(x)] for x in rng.integers(0, 4, size=WL_LEN))
        seqs.append(centre); ab.append(2000 - 100 * g)
        for k in range(m - 1):                                       # distinct single substitutions: position k % 60, the (k // 60 + 1)-th other base
            p, b = k % WL_LEN, "ACGT"[("ACGT".index(centre[k % WL_LEN]) + k // WL_LEN + 1) % 4]
            seqs.append(centre[:p] + b + centre[p + 1:]); ab.append(1)
    assert len(set(seqs)) == len(seqs) and 300 <= len(seqs) <= 3000
    order = np.argsort(-np.asarray(ab), kind="stable")               # as a derep object has them: by abundance
    seqs = [seqs[int(k)] for k in order]
    return seqs, np.asarray(ab, dtype=np.int32)[order], np.full((len(seqs), WL_LEN), 35.0), sizes


def run_worklist(name, device=0):
    """One resident sample run under the case's options: results equal to the oracle's, the list read back - built on the device,
    every unique once, a partition's members (ascending) in chunks that carry its centre, -1 behind them up to a whole chunk."""
    from dada2_amd import api
    from dada2_amd.opts import DadaOpts
    band, kernel = WORKLIST_CASES[name]
    env = {"DADA2HIP_NW_KERNEL": kernel} if kernel else {}
    opts = DadaOpts(BAND_SIZE=band)

    def run(seqs, ab, q):
        s = api.Sample(seqs, ab, None, q, device=device)
        try:
            got = s.run(tperr1(), opts)
            return got, _final_worklist(s)
        finally:
            s.close()
    # what a chunk is under these options (it depends on the read length and the band, not on the reads): from a first run
    probe = worklist_sample(8)
    per = with_env(env, lambda: run(*probe[:3]))[1][2]
    if kernel == "lane":
        assert per == 64, per
    seqs, ab, q, sizes = worklist_sample(per)
    want = _oracle(seqs, ab, q, opts)
    # facts before trust: the oracle's partitions have the sizes the case is about
    assert want.nclust >= 5 and sorted(want.clustering["nunq"].tolist()) == sorted(sizes), (want.clustering["nunq"].tolist(), sizes)
    got, (work, cc, per2, on_device) = with_env(env, lambda: run(seqs, ab, q))
    assert_results_equal(got, want)
    assert per2 == per and on_device == 1, (per2, per, on_device)
    part = np.asarray(got.map) - int(np.min(got.map))                # partition of every unique, from 0
    centre = np.asarray(got.stats["center"])
    off = 0
    for c in range(got.nclust):
        members = np.flatnonzero(part == c)
        nch = -(-members.size // per)
        assert np.array_equal(work[off:off + members.size], members), (name, c)
        assert np.all(work[off + members.size:off + nch * per] == -1), (name, c)
        assert np.all(cc[off // per:off // per + nch] == centre[c]), (name, c, cc[off // per:off // per + nch], centre[c])
        off += nch * per
    assert off == work.size and cc.size * per == work.size
    assert np.array_equal(np.sort(work[work >= 0]), np.arange(len(seqs)))
    return "ok worklist %s per %d, partitions of %s" % (name, per, want.clustering["nunq"].tolist())
