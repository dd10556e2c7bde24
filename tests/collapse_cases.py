"""collapseNoMismatch (R/multiSample.R:104-160) restated for the tests, the tables it is run on, and the brute-force form of what
the device's scan kernel computes per pair.  Seeded, pure numpy, nothing on disk.  Used by tests/test_collapse.py (no GPU),
tests/test_emu_collapse.py (the emulator), tests/test_gpu_collapse.py (the MI355X), tests/golden/make_collapse_golden.py and
tools/collapse_bench.py.

`restate` is the reference's loop, statement by statement, over a `checker` module for nwhamming: oracle.cport (the plain-C
restatement: C_nwalign + eval_pair) or, where it is built, oracle.ref (the reference compiled in place: its C_nwvec call for
vec=True, its C_nwalign for vec=False)."""
import numpy as np

SCORES = (5, -4, -8)          # getDadaOpt("MATCH" / "MISMATCH" / "GAP_PENALTY"): what nwhamming aligns with


def _rnd(rng, n, letters="ACGT"):
    return "".join(letters[int(x)] for x in rng.integers(0, len(letters), size=n))


def _flip(s, p):
    return s[:p] + "ACGT"[("ACGT".index(s[p]) + 1) % 4] + s[p + 1:]


# ---- nwhamming over a checker ---------------------------------------------------------------------------------------------------
def nweval(checker, s1, s2, vec=True, band=-1, scores=SCORES):
    """nweval(s1, s2, vec=, band=) (R/misc.R:222): (match, mismatch, indel) of the checker's alignment."""
    if vec and hasattr(checker, "nwvec_raw"):
        al = checker.nwvec_raw(s1, s2, scores[0], scores[1], scores[2], band, True)
    else:
        al = checker.C_nwalign(s1, s2, scores[0], scores[1], scores[2], None, band, True)
    return checker.eval_pair(al[0], al[1])


def nwhamming(checker, s1, s2, vec=True, band=-1, scores=SCORES):
    ev = nweval(checker, s1, s2, vec, band, scores)
    return ev[1] + ev[2]


def screen(query, ref, min_overlap):
    """The prescreen of multiSample.R:127-131 as two bits: 1 = substr(query, 1, minOverlap) occurs in ref, 2 = the reverse."""
    return (1 if query[:min_overlap] in ref else 0) | (2 if ref[:min_overlap] in query else 0)


# ---- the loop -------------------------------------------------------------------------------------------------------------------
def _order(mat, order_by):
    if order_by is None:
        return np.arange(mat.shape[1])
    key = mat.sum(axis=0, dtype=np.int64) if order_by == "abundance" else (mat > 0).sum(axis=0)
    return np.argsort(-key, kind="stable")          # order(..., decreasing=TRUE) is the stable radix order


def restate(mat, seqs, checker, min_overlap=20, order_by="abundance", identical_only=False, vec=True, band=-1, trace=None):
    """collapseNoMismatch(seqtab, minOverlap, orderBy, identicalOnly, vec, band): (mat [samples, sequences] int64, seqs).
    `trace` (a dict) receives what the tests look at: `queries` (the de-duplicated sequences in processing order), `kept` (in
    kept order), `joined` {query: ref}, `tried` {query: [(ref, hamming)] in the order the loop called nwhamming}, `ncol`."""
    mat = np.asarray(mat, dtype=np.int64)
    # duplicates are folded into their first occurrence (:105-114)
    first = {}
    for i, s in enumerate(seqs):
        first.setdefault(s, i)
    names = [s for i, s in enumerate(seqs) if first[s] == i]
    pos = {s: k for k, s in enumerate(names)}
    st = np.zeros((mat.shape[0], len(names)), dtype=np.int64)
    for i, s in enumerate(seqs):
        st[:, pos[s]] += mat[:, i]
    if trace is not None:
        trace.update(ncol=len(names), queries=[], kept=[], joined={}, tried={})
    if identical_only:
        return st, names
    # sort(getUniques(seqtab), decreasing=TRUE) (:118)
    queries = [names[int(k)] for k in np.argsort(-st.sum(axis=0), kind="stable")]
    kept = []
    collapsed = np.zeros_like(st)
    joined, tried = {}, {}
    for query in queries:
        added = False
        tried[query] = []
        for ref in kept:
            if screen(query, ref, min_overlap):
                h = nwhamming(checker, query, ref, vec, band)
                tried[query].append((ref, h))
                if h == 0:
                    collapsed[:, pos[ref]] += st[:, pos[query]]
                    joined[query] = ref
                    added = True
                    break
        if not added:
            collapsed[:, pos[query]] = st[:, pos[query]]
            kept.append(query)
    in_out = set(kept)
    cols = [k for k, s in enumerate(names) if s in in_out]           # input order, modulo the removed columns (:145)
    out, out_names = collapsed[:, cols], [names[k] for k in cols]
    for ob in (order_by, "abundance"):                               # (:148-156: orderBy, then unconditionally by abundance)
        o = _order(out, ob)
        out, out_names = out[:, o], [out_names[int(k)] for k in o]
    if trace is not None:
        trace.update(queries=queries, kept=kept, joined=joined, tried=tried)
    return out, out_names


def batch_view(trace, min_overlap, batch):
    """What a run in batches of `batch` queries sees, from a trace of `restate`: `screened` = the (query, ref) pairs that pass the
    screen with ref kept before the query's batch or anywhere earlier in it (the pairs that reach nwhamming or would have),
    `own_batch` = the queries whose ref sits earlier in their own batch, `skipped` = the (query, member) pairs where an earlier
    member of the query's batch passes the screen but had itself collapsed."""
    queries, joined = trace["queries"], trace["joined"]
    at = {q: p for p, q in enumerate(queries)}
    screened, own_batch, skipped = 0, [], []
    for b0 in range(0, len(queries), batch):
        members = queries[b0: b0 + batch]
        before = [r for r in queries[:b0] if r not in joined]
        for k, q in enumerate(members):
            for r in before + members[:k]:
                if screen(q, r, min_overlap):
                    screened += 1
                    if at[r] >= b0 and r in joined:
                        skipped.append((q, r))
            if q in joined and at[joined[q]] >= b0:
                own_batch.append(q)
    return dict(screened=screened, own_batch=own_batch, skipped=skipped)


def checker_for(cport, ref=None):
    """oracle.ref where it is built, else oracle.cport."""
    return ref if (ref is not None and ref.available()) else cport


# ---- what k_collapse_scan computes, by brute force ----------------------------------------------------------------------------------
def brute_pair(q, r, min_overlap, match=SCORES[0], mismatch=SCORES[1]):
    """(screen, G, m_max, decision): every gapless diagonal with a non-empty overlap, m its length and mm its mismatches;
    G = max match (m - mm) + mismatch mm, m_max = the longest overlap with mm == 0 (0 if none); decision 0 screened out,
    1 rejected by the bound G > match m_max, 2 needs the alignment."""
    a = np.frombuffer(q.encode(), dtype=np.uint8)
    b = np.frombuffer(r.encode(), dtype=np.uint8)
    lq, lr = len(a), len(b)
    eq = (a[:, None] == b[None, :])
    diag = (np.arange(lq)[:, None] - np.arange(lr)[None, :] + lr - 1).ravel()      # i - j + lr - 1 in [0, lq + lr - 1)
    hits = np.bincount(diag, weights=eq.ravel(), minlength=lq + lr - 1).astype(np.int64)
    m = np.bincount(diag, minlength=lq + lr - 1).astype(np.int64)
    mm = m - hits
    g = int((match * hits + mismatch * mm).max())
    exact = m[mm == 0]
    m_max = int(exact.max()) if exact.size else 0
    sc = screen(q, r, min_overlap)
    return sc, g, m_max, (0 if sc == 0 else (1 if g > match * m_max else 2))


# ---- tables ---------------------------------------------------------------------------------------------------------------------
TABLE_SEED = 7


def make_table(seed=TABLE_SEED, nroots=40, nsamples=3):
    """40 roots of 60-120 nt with seven variants each - end trimmed, start trimmed, extended at the start, extended at the end,
    one mismatch past position 25, one interior deletion, a piece of 8-18 nt -, shuffled, over 3 samples, abundances small
    enough to tie.  Returns (mat int32 [samples, columns], seqs), the columns distinct."""
    rng = np.random.default_rng(seed)
    seqs = []
    for _ in range(nroots):
        root = _rnd(rng, int(rng.integers(60, 121)))
        n = len(root)
        p = int(rng.integers(26, n - 5))
        d = int(rng.integers(10, n - 10))
        a = int(rng.integers(0, n - 18))
        seqs += [root, root[: n - int(rng.integers(1, 12))], root[int(rng.integers(1, 12)):], _rnd(rng, int(rng.integers(1, 9))) + root,
                 root + _rnd(rng, int(rng.integers(1, 9))), _flip(root, p), root[:d] + root[d + 1:], root[a: a + int(rng.integers(8, 19))]]
    seqs = list(dict.fromkeys(seqs))
    seqs = [seqs[int(k)] for k in rng.permutation(len(seqs))]
    mat = rng.integers(0, 6, size=(nsamples, len(seqs)))
    mat[0, mat.sum(axis=0) == 0] = 1
    return mat.astype(np.int32), seqs


def table_fact(mat, seqs, checker, min_overlap=20):
    """The regimes the generated table exists for, on the restatement's own run: pairs that pass the screen (>= 100) and pairs
    among them that do not collapse, queries that collapse into a later ref after failing an earlier one, and kept pairs that
    nwhamming would join but the screen keeps apart - at least 10 of each.  Returns the counts."""
    tr = {}
    out, names = restate(mat, seqs, checker, min_overlap, trace=tr)
    tried = [t for q in tr["queries"] for t in tr["tried"][q]]
    failed = [t for t in tried if t[1] != 0]
    later = [q for q in tr["joined"] if len(tr["tried"][q]) > 1]
    kept = tr["kept"]
    apart = sum(1 for i, q in enumerate(kept) for r in kept[:i] if not screen(q, r, min_overlap) and nwhamming(checker, q, r) == 0)
    counts = dict(columns=len(seqs), kept=len(kept), screened=len(tried), failed=len(failed), later_ref=len(later), apart=apart)
    assert len(tried) >= 100 and len(failed) >= 10 and len(later) >= 10 and apart >= 10, counts
    assert len(kept) == len(names) < len(seqs)
    return counts


def with_duplicates(mat, seqs, seed=11, ndup=25):
    """The table with `ndup` of its columns a second time under the same name (other counts), the columns shuffled again."""
    rng = np.random.default_rng(seed)
    mat, seqs = np.asarray(mat), list(seqs)
    dup = rng.choice(len(seqs), size=ndup, replace=False)
    mat = np.concatenate([mat, rng.integers(0, 6, size=(mat.shape[0], ndup))], axis=1)
    seqs = seqs + [seqs[int(k)] for k in dup]
    o = rng.permutation(len(seqs))
    return mat[:, o].astype(np.int32), [seqs[int(k)] for k in o]


def low_complexity_table(seed=5, ncol=200):
    """200 columns over {A, C}, 8-40 nt: with min_overlap 4 nearly every pair passes the screen and the alignments tie."""
    rng = np.random.default_rng(seed)
    seqs = []
    while len(seqs) < ncol:
        s = _rnd(rng, int(rng.integers(8, 41)), "AC")
        if s not in seqs:
            seqs.append(s)
    mat = rng.integers(0, 5, size=(2, ncol))
    mat[0, mat.sum(axis=0) == 0] = 1
    return mat.astype(np.int32), seqs


def many_pairs_table(seed=3, nroots=3, rootlen=80, ncol=1600, minlen=30):
    """1 600 pieces of three roots of 80 nt (every piece at least 30 nt): pieces of one root that overlap where they lie in it
    align without a mismatch, so the screened pairs survive the bound and, with all 1 600 in one batch, well over 100 000 of them go
    to the aligner (one aligner call takes at most 65 536; the restatement itself needs 1 600 alignments: nearly every piece
    joins the first kept piece of its root)."""
    rng = np.random.default_rng(seed)
    roots = [_rnd(rng, rootlen) for _ in range(nroots)]
    pieces = [root[a: b] for root in roots for a in range(rootlen) for b in range(a + minlen, rootlen + 1)]
    pieces = list(dict.fromkeys(pieces))
    seqs = [pieces[int(k)] for k in rng.permutation(len(pieces))[:ncol]]
    mat = rng.integers(1, 40, size=(2, len(seqs)))
    return mat.astype(np.int32), seqs


# ---- pairs whose lengths straddle the 2-bit word boundaries ------------------------------------------------------------------------
BOUNDARY_LENGTHS = (1, 2, 31, 32, 33, 63, 64, 65, 250, 251, 256, 257, 600)
BOUNDARY_MIN_OVERLAPS = (1, 8, 20, 32, 33, 50, 700)


def boundary_pairs(seed=17):
    """Every length against every length, four contents each: a copy (common start), a copy shifted by three, the shorter a piece
    from the middle of the longer, a copy with one base changed."""
    rng = np.random.default_rng(seed)
    qs, rs = [], []
    for lq in BOUNDARY_LENGTHS:
        for lr in BOUNDARY_LENGTHS:
            base = _rnd(rng, max(lq, lr) + 3)
            q = base[:lq]
            lo, hi = min(lq, lr), max(lq, lr)
            long_ = base[:hi]
            piece = long_[(hi - lo) // 2: (hi - lo) // 2 + lo]
            for r in (base[:lr], base[3: 3 + lr], None, _flip(base[:lr], min(lq, lr) // 2)):
                if r is None:
                    qs.append(long_ if lq >= lr else piece)
                    rs.append(piece if lq >= lr else long_)
                else:
                    qs.append(q)
                    rs.append(r)
    return qs, rs


# ---- the pair-level sweep (tests/golden/collapse_pairs.npz is made from it) -----------------------------------------------------------
def sweep_pairs(seed=2024, n=6000):
    """Random pairs of 4-40 nt over {A, C} and {A, C, G, T}: unrelated, a piece of the other, a shifted copy, a copy with a base
    changed - with min_overlap 4, 8 or 20.  Returns (queries, refs, min_overlaps)."""
    rng = np.random.default_rng(seed)
    qs, rs, mo = [], [], []
    while len(qs) < n:
        letters = "AC" if len(qs) % 2 else "ACGT"
        a = _rnd(rng, int(rng.integers(4, 41)), letters)
        kind = int(rng.integers(0, 5)) if rng.integers(0, 2) else 0          # (half of the pairs unrelated: where the ties are)
        if kind == 0:
            b = _rnd(rng, int(rng.integers(4, 41)), letters)
        elif kind == 1:
            i = int(rng.integers(0, len(a) - 3))
            b = a[i: i + int(rng.integers(4, len(a) - i + 1))]
        elif kind == 2:
            k = int(rng.integers(1, 6))
            b = (a[k:] + _rnd(rng, k, letters))[: 40]
            b = b if len(b) >= 4 else a
        elif kind == 3:
            b = _flip(a, int(rng.integers(0, len(a))))
            if letters == "AC":
                b = b.replace("G", "A").replace("T", "C")
        else:
            b = (_rnd(rng, int(rng.integers(0, 5)), letters) + a[: int(rng.integers(4, len(a) + 1))])[: 40]
        if rng.integers(0, 2):
            a, b = b, a
        if a == b:
            continue
        qs.append(a); rs.append(b); mo.append((4, 8, 20)[len(qs) % 3])
    return qs, rs, mo


# ---- running the product against the above ------------------------------------------------------------------------------------------
_GOLDEN = {}


def golden():
    """tests/golden/collapse_pairs.npz, loaded once."""
    if not _GOLDEN:
        import os
        with np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "collapse_pairs.npz")) as z:
            _GOLDEN.update({k: z[k] for k in z.files})
    return _GOLDEN


def device_collapse(api, mat, seqs, env=None, **kw):
    """api.collapse_no_mismatch under the DADA2HIP_COLLAPSE_* settings of `env` (the library re-reads its environment at every
    boundary call): (mat, seqs, stats)."""
    import os
    env = {k: str(v) for k, v in (env or {}).items()}
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        st = {}
        m, names = api.collapse_no_mismatch(mat, seqs, stats=st, **kw)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    return m, names, st


def assert_same_table(got, want, what=""):
    gm, gn = got[0], got[1]
    wm, wn = want
    assert list(gn) == list(wn), (what, len(gn), len(wn), [k for k, (a, b) in enumerate(zip(gn, wn)) if a != b][:5])
    assert np.array_equal(np.asarray(gm, dtype=np.int64), np.asarray(wm, dtype=np.int64)), what


def check_pairs(api, idx):
    """api.collapse_pairs on the fixture's pairs `idx` (one call per min_overlap) against the fixture's brute-force scan."""
    g = golden()
    idx = np.asarray(idx)
    for mo in sorted(set(int(x) for x in g["min_overlap"][idx])):
        sel = idx[g["min_overlap"][idx] == mo]
        got = api.collapse_pairs([str(x) for x in g["queries"][sel]], [str(x) for x in g["refs"][sel]], min_overlap=mo)
        bad = np.flatnonzero((got != g["scan"][sel]).any(axis=1))
        assert bad.size == 0, (mo, int(sel[bad[0]]), str(g["queries"][sel[bad[0]]]), str(g["refs"][sel[bad[0]]]), got[bad[0]].tolist(),
                               g["scan"][sel[bad[0]]].tolist())
    return len(idx)


STRIDED_PAIRS = 2 * 16384 + 1                # k_collapse_scan's grid is capped at 16 384 blocks: every block a second pair, block 0 a third


def strided_pairs():
    """The fixture's pairs of its most frequent min_overlap, repeated to 32 769 and turned by one: (indices into the fixture,
    min_overlap).  Pair i and pair i + 16 384, which one block takes one after the other, are different pairs."""
    g = golden()
    vals, cnt = np.unique(g["min_overlap"], return_counts=True)
    mo = int(vals[np.argmax(cnt)])
    sel = np.flatnonzero(g["min_overlap"] == mo)
    idx = np.roll(np.resize(sel, STRIDED_PAIRS), 1)
    assert (idx[16384:] != idx[:-16384]).all() and (idx[1:] != idx[:-1]).all()
    return idx, mo


def check_strided_pairs(api):
    """One dada2hip_collapse_pairs call of 32 769 pairs against the fixture's brute-force scan, as check_pairs."""
    g = golden()
    idx, mo = strided_pairs()
    got = api.collapse_pairs([str(x) for x in g["queries"][idx]], [str(x) for x in g["refs"][idx]], min_overlap=mo)
    want = g["scan"][idx]
    assert len({tuple(r) for r in want[:, [0, 3]].tolist()}) >= 4          # screened out, rejected by the bound, to the aligner; both screen bits
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, (mo, "first at pair", int(bad[0]), "of", int(bad.size), str(g["queries"][idx[bad[0]]]), str(g["refs"][idx[bad[0]]]),
                           got[bad[0]].tolist(), want[bad[0]].tolist())
    return len(idx)


def emu_run():
    """The emulator's job (tests/test_emu_collapse.py): collapse_pairs on 300 fixture pairs, the whole function on a 60-column
    cut of the generated table in batches of 8 against the restatement, nweval on 50 pairs."""
    from dada2_amd import api
    from oracle import cport
    g = golden()
    n = check_pairs(api, np.arange(0, 6000, 20))
    mat, seqs = make_table()
    mat, seqs = mat[:, :60], seqs[:60]
    tr = {}
    want = restate(mat, seqs, cport, trace=tr)
    got = device_collapse(api, mat, seqs, env={"DADA2HIP_COLLAPSE_BATCH": 8})
    assert_same_table(got, want, "60 columns, batch 8")
    st = got[2]
    assert st["batches"] == 8 and st["pairs_scanned"] - st["pairs_screened_out"] == batch_view(tr, 20, 8)["screened"], st
    assert len(want[1]) < 60, "nothing collapsed"
    sel = np.arange(7, 6000, 120)
    qs, rs = [str(x) for x in g["queries"][sel]], [str(x) for x in g["refs"][sel]]
    ev = api.nweval(qs, rs, vec=True)
    assert np.array_equal(ev, g["ev_vec"][sel]), np.flatnonzero((ev != g["ev_vec"][sel]).any(axis=1))
    assert np.array_equal(api.nwhamming(qs, rs), g["ev_plain"][sel][:, 1] + g["ev_plain"][sel][:, 2])
    assert api.nwhamming(qs[0], rs[0]) == int(ev[0, 1] + ev[0, 2]) and api.nweval(qs[0], rs[0]).shape == (3,)
    return "ok pairs %d columns 60 -> %d aligned %d nweval %d" % (n, len(want[1]), st["pairs_aligned"], len(qs))


def ring_run(api, checker):
    """The low-complexity table (200 columns over {A, C}, min_overlap 4: the screen passes nearly every pair and the bound
    settles few) in ONE batch under a scratch ring of four waves (DADA2HIP_NW_RING=4): the pairs left to the aligner go out in one
    call of the pair-form lane kernel - more than 512, so its waves wrap their slots - and the table equals the restatement's;
    with the knob unset the same `into` in one trip.  Returns the number of aligned pairs."""
    import aligner_cases as A
    mat, seqs = low_complexity_table()
    exp = restate(mat, seqs, checker, min_overlap=4)
    with A.ring(A.RING_WAVES):
        got = device_collapse(api, mat, seqs, min_overlap=4)
        trips = A.read_ring_trips()
    assert_same_table(got, exp, "low complexity, ring of 4 waves")
    st = got[2]
    assert st["batches"] == 1 and A.RING_MIN_WORK <= st["pairs_aligned"] <= 65536, st
    assert trips == -(-(-(-st["pairs_aligned"] // 64)) // A.RING_WAVES) >= 3, (trips, st["pairs_aligned"], "DADA2HIP_NW_RING ignored?")
    with A.ring(None):
        plain = device_collapse(api, mat, seqs, min_overlap=4)
        assert A.read_ring_trips() == 1
    assert_same_table(plain, exp, "low complexity")
    assert np.array_equal(plain[2]["into"], st["into"]) and plain[2]["pairs_aligned"] == st["pairs_aligned"]
    return st["pairs_aligned"]
