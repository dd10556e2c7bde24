"""assignTaxonomy (src/taxonomy.cpp): the cases of tests/golden/taxonomy.npz, a numpy restatement of the classifier, and the
criteria the device path is held to (tests/test_taxonomy.py, test_emu_taxonomy.py, test_gpu_taxonomy.py).

The restatement adds in float32, one term after the other in the reference's order (numpy's float32 add is IEEE single), over a
table whose logarithm is libm's logf through ctypes - numpy.log on float32 is another function - so its sums are the reference's
bits; what it returns per (query, pass) is the maximum and the SET of genera at it.  The reference breaks ties inside that set
with a std::random_device-seeded engine, so two of its runs differ: the relation to a recorded run is membership, and equality
where the set has one member.

A case is one model and one call: refs, ref_to_genus (0-based), genusmat, seqs, try_rc and the seed of its uniforms.  The
uniforms are unif_buffer(seed, n), the documented generator of include/dada2hip.h restated here (the fixture keeps the seed: the
1 500-nt case alone draws 111 600 doubles)."""
import ctypes
import ctypes.util
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "taxonomy.npz")
EXAMPLE_TRAIN = os.path.join(HERE, "golden", "example_train_set.fa.gz")
EXAMPLE_SEQS = os.path.join(HERE, "golden", "example_seqs.fa")
NKMER, NBOOT, NPASS = 65536, 100, 101
TIE_CAP = 0.10                       # of the cases compared, at most this share of (query, pass) entries may be tied
TIES_ARE_THE_POINT = ("twins", "broken_by_N")

_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.logf.restype = ctypes.c_float
_libm.logf.argtypes = [ctypes.c_float]


def logf(x):
    """libm's logf, elementwise on a float32 array (through its distinct values)."""
    x = np.asarray(x, dtype=np.float32)
    u, inv = np.unique(x.ravel(), return_inverse=True)
    lu = np.array([_libm.logf(float(v)) for v in u], dtype=np.float32)
    return lu[inv].reshape(x.shape)


_CODE = {"A": 0, "C": 1, "G": 2, "T": 3}
_COMP = str.maketrans("ACGTN", "TGCAN")


def rc(s):
    return s.translate(_COMP)[::-1]


def kmers(seq):
    """The valid 8-mer indices of seq in sequence order (tax_kmer: first base most significant; a k-mer with another letter in it is skipped)."""
    out = []
    for i in range(len(seq) - 7):
        k = 0
        for c in seq[i: i + 8]:
            v = _CODE.get(c)
            if v is None:
                k = -1
                break
            k = 4 * k + v
        if k >= 0:
            out.append(k)
    return out


def train_table(refs, ref_to_genus, ngenus):
    """taxonomy.cpp:226-270: float32 [ngenus, 65536]."""
    nref = len(refs)
    cnt = np.zeros((ngenus, NKMER), dtype=np.float32)
    total = np.zeros(NKMER, dtype=np.float32)
    mg1 = np.ones(ngenus, dtype=np.float32)
    for r, g in zip(refs, ref_to_genus):
        ks = np.unique(np.array(kmers(r), dtype=np.int64))
        cnt[g, ks] += np.float32(1)
        total[ks] += np.float32(1)
        mg1[g] += np.float32(1)
    prior = ((total.astype(np.float64) + 0.5) / (1.0 + nref)).astype(np.float32)
    return logf((cnt + prior[None, :]) / mg1[:, None])


def unif_buffer(seed, n):
    """Value i: splitmix64 of seed + (i + 1) * 0x9E3779B97F4A7C15, top 53 bits / 2^53."""
    with np.errstate(over="ignore"):
        z = np.uint64(seed) + (np.arange(n, dtype=np.uint64) + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z ^= z >> np.uint64(31)
    return (z >> np.uint64(11)).astype(np.float64) / 9007199254740992.0


def n_unifs(seqs):
    return len(seqs) * NBOOT * (max(max(len(s) for s in seqs) - 7, 0) // 8)


def _pass_sum(table, ks):
    s = np.zeros(table.shape[0], dtype=np.float32)
    for k in ks:
        s = s + table[:, k]                                     # float32, one term after the other
    return s


def restate(table, seqs, unifs, try_rc=False, trace=None):
    """Per (query, pass): best float32 [n, 101], tied bool [n, 101, ngenus] (all False for a query under 50 nt).  trace (a dict)
    receives "flipped": the queries whose reverse complement was taken."""
    flipped = []
    n, ng = len(seqs), table.shape[0]
    best = np.zeros((n, NPASS), dtype=np.float32)
    tied = np.zeros((n, NPASS, ng), dtype=bool)
    stride = max(max(len(s) for s in seqs) - 7, 0)
    for j, s in enumerate(seqs):
        if len(s) < 50:
            continue
        ka = sorted(kmers(s))
        full = _pass_sum(table, ka)
        if try_rc:
            ka_rc = sorted(kmers(rc(s)))
            full_rc = _pass_sum(table, ka_rc)
            if full_rc.max() > full.max():                       # taxonomy.cpp:173, as floats
                ka, full = ka_rc, full_rc
                flipped.append(j)
        sums = [full]
        A = len(ka)
        u = unifs[j * stride: j * stride + NBOOT * (A // 8)]
        for r in range(NBOOT):
            draws = [ka[int(A * x)] for x in u[r * (A // 8): (r + 1) * (A // 8)]]
            sums.append(_pass_sum(table, draws))
        for p, v in enumerate(sums):
            best[j, p] = v.max()
            tied[j, p] = v == v.max()
    if trace is not None:
        trace["flipped"] = flipped
    return best, tied


def boot_counts(tax, boot_tax, genusmat):
    """taxonomy.cpp:189-195 from a call's own picks."""
    n, nl = len(tax), genusmat.shape[1]
    boot = np.zeros((n, nl), dtype=np.int32)
    for j in range(n):
        if tax[j] < 0:
            continue
        for g in boot_tax[j]:
            for l in range(nl):
                if genusmat[g, l] != genusmat[tax[j], l]:
                    break
                boot[j, l] += 1
    return boot


# ---- the cases ------------------------------------------------------------------------------------------------------------------------
def _mutate(rng, s, rate):
    a = list(s)
    for i in range(len(a)):
        if rng.random_sample() < rate:
            a[i] = "ACGT"[rng.randint(4)]
    return "".join(a)


def _rand(rng, n):
    return "".join("ACGT"[i] for i in rng.randint(0, 4, n))


def _synthetic_model(rng, ngenus, reflen, nfam=4):
    """ngenus genera in nfam families of three levels; one to three references per genus, mutated copies of the genus's ancestor."""
    refs, r2g = [], []
    for g in range(ngenus):
        anc = _rand(rng, reflen)
        for _ in range(1 + g % 3):
            refs.append(_mutate(rng, anc, 0.02))
            r2g.append(g)
    genusmat = np.array([[0, g % nfam, g] for g in range(ngenus)], dtype=np.int32)
    return refs, np.array(r2g, dtype=np.int32), genusmat


def _queries(rng, refs, lengths, rate=0.03):
    out = []
    for L in lengths:
        r = refs[rng.randint(len(refs))]
        o = rng.randint(0, len(r) - L + 1)
        out.append(_mutate(rng, r[o: o + L], rate))
    return out


def build_cases():
    """name -> dict(refs, ref_to_genus, genusmat, seqs, try_rc, seed).  The generator's input; the tests read the fixture."""
    from dada2_amd import api
    cases = {}
    ids, seqs = api.read_fasta(EXAMPLE_TRAIN)
    refs, _, r2g, gm = api.taxonomy_reference(seqs, ids)
    cases["example"] = dict(refs=refs, ref_to_genus=r2g, genusmat=gm, seqs=api.read_fasta(EXAMPLE_SEQS)[1], try_rc=False, seed=1)
    for ng in (1, 63, 64, 65, 129):                              # tiles of 64 genera: one short, one full, one over, three
        rng = np.random.RandomState(100 + ng)
        refs, r2g, gm = _synthetic_model(rng, ng, 160)
        cases["ngenus%d" % ng] = dict(refs=refs, ref_to_genus=r2g, genusmat=gm, seqs=_queries(rng, refs, [60, 72, 90, 64, 120, 81, 57, 100]),
                                      try_rc=False, seed=200 + ng)
    rng = np.random.RandomState(7)                               # genera 3 and 70 (two tiles) with the same references
    refs, r2g, gm = _synthetic_model(rng, 80, 160)
    twin = [r for r, g in zip(refs, r2g) if g == 3]
    refs = [r for r, g in zip(refs, r2g) if g != 70] + twin
    r2g = np.array([g for g in r2g if g != 70] + [70] * len(twin), dtype=np.int32)
    cases["twins"] = dict(refs=refs, ref_to_genus=r2g, genusmat=gm, seqs=_queries(rng, twin, [80, 96, 70]) + _queries(rng, refs, [75]),
                          try_rc=False, seed=8)
    rng = np.random.RandomState(11)                              # lengths mixed in one call: the stride is the 1 500-nt query's
    refs, r2g, gm = _synthetic_model(rng, 20, 1600)
    cases["lengths"] = dict(refs=refs, ref_to_genus=r2g, genusmat=gm, seqs=_queries(rng, refs, [49, 50, 57, 201, 1500, 80]), try_rc=False, seed=12)
    cases["len57"] = dict(refs=refs, ref_to_genus=r2g, genusmat=gm, seqs=_queries(rng, refs, [57, 57, 57, 57]), try_rc=False, seed=13)
    q = list(_queries(rng, refs, [60], rate=0.0)[0])             # 53 k-mers, all but 5 broken: clean bases 0..11, then an N every 8th
    for i in range(12, 60, 8):
        q[i] = "N"
    cases["broken_by_N"] = dict(refs=refs, ref_to_genus=r2g, genusmat=gm, seqs=["".join(q)], try_rc=False, seed=14)
    rng = np.random.RandomState(17)
    refs, r2g, gm = _synthetic_model(rng, 70, 200)
    qs = _queries(rng, refs, [90, 64, 120, 75, 100, 66, 150, 83])
    cases["try_rc"] = dict(refs=refs, ref_to_genus=r2g, genusmat=gm, seqs=[rc(s) if i % 2 else s for i, s in enumerate(qs)], try_rc=True, seed=18)
    return cases


CASE_NAMES = ("example", "ngenus1", "ngenus63", "ngenus64", "ngenus65", "ngenus129", "twins", "lengths", "len57", "broken_by_N", "try_rc")
_G = {}


def golden():
    if "g" not in _G:
        _G["g"] = np.load(GOLDEN, allow_pickle=False)
    return _G["g"]


def load_case(name):
    g = golden()
    c = dict(refs=[str(x) for x in g[name + "/refs"]], ref_to_genus=g[name + "/ref_to_genus"], genusmat=g[name + "/genusmat"],
             seqs=[str(x) for x in g[name + "/seqs"]], try_rc=bool(g[name + "/try_rc"]), seed=int(g[name + "/seed"]),
             ref_runs=[{k: g["%s/run%d_%s" % (name, r, k)] for k in ("tax", "boot", "boot_tax")} for r in (0, 1)])
    c["unifs"] = unif_buffer(c["seed"], n_unifs(c["seqs"]))
    return c


_RESTATED = {}


def restated(name):
    """(table, best, tied) of a case, computed once per process."""
    if name not in _RESTATED:
        c = load_case(name)
        table = train_table(c["refs"], c["ref_to_genus"], c["genusmat"].shape[0])
        tr = {}
        _RESTATED[name] = (table,) + restate(table, c["seqs"], c["unifs"], c["try_rc"], trace=tr) + (tr["flipped"],)
    return _RESTATED[name][:3]


def restated_flips(name):
    restated(name)
    return _RESTATED[name][3]


def picks(run):
    """[n, 101] genus per (query, pass) of a result."""
    return np.concatenate([np.asarray(run["tax"])[:, None], np.asarray(run["boot_tax"])], axis=1)


def assert_picks_in_tie_sets(pk, tied, what):
    """Every pick a member of its tie set (so equal to the unique maximum where the set has one member); -1 exactly where no pass ran."""
    ran = tied.any(axis=2)
    assert np.array_equal(pk >= 0, ran), (what, "NA pattern")
    j, p = np.nonzero(ran)
    ok = tied[j, p, pk[j, p]]
    assert ok.all(), (what, [(int(a), int(b), int(pk[a, b])) for a, b in zip(j[~ok][:5], p[~ok][:5])])


# ---- the device path ------------------------------------------------------------------------------------------------------------------
def with_env(env, f):
    env = {k: str(v) for k, v in (env or {}).items()}
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return f()
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def device_model(api, name):
    """The case's model on the device (the fixture holds the parsed reference: trained from it directly)."""
    c = load_case(name)
    ng = c["genusmat"].shape[0]
    return api.TaxonomyModel.from_parsed(c["refs"], ["g%d;" % k for k in range(ng)], c["ref_to_genus"], c["genusmat"])


def check_case(api, name, slab_settings=(None, 0)):
    """The criteria of the device path on one case; returns (entries, tied entries).  slab_settings: values of DADA2HIP_TAX_SLAB
    to run under (None = the default); their outputs must be identical."""
    c = load_case(name)
    table, best, tied = restated(name)
    want_ntie = tied.sum(axis=2).astype(np.int32)
    with device_model(api, name) as m:
        assert np.array_equal(m.table().view(np.uint32), table.view(np.uint32)), (name, "the model table is not bit-equal")
        runs, stats = [], []
        for slab in slab_settings:
            st = {}
            env = {} if slab is None else {"DADA2HIP_TAX_SLAB": slab}
            runs.append(with_env(env, lambda: api.assign_taxonomy_raw(c["seqs"], m, try_rc=c["try_rc"], seed=c["seed"], unifs=c["unifs"], stats=st)))
            stats.append(st)
        again = api.assign_taxonomy_raw(c["seqs"], m, try_rc=c["try_rc"], seed=c["seed"], unifs=c["unifs"])
        seeded = api.assign_taxonomy_raw(c["seqs"], m, try_rc=c["try_rc"], seed=c["seed"])          # unifs drawn by the library
        other = api.assign_taxonomy_raw(c["seqs"], m, try_rc=c["try_rc"], seed=c["seed"] + 12345, unifs=c["unifs"])
    got = runs[0]
    assert np.array_equal(got["ntie"], want_ntie), (name, "ntie", np.argwhere(got["ntie"] != want_ntie)[:5].tolist())
    pk = picks(got)
    assert_picks_in_tie_sets(pk, tied, name)
    assert np.array_equal(got["boot"], boot_counts(got["tax"], got["boot_tax"], c["genusmat"])), (name, "boot")
    for r, st in zip(runs[1:], stats[1:]):                       # the instances agree
        for k in ("tax", "boot", "boot_tax", "ntie"):
            assert np.array_equal(r[k], got[k]), (name, "instances differ in", k)
    classified = sum(1 for s in c["seqs"] if len(s) >= 50)
    for slab, st in zip(slab_settings, stats):
        assert st["classified"] == classified and st["slab_queries"] + st["gather_queries"] == classified, (name, st)
        assert st["took_reverse_complement"] == len(restated_flips(name)), (name, st)
        if slab == 0:
            assert st["slab_queries"] == 0, (name, st)
    for k in ("tax", "boot", "boot_tax", "ntie"):                # one seed, one answer; the library's own draws are the documented ones
        assert np.array_equal(again[k], got[k]), (name, "two calls differ in", k)
        assert np.array_equal(seeded[k], got[k]), (name, "unifs = NULL differs in", k)
    assert np.array_equal(other["ntie"], got["ntie"]), (name, "ntie depends on the seed")
    diff = picks(other) != pk                                    # another seed: other winners only where there is a tie
    assert not (diff & (want_ntie <= 1)).any(), (name, "the seed changed an untied entry")
    assert_picks_in_tie_sets(picks(other), tied, name + " (other seed)")
    ran = tied.any(axis=2)
    return int(ran.sum()), int((want_ntie > 1).sum()), got, stats


CHUNKED = ("ngenus129", "lengths", "try_rc")                     # three tiles; the slab and the gather instance in one call; tryRC's two passes
TAX_CHUNKS = (1, 3)


def expected_launches(st, try_rc, chunk=None):
    """Two launches (sums, combine) per chunk of every pass over a non-empty list: tryRC's two passes over all classified queries,
    then the gather and the slab instance over theirs."""
    def chunks(n):
        return 0 if n == 0 else (1 if chunk is None else -(-n // chunk))
    return 2 * ((2 * chunks(st["classified"]) if try_rc else 0) + chunks(st["slab_queries"]) + chunks(st["gather_queries"]))


def check_chunks(api, name, chunks=TAX_CHUNKS):
    """check_case under DADA2HIP_TAX_CHUNK = 1, 3 and unset: the criteria hold under each, the outputs are identical, and the
    chunks happened (the queries of a later chunk land at their own offset; the buffers are used again).  Returns the unset run's
    check_case result."""
    c = load_case(name)
    base = check_case(api, name)
    for st in base[3]:
        assert st["launches"] == expected_launches(st, c["try_rc"]), (name, st)
    for chunk in chunks:
        e, t, got, stats = with_env({"DADA2HIP_TAX_CHUNK": chunk}, lambda: check_case(api, name))
        for k in ("tax", "boot", "boot_tax", "ntie"):
            assert np.array_equal(got[k], base[2][k]), (name, "chunks of", chunk, "differ in", k)
        for st, st0 in zip(stats, base[3]):
            assert {k: st[k] for k in TAXONOMY_COUNTS} == {k: st0[k] for k in TAXONOMY_COUNTS}, (name, chunk, st, st0)
            assert st["launches"] == expected_launches(st, c["try_rc"], chunk) > st0["launches"], (name, chunk, st, st0)
    # a value past the automatic one is the automatic one; one below 1 is 1
    for val, chunk in ((10**9, None), (0, 1)):
        st = {}
        with device_model(api, name) as m:
            got = with_env({"DADA2HIP_TAX_CHUNK": val},
                           lambda: api.assign_taxonomy_raw(c["seqs"], m, try_rc=c["try_rc"], seed=c["seed"], unifs=c["unifs"], stats=st))
        assert st["launches"] == expected_launches(st, c["try_rc"], chunk), (name, val, st)
        for k in ("tax", "boot", "boot_tax", "ntie"):
            assert np.array_equal(got[k], base[2][k]), (name, "DADA2HIP_TAX_CHUNK", val, k)
    return base


TAXONOMY_COUNTS = ("classified", "slab_queries", "gather_queries", "took_reverse_complement")


def emu_run():
    """The emulator's job (tests/test_emu_taxonomy.py): the example data, a model of three tiles, the twins, the N query and
    try_rc, each under the slab and the gather instance, held to check_case's criteria; the cases of CHUNKED (the mixed lengths
    among them) also in chunks of 1 and 3 queries (check_chunks)."""
    from dada2_amd import api
    entries = ties = 0
    for name in ("example", "ngenus129", "twins", "lengths", "len57", "broken_by_N", "try_rc"):
        e, t, got, stats = check_chunks(api, name) if name in CHUNKED else check_case(api, name)
        if name not in TIES_ARE_THE_POINT:
            entries += e
            ties += t
        if name == "twins":
            assert_twins(got, restated(name)[2])
    assert ties <= TIE_CAP * entries, (ties, entries)
    return "ok entries %d tied %d" % (entries, ties)


def assert_twins(got, tied):
    """Genera 3 and 70 have the same references: wherever one is at the maximum so is the other; over those entries both are picked."""
    both = tied[:, :, 3] & tied[:, :, 70]
    assert np.array_equal(tied[:, :, 3], tied[:, :, 70]) and both.sum() >= 200, int(both.sum())
    pk = picks(got)[both]
    assert (pk == 3).any() and (pk == 70).any(), (int((pk == 3).sum()), int((pk == 70).sum()))
