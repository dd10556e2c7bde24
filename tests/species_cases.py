"""assignSpecies / addSpecies (R/taxonomy.R:162-360): a restatement of the reference on Python strings, and the cases the device path
is held to (tests/test_species.py pins the restatement to the reference's example data on the CPU; tests/test_emu_species.py and
tests/test_gpu_species.py run the cases below, identically, under the emulator and on the device).

The reference matches with Biostrings (PDict + vcountPDict, fixed = TRUE): query q hits reference r exactly when q occurs in r as
a substring, letter for letter - ``q in r`` on Python strings, a reference's N, IUPAC code or lower-case letter equal to no query
letter - and with tryRC also when the reverse complement of q does.  Every case is compared as exact equality of the per-query
lists of reference indices with that restatement; nothing is left out."""
import math
import os
import random
import re

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
EXAMPLE_SPECIES = os.path.join(HERE, "golden", "example_species_assignment.fa.gz")
EXAMPLE_SEQS = os.path.join(HERE, "golden", "example_seqs.fa")

_COMP = str.maketrans("ACGT", "TGCA")


def rc(s):
    return s.translate(_COMP)[::-1]


# ---- the restatement ------------------------------------------------------------------------------------------------------------------
def restate_hits(seqs, refs, try_rc=False):
    """Per query the ascending list of the references it occurs in (R/taxonomy.R:264-280)."""
    out = []
    for q in seqs:
        p = rc(q)
        out.append([i for i, r in enumerate(refs) if q in r or (try_rc and p in r)])
    return out


def genus_species(ids):
    """:262-263: tokens 2 and 3 of strsplit(id, "\\\\s"), None where missing."""
    g, s = [], []
    for i in ids:
        t = re.split(r"[ \t\n\r\f\v]", i)
        if t and t[-1] == "":
            t.pop()
        g.append(t[1] if len(t) > 1 else None)
        s.append(t[2] if len(t) > 2 else None)
    return g, s


def map_hits(idx, names, keep):
    """mapHits, :163-171."""
    hits = [names[i] for i in idx]
    hits = ["Escherichia/Shigella" if h is not None and ("Escherichia" in h or "Shigella" in h) else h for h in hits]
    unq = list(dict.fromkeys(hits))
    if len(unq) <= keep:
        named = sorted(h for h in unq if h is not None)
        return "/".join(named) if named else None
    return None


def match_genera(gen_tax, gen_binom, split_glyph="/"):
    """matchGenera, :175-185."""
    if gen_tax is None or gen_binom is None:
        return False
    if len(gen_tax) == 0 or len(gen_binom) == 0:
        return False
    return bool(gen_tax == gen_binom or re.search("^" + gen_binom + "[ _" + split_glyph + "]", gen_tax)
                or re.search(split_glyph + gen_binom + "$", gen_tax))


def restate_assign(seqs, refs, ids, allow_multiple=False, try_rc=False):
    """assignSpecies: rows of (Genus, Species), None = NA."""
    keep = (math.inf if allow_multiple else 1) if isinstance(allow_multiple, bool) else int(allow_multiple)
    genus, species = genus_species(ids)
    return [(map_hits(h, genus, 1), map_hits(h, species, keep)) for h in restate_hits(seqs, refs, try_rc)]


def restate_add(taxtab, colnames, seqs, refs, ids, allow_multiple=False, try_rc=False):
    """addSpecies, :347-360: the rows of taxtab with the Species column appended."""
    binom = restate_assign(seqs, refs, ids, allow_multiple, try_rc)
    gcol = colnames.index("Genus") if colnames is not None and "Genus" in colnames else len(taxtab[0]) - 1
    return [list(row) + [b[1] if match_genera(row[gcol], b[0]) else None] for row, b in zip(taxtab, binom)]


def example():
    """(reference sequences, ids, queries) of the reference's example files, read without the package."""
    import gzip

    def fasta(path, opener):
        ids, seqs = [], []
        with opener(path, "rt") as fh:
            for line in fh:
                line = line.rstrip("\r\n")
                if line.startswith(">"):
                    ids.append(line[1:])
                    seqs.append("")
                elif ids:
                    seqs[-1] += line.strip().upper()
        return ids, seqs
    ids, refs = fasta(EXAMPLE_SPECIES, gzip.open)
    return refs, ids, fasta(EXAMPLE_SEQS, open)[1]


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


def _rand(rng, n):
    return "".join(rng.choice("ACGT") for _ in range(n))


def _ids(n):
    return ["r%d Genus%d species%d" % (i, i % 7, i) for i in range(n)]


def device_hits(api, refs, seqs, try_rc=False, env=None, stats=None, model=None):
    """The library's hit lists as plain lists."""
    def run(m):
        return [[int(x) for x in h] for h in with_env(env, lambda: api.species_hits(seqs, m, try_rc=try_rc, stats=stats))]
    if model is not None:
        return run(model)
    with api.SpeciesModel((refs, _ids(len(refs)))) as m:
        return run(m)


def check(api, refs, seqs, try_rc=False, env=None, stats=None, what=""):
    want = restate_hits(seqs, refs, try_rc)
    got = device_hits(api, refs, seqs, try_rc, env, stats)
    assert got == want, (what, [(j, got[j], want[j]) for j in range(len(seqs)) if got[j] != want[j]][:5])
    return want


def _embed(rng, q, length, pos):
    """A random reference of `length` with q at `pos`."""
    bg = _rand(rng, length)
    return bg[:pos] + q + bg[pos + len(q):]


def case_placement(api):
    rng = random.Random(1)
    q = _rand(rng, 40)
    L = 150
    at = [0, 1, 15, 16, 17, 31, 32, 33, 63, 64, 65, L - 40]
    refs = [_embed(rng, q, L, p) for p in at] + [q, q[:39], q[:31], q[:1], _rand(rng, L), ""]
    want = check(api, refs, [q], what="placement")
    assert want[0] == list(range(len(at) + 1))


def case_boundaries(api):
    rng = random.Random(2)
    q = _rand(rng, 40)
    refs = []
    for rowlen in (64, 96, 50):                                  # 64 and 96: the rows lie back to back in the packed words
        for cut in (20, 10, 31, 32, 33):                         # 10 and 31: the split lies inside the 32-base key
            refs += [_rand(rng, rowlen - cut) + q[:cut], q[cut:] + _rand(rng, rowlen - (40 - cut))]
    refs.append(_embed(rng, q, 64, 24))
    want = check(api, refs, [q], what="boundaries")
    assert want[0] == [len(refs) - 1]
    check(api, refs, [q], try_rc=True, what="boundaries rc")


def case_nonacgt_plane(api):
    rng = random.Random(3)
    q = _rand(rng, 40)
    refs, hit = [], []
    for letter in ("N", "W", "lower"):
        for off in (0, 5, 20, 36, 39, 40, -1):                   # inside the occurrence (key and tail), and the letter on either side of it
            r = list(_embed(rng, q, 120, 30))
            i = 30 + off
            r[i] = r[i].lower() if letter == "lower" else letter
            refs.append("".join(r))
            hit.append(off in (40, -1))
    want = check(api, refs, [q], what="plane")
    assert want[0] == [i for i, h in enumerate(hit) if h]
    check(api, refs, [q], try_rc=True, what="plane rc")


def case_keys(api):
    rng = random.Random(4)
    base = _rand(rng, 60)

    def other(c):
        return "ACGT"[("ACGT".index(c) + 1) % 4]
    q33a, q33b = base, base[:32] + other(base[32]) + base[33:]   # equal keys, different at base 33
    qla, qlb = base[:59] + "A", base[:59] + "C"                  # ... at the last base
    B = _rand(rng, 80)
    A = B[:50]                                                   # a proper prefix
    short_src = _rand(rng, 100)
    shorts = [short_src[10:18], short_src[10:30], short_src[40:71], short_src[3:35], short_src[50:83]]   # 8, 20, 31, 32, 33 nt
    refs = [_embed(rng, q33a, 100, 7), _embed(rng, q33b, 100, 19), _embed(rng, qla, 90, 0), _embed(rng, qlb, 90, 30),
            _embed(rng, B, 130, 33), _embed(rng, A, 130, 64), _embed(rng, A, 70, 20), short_src, _embed(rng, short_src[3:35], 32, 0),
            _embed(rng, short_src[40:71], 47, 16), _rand(rng, 200)]
    seqs = [q33a, q33b, qla, qlb, A, B] + shorts + [q33a, B, shorts[0], q33a]   # with repeats
    want = check(api, refs, seqs, what="keys")
    assert want[0] != want[1] and want[0] and want[1] and want[2] != want[3] and want[2] and want[3]
    assert set(want[5]) < set(want[4]) and want[5]
    assert all(want[6 + k] for k in range(5)) and want[11] == want[0]
    check(api, refs, seqs, try_rc=True, what="keys rc")


def case_multiplicity(api):
    rng = random.Random(5)
    q = _rand(rng, 45)
    thrice = _rand(rng, 10) + q + _rand(rng, 3) + q + q + _rand(rng, 20)
    refs = [thrice] + [_embed(rng, q, 60 + i, i % 16) for i in range(70)] + [_rand(rng, 90) for _ in range(5)]
    want = check(api, refs, [q, _rand(rng, 45)], what="multiplicity")
    assert want[0] == list(range(71)) and want[1] == []


def case_try_rc(api):
    rng = random.Random(6)
    q = _rand(rng, 50)
    half = _rand(rng, 20)
    pal = half + rc(half)                                        # its own reverse complement
    assert rc(pal) == pal
    refs = [_embed(rng, rc(q), 120, 31), _embed(rng, q, 100, 3) + _rand(rng, 5) + rc(q), _embed(rng, pal, 90, 17), _embed(rng, q, 77, 27),
            _rand(rng, 120)]
    on = check(api, refs, [q, pal, rc(q)], try_rc=True, what="try_rc on")
    off = check(api, refs, [q, pal, rc(q)], try_rc=False, what="try_rc off")
    assert on[0] == [0, 1, 3] and off[0] == [1, 3] and on[1] == off[1] == [2] and on[2] == [0, 1, 3] and off[2] == [0, 1]


def case_overflow(api):
    rng = random.Random(7)
    refs = ["A" * 500, "AC" * 250, _rand(rng, 300), "A" * 500, "CA" * 250, "A" * 499 + "C", _rand(rng, 64)]
    seqs = ["A" * 40, "A" * 33, "AC" * 20, "CA" * 20, "A" * 32, "AC" * 16, "ACA" + "CA" * 30, "A" * 500, "A" * 501, _rand(rng, 40)]
    for try_rc in (False, True):
        st_small, st_dflt = {}, {}
        want = check(api, refs, seqs, try_rc=try_rc, env={"DADA2HIP_SPECIES_CAND": 64}, stats=st_small, what="overflow, 64 records")
        check(api, refs, seqs, try_rc=try_rc, stats=st_dflt, what="overflow, default")
        assert want[0] == [0, 3, 5] and want[7] == [0, 3] and want[8] == []
        assert st_small["candidate_reruns"] >= 1 and st_dflt["candidate_reruns"] == 0, (st_small, st_dflt)
        assert st_small["candidates"] == st_dflt["candidates"] > 64 and st_small["hits"] == st_dflt["hits"] == sum(len(w) for w in want)
        assert st_small["windows"] == st_dflt["windows"] and st_small["windows_past_bitmap"] == st_dflt["windows_past_bitmap"]


def case_chunking(api):
    rng = random.Random(8)
    refs = [_rand(rng, 180) for _ in range(12)]
    seqs = [refs[i][5 * i: 5 * i + 35 + i] for i in range(8)] + [_rand(rng, 40), refs[3][100:140]]
    st1, st3 = {}, {}
    want = check(api, refs, seqs, try_rc=True, stats=st1, what="one chunk")
    check(api, refs, seqs, try_rc=True, env={"DADA2HIP_SPECIES_CHUNK": 3}, stats=st3, what="chunks of 3")
    assert sum(1 for w in want if w) == 9
    assert st3["windows"] == 4 * st1["windows"] and st3["hits"] == st1["hits"], (st1, st3)


_SWEEP = {}


def sweep_data():
    """200 references of 50-300 nt with 2 % N; 300 queries: half cut from references (33-120 nt), a quarter cut and changed at one
    base, a quarter random.  Built once per process, with its restatement (try_rc off and on)."""
    if not _SWEEP:
        rng = random.Random(9)
        refs = []
        for _ in range(200):
            r = list(_rand(rng, rng.randint(50, 300)))
            for i in range(len(r)):
                if rng.random() < 0.02:
                    r[i] = "N"
            refs.append("".join(r))

        def cut():
            while True:
                r = refs[rng.randrange(len(refs))]
                n = rng.randint(33, 120)
                if n > len(r):
                    continue
                o = rng.randint(0, len(r) - n)
                if "N" not in r[o: o + n]:
                    return r[o: o + n]
        seqs = [cut() for _ in range(150)]
        for _ in range(75):
            s = cut()
            i = rng.randrange(len(s))
            seqs.append(s[:i] + rng.choice([c for c in "ACGT" if c != s[i]]) + s[i + 1:])
        seqs += [_rand(rng, rng.randint(33, 120)) for _ in range(75)]
        _SWEEP.update(refs=refs, seqs=seqs, want={t: restate_hits(seqs, refs, t) for t in (False, True)})
        share = sum(1 for w in _SWEEP["want"][False] if w) / len(seqs)
        assert 0.40 <= share <= 0.70, share                      # both outcomes well represented
    return _SWEEP


def case_sweep(api):
    d = sweep_data()
    with api.SpeciesModel((d["refs"], _ids(len(d["refs"])))) as m:
        for t in (True, False):
            got = device_hits(api, None, d["seqs"], try_rc=t, model=m)
            want = d["want"][t]
            assert got == want, (t, [(j, got[j], want[j]) for j in range(len(want)) if got[j] != want[j]][:5])


def case_two_calls(api):
    rng = random.Random(10)
    refs = [_rand(rng, 150) for _ in range(20)]
    seqs = [refs[i][i: i + 50] for i in range(0, 20, 3)] + [_rand(rng, 50)]
    want = restate_hits(seqs, refs)
    with api.SpeciesModel((refs, _ids(len(refs)))) as m:
        assert m.nref == 20 and m.stats["references"] == 20 and m.stats["bases"] == 3000
        st = {}
        a = device_hits(api, None, seqs, model=m, stats=st)
        b = device_hits(api, None, seqs[::-1], model=m)
        c = device_hits(api, None, seqs, model=m)
    assert a == want and c == want and b == want[::-1]
    assert st["references"] == 20 and st["bases"] == 3000 and st["hits"] == sum(len(w) for w in want) and st["launches"] >= 3, st
    assert st["candidates"] >= st["hits"] and st["windows"] >= st["windows_past_bitmap"] >= st["candidates"], st
    assert st["windows"] == 20 * (150 - 31), st                 # every window of 32 inside its reference, once


EXAMPLE_TAXTAB_COLS = ["Kingdom", "Genus", "Note"]
EXAMPLE_TAXTAB = [["Bacteria", "Lactobacillus", "x"], ["Bacteria", "Bacillus", "x"], ["Bacteria", "Bacillus", "x"],
                  ["Bacteria", None, "x"], ["Bacteria", "Clostridium sensu stricto", "x"], ["Bacteria", "Clostridium", "x"]]


def case_example(api):
    refs, ids, seqs = example()
    for am in (False, True, 2):
        for t in (False, True):
            want = restate_assign(seqs, refs, ids, am, t)
            got = api.assign_species(seqs, EXAMPLE_SPECIES, allow_multiple=am, try_rc=t, n=3)
            assert got.shape == (6, 2) and [tuple(r) for r in got.tolist()] == want, (am, t, got.tolist())
    got = api.assign_species(seqs, EXAMPLE_SPECIES)
    assert tuple(got[0]) == ("Lactobacillus", None) and tuple(got[2]) == ("Virgibacillus", "kekensis")
    assert tuple(got[4]) == ("Clostridium", "hydrogeniformans")
    with api.SpeciesModel(EXAMPLE_SPECIES) as m:
        assert m.nref == 14
        for am in (False, True):
            want = restate_add(EXAMPLE_TAXTAB, EXAMPLE_TAXTAB_COLS, seqs, refs, ids, am)
            got = api.add_species(EXAMPLE_TAXTAB, seqs, m, colnames=EXAMPLE_TAXTAB_COLS, allow_multiple=am)
            assert got.shape == (6, 4) and got.tolist() == want, (am, got.tolist())
        assert [r[3] for r in got.tolist()] == ["mixtipabuli/odoratitofui/similis", None, None, None, "hydrogeniformans", None]
        nocols = [[r[0], r[1]] for r in EXAMPLE_TAXTAB]          # no names: the last column is the genus
        assert api.add_species(nocols, seqs, m).tolist() == restate_add(nocols, None, seqs, refs, ids)


def case_input_errors(api):
    from dada2_amd import _lib
    import pytest
    with api.SpeciesModel((["ACGTACGTAC"], ["a b c"])) as m:
        for bad in (["ACGN"], ["acgt"], ["ACGT", ""]):
            with pytest.raises(ValueError):
                api.species_hits(bad, m)
        assert [list(h) for h in api.species_hits(["ACGTACGTACG", "CGTACG"], m)] == [[], [0]]   # longer than every reference: no hit
        assert api.species_hits([], m) == []
    with pytest.raises(_lib.Dada2HipError) as e:
        _open_empty(api)                                         # nref == 0
    assert e.value.code == 1


def _open_empty(api):
    import ctypes as C
    from dada2_amd import _lib
    h = C.c_void_p()
    eb = C.create_string_buffer(512)
    _lib.check(_lib.lib().dada2hip_species_open(0, (C.c_char_p * 1)(), 0, C.byref(h), None, eb, 512), eb)


# ---- past one sweep of k_species_seed (8 192 references: 2 048 blocks of 4 waves), -m gpu only -----------------------------------------
STRIDED_NREF = 8200
_STRIDED = {}


def strided_data():
    """8 200 references of 40-90 nt, a few with an N and a few of 31, 32 and 33 nt; 21 queries: 35 nt cut from the references either
    side of a wave's and a block's second turn (0, 1, 4 095, 4 096, 8 191, 8 192, 8 193, the last), one embedded in every third
    reference, eight random ones, a whole reference of 31 nt, one across a reference's N and two reverse complements.  Built once per process, with its restatement."""
    if not _STRIDED:
        rng = random.Random(11)
        refs = [_rand(rng, rng.randint(40, 90)) for _ in range(STRIDED_NREF)]
        for i, n in ((5000, 31), (5001, 32), (5002, 33), (8194, 31), (8195, 32), (8196, 33), (17, 33)):
            refs[i] = _rand(rng, n)
        common = _rand(rng, 35)
        for i in range(2, STRIDED_NREF, 3):                      # (2, 5, ...: 8 192 and 8 195 - too short - among them, 0 and 4 095 not)
            if len(refs[i]) >= 35:
                refs[i] = _embed(rng, common, len(refs[i]), rng.randint(0, len(refs[i]) - 35))
        for i in (7, 4100, 8190, 8197, 8199):                    # an N away from the start, where the cuts below come from
            refs[i] = refs[i][:38] + "N" + refs[i][39:]
        refs[8198] = refs[8198][:10] + "N" + refs[8198][11:]     # ... and one inside what would be an occurrence
        at = (0, 1, 4095, 4096, 8191, 8192, 8193, STRIDED_NREF - 1)
        seqs = [refs[i][:35] if i % 2 else refs[i][len(refs[i]) - 35:] for i in at]
        seqs += [common] + [_rand(rng, 35) for _ in range(8)] + [refs[8194]]
        seqs += [refs[8198][:35].replace("N", "A"), rc(refs[4098][:35]), rc(refs[8188][3:38])]   # the N; found with try_rc only
        assert len(seqs) == 21 and len(refs[8194]) == 31 and all("N" not in q for q in seqs)
        want = {t: restate_hits(seqs, refs, t) for t in (False, True)}
        for k, i in enumerate(at):
            assert i in want[False][k], (k, i)
        assert len(want[False][8]) > 2600 and 8192 in want[False][8] and 8194 in want[False][17] and want[True][18] == []
        assert want[False][19] == want[False][20] == [] and want[True][19] == [4098] and want[True][20] == [8188]
        _STRIDED.update(refs=refs, seqs=seqs, want=want)
    return _STRIDED


def check_strided(api):
    """The hit lists against the restatement with try_rc off and on, by default and with a candidate buffer of 256 records, which
    the embedded query alone overflows: the range is halved (r0 > 0) down to where a sweep fits."""
    d = strided_data()
    out = {}
    with api.SpeciesModel((d["refs"], _ids(len(d["refs"])))) as m:
        for t in (False, True):
            for env in (None, {"DADA2HIP_SPECIES_CAND": 256}):
                st = {}
                got = device_hits(api, None, d["seqs"], try_rc=t, env=env, stats=st, model=m)
                want = d["want"][t]
                assert got == want, (t, env, [(j, got[j][:8], want[j][:8]) for j in range(len(want)) if got[j] != want[j]][:5])
                out[(t, env is not None)] = st
            a, b = out[(t, False)], out[(t, True)]
            assert a["candidate_reruns"] == 0 and b["candidate_reruns"] >= 1, (a, b)
            for k in ("candidates", "hits", "windows", "windows_past_bitmap"):
                assert a[k] == b[k], (t, k, a, b)
            assert a["hits"] == sum(len(w) for w in d["want"][t]) and a["candidates"] >= a["hits"] > 256, a
            assert a["windows"] > 0 and a["references"] == STRIDED_NREF, a
    return out


CASES = {"placement": case_placement, "boundaries": case_boundaries, "nonacgt_plane": case_nonacgt_plane, "keys": case_keys,
         "multiplicity": case_multiplicity, "try_rc": case_try_rc, "overflow": case_overflow, "chunking": case_chunking,
         "sweep": case_sweep, "two_calls": case_two_calls, "example": case_example, "input_errors": case_input_errors}
CASE_NAMES = tuple(CASES)


def emu_run():
    """The emulator's job (tests/test_emu_species.py): every case."""
    from dada2_amd import api
    for name in CASE_NAMES:
        CASES[name](api)
    return "ok %d cases" % len(CASE_NAMES)
