"""mergeSequenceTables and its two helpers: the parts that need no GPU.

  * The specification (tests/seqtab_cases.py) against the hand-derived results the cases carry - the worked example, a palindrome,
    both orientations in one table, the order of the tables deciding which orientation survives, repeats="sum" over three and four
    tables - and its two forms against each other on the random tables.
  * The host's part (dada2_amd/csrc/seqtab_plain.h: the row map, the refusals, the flags of tryRC, the rank by first appearance,
    the stable order) through tools/seqtab_plain_check.cpp - plain host C++ with a main of its own, built with the address and
    undefined-behaviour sanitizers, nothing of it loaded into Python - on the same cases, exactly as they run on the card.
  * getSequences and uniquesToFasta; the library's side of the new entry; dada2_amd.api has gained nothing."""
import gzip
import os
import shutil
import subprocess

import numpy as np
import pytest

import seqtab_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
needs_hipcc = pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which(HIPCC)), reason="no hipcc for the host build")
HOST_CASES = ("worked_example", "lengths", "in_table_collapse", "contention", "order", "iupac", "overflow", "validation")


class _Served:
    """dada2_amd.seqtables' merge_sequence_tables as the cases call it, served by something else."""

    def __init__(self):
        from dada2_amd import _lib, seqtables
        self._lib, self._st = _lib, seqtables

    def merge_sequence_tables(self, tables, repeats="error", order_by="abundance", try_rc=False, device=0, stats=None):
        if repeats not in ("error", "sum"):
            raise ValueError('repeats must be "error" or "sum"')
        if order_by not in (None, "abundance", "nsamples"):
            raise ValueError('order_by must be "abundance", "nsamples" or None')
        mat, seqs, names, cmap = self.serve(tables, repeats, order_by, try_rc)
        if stats is not None:
            stats["col_map"] = cmap
        return mat, seqs, names


class SpecModule(_Served):
    def serve(self, tables, repeats, order_by, try_rc):
        try:
            return sc.spec_merge(tables, repeats=repeats, order_by=order_by, try_rc=try_rc)
        except sc.SpecError as e:
            raise self._lib.Dada2HipError(e.code, str(e))


class PlainModule(_Served):
    def __init__(self, exe, tmp):
        super().__init__()
        self.exe, self.tmp = exe, str(tmp)

    def serve(self, tables, repeats, order_by, try_rc):
        mats, cols, rows = self._st._tables(tables)
        lines = ["%d %d %d %d" % (len(mats), repeats == "sum", {None: 0, "abundance": 1, "nsamples": 2}[order_by], bool(try_rc))]
        c0 = r0 = 0
        for m in mats:
            lines.append("%d %d" % m.shape)
            lines += rows[r0:r0 + m.shape[0]] + cols[c0:c0 + m.shape[1]]
            lines += [" ".join(str(int(v)) for v in row) for row in m] if m.shape[1] else []
            r0 += m.shape[0]
            c0 += m.shape[1]
        path = os.path.join(self.tmp, "tables.txt")
        with open(path, "w") as fh:
            fh.write("\n".join(lines) + "\n")
        out = subprocess.run([self.exe, path], capture_output=True, text=True, timeout=300)
        if out.returncode == 3:
            _, code, msg = out.stdout.rstrip("\n").split(" ", 2)
            raise self._lib.Dada2HipError(int(code), msg)
        assert out.returncode == 0, (out.returncode, out.stdout[-1000:], out.stderr[-3000:])
        text = out.stdout.split("\n")
        nr, nc = (int(x) for x in text[0].split())
        names, seqs = text[1:1 + nr], text[1 + nr:1 + nr + nc]
        mat = np.array([[int(x) for x in text[1 + nr + nc + r].split()] for r in range(nr)], dtype=np.int32).reshape(nr, nc)
        cmap = np.array([int(x) for x in text[1 + 2 * nr + nc].split()], dtype=np.int32)
        return np.ascontiguousarray(mat), seqs, names, cmap


@pytest.fixture(scope="module")
def plain_check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("seqtab_plain") / "seqtab_plain_check")
    subprocess.check_call([HIPCC, "-O1", "-g", "-std=c++17", "-Wall", "-Xarch_host", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-x", "c++", os.path.join(ROOT, "tools", "seqtab_plain_check.cpp"), "-o", exe])
    return exe


@pytest.mark.parametrize("name", HOST_CASES)
def test_specification_gives_the_hand_derived_results(name):
    sc.CASES[name](SpecModule())


RANDOM = {"random_repeats": lambda: sc.random_tables(1111), "random": lambda: sc.random_tables(1112, repeat_names=False),
          "small": lambda: sc.random_tables(1114, ntab=5, nrow=3, maxcol=30, npool=40, lo=5, hi=9, both=0.5)}


@pytest.mark.parametrize("name", tuple(RANDOM))
def test_the_two_specifications_agree(name):
    tabs = RANDOM[name]()
    repeats = "error" if name == "random" else "sum"
    for try_rc in (False, True):
        for order_by in ("abundance", "nsamples", None):
            kw = dict(repeats=repeats, order_by=order_by, try_rc=try_rc)
            sc.same(sc.spec_merge_fast(tabs, **kw), sc.spec_merge(tabs, **kw), (name, kw))
    if repeats == "sum":
        for spec in (sc.spec_merge, sc.spec_merge_fast):
            with pytest.raises(sc.SpecError, match="Duplicated sample names detected"):
                spec(tabs, repeats="error")


@needs_hipcc
@pytest.mark.parametrize("name", HOST_CASES)
def test_plain_host_part_under_the_sanitizers(plain_check, tmp_path, name):
    sc.CASES[name](PlainModule(plain_check, tmp_path))


@needs_hipcc
def test_plain_host_part_on_random_tables(plain_check, tmp_path):
    pm = PlainModule(plain_check, tmp_path)
    tabs = sc.random_tables(1115, ntab=6, nrow=4, maxcol=60, npool=120, lo=40, hi=60, both=0.3)
    for try_rc in (False, True):
        for order_by in ("abundance", "nsamples", None):
            sc.check(pm, tabs, "random tables", spec=sc.spec_merge_fast, repeats="sum", order_by=order_by, try_rc=try_rc)


# ---- the two helpers --------------------------------------------------------------------------------------------------------------------

def test_uniques_to_fasta_text(tmp_path):
    from dada2_amd import seqtables as st
    out = str(tmp_path / "u.fasta")
    st.uniques_to_fasta((["ACGTACGTAC", "TTG", "ACGTACGTAC"], [7, 2, 1]), out)
    with open(out, "rb") as fh:
        assert fh.read() == b">sq1;size=7;\nACGTACGTAC\n>sq2;size=2;\nTTG\n>sq3;size=1;\nACGTACGTAC\n"   # input order, duplicates kept
    st.uniques_to_fasta({"ACGTACGTAC": 7, "TTG": 2}, out, width=4)
    with open(out, "rb") as fh:
        assert fh.read() == b">sq1;size=7;\nACGT\nACGT\nAC\n>sq2;size=2;\nTTG\n"
    st.uniques_to_fasta({"GGA": 5}, out, ids=["last one"], mode="a", width=3)
    with open(out, "rb") as fh:
        assert fh.read() == b">sq1;size=7;\nACGT\nACGT\nAC\n>sq2;size=2;\nTTG\n>last one\nGGA\n"
    mat = np.array([[1, 2], [3, 4]], dtype=np.int32)
    st.uniques_to_fasta((mat, ["AAC", "GGT"]), out)
    with open(out, "rb") as fh:
        assert fh.read() == b">sq1;size=4;\nAAC\n>sq2;size=6;\nGGT\n"
    with pytest.raises(ValueError):
        st.uniques_to_fasta({"GGA": 5}, out, ids=["a", "b"])
    with pytest.raises(ValueError):
        st.uniques_to_fasta({"GGA": 5}, out, mode="wb")


def test_get_sequences_of_every_input_kind(tmp_path):
    from dada2_amd import seqtables as st
    from dada2_amd.io import Derep
    assert st.get_sequences(["acg", "TTG", "acg", "ACG"]) == ["ACG", "TTG", "ACG", "ACG"]
    assert st.get_sequences(["acg", "TTG", "acg", "ACG"], collapse=True) == ["ACG", "TTG", "ACG"]   # unique(), then toupper()
    assert st.get_sequences("acgt") == ["ACGT"]
    assert st.get_sequences({"TTG": 3, "ACG": 9}) == ["TTG", "ACG"]
    assert st.get_sequences((["TTG", "ACG", "TTG"], [3, 9, 1])) == ["TTG", "ACG", "TTG"]
    assert st.get_sequences((["TTG", "ACG", "TTG"], [3, 9, 1]), collapse=True) == ["ACG", "TTG"]   # names(tapply(.)): byte order
    mat = np.array([[1, 2], [3, 4]], dtype=np.int32)
    assert st.get_sequences((mat, ["GGT", "AAC"])) == ["GGT", "AAC"]
    d = Derep(seqs=["GGT", "AAC"], abundances=np.array([2, 1], dtype=np.int32), quals=np.zeros((2, 3)), map=np.array([0, 1, 0], dtype=np.int32))
    assert st.get_sequences(d) == ["GGT", "AAC"]
    fa = str(tmp_path / "x.fasta")
    st.uniques_to_fasta({"acgtac": 2, "TTGCA": 1}, fa, width=4)
    assert st.get_sequences(fa) == ["ACGTAC", "TTGCA"]
    with gzip.open(fa + ".gz", "wb") as fh:
        fh.write(b">a\nacgt\nAC\n>b\nTTG\n")
    assert st.get_sequences(fa + ".gz") == ["ACGTAC", "TTG"]
    fq = str(tmp_path / "x.fastq")
    with open(fq, "wb") as fh:
        fh.write(b"@r1\nACGTT\n+\nIIIII\n@r2\nGGA\n+\nIII\n@r3\nACGTT\n+\nIIIII\n")
    assert st.get_sequences(fq) == ["ACGTT", "GGA", "ACGTT"]
    with pytest.raises(ValueError):
        st.get_sequences(12)


# ---- the library's side -------------------------------------------------------------------------------------------------------------------

def test_entry_is_declared_and_registered():
    from dada2_amd import _lib, api, seqtables
    with open(os.path.join(ROOT, "include", "dada2hip.h")) as fh:
        header = fh.read()
    for name in ("dada2hip_seqtab_merge", "dada2hip_seqtab_nrow", "dada2hip_seqtab_ncol", "dada2hip_seqtab_cells", "dada2hip_seqtab_sequences",
                 "dada2hip_seqtab_samples", "dada2hip_seqtab_free"):
        assert name + "(" in header, name
    assert "#define DADA2HIP_SEQTAB_NSTATS %d" % _lib.SEQTAB_NSTATS in header
    assert tuple(_lib.SEQTAB_STATS) == sc.STAT_WORDS == tuple(seqtables.STATS) and len(sc.STAT_WORDS) <= _lib.SEQTAB_NSTATS
    for name in ("merge_sequence_tables", "get_sequences", "uniques_to_fasta"):
        assert hasattr(seqtables, name) and not hasattr(api, name), name
    assert seqtables.rc("ACNRVT") == "ABYNGT"


def test_python_level_refusals_need_no_device():
    from dada2_amd import seqtables as st
    ok = sc.table(["a"], ["ACG"], [[1]])
    for bad, text in (([ok], "At least two"), ([ok, (np.zeros(3, dtype=np.int32), ["A"], ["b"])], "Not a matrix"),
                      ([ok, (np.zeros((1, 2), dtype=np.int32), ["A"], ["b"])], "Sequence table 2"),
                      ([ok, (np.zeros((1, 1)), ["A"], ["b"])], "integer counts"), ([ok, ("ACG", 1)], "triple")):
        with pytest.raises(ValueError, match=text):
            st.merge_sequence_tables(bad)
    with pytest.raises(ValueError, match="order_by"):
        st.merge_sequence_tables([ok, ok], order_by="total")
    with pytest.raises(ValueError, match="repeats"):
        st.merge_sequence_tables([ok, ok], repeats="mean")
