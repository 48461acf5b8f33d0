"""unsegment (Glu) and shuffle (Shf), CPU part: the specification (tests/glue_shuffle_spec.py) on hand cases and against the reference's
laws, the library's surface, tksmseq_glue_joins against the specification (no device), the argument checks of `tksm unsegment` and
`tksm shuffle`, and the piece cutter of `tksm unsegment` (csrc/glue_cut.h) as a stand-alone program, plain and sanitized.  The device
side is in tests/test_glue_shuffle_gpu.py."""
import ctypes
import itertools
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT

import glue_shuffle_spec as gs
import mdf_ops_oracle as mo

EXE = os.path.join(ROOT, "tksm_amd", "tksm")
SEEDS = np.arange(24000, dtype=np.uint64)


def _cli(*args, **kw):
    return subprocess.run([EXE, *[str(a) for a in args]], capture_output=True, text=True, timeout=600, **kw)


def _rec(name, depth=1, comment="", segs=1):
    return f"+{name}\t{depth}\t{comment}\n" + "".join(f"chr1\t{10 * k}\t{10 * k + 5}\t{'+-'[k % 2]}\t{'1A' if k == 0 else ''}\n" for k in range(segs))


def _seg(k):
    return f"chr1\t{10 * k}\t{10 * k + 5}\t{'+-'[k % 2]}\t{'1A' if k == 0 else ''}\n"


# ------------------------------------------------------------------------------------------------ glue_spec by hand
def test_glue_spec_hand_cases():
    text = _rec("a", comment="x=1;") + _rec("b", segs=2, comment="CB=AC;") + _rec("c")
    mols = mo.stream_mdf(text, unroll=True)
    # p = 0 (and below, and NaN): nothing is glued
    for p in (0.0, -1.0, float("nan")):
        assert mo.write_mdf(gs.glue_spec(mols, p, 42)) == text
    # p = 1 (and above): one molecule; a chain of three lists its joiners under Cat in order; the joiners' own comments are dropped
    for p in (1.0, 2.0):
        assert mo.write_mdf(gs.glue_spec(mols, p, 42)) == "+a\t1\tCat=b,c;x=1;\n" + _seg(0) + _seg(0) + _seg(1) + _seg(0)
    assert mols[0]["meta"] == {"x": ["1"]} and len(mols[0]["segments"]) == 1          # (the input is not changed)
    # a head that carries a bare Cat flag still dumps the flag; one with a value gets the ids behind it; keys are dumped sorted
    assert mo.write_mdf(gs.glue_spec(mo.stream_mdf(_rec("a", comment="Cat;") + _rec("b")), 1.0, 1)) == "+a\t1\tCat;\n" + _seg(0) * 2
    assert mo.write_mdf(gs.glue_spec(mo.stream_mdf(_rec("a", comment="z=2;Cat=x;") + _rec("b") + _rec("c")), 1.0, 1)) == "+a\t1\tCat=x,b,c;z=2;\n" + _seg(0) * 3
    # an input without comments still gets Cat
    assert mo.write_mdf(gs.glue_spec(mo.stream_mdf(_rec("a") + _rec("b")), 1.0, 1)) == "+a\t1\tCat=b;\n" + _seg(0) * 2
    # the copies of a depth-3 record are molecules of their own: they glue to each other, under their written ids
    assert mo.write_mdf(gs.glue_spec(mo.stream_mdf(_rec("r", depth=3, comment="k=v;"), unroll=True), 1.0, 1)) == "+r_0\t1\tCat=r_1,r_2;k=v;\n" + _seg(0) * 3
    assert gs.glue_spec([], 0.5, 1) == []


def test_glue_spec_draws_per_unrolled_molecule_and_first_index():
    """the chains follow joins(first + i) molecule by molecule -- inside a depth-3 record as between records -- and molecule 0 of a
    call is a head whatever joins(first) says"""
    seed, p = 7, 0.5
    text = "".join(_rec(f"m{i}", depth=3 if i % 4 == 1 else 1, comment=f"n={i};") for i in range(40))
    mols = mo.stream_mdf(text, unroll=True)
    n = len(mols)
    assert n == 60
    first = next(g for g in range(1000, 2000) if gs.joins_np(seed, p, [g])[0])         # a first index that itself would join
    for f in (0, first, 2**32 - 1, 2**32):
        j = gs.joins_np(seed, p, f + np.arange(n, dtype=np.uint64))
        j[0] = False
        out = gs.glue_spec(mols, p, seed, first=f)
        heads = [i for i in range(n) if not j[i]]
        assert [m["id"] for m in out] == [mols[i]["id"] for i in heads]
        for k, h in enumerate(heads):
            e = heads[k + 1] if k + 1 < len(heads) else n
            assert out[k]["segments"] == [s for i in range(h, e) for s in mols[i]["segments"]]
            assert out[k]["meta"].get("Cat", []) == [mols[i]["id"] for i in range(h + 1, e)] and out[k]["meta"]["n"] == mols[h]["meta"]["n"]
            assert out[k]["depth"] == 1
        # the last chain is there: every input segment is written, the last molecule included
        assert sum(len(m["segments"]) for m in out) == sum(len(m["segments"]) for m in mols)
        assert out[-1]["id"] == mols[-1]["id"] or out[-1]["meta"]["Cat"][-1] == mols[-1]["id"]
        # the copies of one record part ways: some are heads of their own, some are glued
        assert any(re.search(r"_[12]$", m["id"]) for m in out) and any(re.search(r"_[12]$", c) for m in out for c in m["meta"].get("Cat", []))
    assert list(gs.chains(n, p, seed)) == [len(m["meta"].get("Cat", [])) + 1 for m in gs.glue_spec(mols, p, seed)]


def test_glue_rate_is_binomial():
    from scipy.stats import binomtest
    g = np.arange(1, 100_001, dtype=np.uint64)
    for seed in (0, 42):
        k = int(gs.joins_np(seed, 0.1, g).sum())
        pv = binomtest(k, len(g), 0.1).pvalue
        print(f"seed {seed}: {k} of {len(g)} join at p = 0.1, binomial p-value {pv:.4f}")
        assert pv > 1e-3
    assert not gs.joins_np(42, 1.0, [0])[0] and gs.joins_np(42, 1.0, [1])[0]


# ------------------------------------------------------------------------------------------------ shuffle_spec
def test_shuffle_spec_basics():
    for n in (0, 1, 2, 7, 100):
        for seed in (1, 2):
            whole = gs.shuffle_order(n, seed)
            assert sorted(whole) == list(range(n))
            assert gs.shuffle_order(n, seed, 1) == list(range(n))                     # one slot: everything leaves as it came
            for B in (n, n + 1, 10 * n + 3):
                assert gs.shuffle_order(n, seed, B) == whole
            for B in range(2, n):
                assert sorted(gs.shuffle_order(n, seed, B)) == list(range(n)), (n, seed, B)
    assert gs.shuffle_order(100, 1) != gs.shuffle_order(100, 2) != list(range(100))
    # a molecule leaves the buffer only when another arrives: output t - B is one of the first t molecules
    for B in (2, 5, 50):
        o = gs.shuffle_order(100, 3, B)
        assert all(o[k] < B + k for k in range(100 - B))
    mols = mo.stream_mdf(_rec("a", depth=2, comment="k;") + _rec("b"), unroll=True)
    out = gs.shuffle_spec(mols, 5)
    assert sorted(m["id"] for m in out) == ["a_0", "a_1", "b"] and all(m["depth"] == 1 for m in out)


def test_whole_mode_is_uniform_over_the_24_orders():
    from scipy.stats import chisquare
    draws = gs.shuffle_draws(4, SEEDS)
    counts = {p: 0 for p in itertools.permutations(range(4))}
    for k in range(len(SEEDS)):
        counts[tuple(gs.shuffle_order(4, int(SEEDS[k]), 0, (draws[0][k], draws[1][k])))] += 1
    stat, pv = chisquare(list(counts.values()))
    print(f"whole mode, n = 4, {len(SEEDS)} seeds: chi-square {stat:.1f} at 23 degrees of freedom, p = {pv:.4f}")
    assert min(counts.values()) > 0 and pv > 1e-3
    assert gs.shuffle_order(4, 5) == gs.shuffle_order(4, 5, 0, (draws[0][5], draws[1][5]))


def test_windowed_law_matches_the_reference():
    """where molecule 0 ends up at n = 6, B = 3: the specification over 24 000 seeds against shuffle_stream restated with numpy's generator"""
    from scipy.stats import chi2_contingency
    draws = gs.shuffle_draws(6, SEEDS, 3)
    spec = np.zeros(6)
    for k in range(len(SEEDS)):
        spec[gs.shuffle_order(6, int(SEEDS[k]), 3, (draws[0][k], draws[1][k])).index(0)] += 1
    rs = np.random.RandomState(11)
    ref = np.zeros(6)
    for _ in range(len(SEEDS)):
        ref[gs.shuffle_reference(6, 3, rs).index(0)] += 1
    pv = chi2_contingency(np.stack([spec, ref]))[1]
    print(f"position of molecule 0: spec {spec.astype(int).tolist()}, reference {ref.astype(int).tolist()}, p = {pv:.4f}")
    assert pv > 1e-3
    # and the reference without a buffer size is a permutation of everything
    assert sorted(gs.shuffle_reference(9, None, rs)) == list(range(9))


# ------------------------------------------------------------------------------------------------ library and CLI surface
def test_library_exports_and_header():
    from tksm_amd import _lib
    lib = ctypes.CDLL(os.path.join(ROOT, "tksm_amd", "libtksmseq.so"))
    header = open(os.path.join(ROOT, "include", "tksmseq.h")).read()
    for s in ("tksmseq_glue", "tksmseq_glue_joins", "tksmseq_shuffle", "tksmseq_unsegment_main", "tksmseq_shuffle_main"):
        assert hasattr(lib, s), s
        assert re.search(r"\bint " + s + r"\(", header), s
        assert s in _lib.SYMBOLS
    assert "tksmseq_glue_params" in header and "tksmseq_shuffle_params" in header
    assert ctypes.sizeof(_lib.GlueParams) == 32 and ctypes.sizeof(_lib.ShuffleParams) == 24
    from tksm_amd.sequence import Sequencer
    assert callable(Sequencer.glue) and callable(Sequencer.shuffle)


def test_glue_joins_on_the_host_agrees_with_the_spec():
    lib = ctypes.CDLL(os.path.join(ROOT, "tksm_amd", "libtksmseq.so"))
    lib.tksmseq_glue_joins.restype = ctypes.c_int
    lib.tksmseq_glue_joins.argtypes = [ctypes.c_uint64, ctypes.c_double, ctypes.c_uint64]
    g = np.concatenate([np.arange(0, 4000), 2**32 - 1500 + np.arange(3000), 2**40 + np.arange(3000)]).astype(np.uint64)
    assert len(g) == 10_000
    for seed, p in ((0, 0.1), (42, 0.5), (2**63 + 12345, 0.9)):
        want = gs.joins_np(seed, p, g)
        got = np.array([lib.tksmseq_glue_joins(seed, p, int(x)) for x in g], bool)
        assert 0 < want.sum() < len(g) and (got == want).all(), (seed, p)
    for p, v in ((0.0, 0), (-1.0, 0), (float("nan"), 0), (1.0, 1), (2.0, 1)):
        assert all(lib.tksmseq_glue_joins(3, p, x) == v for x in (1, 2, 2**32, 2**32 + 1)) and lib.tksmseq_glue_joins(3, p, 0) == 0


def test_help_exits_zero_and_list_is_unchanged():
    r = _cli("unsegment", "--help")
    assert r.returncode == 0 and "usage: unsegment" in r.stdout and "PROBABILITY" in r.stdout
    r = _cli("shuffle", "--help")
    assert r.returncode == 0 and "usage: shuffle" in r.stdout and "--buffer-size" in r.stdout and "not bound memory" in r.stdout.replace("NOT", "not")
    r = _cli("list")
    assert r.returncode == 0 and r.stdout.split() == ["sequence", "pcr", "truncate", "polyA", "tag", "scb", "flip"]
    r = _cli("glue")
    assert r.returncode == 1 and "Unknown kisim" in r.stderr and "`unsegment` and `shuffle`" in r.stderr


@pytest.mark.parametrize("args,messages,absent", [
    (["unsegment"], ["input is required!", "output is required!", "probability is required!", "usage: unsegment"], []),
    (["unsegment", "-o", "o.mdf", "-p", "0.1"], ["input is required!", "usage: unsegment"], ["output is required!", "probability is required!"]),
    (["unsegment", "-i", "a.mdf", "--probability", "0.1"], ["output is required!"], ["input is required!", "probability is required!"]),
    (["unsegment", "-i", "a.mdf", "-o", "o.mdf"], ["probability is required!", "usage: unsegment"], ["input is required!"]),
    (["unsegment", "-i", "a.mdf", "-o", "o.mdf", "-p", "0.1", "--bogus"], ["Option '--bogus' does not exist"], []),
    (["shuffle"], ["input is required!", "output is required!", "usage: shuffle"], []),
    (["shuffle", "-o", "o.mdf"], ["input is required!", "usage: shuffle"], ["output is required!"]),
    (["shuffle", "-i", "a.mdf", "--buffer-size", "5"], ["output is required!"], ["input is required!"]),
    (["shuffle", "-i", "a.mdf", "-o", "o.mdf", "--buffer-size", "0"], ["buffer-size must be at least 1"], ["usage"]),
    (["shuffle", "-i", "a.mdf", "-o", "o.mdf", "-b", "5"], ["Option '-b' does not exist"], []),          # long only (src/shuffle.cpp:57)
    (["shuffle", "-i", "a.mdf", "-o", "o.mdf", "--bogus"], ["Option '--bogus' does not exist"], []),
])
def test_argument_checks_follow_the_reference(args, messages, absent, tmp_path):
    r = _cli(*args, cwd=tmp_path)
    assert r.returncode == 1, (args, r.stderr)
    for m in messages:
        assert m in r.stderr, (args, m, r.stderr)
    for m in absent:
        assert m not in r.stderr, (args, m, r.stderr)
    assert not (tmp_path / "o.mdf").exists()                               # refused before anything is opened


# ------------------------------------------------------------------------------------------------ the piece cutter, stand-alone
@pytest.fixture(scope="module", params=["plain", "sanitized"])
def cutter(request, tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no C++ compiler"
    exe = tmp_path_factory.mktemp("gluecut_" + request.param) / "glue_cut_check"
    flags = ["-O2"] if request.param == "plain" else ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", *flags, "-I", os.path.join(ROOT, "tksm_amd", "csrc"),
                    os.path.join(ROOT, "tools", "glue_cut_check.cpp"), "-o", str(exe)], check=True)
    return str(exe)


def _records(text):
    """(offset, depth) of every record of an MDF text"""
    out, at = [], 0
    for line in text.splitlines(keepends=True):
        if line.startswith("+"):
            d = line.rstrip("\n").split("\t")
            out.append((at, int(d[1]) if len(d) > 1 and re.fullmatch(r"\d+", d[1]) else 0))
        at += len(line)
    return out


def cut_py(text, first, joins):
    """glue_cut restated: the last record whose first molecule does not join -> (found, offset, molecules before it)"""
    found, n = (0, 0, None), 0
    for at, depth in _records(text):
        if not (first + n < len(joins) and joins[first + n] == "1"):
            found = (1, at, n)
        n += depth
    return found if found[0] else (0, 0, n)


CUT_TEXTS = {
    "empty": "",
    "one": _rec("a"),
    "depths": _rec("a", depth=3) + _rec("b", segs=3) + _rec("c", depth=2) + _rec("d") + _rec("e", depth=4, comment="k=v;") + _rec("f"),
    "no trailing newline": (_rec("a") + _rec("b", depth=2) + _rec("c"))[:-1],
    "header only, no newline": _rec("a") + "+b\t2\t",
    "odd depths": _rec("a") + "+b\t-3\tx;\n" + _seg(1) + "+c\n" + _seg(0) + "+d\t12\t\n" + _seg(2) + _rec("e"),
}


@pytest.mark.parametrize("name", list(CUT_TEXTS))
def test_cutter_agrees_with_its_restatement(cutter, name, tmp_path):
    text = CUT_TEXTS[name]
    f = tmp_path / "t.mdf"
    f.write_bytes(text.encode())
    n = sum(d for _, d in _records(text))
    rs = np.random.RandomState(len(text))
    patterns = ["0", "1" * (n + 8), "0" + "1" * (n + 8), "1" * max(0, n - 1) + "0"] + ["".join(rs.choice(["0", "1"], n + 4, p=[q, 1 - q])) for q in (0.2, 0.5, 0.8) for _ in range(3)]
    for joins in patterns:
        for first in (0, 1, 3):
            got = subprocess.run([cutter, "cut", f, str(first), joins], capture_output=True, text=True, check=True).stdout.split()
            assert tuple(int(x) for x in got) == cut_py(text, first, joins), (name, joins, first)
    # a boundary at offset 0 is reported as one (found, offset 0, nothing before it); no boundary at all counts every molecule
    if text:
        assert cut_py(text, 0, "0" + "1" * (n + 8)) == (1, 0, 0)
        assert cut_py(text, 5, "1" * (n + 8)) == (0, 0, n)


@pytest.mark.parametrize("nbytes", [1, 40, 90, 300, 10_000])
def test_pieces_never_split_a_chain(cutter, nbytes, tmp_path):
    """the reader of `tksm unsegment` (ChunkReader + GlueHold) on records of depth 1 - 3: the pieces join to the input, each starts at a
    record whose first molecule does not join, `first` and the molecule counts are right -- also through a run of joiners many chunks long"""
    rs = np.random.RandomState(5)
    depths = [int(rs.randint(1, 4)) for _ in range(60)]
    text = "".join(_rec(f"m{i}", depth=d, segs=1 + i % 3) for i, d in enumerate(depths))
    n = sum(depths)
    f = tmp_path / "t.mdf"
    f.write_bytes(text.encode())
    run = "1" * 70                                                        # molecules 20 .. 89 all join: no cut for ~35 records
    for joins in ("0" * n, "0" + "1" * n, "".join(rs.choice(["0", "1"], 20)) + run + "".join(rs.choice(["0", "1"], n)), "".join(rs.choice(["0", "1"], n, p=[0.1, 0.9]))):
        r = subprocess.run([cutter, "pieces", f, str(nbytes), joins], capture_output=True, check=True)
        rows = [tuple(int(x) for x in l.split()) for l in r.stdout.decode().splitlines()]
        assert r.stderr.decode() == text and sum(ln for _, _, ln in rows) == len(text)
        starts = {at: None for at, _ in _records(text)}
        at, first = 0, 0
        for k, (f0, mols, ln) in enumerate(rows):
            piece = text[at:at + ln]
            assert f0 == first and mols == sum(d for _, d in _records(piece)) and ln > 0 and at in starts
            assert k == 0 or joins[first] == "0", (nbytes, k)
            at += ln
            first += mols
        assert first == n
        if joins == "0" * n and nbytes < 40:
            assert len(rows) == 60                                         # every record boundary is a cut
        if joins == "0" + "1" * n:
            assert len(rows) == 1                                          # one chain: one piece, whatever the chunk size
    e = tmp_path / "e.mdf"
    e.write_bytes(b"")
    r = subprocess.run([cutter, "pieces", e, str(nbytes), "0"], capture_output=True, check=True)
    assert r.stdout.decode() == "0 0 0\n"                                  # an empty input is one empty piece
