"""map -c without a device: the specification (tests/map_align_spec.py) against itself, an independent Levenshtein and hand-checked cases,
that its rules give sensible alignments, the C interface against the header and the Python declarations, the module's argument checks, and
the host code under sanitizers."""
import ctypes
import json
import os
import random
import re
import subprocess

import pytest

from conftest import ROOT

import map_align_spec as A
import map_spec as M

EXE = os.path.join(ROOT, "tksm_amd", "tksm")
SEED = 1                                           # the seed of the planted-edit reads: chosen so that the condition of the test below holds


def levenshtein(a, b):
    """ten lines, no band: a letter outside ACGT matches nothing"""
    prev = list(range(len(b) + 1))
    for i, x in enumerate(a, 1):
        cur = [i]
        for j, y in enumerate(b, 1):
            cur.append(min(prev[j - 1] + (x != y or x not in "ACGT"), prev[j] + 1, cur[-1] + 1))
        prev = cur
    return prev[-1]


def test_band_reaches_the_corner_and_an_anti_diagonal_has_at_most_w_plus_one_cells():
    for W in (1, 2, 3, 4):
        for dt in range(1, 41):
            for dq in range(1, 41):
                reach = {(0, 0)}
                for s, lo, hi in A.band_rows(dt, dq, W):
                    cells = [i for i in range(max(0, s - dq), min(dt, s) + 1) if A.allowed(i, s - i, dt, dq, W)]
                    assert cells == list(range(lo, hi + 1)) and len(cells) <= W + 1, (dt, dq, W, s)      # consecutive i, as band_rows says
                    reach |= {(i, s - i) for i in cells if {(i - 1, s - i), (i, s - i - 1), (i - 1, s - i - 1)} & reach}
                assert (dt, dq) in reach, (dt, dq, W)
    for dt, dq in ((63, 64), (200, 200), (5000, 4500), (300, 800)):
        assert max(hi - lo + 1 for _, lo, hi in A.band_rows(dt, dq, 63)) <= 64


def test_a_band_that_allows_every_cell_gives_levenshtein():
    rs = random.Random(3)
    full = 0
    for _ in range(400):
        dt, dq = rs.randint(1, 40), rs.randint(1, 40)
        T = "".join(rs.choice("ACGTN") for _ in range(dt))
        Q = A.plant(rs, T, 0.2)[0][:dq] or "A"
        dq = len(Q)
        for W in (1, 2, 3, 4, 63):
            columns, d, cells = A.align_segment(T, Q, W)
            t, q, n = A.cigar_spans(A.cigar(columns, True))
            assert (t, q) == (dt, dq) and d == n["X"] + n["I"] + n["D"] and A.cigar_spans(A.cigar(columns, False))[:2] == (dt, dq)
            assert d >= levenshtein(T, Q)
            if 2 * dt * dq <= W * (dt + dq):
                full += 1
                assert cells == (dt + 1) * (dq + 1) and d == levenshtein(T, Q), (T, Q, W)
    assert full > 400


def test_recorded_cases():
    g = json.load(open(os.path.join(ROOT, "tests", "golden", "map_align_known_answers.json")))
    for s in g["segments"]:
        assert A.align_segment(s["T"], s["Q"], s["W"])[:2] == (s["columns"], s["nm"]), s["name"]
    b = g["band"]
    assert levenshtein(b["T"], b["Q"]) == b["unbanded"] == A.align_segment(b["T"], b["Q"], 63)[1]
    assert A.align_segment(b["T"], b["Q"], 1)[1] > b["unbanded"] and A.align_segment(b["T"], b["Q"], 63)[0] == "D" * 6 + "=" * 12 + "I" * 6
    assert A.cigar("==X=IID", True) == "2=1X1=2I1D" and A.cigar("==X=IID", False) == "4M2I1D"


@pytest.fixture(scope="module")
def planted(tmp_path_factory):
    g = A.generate(tmp_path_factory.mktemp("map_align_planted"), SEED)
    g["out"] = A.map_reads(g["targets"], g["read_list"], eqx=True)
    return g


def test_alignments_of_planted_edits_are_sensible(planted):
    """60 reads of 200 - 600 bases with 8 % planted edits, both strands: every primary line's NM is at most what was planted in its read.
    A condition on SEED (unit cost, a band and waypoints need not find the planted alignment), not a tolerance."""
    g, out = planted, planted["out"]
    assert len(out["nm"]) >= 55 and {l.split("\t")[4] for l in out["paf"].splitlines()} == {"+", "-"}
    for name, nm in out["nm"].items():
        assert nm <= g["planted"][name], name
    assert sum(out["nm"].values()) > 0.5 * sum(g["planted"][n] for n in out["nm"])


def test_lines_agree_with_their_cigar(planted):
    out = planted["out"]
    for line, plain, other in zip(out["paf"].splitlines(), out["plain"].splitlines(), out["other"].splitlines()):
        f, p = line.split("\t"), plain.split("\t")
        assert f[:9] == p[:9] and f[11:15] == p[11:] and len(f) == 17
        t, q, n = A.cigar_spans(f[16][5:])
        assert f[16].startswith("cg:Z:") and (t, q) == (int(f[8]) - int(f[7]), int(f[3]) - int(f[2])) and n["M"] == 0
        assert int(f[9]) == n["="] and int(f[10]) == sum(n.values()) and f[15] == "NM:i:%d" % (n["X"] + n["I"] + n["D"])
        m = A.cigar_spans(other.split("\t")[16][5:])[2]
        assert m["M"] == n["="] + n["X"] and (m["I"], m["D"], m["="], m["X"]) == (n["I"], n["D"], 0, 0)
    a = out["align"]
    assert a["columns"] == a["matches"] + a["mismatches"] + a["inserted"] + a["deleted"] and a["lines"] == out["info"]["lines"]
    with pytest.raises(ValueError):
        A.map_reads(planted["targets"], planted["read_list"][:1], band=64)
    with pytest.raises(ValueError):
        A.map_reads(planted["targets"], planted["read_list"][:1], max_gap=65537)


def test_exports_and_header_agree():
    from tksm_amd import _lib
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "tksmseq.h")).read()
    assert "tksmseq_map_align" in _lib.SYMBOLS and re.search(r"\btksmseq_map_align\s*\(", header) and hasattr(lib, "tksmseq_map_align")
    assert ctypes.sizeof(_lib.AlignParams) == 8 and ctypes.sizeof(_lib.AlignInfo) == 80
    assert ctypes.sizeof(_lib.MapParams) == 56 and ctypes.sizeof(_lib.MapInfo) == 152
    for struct, cls in (("tksmseq_align_params", _lib.AlignParams), ("tksmseq_align_info", _lib.AlignInfo)):
        fields = re.search(rf"typedef struct {struct} \{{(.*?)\}} {struct};", header, re.S).group(1)
        fields = re.sub(r"/\*.*?\*/", "", fields, flags=re.S)
        names = [n.split("[")[0].strip() for part in re.findall(r"(?:uint64_t|int64_t|int32_t|float|double|const char\*)\s+([^;]+);", fields) for n in re.split(r",\s*", part.strip())]
        assert names == [n for n, _ in cls._fields_], struct
    assert [n for n, _ in _lib.AlignInfo._fields_][:9] == list(A.COUNTERS)
    host_h = open(os.path.join(ROOT, "tksm_amd", "csrc", "map_host.h")).read()
    assert int(re.search(r"MAP_ALN_MAX_GAP = (\d+)", host_h).group(1)) == A.MAX_GAP
    # the product does not import the specification, and the kernels of this mode use no floating point either
    for root, _, files in os.walk(os.path.join(ROOT, "tksm_amd")):
        for f in files:
            if f.endswith((".py", ".cpp", ".h", ".hip")):
                assert "map_align_spec" not in open(os.path.join(root, f), errors="replace").read(), f
    for name in ("map_align_kernels.hip", "map_align_kernels.h", "map_kernels.hip"):
        kernels = open(os.path.join(ROOT, "tksm_amd", "csrc", name)).read()
        assert not re.search(r"\b(float|double)\b", re.sub(r"//.*", "", kernels)), name
    import __graft_entry__ as g
    assert g.NO_SPILL_MAP_ALIGN == ("k_map_align_path", "k_map_align", "k_map_align_encode") and "k_map_chain" in g.NO_SPILL_MAP
    import inspect
    from tksm_amd.sequence import Sequencer
    sig = inspect.signature(Sequencer.map).parameters
    assert (sig["align"].default, sig["eqx"].default, sig["align_band"].default) == (False, False, 63)


def _module(*args):
    return subprocess.run([EXE, "map", *[str(a) for a in args]], capture_output=True, text=True)


def test_module_argument_checks_and_exit_codes(tmp_path):
    g = M.generate(tmp_path, seed=3, n_targets=2, n_reads=2)
    out = tmp_path / "o.paf"
    need = ["-r", g["ref"], "--reads", g["reads"], "-o", out, "--devices", "99"]      # (no such device: a call that got past the checks fails with 1)
    for args, what in ((["--eqx"], "--eqx"), (["--align-band", "5"], "--align-band"), (["--eqx", "--align-band", "5"], "--eqx")):
        r = _module(*need, *args)
        assert r.returncode == 2 and f"map: error: {what} needs -c" in r.stderr, r.stderr
    for bad in ("0", "64", "-1"):
        r = _module(*need, "-c", "--align-band", bad)
        assert r.returncode == 2 and "map: error: --align-band must be between 1 and 63" in r.stderr, r.stderr
    assert _module(*need, "-c", "--align-band", "wide").returncode == 2 and _module(*need, "-c", "--align-band").returncode == 2
    r = _module(*need, "-c", "--max-gap", "65537")
    assert r.returncode == 2 and "map: error: --max-gap must be at most 65536 with -c" in r.stderr
    # what is in range goes on to open the device
    for args in (["-c"], ["-c", "--eqx", "--align-band", "1"], ["-c", "--align-band=63", "--max-gap", "65536"], ["--max-gap", "65537"]):
        r = _module(*need, *args)
        assert r.returncode == 1 and "map: error" not in r.stderr, (args, r.stderr)
    assert not out.exists() and not os.path.exists(str(out) + ".tmp")
    text = _module("--help").stdout
    assert "-c [--eqx] [--align-band 63]" in text and "model-sequence" in text


@pytest.fixture(scope="module")
def sanitized(tmp_path_factory):
    """tools/sanitize_map_align_host.cpp built with ASan + UBSan and run: {key: [lines]} of what it printed"""
    d = tmp_path_factory.mktemp("map_align_sanitize")
    exe = d / "sanitize_map_align_host"
    csrc = os.path.join(ROOT, "tksm_amd", "csrc")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-I", csrc, "-o", str(exe),
                    os.path.join(ROOT, "tools", "sanitize_map_align_host.cpp"), os.path.join(csrc, "map_host.cpp"), os.path.join(csrc, "ms_host.cpp"),
                    os.path.join(csrc, "abund_host.cpp"), "-lz"], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, r.stderr
    out = {}
    for line in r.stdout.splitlines():
        key, _, rest = line.partition(" ")
        out.setdefault(key, []).append(rest)
    return out


def test_host_code_under_sanitizers(sanitized):
    s = sanitized
    ok = {l.split(" ")[0]: l.split(" ")[1] == "1" for l in s["check"]}
    assert [k for k, v in ok.items() if v] == ["defaults", "band1", "gap65536"] and len(ok) == 8
    assert all(l.split(" ")[1] == "1" or " ".join(l.split(" ")[2:]).startswith("map: ") for l in s["check"])
    mixed = "=====X===IIDXX===="
    head = "read/1\t200000\t%d\t%d\t%s\ttx\t300000\t10\t%d\t%d\t%d\t%d\ttp:A:%s\tcm:i:9\ts1:i:120\tNM:i:%d\tcg:Z:%s"

    def want(columns, eqx, rel, primary):
        n = {op: columns.count(op) for op in "=XID"}
        t, q = n["="] + n["X"] + n["D"], n["="] + n["X"] + n["I"]
        qs, qe = (4, 4 + q) if not rel else (200000 - 4 - q, 200000 - 4)
        return head % (qs, qe, "+-"[rel], 10 + t, n["="], len(columns), 60 if primary else 0, "P" if primary else "S", n["X"] + n["I"] + n["D"], A.cigar(columns, eqx))

    long1, long2 = "=" * 70000 + "D" + "I" * 66000, "=" * 40000 + "X" * 40000
    assert s["paf"] == [want(mixed, False, 0, True), want(mixed, True, 0, True), want(mixed, True, 1, False), want("=", False, 0, True), want("", False, 0, True),
                        want(long1, True, 0, True), want(long2, False, 1, True)]
    assert s["paf"][5].endswith("cg:Z:70000=1D66000I") and s["paf"][6].endswith("cg:Z:80000M")
    assert s["table"] == ["10 0 0 190", "11 7 12 2", "12 8 13 16", "13 9 14 17", "14 11 16 131072"] and s["table_end"] == ["14 8208"]
    small, large = (int(x) for x in s["bytes"][0].split(" "))
    assert small == 5 * (16 + 32 + 8) + 8 + 14 * 8 + 8208 * 4 and large == (1 << 31) * 56 + 8 + (1 << 36) + (1 << 34) + (1 << 37)
    budget = 128 << 20
    for l in s["waves"]:
        fixed, longest, lines, waves = (int(x) for x in l.split(" "))
        room = (budget - fixed) // ((longest + 1) * 16) if fixed < budget else 0
        assert waves == min(room // 4 * 4, 8192, (lines + 3) // 4 * 4), l
    assert {int(l.split(" ")[3]) for l in s["waves"]} >= {0, 4, 8, 8192}
