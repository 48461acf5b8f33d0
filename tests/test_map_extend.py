"""map --extend without a device: the specification (tests/map_extend_spec.py) against an independent full-matrix maximum and hand-worked
cases, the accuracy it is for on the generator's reads with 10 % error, the lines it writes, and the interface: struct sizes, exported
symbols, the Python signature and the module's argument checks.  tests/test_map_extend_gpu.py compares the device with the spec."""
import ctypes
import inspect
import json
import os
import random
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

import map_align_spec as A
import map_extend_spec as X
import map_spec as M

EXE = os.path.join(ROOT, "tksm_amd", "tksm")
GOLDEN = os.path.join(ROOT, "tests", "golden", "map_extend_known_answers.json")


def best_prefix_score(T, Q):
    """the largest score of an alignment of a prefix of T with a prefix of Q (at least 0: the empty one), over the full matrix, row by row"""
    H = np.zeros((len(T) + 1, len(Q) + 1), dtype=np.int64)
    H[0, :] = -2 * np.arange(len(Q) + 1)
    for i in range(1, len(T) + 1):
        H[i, 0] = -2 * i
        for j in range(1, len(Q) + 1):
            hit = T[i - 1] == Q[j - 1] and T[i - 1] in "ACGT"
            H[i, j] = max(H[i - 1, j - 1] + (1 if hit else -2), H[i - 1, j] - 2, H[i, j - 1] - 2)
    return int(H.max())


def score_of(T, Q, columns):
    """(score, matches, target letters, read letters) of columns over = X I D, each checked against the letters"""
    i = j = score = m = 0
    for c in columns:
        if c in "=X":
            assert (T[i] == Q[j] and T[i] in "ACGT") == (c == "=")
            i, j, score, m = i + 1, j + 1, score + (1 if c == "=" else -2), m + (c == "=")
        elif c == "D":
            i, score = i + 1, score - 2
        else:
            j, score = j + 1, score - 2
    return score, m, i, j


def test_spec_against_a_full_matrix_maximum():
    """with a band and a drop that never bind the best cell's score is the plain maximum over all prefixes, and the columns lead to it"""
    rs = random.Random(17)
    n_moved = 0
    for n in range(300):
        T = "".join(rs.choice("ACGTN" if n % 7 == 0 else "ACGT") for _ in range(rs.randint(0, 40)))
        Q = A.plant(rs, T, rs.choice((0.0, 0.1, 0.3)))[0][:40] if n % 3 else "".join(rs.choice("ACGT") for _ in range(rs.randint(0, 40)))
        e = X.extend(T, Q, 63, 1000)
        assert e["score"] == (best_prefix_score(T, Q) if T and Q else 0), (T, Q)
        assert score_of(T, Q, e["columns"]) == (e["score"], e["m"], e["ei"], e["ej"])
        assert (e["score"] > 0) == (e["ei"] + e["ej"] > 0) and e["steps"] <= len(T) + len(Q)
        n_moved += e["score"] > 0
    assert n_moved > 200


def test_band_and_drop_only_ever_lose_score():
    rs = random.Random(18)
    for n in range(100):
        T = M.random_seq(rs, rs.randint(1, 60))
        Q = A.plant(rs, T, 0.15)[0]
        full = X.extend(T, Q, 63, 1000)
        for B, Z in ((1, 1000), (3, 1000), (63, 1), (63, 6), (2, 4)):
            e = X.extend(T, Q, B, Z)
            assert 0 <= e["score"] <= full["score"] and abs(e["ei"] - e["ej"]) <= B and e["steps"] <= full["steps"]
            assert score_of(T, Q, e["columns"]) == (e["score"], e["m"], e["ei"], e["ej"])


def test_recorded_cases():
    cases = json.load(open(GOLDEN))
    assert {c["name"] for c in cases} == {"tie_across_anti_diagonals", "tie_within_an_anti_diagonal", "indel_at_the_band_edge", "indel_past_the_band_edge",
                                          "penalty_equal_to_the_drop", "penalty_one_above_the_drop", "no_target_letters", "no_read_letters"}
    for c in cases:
        e = X.extend(c["T"], c["Q"], c["B"], c["Z"])
        assert {k: e[k] for k in ("ei", "ej", "score", "m", "columns", "steps")} == {k: c[k] for k in ("ei", "ej", "score", "m", "columns", "steps")}, c["name"]
        assert score_of(c["T"], c["Q"], c["columns"]) == (c["score"], c["m"], c["ei"], c["ej"])


@pytest.fixture(scope="module")
def generated(tmp_path_factory):
    """the generator call of the issue's table, at error 0 and 0.10, mapped with the extension"""
    out = {}
    for error in (0.0, 0.10):
        g = M.generate(tmp_path_factory.mktemp("map_extend_gen"), seed=7, n_targets=20, n_reads=150, lengths=(800, 2000), min_read=400, error=error)
        g["out"] = X.map_reads(g["targets"], g["read_list"])
        out[error] = g
    return out


def end_errors(g, paf):
    """per primary line on the true target: (|tstart - a| + |b - tend|, the bases the line ends outside the truth)"""
    out = []
    for line in paf.splitlines():
        f = line.split("\t")
        tname, _, a, b = g["truth"][f[0]]
        if f[12] == "tp:A:P" and f[5] == tname:
            out.append((abs(int(f[7]) - a) + abs(b - int(f[8])), max(a - int(f[7]), int(f[8]) - b, 0)))
    return out


def test_extended_lines_end_where_the_molecule_ends(generated):
    exact, noisy = generated[0.0], generated[0.10]
    errors = end_errors(exact, exact["out"]["paf"])
    assert len(errors) == 150 and all(e == (0, 0) for e in errors)
    errors, chains = end_errors(noisy, noisy["out"]["paf"]), end_errors(noisy, noisy["out"]["base"])
    mean = sum(e for e, _ in errors) / len(errors)
    print("mean |tstart - a| + |b - tend| at error 0.10: %.2f extended, %.1f chains alone; at most %d bases outside the truth" %
          (mean, sum(e for e, _ in chains) / len(chains), max(o for _, o in errors)))
    assert len(errors) == len(chains) >= 140 and mean < 3 and sum(e for e, _ in chains) / len(chains) > 50
    assert max(o for _, o in errors) <= 10


def test_lines_keep_what_the_extension_may_not_touch(generated):
    g = generated[0.10]
    new, old = g["out"]["paf"].splitlines(), g["out"]["base"].splitlines()
    assert len(new) == len(old) == g["out"]["extend"]["lines"]
    for x, y, (left, right) in zip(new, old, g["out"]["moves"]):
        fx, fy = x.split("\t"), y.split("\t")
        assert fx[:2] == fy[:2] and fx[4:7] == fy[4:7] and fx[11:] == fy[11:] and len(fx) == 15
        assert int(fx[7]) == int(fy[7]) - left["ei"] and int(fx[8]) == int(fy[8]) + right["ei"]
        assert int(fx[3]) - int(fx[2]) == int(fy[3]) - int(fy[2]) + left["ej"] + right["ej"]
        assert int(fx[9]) == int(fy[9]) + left["m"] + right["m"] and int(fx[10]) == max(int(fx[8]) - int(fx[7]), int(fx[3]) - int(fx[2]))
    x = g["out"]["extend"]
    assert x["ends_moved"] <= 2 * x["lines"] and x["matches"] <= min(x["target_gained"], x["read_gained"]) and x["cells"] >= x["antidiagonals"] > x["longest"] > 0


def test_aligned_lines_agree_with_their_cigar(tmp_path):
    g = M.generate(tmp_path, seed=11, n_targets=3, n_reads=12, lengths=(300, 500), min_read=150, error=0.08)
    memo = {}
    plain = X.map_reads(g["targets"], g["read_list"], memo=memo, secondary_ratio=0.0)
    for eqx in (False, True):
        out = X.map_reads(g["targets"], g["read_list"], align=True, eqx=eqx, memo=memo, secondary_ratio=0.0)
        assert out["extend"] == plain["extend"] and len(out["paf"].splitlines()) == len(plain["paf"].splitlines()) > 0
        for line, short, base in zip(out["paf"].splitlines(), plain["paf"].splitlines(), out["base"].splitlines()):
            f, fs, fb = line.split("\t"), short.split("\t"), base.split("\t")
            t, q, n = A.cigar_spans(f[-1][5:])
            assert f[:9] == fs[:9] and f[11:15] == fs[11:15] and t == int(f[8]) - int(f[7]) and q == int(f[3]) - int(f[2])
            assert int(f[10]) == sum(n.values()) and int(f[-2][5:]) == int(f[10]) - int(f[9]) >= int(fb[-2][5:])
            assert not eqx or (int(f[9]) == n["="] and int(f[-2][5:]) == n["X"] + n["I"] + n["D"] and not n["M"])
    for bad in (dict(ext_band=0), dict(ext_band=64), dict(ext_drop=0), dict(ext_drop=1001), dict(ext_max=0), dict(ext_max=32769)):
        with pytest.raises(ValueError):
            X.map_reads(g["targets"], g["read_list"][:1], **bad)


def test_exports_and_header_agree():
    from tksm_amd import _lib
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "tksmseq.h")).read()
    assert "tksmseq_map_extend" in _lib.SYMBOLS and re.search(r"\btksmseq_map_extend\s*\(", header) and hasattr(lib, "tksmseq_map_extend")
    assert ctypes.sizeof(_lib.ExtendParams) == 16 and ctypes.sizeof(_lib.ExtendInfo) == 72
    assert ctypes.sizeof(_lib.AlignParams) == 8 and ctypes.sizeof(_lib.AlignInfo) == 80 and ctypes.sizeof(_lib.MapParams) == 56 and ctypes.sizeof(_lib.MapInfo) == 152
    for struct, cls in (("tksmseq_extend_params", _lib.ExtendParams), ("tksmseq_extend_info", _lib.ExtendInfo)):
        fields = re.search(rf"typedef struct {struct} \{{(.*?)\}} {struct};", header, re.S).group(1)
        fields = re.sub(r"/\*.*?\*/", "", fields, flags=re.S)
        names = [n.split("[")[0].strip() for part in re.findall(r"(?:uint64_t|int64_t|int32_t|float|double)\s+([^;]+);", fields) for n in re.split(r",\s*", part.strip())]
        assert names == [n for n, _ in cls._fields_], struct
    assert [n for n, _ in _lib.ExtendInfo._fields_][:8] == list(X.COUNTERS)
    assert '"map, end extension"' in header or "map, end extension:" in header
    assert "no end extension unless --extend" in header
    # the product does not import the specification, and the kernels of this mode use no floating point
    for root, _, files in os.walk(os.path.join(ROOT, "tksm_amd")):
        for f in files:
            if f.endswith((".py", ".cpp", ".h", ".hip")):
                assert "map_extend_spec" not in open(os.path.join(root, f), errors="replace").read(), f
    for name in ("map_extend_kernels.hip", "map_extend_kernels.h"):
        kernels = open(os.path.join(ROOT, "tksm_amd", "csrc", name)).read()
        assert not re.search(r"\b(float|double)\b", re.sub(r"//.*", "", kernels)), name
    import __graft_entry__ as g
    assert g.NO_SPILL_MAP_EXTEND == ("k_map_extend", "k_map_extend_trace")
    from tksm_amd.sequence import Sequencer
    sig = inspect.signature(Sequencer.map).parameters
    assert (sig["extend"].default, sig["ext_band"].default, sig["ext_drop"].default, sig["ext_max"].default) == (False, 31, 40, 2000)
    assert (sig["ext_band"].default, sig["ext_drop"].default, sig["ext_max"].default) == tuple(X.DEFAULTS[k] for k in ("ext_band", "ext_drop", "ext_max"))


def test_python_refuses_ext_options_without_extend():
    from tksm_amd.sequence import Sequencer
    for bad in (dict(ext_band=5), dict(ext_drop=10), dict(ext_max=100)):
        with pytest.raises(ValueError, match="extend=True"):
            Sequencer.map(None, "reads.fq", "out.paf", **bad)              # (refused before the context is touched)


def _module(*args):
    return subprocess.run([EXE, "map", *[str(a) for a in args]], capture_output=True, text=True)


def test_module_argument_checks_and_exit_codes(tmp_path):
    g = M.generate(tmp_path, seed=3, n_targets=2, n_reads=2)
    out = tmp_path / "o.paf"
    need = ["-r", g["ref"], "--reads", g["reads"], "-o", out, "--devices", "99"]      # (no such device: a call that got past the checks fails with 1)
    for args, what in ((["--ext-band", "5"], "--ext-band"), (["--ext-drop", "5"], "--ext-drop"), (["--ext-max", "5"], "--ext-max"),
                       (["-c", "--ext-max", "5", "--ext-band", "5"], "--ext-max")):
        r = _module(*need, *args)
        assert r.returncode == 2 and f"map: error: {what} needs --extend" in r.stderr, r.stderr
    for option, bad, text in (("--ext-band", ("0", "64", "-1"), "between 1 and 63"), ("--ext-drop", ("0", "1001"), "between 1 and 1000"),
                              ("--ext-max", ("0", "32769"), "between 1 and 32768")):
        for value in bad:
            r = _module(*need, "--extend", option, value)
            assert r.returncode == 2 and f"map: error: {option} must be {text}" in r.stderr, r.stderr
    assert _module(*need, "--extend", "--ext-band", "wide").returncode == 2 and _module(*need, "--extend", "--ext-drop").returncode == 2
    # what is in range goes on to open the device
    for args in (["--extend"], ["--extend", "--ext-band", "63", "--ext-drop", "1000", "--ext-max", "32768"], ["-c", "--eqx", "--extend", "--ext-band=1", "--ext-drop", "1", "--ext-max", "1"]):
        r = _module(*need, *args)
        assert r.returncode == 1 and "map: error" not in r.stderr, (args, r.stderr)
    assert not out.exists() and not os.path.exists(str(out) + ".tmp")
    text = _module("--help").stdout
    assert "-c [--eqx] [--align-band 63]" in text and "[--extend [--ext-band 31] [--ext-drop 40] [--ext-max 2000]]" in text


def test_host_code_under_sanitizers(tmp_path):
    """tools/sanitize_map_extend_host.cpp built with ASan + UBSan and run: the checks, the joined lines and the budget arithmetic"""
    exe = tmp_path / "sanitize_map_extend_host"
    csrc = os.path.join(ROOT, "tksm_amd", "csrc")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-I", csrc, "-o", str(exe),
                    os.path.join(ROOT, "tools", "sanitize_map_extend_host.cpp"), os.path.join(csrc, "map_host.cpp"), os.path.join(csrc, "ms_host.cpp"),
                    os.path.join(csrc, "abund_host.cpp"), "-lz"], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, r.stderr
    s = {}
    for line in r.stdout.splitlines():
        key, _, rest = line.partition(" ")
        s.setdefault(key, []).append(rest)
    ok = {l.split(" ")[0]: l.split(" ")[1] == "1" for l in s["check"]}
    assert [k for k, v in ok.items() if v] == ["defaults", "lowest", "highest"] and len(ok) == 10
    assert all(l.split(" ")[1] == "1" or " ".join(l.split(" ")[2:]).startswith("map: extend ") for l in s["check"])
    mid = "=" * 20 + "X" + "=" * 5 + "I" + "=" * 9
    parts = [("==X==", mid, "=D==="), ("==XX", "X" + mid + "I", "I=="), ("", mid, "==="), ("=I=", mid, ""), ("", mid, ""), ("=" * 70000 + "D", mid, "X" + "=" * 66000)]
    want, plain = [], []
    for eqx in (False, True):
        for rel in (0, 1):
            for left, chain, right in parts:
                n = {op: chain.count(op) for op in "=XID"}
                gained = [(p.count("=") + p.count("X") + p.count("D"), p.count("=") + p.count("X") + p.count("I"), p.count("=")) for p in (left, right)]
                columns = left + chain + right
                tstart, tend = 100000 - gained[0][0], 100000 + n["="] + n["X"] + n["D"] + gained[1][0]
                qs, qe = 90000 - gained[0][1], 90000 + n["="] + n["X"] + n["I"] + gained[1][1]
                head = "read/1\t200000\t%d\t%d\t%s\ttx\t300000" % ((qs, qe, "+") if not rel else (200000 - qe, 200000 - qs, "-")) + "\t%d\t%d" % (tstart, tend)
                tags = "\t60\ttp:A:P\tcm:i:9\ts1:i:120"
                want.append(head + "\t%d\t%d" % (columns.count("="), len(columns)) + tags + "\tNM:i:%d\tcg:Z:%s" % (len(columns) - columns.count("="), A.cigar(columns, eqx)))
                plain.append(head + "\t%d\t%d" % (101 + gained[0][2] + gained[1][2], max(tend - tstart, qe - qs)) + tags)
    assert s["paf"] == want and s["plain"] == plain
    assert s["bytes"] == ["%d %d %d" % (10 * 48 + 16, 10 * 48 + 16 + 7 * 80 + 400 + 400, (1 << 32) * 128 + 16 + (1 << 35) + (1 << 37))]
