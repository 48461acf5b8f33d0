"""map --split without a device: the specification (tests/map_split_spec.py) against map_spec, map_align_spec and map_extend_spec where the
feature is off or has nothing to add, the properties of the lines it adds (intervals, tags, mapq), the crafted cases the device tests use,
recorded answers, glued reads of whole targets, and the interface: struct sizes, exported symbols, the Python signature and the module's
argument checks.  tests/test_map_split_gpu.py compares the device with the spec.

The tests of the specification alone (spec against spec, its properties, the crafted and recorded cases, glued whole targets, the ranges)
need tests/map_split_spec.py and nothing of the product: they pin the reference the device tests compare with.  The tests that need the
feature itself, and fail on a build without it, are test_exports_and_header_agree, test_python_refuses_split_options_without_split,
test_module_argument_checks_and_exit_codes and test_host_code_under_sanitizers here, and every test of tests/test_map_split_gpu.py."""
import ctypes
import inspect
import json
import os
import random
import re
import subprocess

import pytest

from conftest import ROOT

import map_align_spec as A
import map_extend_spec as X
import map_spec as M
import map_split_spec as S

EXE = os.path.join(ROOT, "tksm_amd", "tksm")
GOLDEN = os.path.join(ROOT, "tests", "golden", "map_split_known_answers.json")


@pytest.fixture(scope="module")
def generated(tmp_path_factory):
    """glued reads on 20 targets, error-free and with 5 % substitutions: the spec with and without split, and map_spec"""
    out = {}
    for error in (0.0, 0.05):
        g = S.generate(tmp_path_factory.mktemp("map_split_gen"), seed=7, n_targets=20, n_reads=100, lengths=(600, 1500), error=error)
        g["memo"] = {}
        g["on"] = S.map_reads(g["targets"], g["read_list"], memo=g["memo"])
        g["off"] = S.map_reads(g["targets"], g["read_list"], split=False, memo=g["memo"])
        g["base"] = M.map_reads(g["targets"], g["read_list"])
        out[error] = g
    return out


def rows_by_read(paf):
    out = {}
    for line in paf.splitlines():
        out.setdefault(line.split("\t")[0], []).append(line)
    return out


def tag(fields, name):
    hits = [f[5:] for f in fields[12:] if f.startswith(name + ":i:")]
    return int(hits[0]) if hits else None


def test_split_off_is_map_spec(generated):
    for g in generated.values():
        assert g["off"]["paf"] == g["base"]["paf"] and g["off"]["info"] == g["base"]["info"] and "split" not in g["off"]


def test_split_off_is_the_aligned_and_the_extended_spec(tmp_path):
    g = S.generate(tmp_path, seed=11, n_targets=4, n_reads=15, lengths=(300, 500), min_piece=150, error=0.03)
    for mode in (dict(align=True), dict(align=True, eqx=True)):
        off, want = S.map_reads(g["targets"], g["read_list"], split=False, **mode), A.map_reads(g["targets"], g["read_list"], **mode)
        assert off["paf"] == want["paf"] and off["align"] == want["align"] and off["info"] == want["info"]
    for mode in (dict(), dict(align=True, eqx=True)):
        off, want = S.map_reads(g["targets"], g["read_list"], split=False, extend=True, **mode), X.map_reads(g["targets"], g["read_list"], **mode)
        assert off["paf"] == want["paf"] and off["extend"] == want["extend"] and off["info"] == want["info"]
        assert not mode or off["align"] == want["align"]


def test_reads_without_a_supplementary_keep_their_lines(generated):
    for g in generated.values():
        on, base = rows_by_read(g["on"]["paf"]), rows_by_read(g["base"]["paf"])
        assert set(on) == set(base)
        untouched = [name for name in on if len([l for l in on[name] if "\ttp:A:P\t" in l]) == 1]
        assert 20 <= len(untouched) < len(on)
        for name in untouched:
            assert on[name] == base[name]


def test_primary_and_secondaries_are_map_specs(generated):
    for g in generated.values():
        on, base = rows_by_read(g["on"]["paf"]), rows_by_read(g["base"]["paf"])
        n_supp = 0
        for name, rows in on.items():
            n = len(base[name])
            strip = [re.sub(r"\tsn:i:\d+\tsi:i:\d+", "", l) for l in rows[:n]]
            assert strip == base[name]
            assert strip[1:] == rows[1:n]                                      # secondaries carry no tag
            assert all("\ttp:A:P\t" in l for l in rows[n:])
            n_supp += len(rows) - n
        s = g["on"]["split"]
        assert n_supp == s["supplementary"] > 50 and g["on"]["info"]["lines"] == g["base"]["info"]["lines"] + n_supp
        assert g["on"]["info"]["lines"] == g["on"]["info"]["mapped"] + g["on"]["info"]["secondary"] + s["supplementary"]
        assert s["rounds"] >= g["on"]["info"]["chained_groups"] + s["later_chains"] > g["on"]["info"]["chained_groups"]


def test_accepted_intervals_and_tags(generated):
    for g in generated.values():
        for name, rows in rows_by_read(g["on"]["paf"]).items():
            fields = [l.split("\t") for l in rows]
            p_lines = [f for f in fields if f[12] == "tp:A:P"]
            iv = [(int(f[2]), int(f[3])) for f in p_lines]
            for i in range(len(iv)):
                for j in range(i):
                    assert S.shared(iv[i], iv[j]) <= 30
            assert len(p_lines) <= 8
            if len(p_lines) == 1:
                assert all(len(f) == 15 for f in fields)
                continue
            assert all(tag(f, "sn") == len(p_lines) and f[15].startswith("sn:i:") and f[16].startswith("si:i:") and len(f) == 17 for f in p_lines)
            order = sorted(range(len(iv)), key=lambda i: (iv[i], i))
            assert [tag(p_lines[i], "si") for i in order] == list(range(len(iv)))
            assert all(len(f) == 15 for f in fields if f[12] == "tp:A:S")
            assert all(0 <= int(f[11]) <= 60 for f in fields)


def test_supplementary_lines_follow_alignment_and_extension(tmp_path):
    """-c and --extend change no selection: the same lines, and a supplementary line's CIGAR consumes exactly its intervals"""
    g = S.generate(tmp_path, seed=13, n_targets=5, n_reads=15, lengths=(300, 600), min_piece=150, error=0.04)
    memo = {}
    plain = S.map_reads(g["targets"], g["read_list"], memo=memo)
    assert plain["split"]["supplementary"] >= 5
    for mode in (dict(align=True, eqx=True), dict(extend=True), dict(align=True, extend=True)):
        out = S.map_reads(g["targets"], g["read_list"], memo=memo, **mode)
        assert out["split"] == plain["split"] and out["info"] == plain["info"]
        for line, short in zip(out["paf"].splitlines(), plain["paf"].splitlines()):
            f, fs = line.split("\t"), short.split("\t")
            n_tags = len(fs) - 12
            assert f[:2] == fs[:2] and f[4:7] == fs[4:7] and f[11:12 + n_tags] == fs[11:]
            assert int(f[2]) <= int(fs[2]) and int(f[3]) >= int(fs[3]) and int(f[7]) <= int(fs[7]) and int(f[8]) >= int(fs[8])
            if not mode.get("extend"):
                assert f[:9] == fs[:9]
            if mode.get("align"):
                assert f[-2].startswith("NM:i:") and len(f) == len(fs) + 2
                t, q, _ = A.cigar_spans(f[-1][5:])
                assert t == int(f[8]) - int(f[7]) and q == int(f[3]) - int(f[2])


def test_crafted_cases_reach_what_they_are_for():
    targets, reads, P = S.edge_case()
    memo = {}
    out = {name: S.map_reads(targets, reads, memo=memo, **v, **P) for name, v in S.VARIANTS.items()}
    rows = {name: rows_by_read(o["paf"]) for name, o in out.items()}
    lines = out["defaults"]["lines"]
    k = P["k"]
    # every piece of a tile case with at least min_count anchors is a chain of its own, written by descending size (the first four: `chains`)
    index = M.build_index([s for _, s in targets], k, P["w"])[0]
    for sizes in S.TILE_SIZES:
        name = "tile_" + "_".join(map(str, sizes))
        for strand in "fr":
            got = [c["cnt"] for _, _, kind, c in lines[name + strand]]
            assert got == sorted((n for n in sizes if n >= P["min_count"]), reverse=True)[:4], (sizes, got)
            groups = A.groups_of(dict(reads)[name + strand], index, dict(M.DEFAULTS, **P))
            assert [len(a) for a in groups.values()] == [sum(sizes)]
    # the group sizes around the tiles, and the list positions [a, b) that round 1 removes: b (or a, when b is the end) at 63, 64 and 65
    assert {sum(s) for s in S.TILE_SIZES} == {63, 64, 65, 128, 129}
    edges = set()
    for sizes in S.TILE_SIZES:
        a = sum(sizes[:sizes.index(max(sizes))])
        edges.add((sum(sizes), a if a + max(sizes) == sum(sizes) and a else a + max(sizes)))
    assert edges >= {(n, e) for n in (128, 129) for e in (63, 64, 65)}
    # a round that leaves min_count - 1, min_count and no anchors
    assert len(lines["tile_61_2f"]) == 1 and len(lines["tile_60_3f"]) == 2 and len(lines["tile_63f"]) == 1 and lines["tile_60_3f"][1][3]["cnt"] == 3
    # chains = 1: no later round; the six pieces of `many` reach chains = 2 and 4, and 16 takes them all
    assert out["chains_1"]["split"]["later_chains"] == 0 and out["chains_1"]["split"]["rounds"] == out["chains_1"]["info"]["chained_groups"]
    assert [len(rows[v]["manyf"]) for v in ("chains_1", "chains_2", "defaults", "limits")] == [1, 2, 4, 6]
    # a link of a later round over more than 64 original anchors
    groups = A.groups_of(dict(reads)["spanf"], index, dict(M.DEFAULTS, **P))
    anchors = groups[([n for n, _ in targets].index("span"), 0)]
    later = lines["spanf"][1][3]
    at = [anchors.index(a) for a in later["anchors"]]
    assert later["round"] == 1 and 64 < max(b - a for a, b in zip(at, at[1:])) <= 90 and later["cnt"] >= 90
    # read intervals that share exactly `overlap` and one more
    assert len(rows["defaults"]["ov30f"]) == 2 and len(rows["defaults"]["ov31f"]) == 1 and len(rows["overlap_0"]["ov30f"]) == 1
    f = [l.split("\t") for l in rows["defaults"]["ov30f"]]
    assert S.shared((int(f[0][2]), int(f[0][3])), (int(f[1][2]), int(f[1][3]))) == 30
    assert out["defaults"]["split"]["rejected_overlap"] > out["limits"]["split"]["rejected_overlap"] == 0
    # equal scores across targets, strands and rounds
    eq = [(t, rel, kind, c["round"], c["score"]) for t, rel, kind, c in lines["eqf"]]
    assert eq == [("eq_a", 0, "primary", 0, 150), ("eq_a", 1, "secondary", 0, 150), ("eq_b", 0, "secondary", 0, 150), ("eq_b", 1, "secondary", 0, 150),
                  ("eq_a", 0, "supplementary", 1, 150)]
    assert [l.split("\t")[11] for l in rows["defaults"]["eqf"]] == ["0"] * 5              # (the supplementary line's s2 is a chain of its own score)
    # segments - 1 acceptances with a further candidate waiting
    five = {v: sum("\ttp:A:P\t" in l for l in rows[v]["fivef"]) for v in ("segments_2", "segments_3", "defaults")}
    assert five == {"segments_2": 2, "segments_3": 3, "defaults": 3} and sum("\ttp:A:S" in l for l in rows["defaults"]["fivef"]) == 2
    assert len(rows["limits"]["eqf"]) == 8


def test_recorded_cases():
    cases = json.load(open(GOLDEN))
    targets, reads, P = S.edge_case()
    assert {c["variant"] for c in cases} == set(S.VARIANTS) and len(cases) == 2 * len(S.VARIANTS)
    memo = {}
    for c in cases:
        out = S.map_reads(targets, reads, memo=memo, **c["mode"], **S.VARIANTS[c["variant"]], **P)
        assert out["paf"] == c["paf"] and out["split"] == c["split"] and out["info"] == c["info"], (c["variant"], c["mode"])


def test_glued_whole_targets_give_a_line_a_piece():
    """error-free reads glued from whole, distinct random targets: one of 1 000 to 1 200 letters and one or two of 520 to 700 (longer than the
    bandwidth; below 0.8 of the longest, so that step A writes none of them as a secondary): as many tp:A:P lines as pieces, each on its own
    target and over all of it up to the first and last minimizer"""
    rs = random.Random(2024)
    targets, reads, truth = [], [], {}
    for r in range(30):
        n = 2 + r % 2
        mine = [("g%02d_%d" % (r, i), M.random_seq(rs, rs.randint(1000, 1200) if i == r % n else rs.randint(520, 700))) for i in range(n)]
        targets += mine
        text = "".join(M.revcomp(seq) if (r + i) % 3 == 0 else seq for i, (_, seq) in enumerate(mine))
        reads.append(("glued%02d" % r, text if r % 5 else M.revcomp(text)))
        truth["glued%02d" % r] = {name for name, _ in mine}
    out = S.map_reads(targets, reads)
    assert out["info"]["secondary"] == 0 and out["split"]["supplementary"] == sum(len(v) - 1 for v in truth.values()) == 45
    for name, rows in rows_by_read(out["paf"]).items():
        f = [l.split("\t") for l in rows]
        assert {x[5] for x in f} == truth[name] and len(f) == len(truth[name]) and all(x[12] == "tp:A:P" for x in f)
        assert all(int(x[11]) == 60 for x in f[1:]) and 0 < int(f[0][11]) < 60          # (the primary's mapq is step A's: s2 is the next round-1 chain)
        assert all(int(x[7]) < 40 and int(x[6]) - int(x[8]) < 40 for x in f)
    assert abs(out["estimate"] - 45 / (30 + 45 - 1)) < 1e-12


def test_parameter_ranges():
    targets, reads, P = S.edge_case()
    for bad in (dict(split_chains=0), dict(split_chains=17), dict(split_overlap=-1), dict(split_overlap=1 << 31), dict(split_segments=1), dict(split_segments=65)):
        with pytest.raises(ValueError):
            S.map_reads(targets, reads[:1], **bad, **P)


def test_exports_and_header_agree():
    from tksm_amd import _lib
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "tksmseq.h")).read()
    assert "tksmseq_map_split" in _lib.SYMBOLS and re.search(r"\btksmseq_map_split\s*\(", header) and hasattr(lib, "tksmseq_map_split")
    assert ctypes.sizeof(_lib.SplitParams) == 16 and ctypes.sizeof(_lib.SplitInfo) == 48
    assert ctypes.sizeof(_lib.ExtendParams) == 16 and ctypes.sizeof(_lib.ExtendInfo) == 72 and ctypes.sizeof(_lib.MapParams) == 56 and ctypes.sizeof(_lib.MapInfo) == 152
    for struct, cls in (("tksmseq_split_params", _lib.SplitParams), ("tksmseq_split_info", _lib.SplitInfo)):
        fields = re.search(rf"typedef struct {struct} \{{(.*?)\}} {struct};", header, re.S).group(1)
        fields = re.sub(r"/\*.*?\*/", "", fields, flags=re.S)
        names = [n.split("[")[0].strip() for part in re.findall(r"(?:uint64_t|int64_t|int32_t|float|double)\s+([^;]+);", fields) for n in re.split(r",\s*", part.strip())]
        assert names == [n for n, _ in cls._fields_], struct
    assert [n for n, _ in _lib.SplitInfo._fields_][:5] == list(S.COUNTERS)
    assert "map, split reads:" in header and "choices, not measurements" in header.split("map, split reads:")[1]
    argtypes = lib.tksmseq_map_split.argtypes
    assert len(argtypes) == 11 and argtypes[4]._type_ is _lib.SplitParams and argtypes[10]._type_ is _lib.SplitInfo
    # the product does not import the specification, and the kernels of this mode use no floating point
    for root, _, files in os.walk(os.path.join(ROOT, "tksm_amd")):
        for f in files:
            if f.endswith((".py", ".cpp", ".h", ".hip")):
                assert "map_split_spec" not in open(os.path.join(root, f), errors="replace").read(), f
    for name in ("map_split_kernels.hip", "map_split_kernels.h"):
        kernels = open(os.path.join(ROOT, "tksm_amd", "csrc", name)).read()
        assert not re.search(r"\b(float|double)\b", re.sub(r"//.*", "", kernels)), name
    import __graft_entry__ as g
    assert g.NO_SPILL_MAP_SPLIT == ("k_map_chain_split", "k_map_select_split")
    from tksm_amd.sequence import Sequencer
    sig = inspect.signature(Sequencer.map).parameters
    assert (sig["split"].default, sig["split_chains"].default, sig["split_overlap"].default, sig["split_segments"].default) == (False, 4, 30, 8)
    assert tuple(sig[k].default for k in S.DEFAULTS) == tuple(S.DEFAULTS.values())


def test_python_refuses_split_options_without_split():
    from tksm_amd.sequence import Sequencer
    for bad in (dict(split_chains=2), dict(split_overlap=0), dict(split_segments=3)):
        with pytest.raises(ValueError, match="split=True"):
            Sequencer.map(None, "reads.fq", "out.paf", **bad)                  # (refused before the context is touched)


def _module(*args):
    return subprocess.run([EXE, "map", *[str(a) for a in args]], capture_output=True, text=True)


def test_module_argument_checks_and_exit_codes(tmp_path):
    g = M.generate(tmp_path, seed=3, n_targets=2, n_reads=2)
    out = tmp_path / "o.paf"
    need = ["-r", g["ref"], "--reads", g["reads"], "-o", out, "--devices", "99"]      # (no such device: a call that got past the checks fails with 1)
    for args, what in ((["--split-chains", "2"], "--split-chains"), (["--split-overlap", "5"], "--split-overlap"), (["--split-segments", "5"], "--split-segments"),
                       (["-c", "--extend", "--split-segments", "5", "--split-chains", "5"], "--split-segments")):
        r = _module(*need, *args)
        assert r.returncode == 2 and f"map: error: {what} needs --split" in r.stderr, r.stderr
    for option, bad, text in (("--split-chains", ("0", "17", "-1"), "between 1 and 16"), ("--split-overlap", ("-1", "2147483648"), "between 0 and 2147483647"),
                              ("--split-segments", ("1", "65"), "between 2 and 64")):
        for value in bad:
            r = _module(*need, "--split", option, value)
            assert r.returncode == 2 and f"map: error: {option} must be {text}" in r.stderr, r.stderr
    assert _module(*need, "--split", "--split-chains", "many").returncode == 2 and _module(*need, "--split", "--split-overlap").returncode == 2
    # what is in range goes on to open the device
    for args in (["--split"], ["--split", "--split-chains", "16", "--split-overlap", "2147483647", "--split-segments", "64"],
                 ["-c", "--eqx", "--extend", "--split", "--split-chains=1", "--split-overlap", "0", "--split-segments", "2"]):
        r = _module(*need, *args)
        assert r.returncode == 1 and "map: error" not in r.stderr, (args, r.stderr)
    assert not out.exists() and not os.path.exists(str(out) + ".tmp")
    text = _module("--help").stdout
    assert "[--split [--split-chains 4] [--split-overlap 30] [--split-segments 8]]" in text and "[--extend [--ext-band 31] [--ext-drop 40] [--ext-max 2000]]" in text


def test_host_code_under_sanitizers(tmp_path):
    """tools/sanitize_map_split_host.cpp built with ASan + UBSan and run: the checks, the tagged lines, the ranks and the budget arithmetic"""
    exe = tmp_path / "sanitize_map_split_host"
    csrc = os.path.join(ROOT, "tksm_amd", "csrc")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-I", csrc, "-o", str(exe),
                    os.path.join(ROOT, "tools", "sanitize_map_split_host.cpp"), os.path.join(csrc, "map_host.cpp"), os.path.join(csrc, "ms_host.cpp"),
                    os.path.join(csrc, "abund_host.cpp"), "-lz"], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, r.stderr
    s = {}
    for line in r.stdout.splitlines():
        key, _, rest = line.partition(" ")
        s.setdefault(key, []).append(rest)
    ok = {l.split(" ")[0]: l.split(" ")[1] == "1" for l in s["check"]}
    assert [k for k, v in ok.items() if v] == ["defaults", "lowest", "highest"] and len(ok) == 9
    assert all(l.split(" ")[1] == "1" or " ".join(l.split(" ")[2:]).startswith("map: split ") for l in s["check"])
    head = "read/1\t1000\t100\t300\t+\ttx\t5000\t40\t240\t190\t200\t60\ttp:A:P\tcm:i:9\ts1:i:120"
    assert s["paf"] == [head, head + "\tsn:i:3\tsi:i:2", head.replace("\t190\t200\t", "\t180\t205\t") + "\tsn:i:3\tsi:i:2\tNM:i:25\tcg:Z:100M5I100M",
                        head.replace("\t190\t200\t", "\t180\t205\t") + "\tNM:i:25\tcg:Z:100M5I100M"]
    assert s["ranks"] == ["2 0 3 1", "0", ""]
    assert s["bytes"] == ["%d %d %d" % (4 + (4 * 64 + 2) // 3, 4 + 16 * 64, 4 + 64)]
