"""barcode-match without a GPU: the specification (tests/barcode_spec.py) against a case worked out by hand
(tests/golden/barcode_match_known_answers.json), its infix distance against brute force, its matches file through the reader of
`abundance --lr-br`, a round trip of reads built from strings, the generator's planted classes, the ABI and the module's argument checks."""
import ctypes
import json
import os
import random
import re
import subprocess

import pytest

from conftest import GOLDEN, ROOT

import abundance_spec
import barcode_spec as B

EXE = os.path.join(ROOT, "tksm_amd", "tksm")
KNOWN = json.load(open(os.path.join(GOLDEN, "barcode_match_known_answers.json")))


def write_known(d):
    paths = {"reads": os.path.join(str(d), "known.fq"), "whitelist": os.path.join(str(d), "known.txt")}
    for what, path in paths.items():
        with open(path, "w") as f:
            f.write(KNOWN[what])
    return paths


def levenshtein(a, b):
    prev = list(range(len(b) + 1))
    for i in range(1, len(a) + 1):
        cur = [i] + [0] * len(b)
        for j in range(1, len(b) + 1):
            cur[j] = min(prev[j] + 1, cur[j - 1] + 1, prev[j - 1] + (a[i - 1] != b[j - 1] or a[i - 1] not in B.ACGT))
        prev = cur
    return prev[-1]


@pytest.fixture(scope="module")
def generated(tmp_path_factory):
    d = tmp_path_factory.mktemp("barcode_cpu")
    g = B.generate(d, seed=7)
    g["out"] = B.run(g["reads"], g["whitelist"])
    return g


def test_specification_gives_the_hand_counted_files(tmp_path):
    p = write_known(tmp_path)
    out = B.run(p["reads"], p["whitelist"], **KNOWN["params"])
    for what in ("matches", "segments", "selected", "info"):
        assert out[what] == KNOWN[what], what
    (tmp_path / "m.tsv").write_text(out["matches"])
    assert abundance_spec.parse_lr_br(str(tmp_path / "m.tsv")) == KNOWN["lr_br"]


def test_infix_against_brute_force_over_all_substrings():
    rs = random.Random(5)
    for _ in range(300):
        P = "".join(rs.choice("ACGT") for _ in range(rs.randint(1, 7)))
        T = "".join(rs.choice("ACGTN") for _ in range(rs.randint(0, 12)))
        every = {(a, b): levenshtein(P, T[a:b]) for b in range(len(T) + 1) for a in range(b + 1)}
        d = min(every.values())
        e = min(b for (a, b), v in every.items() if v == d)
        assert B.infix(P, T) == (d, e), (P, T)
    for _ in range(40):
        L, T = rs.randint(4, 9), "".join(rs.choice("ACGTN") for _ in range(rs.randint(0, 20)))
        pats = ["".join(rs.choice("ACGT") for _ in range(L)) for _ in range(7)]
        assert list(B.infix_many(pats, T)) == [B.infix(p, T)[0] for p in pats]


def test_matches_file_through_the_reader_of_abundance(generated, tmp_path):
    (tmp_path / "m.tsv").write_text(generated["out"]["matches"])
    rows = [l.split("\t") for l in generated["out"]["matches"].splitlines()]
    assert all(len(r) == 5 for r in rows) and len(rows) > 100
    got = abundance_spec.parse_lr_br(str(tmp_path / "m.tsv"))
    assert got == {r[0]: r[4] for r in rows if r[2] == "1"} and 0 < len(got) < len(rows)


def test_generator_plants_every_class(generated):
    g, out = generated, generated["out"]
    p, L = g["params"], g["L"]
    m = {l.split("\t")[0]: l.split("\t") for l in out["matches"].splitlines()}
    s = {l.split("\t")[0]: l.split("\t") for l in out["segments"].splitlines()}
    exact = dict(l.split("\t") for l in out["selected"].splitlines())
    c = g["classes"]
    wanted = ("forward", "reverse", "adapter_at_max", "adapter_over_max", "adapter_ends_at_window", "adapter_ends_past_window", "adapter_both_ends",
              "shorter_than_adapter", "ends_inside_barcode", "ends_after_barcode", "adapter_with_n", "barcode_substitution", "barcode_insertion",
              "barcode_deletion", "barcode_at_max_errors", "barcode_over_max_errors", "barcode_with_n", "lower_case", "two_tied", "more_than_eight_tied",
              "homopolymer", "exact_at_min", "exact_below_min", "never_seen", "no_adapter")
    assert all(c.get(k) for k in wanted), [k for k in wanted if not c.get(k)]
    one = lambda k: c[k][0]
    assert all(s[n][2] == "+" for n in c["forward"]) and all(s[n][2] == "-" for n in c["reverse"])
    assert int(s[one("adapter_at_max")][1]) == p["max_adapter_errors"] and one("adapter_over_max") not in s
    assert s[one("adapter_ends_at_window")][1] == "0" and int(s[one("adapter_ends_at_window")][3]) == p["window"] - p["pad"]
    assert s[one("adapter_ends_past_window")][1] == "1" and one("adapter_ends_past_window") in m
    assert s[one("adapter_both_ends")][1:3] == ["0", "+"]
    assert one("shorter_than_adapter") not in s and one("no_adapter") not in s
    assert len(s[one("ends_inside_barcode")][4]) == p["pad"] + L - L // 2 and one("ends_inside_barcode") not in m
    assert len(s[one("ends_after_barcode")][4]) == p["pad"] + L and m[one("ends_after_barcode")][1] == "0"
    assert s[one("adapter_with_n")][1] == "1" and one("adapter_with_n") in m
    for k in ("barcode_substitution", "barcode_insertion", "barcode_deletion", "barcode_with_n"):
        assert m[one(k)][1:3] == ["1", "1"], k
    assert "N" in s[one("barcode_with_n")][4]
    assert int(m[one("barcode_at_max_errors")][1]) == p["max_errors"] and one("barcode_over_max_errors") in s and one("barcode_over_max_errors") not in m
    assert m[one("lower_case")][1] == "0" and s[one("lower_case")][4].isupper()
    assert m[one("two_tied")][1:3] == ["1", "2"] and m[one("two_tied")][4].count(",") == 1
    many = m[one("more_than_eight_tied")]
    assert many[2] == "10" and many[4].count(",") == B.LIST - 1
    homo = "A" * L
    assert int(exact[homo]) == 6 and all(m[n][4] == homo for n in c["homopolymer"])
    assert int(exact[c["exact_at_min"][0]]) == p["min_exact"] and c["exact_below_min"][0] not in exact and c["never_seen"][0] not in exact
    assert c["exact_below_min"][0] in g["barcodes"] and c["never_seen"][0] in g["barcodes"]
    i = out["info"]
    assert i["reads"] == g["n_reads"] == i["no_adapter"] + i["forward"] + i["reverse"]
    assert i["forward"] + i["reverse"] == i["no_barcode"] + i["unique"] + i["ambiguous"] and i["ambiguous"] == 2 and i["no_barcode"] >= 3


def test_round_trip_of_reads_built_from_strings(tmp_path):
    """cDNA + polyA + 10 random bases + CB + the reverse complement of the adapter, randomly reverse-complemented, an outer adapter of 28
    bases on both sides: with revcomp_barcodes every read returns its own CB at distance 0, alone"""
    rs = random.Random(11)
    rnd = lambda n: "".join(rs.choice("ACGT") for _ in range(n))
    cbs = []
    while len(cbs) < 24:
        b = rnd(16)
        if b not in cbs:
            cbs.append(b)
    outer5, outer3 = rnd(28), rnd(28)
    reads, truth = [], {}
    for k in range(96):
        cb = cbs[k % len(cbs)]
        mol = rnd(rs.randint(200, 500)) + "A" * rs.randint(20, 40) + rnd(10) + cb + B.revcomp(B.DEFAULT_ADAPTER)
        if rs.random() < 0.5:
            mol = B.revcomp(mol)
        reads.append((f"mol{k}", outer5 + mol + outer3))
        truth[f"mol{k}"] = cb
    (tmp_path / "r.fq").write_text("".join(f"@{n}\n{s}\n+\n{'I' * len(s)}\n" for n, s in reads))
    (tmp_path / "w.txt").write_text("\n".join(cbs) + "\n")
    out = B.run(str(tmp_path / "r.fq"), str(tmp_path / "w.txt"), revcomp_barcodes=True)
    rows = {l.split("\t")[0]: l.split("\t") for l in out["matches"].splitlines()}
    assert {n: (r[1], r[2], r[4]) for n, r in rows.items()} == {n: ("0", "1", cb) for n, cb in truth.items()}
    assert out["info"]["unique"] == 96 and out["info"]["candidates"] == 24
    assert 20 < out["info"]["forward"] < 76
    # without the flag the spellings do not match: nothing is selected
    assert B.run(str(tmp_path / "r.fq"), str(tmp_path / "w.txt"))["info"]["unique"] == 0


def test_specification_refuses_what_the_rules_refuse(tmp_path):
    p = write_known(tmp_path)
    for bad in ({"adapter": "ACG"}, {"adapter": "ACGTN"}, {"window": 5}, {"pad": 17}, {"max_adapter_errors": 6}, {"max_errors": 4}, {"min_exact": -1}):
        with pytest.raises(ValueError):
            B.run(p["reads"], p["whitelist"], **dict(KNOWN["params"], **bad))
    for text in ("GGTT\nGGT\n", "GGTT\nGGTN\n", "GGTT\nCCCC\nGGTT\n", "\n\n", "ggtt\n"):
        (tmp_path / "bad.txt").write_text(text)
        with pytest.raises(ValueError):
            B.run(p["reads"], str(tmp_path / "bad.txt"), **KNOWN["params"])
    (tmp_path / "twice.fq").write_text("@a\nACGT\n+\nIIII\n@a\nACGT\n+\nIIII\n")
    with pytest.raises(ValueError):
        B.run(str(tmp_path / "twice.fq"), p["whitelist"], **KNOWN["params"])


def test_exports_and_header_agree():
    from tksm_amd import _lib
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "tksmseq.h")).read()
    for s in ("tksmseq_barcode_match", "tksmseq_barcode_match_main"):
        assert s in _lib.SYMBOLS and re.search(rf"\b{s}\s*\(", header) and hasattr(lib, s)
    assert ctypes.sizeof(_lib.BarcodeMatchParams) == 64 and ctypes.sizeof(_lib.BarcodeMatchInfo) == 136
    for struct, cls in (("tksmseq_barcode_match_info", _lib.BarcodeMatchInfo), ("tksmseq_barcode_match_params", _lib.BarcodeMatchParams)):
        fields = re.search(rf"typedef struct {struct} \{{(.*?)\}} {struct};", header, re.S).group(1)
        fields = re.sub(r"/\*.*?\*/", "", fields, flags=re.S)
        names = [n.split("[")[0] for part in re.findall(r"(?:uint64_t|int64_t|int32_t|float|double|const char\*)\s+([^;]+);", fields) for n in re.split(r",\s*", part.strip())]
        assert names == [n for n, _ in cls._fields_], struct
    kernels_h = open(os.path.join(ROOT, "tksm_amd", "csrc", "bm_kernels.h")).read()
    assert int(re.search(r"BM_CAND_TILE = (\d+)", kernels_h).group(1)) == _lib.BM_CAND_TILE
    assert int(re.search(r"BM_TARGET_WAVES = (\d+)", kernels_h).group(1)) == _lib.BM_TARGET_WAVES
    assert int(re.search(r"BM_LIST = (\d+)", kernels_h).group(1)) == _lib.BM_LIST == B.LIST
    # the product does not import the specification, and the kernels of this module use no floating point
    for root, _, files in os.walk(os.path.join(ROOT, "tksm_amd")):
        for f in files:
            if f.endswith((".py", ".cpp", ".h", ".hip")):
                assert "barcode_spec" not in open(os.path.join(root, f), errors="replace").read(), f
    kernels = open(os.path.join(ROOT, "tksm_amd", "csrc", "bm_kernels.hip")).read()
    assert not re.search(r"\b(float|double)\b", re.sub(r"//.*", "", kernels))
    import __graft_entry__ as g
    assert "k_bm_match" in g.NO_SPILL_BM


def _module(*args):
    return subprocess.run([EXE, "barcode-match", *[str(a) for a in args]], capture_output=True, text=True)


def test_module_argument_checks_and_exit_codes(tmp_path):
    p = write_known(tmp_path)
    out = tmp_path / "m.tsv"
    need = ["--reads", p["reads"], "--whitelist", p["whitelist"], "-o", out]
    r = _module()
    assert r.returncode == 2 and "barcode-match: error:" in r.stderr and "--reads, --whitelist, -o/--output" in r.stderr
    r = _module(*need[:4])
    assert r.returncode == 2 and "-o/--output" in r.stderr and "--reads" not in r.stderr
    r = _module(*need, "--nope")
    assert r.returncode == 2 and "--nope" in r.stderr
    r = _module(*need, "-i", "x")
    assert r.returncode == 2 and "-i" in r.stderr
    for flag, bad in (("--window", "3"), ("--window", "21"), ("--max-adapter-errors", "22"), ("--max-adapter-errors", "-1"), ("--pad", "17"), ("--pad", "-1"),
                      ("--max-errors", "32"), ("--max-errors", "-1"), ("--min-exact", "-1"), ("--chunk-reads", "-1"), ("--adapter", "ACG"), ("--adapter", "ACGTNACGT"),
                      ("--adapter", "A" * 33)):
        r = _module(*need, flag, bad)
        assert r.returncode == 2 and f"barcode-match: error: {flag} must" in r.stderr, (flag, bad, r.stderr)
    r = _module(*need, "--pad", "four")
    assert r.returncode == 2
    r = _module(*need, "--verbosity", "LOUD")
    assert r.returncode == 1 and "unknown verbosity level" in r.stderr
    assert _module("-h").returncode == 0 and "--revcomp-barcodes" in _module("--help").stdout
    assert not out.exists()
    r = subprocess.run([EXE, "list"], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.split() == ["sequence", "pcr", "truncate", "polyA", "tag", "scb", "flip"]
    r = subprocess.run([EXE, "nonesuch"], capture_output=True, text=True)
    assert r.returncode == 1 and "Unknown kisim" in r.stderr and "`unsegment` and `shuffle`" in r.stderr and "also `mutate` and `barcode-match`" in r.stderr
