"""model-sequence without a GPU: the specification (tests/model_seq_spec.py) against a case counted by hand
(tests/golden/model_seq_known_answers.json), its files through the oracle's loaders, the op counts, pass totals and counters of the
shapes that the device's tests expand (M.shape_cases), the host code (FASTQ and PAF readers, the writers) under ASan / UBSan in a
stand-alone program, and the module's argument checks."""
import ctypes
import gzip
import json
import os
import re
import subprocess

import pytest

from conftest import GOLDEN, ROOT

import model_seq_spec as M

EXE = os.path.join(ROOT, "tksm_amd", "tksm")
KNOWN = json.load(open(os.path.join(GOLDEN, "model_seq_known_answers.json")))


def write_known(d):
    paths = {}
    for what, name in (("reference", "ref.fa"), ("reads", "reads.fq"), ("alignment", "aln.paf")):
        paths[what] = os.path.join(str(d), name)
        with open(paths[what], "w") as f:
            f.write(KNOWN[what])
    return paths


def known_error_text():
    kmers = ["".join(M.ACGT[(i >> (2 * (2 - j))) & 3] for j in range(3)) for i in range(64)]
    return "".join(KNOWN["error_lines"].get(k, k + ",1.000000;") + "\n" for k in kmers)


@pytest.fixture(scope="module")
def generated(tmp_path_factory):
    d = tmp_path_factory.mktemp("model_seq_cpu")
    g = M.generate(d, seed=7, n_alignments=40, long_columns=1500, group=5)
    g["dir"] = d
    g["out"] = M.run(g["reference"], g["reads"], g["alignment"], min_occur=1)
    return g


def test_specification_gives_the_hand_counted_files(tmp_path):
    p = write_known(tmp_path)
    got = M.run(p["reference"], p["reads"], p["alignment"], **KNOWN["params"])
    assert got["error"] == known_error_text()
    assert got["qscore"] == KNOWN["qscore"]
    assert {k: got["info"][k] for k in KNOWN["info"]} == KNOWN["info"]
    # the gzipped inputs read the same
    for what in ("reads", "alignment", "reference"):
        with gzip.open(p[what] + ".gz", "wt") as f:
            f.write(KNOWN[what])
    again = M.run(p["reference"] + ".gz", [p["reads"] + ".gz"], p["alignment"] + ".gz", **KNOWN["params"])
    assert again["error"] == got["error"] and again["qscore"] == got["qscore"]


def test_specification_cuts_and_forced_keys(tmp_path):
    p = write_known(tmp_path)
    kw = dict(KNOWN["params"])
    kw["max_output"] = 2
    keys = [ln.split(";")[0] for ln in M.run(p["reference"], p["reads"], p["alignment"], **kw)["qscore"].splitlines()]
    assert keys == ["overall", "=", "I", "X"]                  # === (3) gives way; the three one-letter keys stay
    kw["max_output"] = 4
    keys = [ln.split(";")[0] for ln in M.run(p["reference"], p["reads"], p["alignment"], **kw)["qscore"].splitlines()]
    assert keys == ["overall", "=", "===", "I", "X"]
    kw.update(max_output=10000, min_occur=3)
    keys = [ln.split(";")[0] for ln in M.run(p["reference"], p["reads"], p["alignment"], **kw)["qscore"].splitlines()]
    assert keys == ["overall", "=", "===", "I", "X"]
    kw.update(min_occur=1, max_alt=0)
    assert "ACG,0.666667;\n" in M.run(p["reference"], p["reads"], p["alignment"], **kw)["error"]
    kw.update(max_alt=25, max_alignments=1)
    one = M.run(p["reference"], p["reads"], p["alignment"], **kw)
    assert one["info"]["used"] == 1 and one["info"]["lines"] == 1 and isinstance(one["qscore"], ValueError) and "'I'" in str(one["qscore"])


def test_generator_plants_every_class(generated):
    c, info = generated["classes"], generated["out"]["info"]
    for what in ("strand_plus", "strand_minus", "ops_M", "ops_=X", "insertion_first_column", "insertion_last_column", "del_run_max_del",
                 "del_run_max_del_plus_1", "alternative_K_plus_4", "alternative_K_plus_5", "reference_N", "read_N", "lower_case", "alignment_of_K",
                 "alignment_of_K_minus_1", "ends_at_contig_end", "read_with_several_lines", "tp_A_S", "no_cigar", "unknown_read", "unknown_target"):
        assert c.get(what, 0) >= 1, what
    for k in ("skipped_no_cigar", "skipped_supplementary", "skipped_unknown_read", "skipped_unknown_target", "skipped_cigar_op", "alternatives_too_long",
              "windows_max_del", "keys_too_long"):
        assert info[k] >= 1, k
    assert re.search(r"[acgt]", open(generated["reference"]).read())
    assert any("N" in seq for seq in open(generated["reads"]).read().split("\n")[1::4])


@pytest.fixture(scope="module")
def shaped(tmp_path_factory):
    """M.generate_shapes and, per shape, the CIGARs and the specification's counters of its two alignments taken alone"""
    g = M.generate_shapes(tmp_path_factory.mktemp("model_seq_shapes"))
    reads, ref = M.read_fastq(g["reads"]), M.read_fasta(g["reference"])
    used, _ = M.parse_paf(g["alignment"], reads, ref)
    by_read = {a["read"]: a for a in used}
    cigar = {ln.split("\t")[0]: ln.rstrip("\n").split("\tcg:Z:")[1] for ln in open(g["alignment"]) if "\tcg:Z:" in ln and "\ttp:A:S" not in ln}
    g["cigars"] = {what: [cigar[r] for r in names] for what, names in g["shape_reads"].items()}
    g["strands"] = {what: [by_read[r]["strand"] for r in names] for what, names in g["shape_reads"].items()}
    g["counters"] = {what: [M.count(ref, reads, [by_read[r]])[4] for r in names] for what, names in g["shape_reads"].items()}
    return g


def ops_of(shaped, what):
    """the host's ops of a shape: the same on both strands and in both CIGAR styles"""
    plus, minus = (M.host_ops(c) for c in shaped["cigars"][what])
    assert plus == minus and shaped["strands"][what] == ["+", "-"]
    return plus


def test_host_merge_rule_of_the_helper():
    assert M.host_ops("3M2=1X0I4I0D2D2D1M") == [(6, "M"), (4, "I"), (4, "D"), (1, "M")]
    assert M.host_ops("5=") == M.host_ops("2X3M") == [(5, "M")] and M.pass_columns("1=1I1=1D", 2) == [2, 2] and M.pass_columns("1=1I1=", 2) == [2, 1]


def test_shapes_have_the_op_counts_and_the_pass_totals(shaped):
    """every shape of M.shape_cases is in the PAF with the number of ops, the columns per pass of 64 ops and the long op in the lane that it
    is there for (counted by M.host_ops, the host's rule, from the CIGAR text as written)"""
    assert set(shaped["cigars"]) == set(M.shape_cases()) and len(shaped["cigars"]) == 30
    styles = {c for pair in shaped["cigars"].values() for c in pair}
    assert any("M" in c for c in styles) and any("X" in c or "=" in c for c in styles)
    passes = {1: [1], 2: [21], 63: [63], 64: [64], 65: [64, 1], 127: [64, 63], 128: [64, 64], 129: [64, 64, 1], 192: [64, 64, 64], 193: [64, 64, 64, 1]}
    for n, columns in passes.items():
        assert len(ops_of(shaped, "ops_%d" % n)) == n and [M.pass_columns(c) for c in shaped["cigars"]["ops_%d" % n]] == [columns, columns]
    for total in (64, 65, 127, 128, 129):
        what = "first_pass_%d_columns" % total
        assert len(ops_of(shaped, what)) == 71 and M.pass_columns(shaped["cigars"][what][0]) == [total, 7]
    for n in (63, 64, 65, 1000, 5000):
        assert ops_of(shaped, "one_op_%d" % n) == [(n, "M")]
    for code, length in (("D", 3000), ("I", 300)):
        for at, n_ops in ((0, 4), (1, 3), (63, 65), (64, 66)):
            ops = ops_of(shaped, "%s%d_as_op_%d" % (code, length, at))
            assert len(ops) == n_ops and ops[at] == (length, code) and ops[at + 1] == (12, "M") and (at == 0 or ops[at - 1] == (12, "M"))
            assert sum(n >= 7 for n, o in ops if o == code) == 1
    for what, run in (("del_max_del_behind_a_long_window", 6), ("del_max_del_plus_1_behind_a_long_window", 7)):
        assert [n for n, o in ops_of(shaped, what) if o == "D"] == [6, 6, 6, 6, 6, run]


def test_counters_of_the_long_deletion_and_of_the_runs_at_max_del(shaped):
    """By the header's rule a window with a run of more than max_del (6) 'D's is not counted, whatever its length.  The 3 000 'D's lie
    between the read positions a - 1 and a, and the window of read position i and half-width h holds them when i - h <= a - 1 and
    i + h >= a: for h = 1, 2, 3, 4 ((9 - 1) / 2) these are the 2 h positions a - h .. a - 1 + h, all inside the read, since 12 '=' stand on
    either side: 2 + 4 + 6 + 8 = 20 windows.  No other run of the alignment is longer than 1.  A deletion that the alignment starts with
    lies in no window."""
    for at, want in ((0, 0), (1, 20), (63, 20), (64, 20)):
        for info in shaped["counters"]["D3000_as_op_%d" % at]:
            assert info["windows_max_del"] == want and info["keys_too_long"] == 0, at
    for at in (0, 1, 63, 64):
        for info in shaped["counters"]["I300_as_op_%d" % at]:
            assert info["windows_max_del"] == 0 and info["alternatives_too_long"] == (7 - 1 if at else 0), at
    # '=DDDDDD' five times and '=': 6 read positions over 36 letters.  The windows of 7 and 9 read positions (h = 3, 4) over them are longer
    # than 29 letters; the one more run of 6 'D's leaves them keys_too_long, a run of 7 puts those that hold it under windows_max_del
    six, seven = shaped["counters"]["del_max_del_behind_a_long_window"], shaped["counters"]["del_max_del_plus_1_behind_a_long_window"]
    for info in six:
        assert info["windows_max_del"] == 0 and info["keys_too_long"] > 0
    for info, base in zip(seven, six):
        assert info["windows_max_del"] == 20 and 0 < info["keys_too_long"] < base["keys_too_long"]


def test_specifications_files_load_in_the_oracles_loaders(generated, po):
    d = generated["dir"]
    (d / "spec.error").write_text(generated["out"]["error"])
    with gzip.open(d / "spec.qscore.gz", "wt") as f:
        f.write(generated["out"]["qscore"])
    em, qm = po.ErrorModel(str(d / "spec.error")), po.QScoreModel(str(d / "spec.qscore.gz"))
    assert em.k == 7 and em.type == 1 and 2 <= em.max_alts <= 26 and len(em.nalts) == 4 ** 7
    keys = [ln.split(";")[0] for ln in generated["out"]["qscore"].splitlines()[1:]]
    assert qm.kmer_size == 9 and set(qm.scores) == set(keys) and {"=", "X", "I"} <= set(keys)
    assert all(len(k) <= 29 and k[0] != "D" and k[-1] != "D" and "D" * 7 not in k for k in keys)
    # the lines have the shape of the shipped files
    shipped = gzip.open(os.path.join(ROOT, "tksm_amd", "models", "badread", "nanopore2020.qscore.gz"), "rt").read().splitlines()
    shape = re.compile(r"^[=XID]+;\d+;(\d+:(0|1)\.\d*,)+$")
    assert all(shape.match(ln) for ln in shipped[1:50]) and all(shape.match(ln) for ln in generated["out"]["qscore"].splitlines()[1:])
    assert all(re.match(r"^[ACGT]{7},\d\.\d{6};([ACGT]+,\d\.\d{6};)*$", ln) for ln in generated["out"]["error"].splitlines())


@pytest.fixture(scope="module")
def host_program(generated):
    """tools/sanitize_ms_host.cpp built with ASan + UBSan and run on the generated files: {key: [lines]} of what it printed"""
    d = generated["dir"]
    exe = d / "sanitize_ms_host"
    csrc = os.path.join(ROOT, "tksm_amd", "csrc")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-I", csrc, "-o", str(exe),
                    os.path.join(ROOT, "tools", "sanitize_ms_host.cpp"), os.path.join(csrc, "ms_host.cpp"), os.path.join(csrc, "abund_host.cpp"), "-lz"], check=True)
    (d / "host_out").mkdir()
    r = subprocess.run([str(exe), generated["reference"], generated["reads"], generated["alignment"], str(d / "host_out")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr
    out = {}
    for line in r.stdout.splitlines():
        key, _, rest = line.partition(" ")
        out.setdefault(key, []).append(rest)
    return d / "host_out", out


def test_host_readers_under_sanitizers_match_the_specification(generated, host_program):
    _, out = host_program
    reads = M.read_fastq(generated["reads"])
    ref = M.read_fasta(generated["reference"])
    bases = "".join(s for s, _ in reads.values())
    quals = [q for _, qs in reads.values() for q in qs]
    want = sum((i % 1000 + 1) * (ord(b) + 3 * q) for i, (b, q) in enumerate(zip(bases, quals)))
    assert out["fastq"] == [f"{len(reads)} {len(bases)} {want}"]
    used, info = M.parse_paf(generated["alignment"], reads, ref)
    tid = {name: i for i, name in enumerate(ref)}
    want = sum((i + 1) * (a["qstart"] + 3 * a["qend"] + 5 * a["tstart"] + 7 * a["tend"] + 11 * (a["strand"] == "-") + 13 * sum(n for n, _ in a["ops"]) + 17 * tid[a["target"]])
               for i, a in enumerate(used))
    assert out["paf"] == [f"{len(used)} {info['lines']} {info['skipped_no_cigar']} {info['skipped_supplementary']} {info['skipped_unknown_read']} "
                          f"{info['skipped_unknown_target']} {info['skipped_cigar_op']} {want}"]
    for key, size in (("fastq_cut", os.path.getsize(generated["reads"])), ("paf_cut", os.path.getsize(generated["alignment"]))):
        ok, bad = [int(v) for v in out[key][0].split()]
        assert ok >= 1 and bad >= 1 and ok + bad == (size + 996) // 997


def test_host_readers_on_malformed_input(host_program):
    _, out = host_program
    fq = [c.split(" ", 3) for c in out["fastq_case"]]
    assert [int(c[0]) for c in fq] == [1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 0]
    assert [c[1:3] for c in fq if c[0] == "1"] == [["0", "0"], ["0", "0"], ["1", "4"], ["1", "5"], ["2", "3"], ["1", "0"]]
    assert "differ in length" in fq[4][3] and "ends inside the record" in fq[5][3] and "ends inside the record" in fq[6][3]      # truncated records
    assert "'@'" in fq[7][3] and "'+'" in fq[8][3] and "quality outside" in fq[9][3] and "quality outside" in fq[10][3]         # 0x7f is above '~'
    assert "record 2" in fq[11][3] and "came before" in fq[11][3]
    assert out["fastq_values"] == ["ACGTN 0 0 93 93 40"]
    cases = {c.split(" ")[0]: c.split(" ", 10) for c in out["paf_case"]}
    ok = {k for k, c in cases.items() if c[1] == "1"}
    assert ok == {"good", "mixed_ops", "empty", "clip", "no_cg", "supplementary", "unknown_read", "unknown_target", "max_alignments"}
    assert cases["good"][2:4] == ["1", "1"] and cases["mixed_ops"][2:4] == ["1", "5"] and cases["empty"][2:5] == ["0", "0", "0"]
    assert cases["max_alignments"][2:5] == ["2", "2", "2"]      # the third line (a bad one) is never read
    for name, col in (("no_cg", 5), ("supplementary", 6), ("unknown_read", 7), ("unknown_target", 8), ("clip", 9)):
        assert cases[name][2] == "0" and [cases[name][c] for c in range(5, 10)] == ["1" if c == col else "0" for c in range(5, 10)], name
    why = {"nine_columns": "fewer than 12 columns", "wrong_read_length": "does not consume", "wrong_target_length": "does not consume", "no_number": "no CIGAR",
           "trailing_number": "no CIGAR", "empty_cigar": "no CIGAR", "garbage_op": "no CIGAR", "huge_op": "no CIGAR", "not_a_number": "column 3 is no integer",
           "negative": "column 3 is no integer", "two_to_the_31": "column 4 is no integer", "start_after_end": "query range", "end_after_length": "query range",
           "target_end_after_contig": "target range", "column_2": "column 2 differs", "strand": "column 5", "binary": "fewer than 12 columns"}
    for name, text in why.items():
        assert cases[name][1] == "0" and "PAF line 1: " in cases[name][10] and text in cases[name][10], name
    assert cases["second_line_bad"][1] == "0" and "PAF line 3: " in cases["second_line_bad"][10]
    assert set(cases) == ok | set(why) | {"second_line_bad"}


def test_fastq_list_loader_under_sanitizers(host_program):
    """load_fastq_list (ms_host.cpp), the one loader of model-sequence, barcode-match and map: the library's return codes: 0 ok, 2 I/O (EIO), 1 malformed (EINVAL), 6 limit (ELIMIT)"""
    d, out = host_program
    cases = {c.split(" ")[0]: c.split(" ", 4) for c in out["list_case"]}
    assert set(cases) == {"two", "empty_entries", "empty", "comma", "missing", "cut", "duplicate", "gz", "limit_after_second", "limit_after_first"}
    for name in ("two", "empty_entries", "gz"):                   # the same MsReads as the two files' text laid end to end; empty entries are skipped
        assert cases[name][1:] == ["0", "4", "1", ""], name
    assert cases["empty"][1:] == ["0", "0", "1", ""] and cases["comma"][1:] == ["0", "0", "1", ""]
    # a missing second file: abund_read_file's own message, and the first file's reads stay appended
    assert cases["missing"][1:4] == ["2", "2", "1"] and cases["missing"][4] == out["list_io_message"][0] and "nosuch.fq" in cases["missing"][4]
    assert cases["cut"][1:4] == ["1", "3", "-1"] and cases["cut"][4].startswith(f"{d}/cut.fq: FASTQ record 2: ") and "ends inside the record" in cases["cut"][4]
    assert cases["duplicate"][1:4] == ["1", "3", "-1"] and cases["duplicate"][4] == f"{d}/dup.fq: FASTQ record 2: a read of this name came before"
    # the count after every file (map, barcode-match): the limit is met by the file that brings the reads to it, what was read stays
    # (no message of the loader's: the two callers that count word the limit themselves)
    assert cases["limit_after_second"][1:] == ["6", "4", "1", ""] and cases["limit_after_first"][1:] == ["6", "2", "1", ""]
    assert out["list_names"] == ["a1 a2 b1 b2 "]


def test_host_writers_under_sanitizers(host_program):
    d, out = host_program
    assert out["error_lines"] == ["64"] and out["select"] == ["1 3"] and out["select_all"] == ["1 4"]
    assert out["select_missing"][0].startswith("0 ") and "'I'" in out["select_missing"][0]
    assert out["key_text"] == ["=D= " + "X" * 29 + " " + "X" * 29]
    assert out["write"] == ["1 1 1 0"] and out["gz_round_trip"] == ["1"]
    text = (d / "e.model").read_text()
    assert text.splitlines()[0] == "AAA,0.500000;AAAC,0.250000;AA,0.250000;" and text.splitlines()[1] == "AAC,1.000000;" and text.splitlines()[63] == "TTT,0.000000;TTTTTTT,0.666667;"
    assert gzip.open(d / "e.model.gz", "rt").read() == text
    assert (d / "q.model").read_text() == "overall;8;0:0.125,10:0.5,93:0.375,\n=;5;10:0.8,93:0.2,\nI;2;93:1.,\nX;1;0:1.,\n"
    assert not list(d.glob("*.tmp")) and not (d / "no").exists()


def _module(*args):
    return subprocess.run([EXE, "model-sequence", *[str(a) for a in args]], capture_output=True, text=True)


def test_module_argument_checks_and_exit_codes(tmp_path):
    p = write_known(tmp_path)
    need = ["--reference", p["reference"], "--reads", p["reads"], "--alignment", p["alignment"]]
    out = tmp_path / "e.model"
    r = _module("--error-model", out)
    assert r.returncode == 2 and "model-sequence: error:" in r.stderr and "--reference, --reads, --alignment" in r.stderr
    r = _module(*need[:4], "--error-model", out)
    assert r.returncode == 2 and "--alignment" in r.stderr and "--reads" not in r.stderr
    r = _module(*need)
    assert r.returncode == 2 and "model-sequence: error: at least one of --error-model and --qscore-model is required" in r.stderr
    r = _module(*need, "--error-model", out, "--nope")
    assert r.returncode == 2 and "--nope" in r.stderr
    r = _module(*need, "--error-model", out, "-o", "x")
    assert r.returncode == 2 and "-o" in r.stderr
    for flag, bad in (("--error-k", "2"), ("--error-k", "9"), ("--qscore-k", "8"), ("--qscore-k", "31"), ("--qscore-k", "0"), ("--max_alt", "32"), ("--max_alt", "-1"),
                      ("--max_del", "-1"), ("--min_occur", "-5"), ("--max_output", "-1"), ("--max_alignments", "-1")):
        r = _module(*need, "--error-model", out, flag, bad)
        assert r.returncode == 2 and f"model-sequence: error: {flag} must" in r.stderr, (flag, bad)
    r = _module(*need, "--error-model", out, "--error-k", "seven")
    assert r.returncode == 2
    r = _module(*need, "--error-model", out, "--verbosity", "LOUD")
    assert r.returncode == 1 and "unknown verbosity level" in r.stderr
    assert _module("-h").returncode == 0 and "--qscore-model" in _module("--help").stdout
    assert not out.exists()
    r = subprocess.run([EXE, "list"], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.split() == ["sequence", "pcr", "truncate", "polyA", "tag", "scb", "flip"]


def test_exports_and_header_agree():
    from tksm_amd import _lib
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "tksmseq.h")).read()
    for s in ("tksmseq_model_sequence", "tksmseq_model_sequence_main"):
        assert s in _lib.SYMBOLS and re.search(rf"\b{s}\s*\(", header) and hasattr(lib, s)
    assert ctypes.sizeof(_lib.ModelSequenceParams) == 48 and ctypes.sizeof(_lib.ModelSequenceInfo) == 176
    fields = re.search(r"typedef struct tksmseq_model_sequence_info \{(.*?)\} tksmseq_model_sequence_info;", header, re.S).group(1)
    fields = re.sub(r"/\*.*?\*/", "", fields, flags=re.S)
    names = [n.split("[")[0] for part in re.findall(r"(?:uint64_t|float|double)\s+([^;]+);", fields) for n in re.split(r",\s*", part.strip())]
    assert names == [n for n, _ in _lib.ModelSequenceInfo._fields_]
    # the product does not import the specification, and the kernels of this module use no floating point
    for root, _, files in os.walk(os.path.join(ROOT, "tksm_amd")):
        for f in files:
            if f.endswith((".py", ".cpp", ".h", ".hip")):
                assert "model_seq_spec" not in open(os.path.join(root, f), errors="replace").read(), f
    kernels = open(os.path.join(ROOT, "tksm_amd", "csrc", "ms_kernels.hip")).read()
    assert not re.search(r"\b(float|double)\b", re.sub(r"//.*", "", kernels))
