"""map -g without a device: the specification (tests/map_targets_spec.py) against a per-letter implementation and against its recorded answers,
the properties of the projection, the host code of the product under the sanitizers against the specification, and the interface: the
header, the exported symbols, the Python signatures and the argument checks of the module."""
import ctypes
import inspect
import json
import os
import random
import re
import subprocess

import pytest

import map_targets_spec as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "map_targets_known_answers.json")
EXE = os.path.join(ROOT, "tksm_amd", "tksm")
COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}


def random_genome(rs, sizes, exotic=0.02):
    """letters of ACGT with some N, lower case and IUPAC codes"""
    return {name: "".join(rs.choice("NnacgtRY") if rs.random() < exotic else rs.choice("ACGT") for _ in range(n)) for name, n in sizes.items()}


def naive_target(genome, exons):
    """letter by letter: the target of the exons (contig, start, end, strand), every letter with its own genome position"""
    out = []
    for c, a, b, strand in exons:
        positions = range(a, b) if strand == "+" else range(b - 1, a - 1, -1)
        for g in positions:
            x = genome[c][g].upper()
            x = x if x in COMP else "N"
            out.append(x if strand == "+" or x == "N" else COMP[x])
    return "".join(out)


def test_splice_against_a_per_letter_implementation():
    rs = random.Random(11)
    genome = random_genome(rs, {"g1": 700, "g2": 333, "g3": 64})
    genome["gd"] = None
    table, want, counters = [], [], dict(skipped_empty=0, skipped_unknown_contig=0, skipped_bad_exon=0)
    for t in range(300):
        exons = []
        for _ in range(rs.choice((0, 1, 1, 2, 3, 5, 9))):
            c = rs.choice(("g1", "g1", "g2", "g3"))
            a = rs.randrange(len(genome[c]))
            b = min(len(genome[c]), a + rs.choice((0, 1, 1, 2, 15, 16, 17, 31, 32, 33, 64, 65, 100)))
            exons.append((c, a, b, rs.choice("+-")))
        kind = rs.random()
        if kind < 0.05 and exons:
            exons[rs.randrange(len(exons))] = ("gX" if kind < 0.03 else "gd", 0, 5, "+")
        elif kind < 0.10 and exons:
            c = exons[-1][0]
            exons[-1] = (c, 10, 5, "+") if kind < 0.07 else (c, len(genome[c]) - 3, len(genome[c]) + 1, "-")
        table.append(("tx%d" % t, exons))
        if all(a == b for _, a, b, _ in exons):
            counters["skipped_empty"] += 1
        elif any(c in ("gX", "gd") for c, _, _, _ in exons):
            counters["skipped_unknown_contig"] += 1
        elif any(b < a or b > len(genome[c]) for c, a, b, _ in exons):
            counters["skipped_bad_exon"] += 1
        else:
            want.append(("tx%d" % t, naive_target(genome, exons)))
    got = T.targets(genome, table)
    assert list(zip(got["names"], got["seqs"])) == want
    assert min(counters.values()) > 0 and {k: got["info"][k] for k in counters} == counters
    assert got["info"]["transcripts"] == 300 == got["info"]["targets"] + sum(counters.values())
    assert got["info"]["letters"] == sum(len(s) for _, s in want) and got["lengths"] == [len(s) for _, s in want]
    # the layout: a target starts a validity word, and the bits behind its end are clear
    assert got["voff"][0] == 0 and all(b - a == (n + 31) // 32 for a, b, n in zip(got["voff"], got["voff"][1:], got["lengths"]))
    assert got["info"]["image_vwords"] == got["voff"][-1] == len(got["valid"]) and len(got["codes"]) == 2 * len(got["valid"])
    for v, (_, seq) in zip(got["voff"], want):
        words = (len(seq) + 31) // 32
        valid = sum(w << (32 * i) for i, w in enumerate(got["valid"][v:v + words]))
        codes = sum(w << (32 * i) for i, w in enumerate(got["codes"][2 * v:2 * (v + words)]))
        assert valid == sum(1 << g for g, x in enumerate(seq) if x != "N")
        assert codes == sum("ACGT".index(x) << (2 * g) for g, x in enumerate(seq) if x != "N")
    assert {len(s) for _, s in want} >= {1, 32, 64} and any("N" in s for _, s in want)
    text = T.fasta(got, 60).decode()
    assert text.count(">") == len(want) and "".join(text.split("\n")[1:3]).startswith(want[0][1][:60])
    one = T.fasta(got, 0).decode().split("\n")
    assert one[0::2][:-1] == [">" + n for n, _ in want] and one[1::2] == [s for _, s in want]


def random_transcript(rs, glen, minus):
    """a projectable transcript of 1 to 6 exons on a genome of glen letters: exons in file order, some touching (a gap of 0)"""
    n = rs.randint(1, 6)
    cuts = sorted(rs.sample(range(1, glen), 2 * n))
    exons = [(cuts[2 * i], cuts[2 * i + 1]) for i in range(n)]
    if n > 1 and rs.random() < 0.5:
        i = rs.randrange(n - 1)
        exons[i + 1] = (exons[i][1], exons[i + 1][1])                              # a gap of 0
    exons = [("g", a, b, minus) for a, b in exons]
    return exons[::-1] if minus else exons


def random_cigar(rs, tlen, eqx=True):
    """a valid CIGAR over target letters [a, b) of a target of tlen letters: (a, b, read letters, text)"""
    a = rs.randrange(tlen)
    b = rs.randint(a + 1, tlen)
    runs, left = [], b - a
    while left:
        op = rs.choice("==XDI" if eqx else "MMDI")
        if runs and runs[-1][1] == op:
            continue
        n = rs.randint(1, 12)
        if op != "I":
            n = min(n, left)
            left -= n
        runs.append((n, op))
    if rs.random() < 0.3 and runs[-1][1] != "I":
        runs.append((rs.randint(1, 4), "I"))
    return a, b, sum(n for n, op in runs if op != "D"), "".join("%d%s" % r for r in runs)


def paf_line(tid, tlen, a, b, qlen, rel, cg):
    nm = sum(n for n, op in T.cigar_runs(cg) if op in "XID")
    eq = sum(n for n, op in T.cigar_runs(cg) if op in "=M")
    return "\t".join(str(x) for x in ["read", qlen + 7, 3, 3 + qlen, "+-"[rel], tid, tlen, a, b, eq, sum(n for n, _ in T.cigar_runs(cg)), 60,
                                        "tp:A:P", "cm:i:5", "s1:i:50", "NM:i:%d" % nm, "cg:Z:" + cg])


def test_projection_properties():
    rs = random.Random(5)
    glen = 300                                                                  # (short exons: most lines cross a junction)
    crossed = 0
    for case in range(400):
        minus = case % 2 == 1
        exons = random_transcript(rs, glen, minus)
        tlen = sum(b - a for _, a, b, _ in exons)
        a, b, qlen, cg = random_cigar(rs, tlen, eqx=case % 3 != 0)
        rel = rs.randrange(2)
        line = paf_line("tx", tlen, a, b, qlen, rel, cg)
        out, junctions = T.project_line(line, ("tx", glen), exons)
        f, g = line.split("\t"), out.split("\t")
        # what stays
        assert g[:4] == f[:4] and g[9:16] == f[9:16] and g[-1] == "tx:Z:tx" and len(g) == len(f) + 1
        assert g[4] == "+-"[rel ^ minus] and g[5] == "g" and g[6] == str(glen)
        # the interval, and the letters the CIGAR consumes
        runs = T.cigar_runs(g[16][5:])
        assert sum(n for n, op in runs if op in "M=XDN") == int(g[8]) - int(g[7])
        assert sum(n for n, op in runs if op in "M=XI") == qlen == int(f[3]) - int(f[2])
        assert all(x[1] != y[1] for x, y in zip(runs, runs[1:])) and all(n > 0 for n, _ in runs)
        assert runs[0][1] != "N" and runs[-1][1] != "N" and junctions == sum(op == "N" for _, op in runs)
        lo, hi = min(a for _, a, _, _ in exons), max(b for _, _, b, _ in exons)
        assert lo <= int(g[7]) < int(g[8]) <= hi
        # the = count and NM do not change
        before = T.cigar_runs(cg)
        for ops in ("=M", "X", "I", "D"):
            assert sum(n for n, op in runs if op in ops) == sum(n for n, op in before if op in ops)
        # G is monotone over the interval, and its ends are the columns
        pos = [T.genome_position(exons, x)[0] for x in range(a, b)]
        assert all((q < p) if minus else (q > p) for p, q in zip(pos, pos[1:]))
        assert (int(g[7]), int(g[8])) == ((pos[-1], pos[0] + 1) if minus else (pos[0], pos[-1] + 1))
        # without a CIGAR: the same columns, and the exon boundaries crossed
        plain, crossed_here = T.project_line("\t".join(f[:15]), ("tx", glen), exons)
        assert plain.split("\t")[:15] == g[:15] and crossed_here == T.genome_position(exons, b - 1)[1] - T.genome_position(exons, a)[1] >= junctions
        crossed += junctions
        # the mirrored transcript of the mirrored genome gives the mirrored line
        mirrored = [("g", glen - e, glen - s, not m) for _, s, e, m in exons]
        mout, mj = T.project_line(line, ("tx", glen), mirrored)
        m = mout.split("\t")
        assert mj == junctions and m[4] != g[4] and (int(m[7]), int(m[8])) == (glen - int(g[8]), glen - int(g[7]))
        assert T.cigar_runs(m[16][5:]) == runs[::-1] and m[:4] + m[9:16] + m[17:] == g[:4] + g[9:16] + g[17:]
    assert crossed > 200


def test_an_insertion_at_a_junction_stays_with_the_exon_before_it():
    exons = [("g", 100, 110, False), ("g", 150, 160, False)]
    line = paf_line("tx", 20, 5, 15, 13, 0, "5=3I5=")
    assert T.project_line(line, ("tx", 1000), exons)[0].split("\t")[16] == "cg:Z:5=3I40N5="
    minus = [("g", 150, 160, True), ("g", 100, 110, True)]
    out = T.project_line(line, ("tx", 1000), minus)[0].split("\t")
    assert out[16] == "cg:Z:5=40N3I5=" and (out[4], out[7], out[8]) == ("-", "105", "155")
    # a deletion over the junction is cut there; touching exons give no N and the pieces merge again
    assert T.project_line(paf_line("tx", 20, 5, 15, 6, 0, "3=4D3="), ("tx", 1000), exons)[0].split("\t")[16] == "cg:Z:3=2D40N2D3="
    touching = [("g", 100, 110, False), ("g", 110, 120, False)]
    out, j = T.project_line(paf_line("tx", 20, 5, 15, 6, 0, "3=4D3="), ("tx", 1000), touching)
    assert out.split("\t")[16] == "cg:Z:3=4D3=" and j == 0


def test_recorded_cases():
    want = json.load(open(GOLDEN))
    t = T.targets(T.HOST_GENOME, T.HOST_TABLE)
    for key in ("info", "names", "lengths", "voff", "projectable", "seqs", "codes", "valid"):
        assert t[key] == want[key], key
    assert T.fasta(t, 7).decode() == want["fasta_7"]
    assert want["names"] == ["A", "B", "G", "H", "I", "M", "N"] and want["info"]["skipped_empty"] == 2 and want["info"]["skipped_unknown_contig"] == 3
    for c in want["lines"]:
        i = t["names"].index(c["target"])
        assert list(T.project_line(c["line"], (c["target"], len(T.HOST_GENOME[t["exons"][i][0][0]])), t["exons"][i])) == [c["projected"], c["junctions"]]
    by = {c["line"].split("\t")[0] + c["line"].split("\t")[4] + str("cg:Z:" in c["line"]): c["projected"].split("\t") for c in want["lines"]}
    assert by["r1+True"][4:9] + by["r1+True"][-2:] == ["+", "c1", "100", "10", "45", "cg:Z:20M10N5M", "tx:Z:A"]
    assert by["r5-True"][4:9] + by["r5-True"][-2:] == ["+", "c1", "100", "50", "80", "cg:Z:5M5N20M", "tx:Z:B"]
    assert by["r4+True"][-2] == "cg:Z:1=1D10N3D5I2=" and by["r8+True"][-2] == "cg:Z:1=4I2D1=2N1="


def test_host_code_under_sanitizers(tmp_path):
    """tools/sanitize_map_targets_host.cpp built with ASan + UBSan and run: the selection and its counters, the layout, the FASTA formatter and
    the projection, each against the specification on the same table"""
    exe = tmp_path / "sanitize_map_targets_host"
    csrc = os.path.join(ROOT, "tksm_amd", "csrc")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-I", csrc, "-o", str(exe),
                    os.path.join(ROOT, "tools", "sanitize_map_targets_host.cpp"), os.path.join(csrc, "map_host.cpp"), os.path.join(csrc, "ms_host.cpp"),
                    os.path.join(csrc, "abund_host.cpp"), "-lz"], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, r.stderr
    s = {}
    for line in r.stdout.splitlines():
        key, _, rest = line.partition(" ")
        s.setdefault(key, []).append(rest)
    assert s["genome"] == ["c1 " + T.HOST_GENOME["c1"], "c2 " + T.HOST_GENOME["c2"]]
    t = T.targets(T.HOST_GENOME, T.HOST_TABLE)
    assert s["info"] == ["0 " + " ".join(str(t["info"][k]) for k in T.COUNTERS)]
    assert s["target"] == ["%s %d %d %d" % row for row in zip(t["names"], t["lengths"], t["voff"], t["projectable"])]
    gstart = {"c1": 0, "c2": 4096}
    exons = []
    for name, kept in zip(t["names"], t["exons"]):
        cum = 0
        for c, a, b, minus in kept:
            exons.append("%s %d %d %d %d %d %d" % (name, gstart[c] + a, cum, b - a, minus, a, b))
            cum += b - a
    assert s["exon"] == exons
    assert s["empty"] == ["1 map: no transcript of the table can be a target"]
    assert s["fasta"] == ["%d %s" % (w, T.fasta(t, w).decode().replace("\n", "|")) for w in (60, 0, 1, 7, 33)]
    assert len(s["line"]) == len(s["project"]) == 12
    for given, got in zip(s["line"], s["project"]):
        name, _, line = given.partition(" ")
        i = t["names"].index(name)
        want, junctions = T.project_line(line, (name, len(T.HOST_GENOME[t["exons"][i][0][0]])), t["exons"][i])
        assert got == "%d %s" % (junctions, want), line


def test_exports_and_header_agree():
    from tksm_amd import _lib
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "tksmseq.h")).read()
    names = ("tksmseq_targets_from_transcripts", "tksmseq_targets_get", "tksmseq_targets_download", "tksmseq_targets_write_fasta", "tksmseq_targets_free",
             "tksmseq_map_targets")
    for name in names:
        assert name in _lib.SYMBOLS and re.search(rf"\b{name}\s*\(", header) and hasattr(lib, name), name
    assert ctypes.sizeof(_lib.TargetsInfo) == 80 and ctypes.sizeof(_lib.MapTargetsParams) == 8 and ctypes.sizeof(_lib.ProjectInfo) == 32
    for struct, cls in (("tksmseq_targets_info", _lib.TargetsInfo), ("tksmseq_map_targets_params", _lib.MapTargetsParams), ("tksmseq_project_info", _lib.ProjectInfo)):
        fields = re.search(rf"typedef struct {struct} \{{(.*?)\}} {struct};", header, re.S).group(1)
        fields = re.sub(r"/\*.*?\*/", "", fields, flags=re.S)
        got = [n.split("[")[0].strip() for part in re.findall(r"(?:uint64_t|int64_t|int32_t|float|double)\s+([^;]+);", fields) for n in re.split(r",\s*", part.strip())]
        assert got == [n for n, _ in cls._fields_], struct
    assert [n for n, _ in _lib.TargetsInfo._fields_][:9] == list(T.COUNTERS) and [n for n, _ in _lib.ProjectInfo._fields_] == list(T.PROJECT_COUNTERS)
    assert "map, annotated targets:" in header
    argtypes = lib.tksmseq_map_targets.argtypes
    assert len(argtypes) == 14 and argtypes[2]._type_ is _lib.MapTargetsParams and argtypes[13]._type_ is _lib.ProjectInfo
    # the product does not import the specification, and the splice kernel uses no floating point
    for root, _, files in os.walk(os.path.join(ROOT, "tksm_amd")):
        for f in files:
            if f.endswith((".py", ".cpp", ".h", ".hip")):
                assert "map_targets_spec" not in open(os.path.join(root, f), errors="replace").read(), f
    for name in ("map_targets_kernels.hip", "map_targets_kernels.h"):
        kernels = open(os.path.join(ROOT, "tksm_amd", "csrc", name)).read()
        assert not re.search(r"\b(float|double)\b", re.sub(r"//.*", "", kernels)), name


def test_python_signatures():
    from tksm_amd.sequence import Sequencer, Targets
    sig = inspect.signature(Sequencer.map).parameters
    assert (sig["targets"].default, sig["genome_coords"].default) == (None, False)
    assert list(inspect.signature(Sequencer.targets).parameters) == ["self"]
    assert inspect.signature(Targets.write_fasta).parameters["line_width"].default == 60
    for name in ("download", "write_fasta", "free"):
        assert callable(getattr(Targets, name))
    with pytest.raises(ValueError, match="targets="):
        Sequencer.map(None, "reads.fq", "out.paf", genome_coords=True)             # (refused before the context is touched)


def _module(*args):
    return subprocess.run([EXE, "map", *[str(a) for a in args]], capture_output=True, text=True)


def test_module_argument_checks_and_exit_codes(tmp_path):
    out, fa = tmp_path / "o.paf", tmp_path / "t.fa"
    need = ["-r", tmp_path / "genome.fa", "--reads", tmp_path / "reads.fq", "-o", out, "--devices", "99"]   # (no such device: what got past the checks fails with 1)
    r = _module(*need, "--genome-coords")
    assert r.returncode == 2 and "map: error: --genome-coords needs -g" in r.stderr, r.stderr
    r = _module(*need, "--targets-out", fa)
    assert r.returncode == 2 and "map: error: --targets-out needs -g" in r.stderr, r.stderr
    # with -g --targets-out the FASTA may be the only output; --reads and -o come together
    base = ["-r", tmp_path / "genome.fa", "-g", tmp_path / "genes.gtf", "--devices", "99"]
    r = _module(*base, "--targets-out", fa, "--reads", tmp_path / "reads.fq")
    assert r.returncode == 2 and "the following arguments are required: -o/--output" in r.stderr, r.stderr
    r = _module(*base, "--targets-out", fa, "-o", out)
    assert r.returncode == 2 and "the following arguments are required: --reads" in r.stderr, r.stderr
    r = _module(*base)
    assert r.returncode == 2 and "the following arguments are required: --reads, -o/--output" in r.stderr, r.stderr
    r = _module("-g", tmp_path / "genes.gtf", "--targets-out", fa)
    assert r.returncode == 2 and "the following arguments are required: -r/--reference" in r.stderr, r.stderr
    r = _module(*base, "--targets-out", fa, "--genome-coords")
    assert r.returncode == 2 and "map: error: --genome-coords needs --reads and -o" in r.stderr, r.stderr
    # what passes the checks goes on to open the device
    for args in ([*base, "--targets-out", fa], [*need, "-g", tmp_path / "genes.gtf"], [*need, "--gtf", "a.gtf,b.gtf", "--genome-coords", "--targets-out", fa, "-c", "--split"]):
        r = _module(*args)
        assert r.returncode == 1 and "map: error" not in r.stderr, (args, r.stderr)
    assert not out.exists() and not fa.exists()
    text = _module("--help").stdout
    assert "[-g GTF[,GTF...] [--genome-coords] [--targets-out CDNA.fa[.gz]]]" in text
