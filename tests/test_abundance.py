"""abundance without a GPU: the specification (tests/abundance_spec.py) against the files the reference's own script wrote
(tests/golden/abundance/, tests/golden/make_abundance_golden.py), the host code (PAF reader and interner, lr-br and whitelist readers, the
--cb-count draws, the writer) under ASan / UBSan in a stand-alone program, and the module's argument checks."""
import ctypes
import gzip
import json
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

import abundance_spec as A

AB = os.path.join(GOLDEN, "abundance")
PAF = os.path.join(AB, "reads.paf")
LR = os.path.join(AB, "lr_matches.tsv")
EXE = os.path.join(ROOT, "tksm_amd", "tksm")
RUNS = {"default": {}, "em0": {"em_iterations": 0}, "em1": {"em_iterations": 1}, "lr_br": {"lr_br": LR}}


@pytest.mark.parametrize("name", list(RUNS))
def test_spec_reproduces_the_reference_written_tables(name):
    got = A.run(PAF, **RUNS[name])
    assert got["tsv"] == open(os.path.join(AB, f"expected_{name}.tsv")).read()


def test_spec_abundance_vector_and_the_planted_reads():
    ref = json.load(open(os.path.join(AB, "expected_abundance.json")))
    got = A.run(PAF)
    assert len(got["surviving"]) == ref["surviving_reads"]
    want = np.array([float(ref["abundance"].get(t, "0.0")) for t in got["transcripts"]])
    assert (want > 0).sum() == len(ref["abundance"])
    rel = np.abs(got["abundance"] - want)[want > 0] / want[want > 0]
    print(f"worst relative difference {rel.max():.3g}")
    assert rel.max() <= 1e-12 and (got["abundance"][want == 0] == 0).all()
    t = got["transcripts"].index
    hits = got["uniform_hits"]
    name = lambda k: f"ENST{k:05d}.{1 + k % 4}"      # noqa: E731
    assert hits["edge_ratio_95_96"] == [(t(name(3)), 0.5), (t(name(5)), 0.5)]
    assert hits["edge_ratio_19_20"] == [(t(name(6)), 1.0)]
    assert hits["edge_start_19_best"] == [(t(name(8)), 0.5), (t(name(10)), 0.5)]
    assert hits["edge_start_20_best"] == [(t(name(11)), 0.5), (t(name(13)), 0.5)]
    assert hits["edge_half_exactly"] == [(t(name(14)), 1.0)] and "edge_half_under" not in hits
    assert hits["edge_tie_later_full"] == [(t(name(17)), 1.0)] and "edge_tie_drops" not in hits
    assert hits["edge_same_transcript"] == [(t(name(21)), 0.5), (t(name(21)), 0.5)]
    assert hits["edge_first_length"] == [(t(name(23)), 1.0)]
    assert "ENSTDROP.1" in got["transcripts"] and "ENSTDROP.1" not in got["tsv"]
    lines = open(PAF).read().splitlines()
    reads = [ln.split("\t")[0] for ln in lines]
    apart = sum(1 for r in set(reads) if (lambda at: at[-1] - at[0] + 1 > len(at))([i for i, x in enumerate(reads) if x == r]))
    assert apart >= 25, "the fixture must hold reads whose lines are not adjacent"


def test_spec_cell_draws():
    """the --cb-count statement: letters within the IUPAC sets, whitelist draws with replacement, weights and dropout entry, the inverse CDF"""
    bc = A.barcodes_from_pattern("NRYKMSWBDHVACGT", 200, 42)
    for b in bc:
        assert len(b) == 15 and all(c in A.IUPAC[p] for c, p in zip(b, "NRYKMSWBDHVACGT")) and b.endswith("ACGT")
    assert len(set(b[0] for b in bc)) == 4 and bc == A.barcodes_from_pattern("NRYKMSWBDHVACGT", 200, 42) != A.barcodes_from_pattern("NRYKMSWBDHVACGT", 200, 43)
    assert A.barcodes_from_pattern("NRYKMSWBDHVACGT", 5, 42) == bc[:5]          # keyed by (barcode, position): a prefix
    wl = ["AAA", "CCC", "", "GGG"]
    drawn = A.barcodes_from_whitelist(wl, 400, 7)
    assert set(drawn) == set(wl) and drawn[:6] == A.barcodes_from_whitelist(wl, 6, 7)
    cdf = A.cell_cdf(4, 42, 10.0, 1.0, 0.2)
    w = np.diff(np.concatenate([[0.0], cdf]))
    assert (w > 0).all() and abs(w[-1] / cdf[-1] - 0.2) < 1e-12
    assert list(A.cell_cdf(3, 42, 10.0, 1.0, 1.0)) == [0, 0, 0, 1] and (A.draw_cells(50, 1, A.cell_cdf(3, 42, 10.0, 1.0, 1.0)) == 3).all()
    assert A.cell_cdf(4, 42, 10.0, 1.0, 0.0)[-1] == A.cell_cdf(4, 42, 10.0, 1.0, 0.0)[-2] and (A.draw_cells(5000, 1, A.cell_cdf(4, 42, 10.0, 1.0, 0.0)) < 4).all()
    k = A.draw_cells(20000, 5, cdf)
    assert (k[:100] == A.draw_cells(100, 5, cdf)).all()                         # keyed by the read's index: a prefix
    share = np.bincount(k, minlength=5) / 20000.0
    assert np.abs(share - w / cdf[-1]).max() < 0.02


def _ordered_against_the_specification(paf, what, **kw):
    """abundance_spec.ordered_run (the device's documented order of addition) against abundance_spec.run (left to right): the same rows,
    every number within the 1e-9 gate of tests/test_abundance_gpu.py"""
    spec, got = A.run(paf, **kw), A.ordered_run(paf, **kw)
    assert [(n, c) for n, c, _ in got["rows"]] == [(n, c) for n, c, _ in spec["rows"]] and len(spec["rows"]) > 0
    pairs = {"abundance": (got["abundance"], spec["abundance"]), "tpm": (got["tpm"], np.array([t for _, _, t in spec["rows"]])),
             "final weights": (got["hit_weights"], np.array([w for hits in spec["hits"].values() for _, w in hits])),
             "uniform weights": (got["uniform_weights"], np.array([w for hits in spec["uniform_hits"].values() for _, w in hits]))}
    for k, (a, b) in pairs.items():
        assert a.shape == b.shape and np.isfinite(a).all(), k
        rel = np.abs(a - b)[b > 0] / b[b > 0]
        print(f"{what}: {k}: worst relative difference {rel.max():.3g}")
        assert rel.max() <= 1e-9 and (a[b == 0] == 0).all(), k
    assert (pairs["uniform weights"][0] == pairs["uniform weights"][1]).all()
    return got


@pytest.mark.parametrize("name", list(RUNS))
def test_ordered_run_agrees_with_the_specification_on_the_fixture(name):
    _ordered_against_the_specification(PAF, name, **RUNS[name])


def test_ordered_run_agrees_with_the_specification_on_a_synthetic_case(tmp_path):
    """a (transcript, cell) segment of three chunks, 700 transcripts (three blocks), a run of transcripts without hits, unnamed reads"""
    def line(rid, t, matches, block=950):
        return f"{rid}\t1000\t0\t{block}\t+\t{t}\t9000\t0\t{block}\t{matches}\t{block}\t60\n"
    lines, cells = [], []
    for i in range(2600):
        lines.append(line(f"b{i}", "big", 900))
        if i % 5 == 0:
            lines.append(line(f"b{i}", f"s{i // 5 % 300}", 870 + i % 25))
        if i % 4:
            cells.append(f"b{i}\t0\t1\t0\tC{i % 3 % (1 + i % 2)}\n")
        if i == 1300:
            lines += [line(f"d{j}", f"h{j}", 390, 400) for j in range(30)]
    lines += [line(f"u{i}", f"v{i}", 900) for i in range(400)]
    paf, lr = tmp_path / "a.paf", tmp_path / "cells.tsv"
    paf.write_text("".join(lines))
    lr.write_text("".join(cells))
    for kw in ({}, {"lr_br": lr}, {"lr_br": lr, "em_iterations": 0}, {"em_iterations": 1}):
        got = _ordered_against_the_specification(paf, f"synthetic {sorted(kw)}", **kw)
        assert len(got["abundance"]) == 731 and (got["abundance"][[t for t, n in enumerate(A.parse_paf(paf)[0]) if n.startswith("h")]] == 0).all()


def test_ordered_runs_trees_are_the_documented_ones():
    """inputs on which another pairing gives another double: 2^53 + 1 rounds to 2^53, 2^53 + 2 is exact"""
    big = 2.0 ** 53
    v = np.zeros(64)
    v[[0, 32, 48]] = big, 1.0, 1.0
    assert A._wave_tree(v) == big                                    # (0 + 32) loses the 1, then (16 + 48) = 1 is lost too; neighbours first gives 2^53 + 2
    v = np.zeros(256)
    v[[0, 128, 192]] = big, 1.0, 1.0
    assert A._block_tree(v) == big + 2.0                             # (w0 + w1) + (w2 + w3); (w0 + w2) + (w1 + w3) gives 2^53
    x = np.zeros(1025)
    x[[0, 64, 1024]] = big, 1.0, 1.0                                 # lane 0 adds 0, 64, ... in order: the 1 is lost; position 1024 is the second chunk
    sums, total = A.segment_sums(x, [0, 1025])
    assert sums[0] == big and total == big
    sums, total = A.segment_sums(np.ones(600), np.arange(601))       # 600 segments: three blocks, the total by one block
    assert (sums == 1.0).all() and total == 600.0
    parts = np.zeros(257)
    parts[[0, 256]] = big, 1.0                                       # thread 0 adds parts 0 and 256
    assert A._block_tree(A._strided(parts, 256)) == big


@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    """tools/sanitize_abund_host.cpp built with ASan + UBSan and run on the fixtures: {key: [lines]} of what it printed"""
    d = tmp_path_factory.mktemp("abund_host")
    exe = d / "sanitize_abund_host"
    csrc = os.path.join(ROOT, "tksm_amd", "csrc")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-I", csrc, "-o", str(exe),
                    os.path.join(ROOT, "tools", "sanitize_abund_host.cpp"), os.path.join(csrc, "abund_host.cpp"), "-lz"], check=True)
    r = subprocess.run([str(exe), PAF, LR, str(d)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr
    out = {}
    for line in r.stdout.splitlines():
        key, _, rest = line.partition(" ")
        out.setdefault(key, []).append(rest)
    return d, out


def test_host_code_under_sanitizers_matches_the_specification(host_program):
    d, out = host_program
    tnames, reads = A.parse_paf(PAF)
    recs = [r for rs in reads.values() for r in rs]
    want = sum((i + 1) * (r["tid"] + 3 * r["target_start"] + 5 * r["num_matches"] + 7 * r["block"]) for i, r in enumerate(recs))
    qsum = sum((i + 1) * rs[0]["query_length"] for i, rs in enumerate(reads.values()))
    n_lines = len(open(PAF).read().splitlines())
    assert out["paf"] == [f"{len(reads)} {len(tnames)} {len(recs)} {n_lines} {want} {qsum}"]
    assert out["first"] == [f"{list(reads)[0]} {list(reads)[-1]} {tnames[0]} {tnames[-1]}"]
    ok, bad = [int(v) for v in out["truncated"][0].split()]
    assert ok >= 1 and bad >= 1 and ok + bad == (os.path.getsize(PAF) + 996) // 997
    parse = [p.split(" ", 4) for p in out["parse"]]
    assert [int(p[0]) for p in parse] == [1, 0, 0, 0, 1, 1, 1, 0, 0, 0, 0, 1, 0, 1, 1, 0, 0]
    assert all("PAF line 1" in p[4] for p in parse if p[0] == "0" and p is not parse[12]) and "PAF line 2" in parse[12][4]
    assert out["group"] == ["0 2 3 | 0:0:1:1 1:5:6:7 1:0:1:1 | 1 2"]
    lr = A.parse_lr_br(LR)
    assert out["lrbr"] == [f"{len(lr)} {sum(sum((k + '=' + v).encode()) for k, v in lr.items())}"]
    assert [p.split(" ")[:3] for p in out["lrparse"]] == [["1", "0", "-"], ["1", "1", "BC"], ["1", "1", "BC"], ["0", "0", "-"], ["0", "0", "-"], ["1", "0", "-"],
                                                          ["1", "1", "Y"], ["1", "0", "-"], ["0", "0", "-"]]
    assert out["whitelist"] == ["4 AAA|CCC||GGG"] and out["pattern_ok"] == ["1 0"]
    assert out["barcodes"][0].split() == A.barcodes_from_pattern("NRYKMSWBDHVACGT", 5, 42)
    assert out["drawn"][0] == " ".join(f"[{b}]" for b in A.barcodes_from_whitelist(["AAA", "CCC", "", "GGG"], 6, 7))
    got, want = np.array([float(v) for v in out["cdf"][0].split()]), A.cell_cdf(4, 42, 10.0, 1.0, 0.2)
    assert np.abs(got / want - 1).max() <= 1e-14                      # (two maths libraries: an ulp of exp, log or cos)
    assert out["cdf_all_dropout"] == ["0 0 0 1"] and out["cdf_none"] == ["1"] and out["args"] == ["1 0 0 0 0 0"]
    assert out["tsv_ok"] == ["1"] and out["tsv_bad"] == ["0"] and out["write"] == ["1 1 0"] and out["gz_round_trip"] == ["1"] and out["missing"] == ["0"]
    text = open(d / "a.tsv").read()
    assert text == "target_id\ttpm\tcell\nt0\t500000.000\t.\nt1\t250000.000\tACGT\nt1\t0.001\t.\nt1\t123.457\tACGT\n"      # 0.000999 and 0 are skipped
    assert gzip.open(d / "a.tsv.gz", "rt").read() == text
    assert not os.path.exists(d / "a.tsv.tmp") and not os.path.exists(d / "no")


def _module(*args):
    return subprocess.run([EXE, "abundance", *[str(a) for a in args]], capture_output=True, text=True)


def test_module_argument_checks_and_exit_codes(tmp_path):
    out = tmp_path / "a.tsv"
    r = _module("-o", out)
    assert r.returncode == 2 and "abundance: error:" in r.stderr and "-p/--paf" in r.stderr and "-o/--output" not in r.stderr
    r = _module("-p", PAF)
    assert r.returncode == 2 and "-o/--output" in r.stderr
    r = _module()
    assert r.returncode == 2 and "-p/--paf, -o/--output" in r.stderr
    r = _module("-p", PAF, "-o", out, "--nope")
    assert r.returncode == 2 and "--nope" in r.stderr
    r = _module("-p", PAF, "-o", out, "-em", "ten")
    assert r.returncode == 2
    r = _module("-p", PAF, "-o", out, "--cb-count", "4", "-m", LR)
    assert r.returncode == 2 and "abundance: error: --lr-br must not be set with --cb-count" in r.stderr
    r = _module("-p", PAF, "-o", out, "--cb-count", "4", "--cb-pattern", "NNXN")
    assert r.returncode == 2 and "abundance: error: --cb-pattern must contain only valid IUPAC nucleotide letters: <X> not in A,C,G,T,R,Y,K,M,S,W,B,D,H,V,N" in r.stderr
    r = _module("-p", PAF, "-o", out, "--cb-count", "4", "--cb-pattern", "")
    assert r.returncode == 2 and "--cb-pattern or --cb-txt must be set with --cb-count" in r.stderr
    for bad in ("1.5", "-0.1", "nan"):
        r = _module("-p", PAF, "-o", out, "--cb-count", "4", "--cb-dropout", bad)
        assert r.returncode == 2 and "abundance: error: --cb-dropout must be between 0 and 1" in r.stderr, bad
    for bad in ("10,0", "10,-1", "10", "1,2,3", "a,b"):
        r = _module("-p", PAF, "-o", out, "--cb-count", "4", "--cb-lognorm-params", bad)
        assert r.returncode == 2 and "--cb-lognorm-params" in r.stderr, bad
    r = _module("-p", PAF, "-o", out, "--verbosity", "LOUD")
    assert r.returncode == 1 and "unknown verbosity level" in r.stderr
    r = _module("--list")
    assert r.returncode == 0 and r.stdout.split() == ["help", "paf", "lr_br", "cb_count", "cb_lognorm_params", "cb_pattern", "cb_dropout", "cb_txt", "output",
                                                      "em_iterations", "random_seed", "verbose", "list", "devices", "verbosity", "log_file"]
    assert _module("-h").returncode == 0
    assert not out.exists()
    r = subprocess.run([EXE, "list"], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.split() == ["sequence", "pcr", "truncate", "polyA", "tag", "scb", "flip"]


def test_module_has_no_cpu_fallback(tmp_path):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    r = _module("-p", PAF, "-o", tmp_path / "a.tsv")
    assert r.returncode == 1 and "no HIP device" in r.stderr and not (tmp_path / "a.tsv").exists()


def test_exports_and_header_agree():
    from tksm_amd import _lib
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "tksmseq.h")).read()
    names = [s for s in _lib.SYMBOLS if s.startswith("tksmseq_abundance")]
    assert len(names) == 12
    for s in names:
        assert re.search(rf"\b{s}\s*\(", header) and hasattr(lib, s)
    assert ctypes.sizeof(_lib.AbundanceParams) == 72
    src = open(os.path.join(ROOT, "tksm_amd", "csrc", "abund_kernels.h")).read()
    assert f"ABUND_CHUNK = {_lib.ABUND_CHUNK};" in src
    for stream, what in ((57, "ST_ABUND_BC"), (58, "ST_ABUND_BC_TXT"), (59, "ST_ABUND_WEIGHT"), (60, "ST_ABUND_CELL")):
        assert f"stream {stream}" in header and re.search(rf"{what} = {stream}\b", open(os.path.join(ROOT, "tksm_amd", "csrc", "abund_host.h")).read())
    assert (A.ST_BC, A.ST_BC_TXT, A.ST_WEIGHT, A.ST_CELL) == (57, 58, 59, 60)
    # the product does not import the specification
    for root, _, files in os.walk(os.path.join(ROOT, "tksm_amd")):
        for f in files:
            if f.endswith((".py", ".cpp", ".h", ".hip")):
                assert "abundance_spec" not in open(os.path.join(root, f), errors="replace").read(), f
