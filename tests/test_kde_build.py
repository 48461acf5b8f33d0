"""model-truncation without a GPU: the numpy specification (tests/kde_spec.py) against scikit-learn run exactly (leaf_size >= N: one leaf,
brute force) and against the three model files the reference's own script wrote (tests/golden/kde_build/, default kd_tree: approximate, so
only cells >= 1e-9 of the maximum are compared, at relative 1e-5 -- about 25 x the 3.8e-7 measured for the tree), the seeded bandwidth
search against GridSearchCV on the same subsample, the host code (PAF reader, histogram, model writer) under ASan / UBSan in a stand-alone
program, and the module's argument checks."""
import json
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

import kde_spec as K

KB = os.path.join(GOLDEN, "kde_build")
PAF = os.path.join(KB, "reads.paf")
EXE = os.path.join(ROOT, "tksm_amd", "tksm")
SETTINGS = {"model_default": {}, "model_lengths": {"model_lengths": True}, "model_end_ratio": {"end_ratio": 0.3}}


@pytest.fixture(scope="module")
def xy():
    return K.read_paf(PAF)[0]


def test_spec_grid_is_the_exact_density(xy):
    """vs KernelDensity with one leaf (brute force) and vs the cell-by-cell log-sum-exp: relative 1e-10 in every cell >= 1e-290, absolute
    1e-290 below"""
    sk = pytest.importorskip("sklearn.neighbors")
    _, c = K.grid_axes(0, 3000, 100)
    X, Y = np.meshgrid(c, c, indexing="ij")
    pts = np.stack([X.ravel(), Y.ravel()], 1).astype(float)
    for h in (120.0, 30.0):
        want = np.exp(sk.KernelDensity(bandwidth=h, leaf_size=len(xy) + 1, rtol=0, atol=0).fit(xy).score_samples(pts)).reshape(len(c), len(c))
        got = K.kde_grid_spec(xy, c, c, h)
        big = want >= 1e-290
        rel = np.abs(got[big] / want[big] - 1).max()
        print(f"h={h}: worst relative {rel:.3g} in {big.sum()} cells")
        assert rel <= 1e-10 and (np.abs(got[~big] - want[~big]) <= 1e-290).all()
    bf = K.kde_grid_bruteforce(xy[:300], c[:7], c[5:12], 120.0)
    assert np.abs(K.kde_grid_spec(xy[:300], c[:7], c[5:12], 120.0) / bf - 1).max() <= 1e-12


@pytest.mark.parametrize("name", list(SETTINGS))
def test_spec_matches_the_reference_written_models(name):
    ref = json.load(open(os.path.join(KB, name + ".json")))
    got = K.model_spec(PAF, bandwidth=120.0, grid_end=3000, **SETTINGS[name])
    assert [p["name"] for p in got] == [p["name"] for p in ref] == ["KDE_mtx", "end_mtx"]
    for a, b in zip(got, ref):
        assert a["shape"] == b["shape"] and a["labels"] == b["labels"]
    assert got[1]["data"] == ref[1]["data"]                       # integer work: equal to numpy's histogram
    a, b = np.array(got[0]["data"]), np.array(ref[0]["data"])
    inside = b >= 1e-9 * b.max()
    assert inside.sum() * 3 >= inside.size, "the mask must not hide a failure"
    worst = np.abs(a[inside] / b[inside] - 1).max()
    print(f"{name}: {inside.sum()} of {inside.size} cells compared, worst ratio - 1 = {worst:.3g}")
    assert worst <= 1e-5


def test_spec_bandwidth_search_matches_grid_search_cv(xy):
    ms = pytest.importorskip("sklearn.model_selection")
    nb = pytest.importorskip("sklearn.neighbors")
    bw, scores, folds, draws = K.cv_bandwidth_spec(xy, 42, 1500, with_folds=True)
    best = []
    for r in range(3):
        order = np.sort(scores[r])[::-1]
        assert (order[0] - order[1]) / abs(order[0]) > 1e-6, "choose another seed for the fixture"
        pts = xy[draws[r]]
        gs = ms.GridSearchCV(nb.KernelDensity(leaf_size=len(pts) + 1, rtol=0, atol=0), {"bandwidth": np.arange(50, 1000, 100)}, cv=3).fit(pts)
        for f in range(3):
            want = gs.cv_results_[f"split{f}_test_score"]
            assert np.abs(folds[r, f] / want - 1).max() <= 1e-9, (r, f)
        assert K.BANDWIDTHS[int(np.argmax(scores[r]))] == gs.best_params_["bandwidth"]
        best.append(gs.best_params_["bandwidth"])
    assert bw == np.median(best)
    assert list(K.fold_bounds(1501)) == [0, 501, 1001, 1501] and list(K.fold_bounds(1502)) == [0, 501, 1002, 1502]


def test_spec_small_behaviours(tmp_path):
    counts, labels = K.end_histogram([1.0, 0.99, 0.995, 0.0, 0.01])
    assert counts[99] == 3 and counts[0] == 1 and counts[1] == 1 and sum(counts) == 5 and len(labels) == 100 and labels[-1] == 1.0
    assert K.end_histogram([0.2, 0.9, 1.0], end_ratio=0.3)[0][30 if 0.3 >= np.arange(0, 1.01, 0.01)[30] else 29] == 3
    idx, c = K.grid_axes(0, 1050, 100)                            # end - start no multiple of the step: the last index is 1000
    assert list(idx) == list(range(0, 1001, 100)) and list(c) == list(range(50, 1000, 100))
    assert list(K.grid_axes(0, 100, 100)[1]) == [50]
    with pytest.raises(ValueError):
        K.grid_axes(0, 99, 100)
    paf = tmp_path / "t.paf"
    paf.write_text("a\t1\t0\t1\t+\tt\t1000\t100\t700\ttp:A:P\nb\t1\t0\t1\t-\tt\t1000\t100\t700\ttp:A:P\nc\t1\t0\t1\t+\tt\t500\t0\t500\ttp:A:P\nd\t1\t0\t1\t+\tt\t9\t1\t2\ttp:A:S\n")
    pts, ratios = K.read_paf(paf)
    assert pts.tolist() == [[400, 1000], [400, 1000], [0, 500]] and ratios == [0.75, 0.25]
    pts, ratios = K.read_paf(paf, model_lengths=True)
    assert pts.tolist() == [[1000, 600], [1000, 600], [500, 500]] and ratios == [0.75, 0.25]


@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    """tools/sanitize_kde_host.cpp built with ASan + UBSan and run on the fixture PAF: {key: [lines]} of what it printed"""
    d = tmp_path_factory.mktemp("kde_host")
    exe = d / "sanitize_kde_host"
    csrc = os.path.join(ROOT, "tksm_amd", "csrc")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-I", csrc, "-o", str(exe),
                    os.path.join(ROOT, "tools", "sanitize_kde_host.cpp"), os.path.join(csrc, "kde_host.cpp")], check=True)
    r = subprocess.run([str(exe), PAF, str(d)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr
    out = {}
    for line in r.stdout.splitlines():
        key, _, rest = line.partition(" ")
        out.setdefault(key, []).append(rest)
    return d, out


def test_host_code_under_sanitizers_matches_numpy_and_the_reference(host_program):
    d, out = host_program
    for ml, name in ((0, "model_default"), (1, "model_lengths")):
        pts, ratios = K.read_paf(PAF, model_lengths=bool(ml))
        f = out["sample"][ml].split()
        assert [int(f[0]), int(f[1]), int(f[2])] == [ml, len(pts), len(ratios)] and float(f[3]) == pts[:, 0].sum() and float(f[4]) == pts[:, 1].sum()
        ref = json.load(open(os.path.join(KB, name + ".json")))
        assert [int(v) for v in out["hist"][ml].split()[1:]] == ref[1]["data"]
        assert out["write"][ml] == f"{ml} 1"
        got = json.load(open(d / f"model_{ml}.json"))           # the writer's file: parses, integer labels, the reference's end_mtx
        assert got[1] == ref[1] and got[0]["labels"] == ref[0]["labels"] and got[0]["shape"] == [30, 30]
        P = (1.0 / (np.arange(900) + 3)).reshape(30, 30)
        assert got[0]["data"] == list(P.T.flatten())              # %.17g round-trips every double; data is P.T flattened
        assert not os.path.exists(d / f"model_{ml}.json.tmp")
    assert out["unwritable"] == ["0"] and out["nonfinite"] == ["0"] and not os.path.exists(d / "inf.json") and not os.path.exists(d / "inf.json.tmp")
    # the edge rule, against numpy on the same doubles
    r = [0.0, 0.01, 0.0099999999999999985, 0.29, 0.28999999999999998, 0.29000000000000004, 0.57, 0.58, 0.99, 1.0, 1.0000000000000002, -1e-300, -0.0,
         float("nan"), float("inf"), 0.07, 0.07000000000000001, 0.14, 0.14000000000000001]
    finite = [v for v in r if np.isfinite(v)]
    counts, edges = np.histogram(finite, bins=np.arange(0, 1.01, 0.01))
    assert [int(v) for v in out["edges"][0].split()] == [int(c) for c in counts]
    assert [float(v) for v in out["labels"][0].split()] == list(edges[1:])
    # malformed and odd PAF lines: 13 texts x 2 modes
    parse = [p.split(" ", 4) for p in out["parse"]]
    assert len(parse) == 26
    ok = [int(p[1]) for p in parse[::2]]
    assert ok == [1, 1, 0, 0, 1, 1, 0, 0, 1, 0, 1, 1, 0]
    assert "PAF line 1" in parse[4][4] and [int(parse[8][2]), int(parse[8][3])] == [1, 1] and [int(parse[20][2]), int(parse[20][3])] == [1, 0]
    assert int(parse[22][2]) == 0 and "PAF line 1" in parse[24][4]
    for line in out["axes"]:
        a, b, s, ok, *rest = line.split()
        try:
            idx, c = K.grid_axes(int(a), int(b), int(s)) if int(s) > 0 else (None, None)
        except ValueError:
            idx = None
        assert int(ok) == (idx is not None), line
        if idx is not None:
            bar = rest.index("|")
            assert [int(v) for v in rest[:bar]] == list(idx) and [float(v) for v in rest[bar + 1:]] == list(c)


def _module(*args):
    return subprocess.run([EXE, "model-truncation", *[str(a) for a in args]], capture_output=True, text=True)


def test_module_argument_checks_and_exit_codes(tmp_path):
    out = tmp_path / "m.json"
    r = _module("-o", out)
    assert r.returncode == 2 and "-i/--input" in r.stderr and "-o/--output" not in r.stderr
    r = _module("-i", PAF)
    assert r.returncode == 2 and "-o/--output" in r.stderr
    r = _module()
    assert r.returncode == 2 and "-i/--input, -o/--output" in r.stderr
    r = _module("-i", PAF, "-o", out, "--nope")
    assert r.returncode == 2 and "--nope" in r.stderr
    r = _module("-i", PAF, "-o", out, "--grid-step", "ten")
    assert r.returncode == 2
    for bad in ("1.5", "-0.5", "nan"):
        r = _module("-i", PAF, "-o", out, "--end-ratio", bad)
        assert r.returncode == 1 and "--end-ratio" in r.stderr, bad
    r = _module("-i", PAF, "-o", out, "--verbosity", "LOUD")
    assert r.returncode == 1 and "unknown verbosity level" in r.stderr
    r = _module("--list")
    assert r.returncode == 0 and r.stdout.split() == ["help", "input", "output", "bandwidth", "grid_start", "grid_end", "grid_step", "threads", "model_lengths", "list",
                                                      "end_ratio", "seed", "cv_samples", "devices", "verbosity", "log_file"]
    assert _module("-h").returncode == 0
    assert not out.exists()
    r = subprocess.run([EXE, "list"], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.split() == ["sequence", "pcr", "truncate", "polyA", "tag", "scb", "flip"]


def test_module_has_no_cpu_fallback(tmp_path):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    r = _module("-i", PAF, "-o", tmp_path / "m.json", "--grid-end", "3000")
    assert r.returncode == 1 and "no HIP device" in r.stderr and not (tmp_path / "m.json").exists()


def test_exports_and_header_agree():
    from tksm_amd import _lib
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "tksmseq.h")).read()
    for s in ("tksmseq_kde_grid", "tksmseq_kde_cv_bandwidth", "tksmseq_model_truncation", "tksmseq_model_truncation_main"):
        assert re.search(rf"\b{s}\s*\(", header) and s in _lib.SYMBOLS and hasattr(lib, s)
    import ctypes
    assert ctypes.sizeof(_lib.KdeModelParams) == 64
    src = open(os.path.join(ROOT, "tksm_amd", "csrc", "kde_kernels.h")).read()
    assert f"KDE_CHUNK = {_lib.KDE_CHUNK};" in src
