"""model-truncation on the device (-m gpu): tksmseq_kde_grid, tksmseq_kde_cv_bandwidth, tksmseq_model_truncation, `tksm model-truncation`
and tksm_amd.build_tail_model against the numpy specification (tests/kde_spec.py) and the files the reference's own script wrote
(tests/golden/kde_build/, tests/golden/make_kde_build_golden.py).

The gate of a density: relative 1e-10 in cells >= 1e-290, absolute 1e-290 below.  It is derived, not measured: a cell is a sum of N
non-negative terms (N 2^-53 relative), each the exponential of an argument of at most 745 known to a few ulp (745 x 2^-52 relative per ulp
of the argument) and a few ulp of exp itself -- below 1e-10 for N <= 1e5."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ERR_MODEL, GOLDEN, QS_MODEL, ROOT

sys.path.insert(0, os.path.join(ROOT, "oracle"))

import kde_spec as K  # noqa: E402

pytestmark = pytest.mark.gpu
KB = os.path.join(GOLDEN, "kde_build")
PAF = os.path.join(KB, "reads.paf")
EXE = os.path.join(ROOT, "tksm_amd", "tksm")
SETTINGS = {"model_default": ([], {}), "model_lengths": (["--model-lengths"], {"model_lengths": True}),
            "model_end_ratio": (["--end-ratio", "0.3"], {"end_ratio": 0.3})}


@pytest.fixture(scope="module")
def S():
    from tksm_amd.sequence import Sequencer
    s = Sequencer(0)
    yield s
    s.close()


def gate(got, want, what=""):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, what
    assert np.isfinite(got).all(), f"{what}: NaN or inf"
    big = want >= 1e-290
    rel = np.abs(got[big] - want[big]) / want[big] if big.any() else np.zeros(1)
    small = np.abs(got[~big] - want[~big]) if (~big).any() else np.zeros(1)
    print(f"{what}: worst relative {rel.max():.3g} in {int(big.sum())} cells, worst absolute below 1e-290: {small.max():.3g}")
    assert rel.max() <= 1e-10, what
    assert small.max() <= 1e-290, what


def sample(n, seed=1):
    rs = np.random.RandomState(seed)
    tlen = np.clip(rs.lognormal(7.0, 0.45, n), 300, 2900).astype(np.int64)
    trunc = np.minimum(tlen - 100, rs.gamma(1.6, 140.0, n)).astype(np.int64) * (rs.rand(n) < 0.8)
    return np.stack([trunc, tlen], axis=1).astype(np.float64)


def centres(g, end=3000):
    return (np.arange(g) + 0.5) * (end / g)


UNEVEN_X = np.cumsum(np.random.RandomState(5).gamma(2.0, 40.0, 40))
UNEVEN_Y = np.cumsum(np.random.RandomState(6).gamma(2.0, 70.0, 23)) - 50.0
_CASES = [(n, centres(17), centres(17)) for n in (1, 3, 5, 4096, 4097)] + \
         [(20000, centres(1), centres(1)), (20000, centres(16), centres(16)), (20000, centres(17), centres(17)), (20000, centres(30), centres(30)),
          (20000, UNEVEN_X, UNEVEN_Y), (5, UNEVEN_X, UNEVEN_Y), (20000, centres(100), centres(100)),
          (300, centres(130), centres(129))]                    # more than one 128-point block of tiles on both axes


@pytest.mark.parametrize("n,px,py", _CASES, ids=[f"n{n}-{len(a)}x{len(b)}" for n, a, b in _CASES])
def test_kde_grid_matches_the_specification(S, n, px, py):
    """sample sizes around the chunk (4096 samples: one chunk exactly, one chunk + 1, five chunks) and grids around the 16-point tile
    and the 128-point tile block, square and rectangular with unevenly spaced points"""
    from tksm_amd import _lib
    assert _lib.KDE_CHUNK == 4096
    xy = sample(n)
    gate(S.kde_grid(xy, px, py, 120.0), K.kde_grid_spec(xy, px, py, 120.0), f"n={n} grid {len(px)}x{len(py)}")


def test_kde_grid_is_not_transposed(S):
    """one sample, asymmetric axes: the density peaks at the (i, j) the sample sits at, not at (j, i)"""
    px, py = np.arange(0.0, 2000.0, 100.0), np.arange(0.0, 3500.0, 100.0)
    got = S.kde_grid(np.array([[300.0, 2900.0]]), px, py, 50.0)
    assert np.unravel_index(np.argmax(got), got.shape) == (3, 29)
    gate(got, K.kde_grid_bruteforce(np.array([[300.0, 2900.0]]), px, py, 50.0), "single sample vs brute force")


def test_kde_grid_underflow_and_large_coordinates(S):
    """bandwidth 5 on the default 0 - 10 000 grid: almost every cell underflows; zeros stay zeros, nothing is NaN or inf.  Coordinates at
    2e6: the differences are exact, the exponent's range is what is exercised."""
    xy = sample(3000, seed=2)
    _, c = K.grid_axes(0, 10000, 100)
    got, want = S.kde_grid(xy, c, c, 5.0), K.kde_grid_spec(xy, c, c, 5.0)
    assert (want == 0).mean() > 0.9 and np.array_equal(got == 0, want == 0)
    gate(got, want, "bandwidth 5")
    far = sample(3000, seed=3) + 2e6
    cf = centres(30) + 2e6
    gate(S.kde_grid(far, cf, cf, 120.0), K.kde_grid_spec(far, cf, cf, 120.0), "coordinates at 2e6")
    got = S.kde_grid(far, c, c, 120.0)                            # every sample 2e6 away from every cell: all zero
    assert np.isfinite(got).all() and (got == 0).all()


def test_kde_grid_is_deterministic(S):
    xy = sample(20000)
    a = S.kde_grid(xy, centres(100), centres(100), 120.0)
    b = S.kde_grid(xy, centres(100), centres(100), 120.0)
    assert a.tobytes() == b.tobytes()


@pytest.mark.parametrize("cv_samples", [1500, 1501])
def test_cv_bandwidth_matches_the_specification(S, cv_samples):
    """integer-valued samples with duplicate rows, drawn with replacement (so a test point often coincides with a train point: d2min = 0),
    and one point far from all others that the first repeat draws exactly once (its nearest train point is thousands of units away:
    every other exponent underflows at the small bandwidths)"""
    xy = sample(3000, seed=4)
    xy[100:140] = xy[200:240]
    draw = K.cv_draw(len(xy), 7, cv_samples, 0)
    counts = np.bincount(draw, minlength=len(xy))
    assert counts.max() >= 2
    once = int(np.flatnonzero(counts == 1)[0])
    xy[once] = (9000.0, -4000.0)
    assert len(np.unique(xy, axis=0)) < len(xy)
    bw, scores = S.kde_cv_bandwidth(xy, seed=7, cv_samples=cv_samples)
    want_bw, want = K.cv_bandwidth_spec(xy, 7, cv_samples)
    rel = np.abs(scores - want) / np.abs(want)
    print(f"cv_samples {cv_samples}: bandwidth {bw} (spec {want_bw}), worst relative score difference {rel.max():.3g}")
    assert np.isfinite(scores).all() and rel.max() <= 1e-9
    assert bw == want_bw
    bw2, scores2 = S.kde_cv_bandwidth(xy, seed=7, cv_samples=cv_samples)
    assert bw2 == bw and scores2.tobytes() == scores.tobytes()


def _module(*args):
    return subprocess.run([EXE, "model-truncation", *[str(a) for a in args]], capture_output=True, text=True)


@pytest.mark.parametrize("name", list(SETTINGS))
def test_module_on_the_fixture_paf(tmp_path, name):
    flags, kw = SETTINGS[name]
    out = tmp_path / "model.json"
    r = _module("-i", PAF, "-o", out, "-b", "120", "--grid-end", "3000", "-t", "4", *flags)
    assert r.returncode == 0, r.stderr
    got = json.load(open(out))
    ref = json.load(open(os.path.join(KB, name + ".json")))
    assert [p["name"] for p in got] == ["KDE_mtx", "end_mtx"]
    for a, b in zip(got, ref):
        assert a["shape"] == b["shape"] and a["labels"] == b["labels"]
    assert got[1]["data"] == ref[1]["data"] and all(isinstance(v, int) for v in got[0]["labels"] + got[1]["data"])
    want = K.model_spec(PAF, bandwidth=120.0, grid_end=3000, **kw)
    gate(got[0]["data"], want[0]["data"], name)
    assert not os.path.exists(str(out) + ".tmp")


def test_module_bandwidth_search_names_the_specifications_bandwidth(tmp_path):
    out, log = tmp_path / "model.json", tmp_path / "log.txt"
    r = _module("-i", PAF, "-o", out, "-b", "-1", "--cv-samples", "1500", "--grid-end", "3000", "-s", "11", "--log-file", log)
    assert r.returncode == 0, r.stderr
    xy, _ = K.read_paf(PAF)
    bw, _ = K.cv_bandwidth_spec(xy, 11, 1500)
    assert f"bandwidth: {bw:.17g}" in open(log).read()
    gate(json.load(open(out))[0]["data"], K.model_spec(PAF, bandwidth=bw, grid_end=3000)[0]["data"], "searched bandwidth")


def test_written_model_round_trips_through_truncate(S, tmp_path):
    """the written model through `tksm truncate --kde-model` on the splice corpus == the oracle's truncation with the same file"""
    import mdf_ops_oracle as mo
    model_path = tmp_path / "model.json"
    S.model_truncation(PAF, model_path, bandwidth=120.0, grid_end=3000)
    src = os.path.join(GOLDEN, "splice_corpus", "mols.mdf")
    out = tmp_path / "trc.mdf"
    r = subprocess.run([EXE, "truncate", "-i", src, "-o", str(out), "--kde-model", str(model_path), "-s", "31"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    model = mo.TruncationModel(json.load(open(model_path)))
    # (every transform here takes molecules depth-unrolled -- include/tksmseq.h: a depth-0 molecule of the corpus has no copy and no index)
    mols = [md for md in mo.stream_mdf(open(src).read(), unroll=True) if md["depth"] > 0]
    want = mo.write_mdf([mo.trc_spec(md, g, 31, model=model, always_end=False, models_length=False) for g, md in enumerate(mols)])
    assert open(out).read() == want


def test_build_tail_model_loads_and_runs(tmp_path):
    import tksm_amd
    from tksm_amd.sequence import Sequencer
    rs = np.random.RandomState(9)
    n = 2000
    mapped = np.clip(rs.lognormal(6.6, 0.5, n), 200, 1900).astype(int)
    unmapped = np.where(rs.rand(n) < 0.4, np.clip(rs.gamma(2.0, 60.0, n) + 0.05 * mapped, 1, 700), 0).astype(int)
    labels = np.arange(0, 2000, 50)
    begin = [0.25, 0.25, 0.25, 0.25]
    trans = [[0.55, 0.15, 0.20, 0.10], [0.20, 0.45, 0.25, 0.10], [0.30, 0.10, 0.50, 0.10], [0.15, 0.30, 0.15, 0.40]]
    path = tmp_path / "tail.json"
    dc = tksm_amd.build_tail_model(mapped, unmapped, labels, labels, begin, trans, 60.0, path)
    ref = json.load(open(os.path.join(GOLDEN, "tail_model_reference.json")))
    got = json.load(open(path))
    assert set(got) == set(ref) and got["bases"] == ref["bases"] and got["ratio"] == float((unmapped > 0).mean())
    gate(np.array(got["grid"]), K.kde_grid_spec(np.stack([mapped, unmapped], 1).astype(float), labels, labels, 60.0), "tail model grid")
    assert np.array(dc["grid"]).shape == (40, 40)
    with pytest.raises(ValueError):
        tksm_amd.build_tail_model(mapped, unmapped, labels, labels[:-1], begin, trans, 60.0, tmp_path / "no.json")
    s = Sequencer(0)
    try:
        s.set_identity(84.0, 99.0, 5.5)
        s.load_error_model(ERR_MODEL)
        s.load_qscore_model(QS_MODEL)
        s.add_contig("c0", rs.choice(np.frombuffer(b"ACGT", np.uint8), 20000).tobytes().decode())
        s.load_tail_model(str(path))
        b = s.batch_from_mdf("".join(f"+m{i}\t1\t\nc0\t{100 * i}\t{100 * i + 600}\t+\t\n" for i in range(32)))
        recs = s.run(b, target="badread", fastq=True, compute_qual=True, seed=5).records()
        assert len(recs) == 32 and all(r.startswith(b"@") and f"molecule_id=m{i}\n".encode() in r for i, r in enumerate(recs))
    finally:
        s.close()


def test_errors(S, tmp_path):
    from tksm_amd import _lib as L
    from tksm_amd.sequence import TksmSeqError
    xy, c = sample(10), centres(4)

    def code(fn, *a, **k):
        with pytest.raises(TksmSeqError) as e:
            fn(*a, **k)
        return e.value.code
    for h in (0.0, -1.0, float("nan"), float("inf")):
        assert code(S.kde_grid, xy, c, c, h) == L.EINVAL
    assert code(S.kde_grid, np.empty((0, 2)), c, c, 100.0) == L.EINVAL
    assert code(S.kde_grid, np.array([[np.nan, 1.0]]), c, c, 100.0) == L.EINVAL
    assert code(S.kde_grid, xy, centres(4097), c, 100.0) == L.ELIMIT
    assert code(S.kde_grid, xy, c, centres(4097), 100.0) == L.ELIMIT
    out = np.empty((4, 4))
    assert S._lib.tksmseq_kde_grid(S._ctx, xy.ctypes.data, 1 << 31, c.ctypes.data, 4, c.ctypes.data, 4, 100.0, out.ctypes.data) == L.ELIMIT     # (checked before anything is read)
    assert code(S.kde_cv_bandwidth, np.empty((0, 2)), 1, 100) == L.EINVAL
    assert code(S.kde_cv_bandwidth, xy, 1, 2) == L.EINVAL
    assert code(S.kde_cv_bandwidth, xy, 1, (1 << 24) + 1) == L.ELIMIT
    assert code(S.model_truncation, PAF, tmp_path / "m.json", grid_start=0, grid_end=50, grid_step=100) == L.EINVAL
    assert code(S.model_truncation, PAF, tmp_path / "m.json", end_ratio=1.5) == L.EINVAL
    assert code(S.model_truncation, PAF, tmp_path / "m.json", grid_start=0, grid_end=4097 * 100, grid_step=100) == L.ELIMIT
    assert code(S.model_truncation, PAF, tmp_path / "m.json", grid_start=0, grid_end=10 ** 12, grid_step=1) == L.ELIMIT
    assert code(S.model_truncation, tmp_path / "missing.paf", tmp_path / "m.json") == L.EIO
    # the module: an empty PAF, one without a primary alignment, a malformed line, an unwritable output -- exit 1, nothing left behind
    empty, second, bad = tmp_path / "empty.paf", tmp_path / "second.paf", tmp_path / "bad.paf"
    empty.write_text("")
    second.write_text("r0\t100\t0\t100\t+\tt0\t500\t0\t100\t100\t100\t0\ttp:A:S\n")
    bad.write_text("r0\t100\t0\t100\t+\tt0\tfive\t0\t100\t100\t100\t0\ttp:A:P\n")
    for paf, msg in ((empty, "no primary alignment"), (second, "no primary alignment"), (bad, "PAF line 1")):
        r = _module("-i", paf, "-o", tmp_path / "m.json")
        assert r.returncode == 1 and msg in r.stderr, r.stderr
        assert not (tmp_path / "m.json").exists()
    target = tmp_path / "no" / "such" / "dir" / "m.json"
    r = _module("-i", PAF, "-o", target, "--grid-end", "3000")
    assert r.returncode == 1 and "cannot write" in r.stderr
    assert not os.path.exists(os.path.dirname(str(target)))
