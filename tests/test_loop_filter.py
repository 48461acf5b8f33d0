"""The bounds table that lets k_loop decide most draws without asking for the k-mer's first threshold (tksm_amd/csrc/loop_filter.h),
on the CPU: tools/loop_filter_check.cpp -- the builder api.cpp calls and the classification the kernel calls -- against a numpy
restatement, from a plain build and from one under AddressSanitizer + UBSan.  The property that matters: a draw the table decides
is never decided against `dw < t0`, at the thresholds themselves and at the table's byte boundaries."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import MODELS, ROOT

BITS = 11
KEYS = 1 << BITS
NOOP, CHANGE, UNDECIDED = 0, 1, 2


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def checker(request, tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no C++ compiler"
    exe = tmp_path_factory.mktemp("loopfilter_" + request.param) / "loop_filter_check"
    flags = ["-O2"] if request.param == "plain" else ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                                                       "-fno-omit-frame-pointer"]
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", *flags, "-I", os.path.join(ROOT, "tksm_amd", "csrc"),
                    os.path.join(ROOT, "tools", "loop_filter_check.cpp"), "-o", str(exe)], check=True)
    return str(exe)


def table_numpy(t0):
    key = (np.arange(len(t0), dtype=np.uint32) >> 2) & (KEYS - 1)
    top = (t0 >> 24).astype(np.int64)
    lo, hi = np.full(KEYS, 256, np.int64), np.full(KEYS, -1, np.int64)
    np.minimum.at(lo, key, top)
    np.maximum.at(hi, key, top)
    empty = hi < 0
    lo[empty], hi[empty] = 0, 255
    return key, lo, hi


def probes(t0, key, lo, hi):
    """(kx, dw) pairs: every k-mer at t0 - 1, t0, t0 + 1 and at the four edges of its key's byte bounds, where in range"""
    kx = np.arange(len(t0), dtype=np.int64)
    t = t0.astype(np.int64)
    l24, h24 = lo[key] << 24, (hi[key] + 1) << 24
    dws = [t - 1, t, t + 1, l24 - 1, l24, h24 - 1, h24]
    k2 = np.concatenate([kx] * len(dws))
    dw = np.concatenate(dws)
    ok = (dw >= 0) & (dw <= 0xFFFFFFFF)
    return k2[ok].astype(np.uint32), dw[ok].astype(np.uint32)


def run_checker(exe, d, t0, pairs=None):
    t0.astype("<u4").tofile(d / "t0.bin")
    cmd = [exe, str(d / "t0.bin"), str(d / "table.bin")]
    if pairs is not None:
        np.stack(pairs, axis=1).astype("<u4").tofile(d / "pairs.bin")
        cmd += [str(d / "pairs.bin"), str(d / "classes.bin")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    tab = np.fromfile(d / "table.bin", "<u2")
    return tab, (np.fromfile(d / "classes.bin", np.uint8) if pairs is not None else None)


def check_thresholds(exe, d, t0):
    """table and classes equal the restatement; no decided probe contradicts dw < t0.  -> the decided share under uniform k-mers
    and uniform dw, from the table"""
    t0 = np.asarray(t0, np.uint32)
    key, lo, hi = table_numpy(t0)
    kx, dw = probes(t0, key, lo, hi)
    tab, cls = run_checker(exe, d, t0, (kx, dw))
    assert tab.shape == (KEYS,)
    assert np.array_equal(tab & 0xff, lo) and np.array_equal(tab >> 8, hi)
    top = (dw >> 24).astype(np.int64)
    want = np.where(top < lo[key[kx]], NOOP, np.where(top > hi[key[kx]], CHANGE, UNDECIDED))
    assert np.array_equal(cls, want)
    below = dw < t0[kx]
    assert below[cls == NOOP].all(), "a draw proved to change nothing is not below its k-mer's threshold"
    assert not below[cls == CHANGE].any(), "a draw proved to change something is below its k-mer's threshold"
    assert (dw[cls == CHANGE] > t0[kx[cls == CHANGE]]).all()
    return float(np.mean((lo[key] + 255 - hi[key]) / 256.0))


def threshold_sets(nk):
    rs = np.random.RandomState(nk % 1009)
    yield "random", rs.randint(0, 1 << 32, nk, dtype=np.uint64).astype(np.uint32)
    for v in (0, 0x51234567, 0xFFFFFFFF):
        yield f"equal-{v:#x}", np.full(nk, v, np.uint32)
    yield "0-and-max", np.where(rs.randint(0, 2, nk) == 1, 0xFFFFFFFF, 0).astype(np.uint32)
    yield "0-and-max-by-key", np.where((np.arange(nk) >> 2) & 1, 0xFFFFFFFF, 0).astype(np.uint32)
    m = rs.randint(0, 256, nk).astype(np.int64) << 24                  # multiples of 2^24 and their neighbours
    yield "byte-edges", np.clip(m + rs.randint(-1, 2, nk), 0, 0xFFFFFFFF).astype(np.uint32)
    step = (np.arange(nk, dtype=np.int64) * 2654435761 >> 7) % 256       # neighbours under one key one step apart
    yield "byte-edges-by-step", np.clip(((step + (np.arange(nk) & 1)) << 24) - (np.arange(nk) >> 1 & 1), 0, 0xFFFFFFFF).astype(np.uint32)


@pytest.mark.parametrize("k", [5, 7, 8])
def test_table_and_classes_on_synthetic_thresholds(checker, tmp_path, k):
    nk = 4 ** k
    for name, t0 in threshold_sets(nk):
        assert len(t0) == nk, name
        share = check_thresholds(checker, tmp_path, t0)
        if name.startswith("equal"):
            assert share == 255 / 256, name                              # one undecided byte per k-mer


def test_keys_without_a_kmer_are_never_decided(checker, tmp_path):
    """k = 5: 256 keys are populated; the other 1792 entries are {0, 255}.  nk = 0: all of them."""
    tab, _ = run_checker(checker, tmp_path, np.full(4 ** 5, 0x80000000, np.uint32))
    assert (tab[:256] == 0x8080).all() and (tab[256:] == 0xff00).all()
    tab, _ = run_checker(checker, tmp_path, np.zeros(0, np.uint32))
    assert (tab == 0xff00).all()


_MODEL_T0 = {}


# the share of draws the table decides, k-mers and dw uniform: computed with floor / ceil bounds 0.911 / 0.850 / 0.929; the top-byte
# rule loses at most 1/256 per side, the rest is margin
@pytest.mark.parametrize("model,least", [("nanopore2020", 0.89), ("nanopore2018", 0.83), ("pacbio2016", 0.91)])
def test_shipped_models(checker, tmp_path, po, model, least):
    if model not in _MODEL_T0:                                       # (parsed once for both builds of the checker)
        em = po.ErrorModel(os.path.join(MODELS, f"{model}.error.gz"))
        assert em.type == 1 and em.cdf.shape[0] == 4 ** em.k
        _MODEL_T0[model] = np.ascontiguousarray(em.cdf[:, 0])
    share = check_thresholds(checker, tmp_path, _MODEL_T0[model])
    print(f"{model}: decided share {share:.4f}")
    assert share >= least
