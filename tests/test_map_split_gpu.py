"""map --split on the device against the specification (tests/map_split_spec.py): the PAF bytes and the integer counters of all info blocks,
no tolerance, without -c, with -c --eqx, with --extend and with both.  Shapes, each small and reaching one thing (map_split_spec.edge_case,
pinned on the CPU by tests/test_map_split.py): groups of 63, 64, 65, 128 and 129 anchors whose removed positions end just before, on and
just after a tile of 64, rounds that leave min_count - 1, min_count and no anchors, chains = 1 and a group that reaches `chains`, a link of
a later round over more than 64 original anchors, read intervals that share exactly `overlap` letters and one more, equal scores across
targets, strands and rounds, and more candidates than `segments` accepts; then the generated set, chunk sizes, the split-NULL call and the
module with its logged estimate."""
import ctypes
import os
import re
import subprocess

import pytest

from conftest import ROOT

import map_align_spec as A
import map_extend_spec as X
import map_spec as M
import map_split_spec as S

pytestmark = pytest.mark.gpu

EXE = os.path.join(ROOT, "tksm_amd", "tksm")
MODES = {"plain": dict(), "c_eqx": dict(align=True, eqx=True), "extend": dict(extend=True), "c_eqx_extend": dict(align=True, eqx=True, extend=True)}


def device(targets, reads, d, tag="dev", split=True, **params):
    """the device's PAF and counters for targets and reads given as [(name, letters)]"""
    from tksm_amd.sequence import Sequencer
    fq = M.write_fastq(os.path.join(str(d), tag + ".fq"), reads)
    out = os.path.join(str(d), tag + ".paf")
    s = Sequencer(0)
    try:
        for name, seq in targets:
            s.add_contig(name, seq)
        info = s.map(fq, out, split=split, **params)
    finally:
        s.close()
    assert not [f for f in os.listdir(str(d)) if f.endswith(".tmp")]
    return {"paf": open(out).read(), "info": info}


def same(dev, spec, mode):
    assert dev["paf"] == spec["paf"]
    assert {k: dev["info"][k] for k in M.COUNTERS} == spec["info"]
    s = dev["info"]["split"]
    assert {k: s[k] for k in S.COUNTERS} == spec["split"]
    assert dev["info"]["lines"] == dev["info"]["mapped"] + dev["info"]["secondary"] + s["supplementary"]
    assert s["split_ms"] > 0 or not dev["info"]["chained_groups"]
    if mode.get("extend"):
        assert {k: dev["info"]["extend"][k] for k in X.COUNTERS} == spec["extend"] and spec["extend"]["lines"] == dev["info"]["lines"]
    if not mode.get("align"):
        assert "align" not in dev["info"]
        return
    assert {k: dev["info"]["align"][k] for k in A.COUNTERS} == spec["align"] and spec["align"]["lines"] == dev["info"]["lines"]
    for line in dev["paf"].splitlines():
        f = line.split("\t")
        t, q, n = A.cigar_spans(f[-1][5:])
        assert f[-1].startswith("cg:Z:") and t == int(f[8]) - int(f[7]) and q == int(f[3]) - int(f[2])          # every line, the supplementary ones among them
        assert f[-2].startswith("NM:i:") and int(f[10]) == sum(n.values()) and int(f[-2][5:]) == int(f[10]) - int(f[9])


@pytest.fixture(scope="module")
def edge():
    targets, reads, params = S.edge_case()
    return {"targets": targets, "reads": reads, "params": params, "memo": {}}


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("variant", list(S.VARIANTS))
def test_crafted_cases(edge, tmp_path, variant, mode):
    kw = dict(S.VARIANTS[variant], **MODES[mode], **edge["params"])
    spec = S.map_reads(edge["targets"], edge["reads"], memo=edge["memo"], **kw)
    same(device(edge["targets"], edge["reads"], tmp_path, **kw), spec, MODES[mode])
    assert spec["split"]["supplementary"] > 0


@pytest.mark.parametrize("chunk_reads", [1, 7])
def test_crafted_cases_in_chunks(edge, tmp_path, chunk_reads):
    kw = dict(MODES["c_eqx_extend"], **edge["params"])
    spec = S.map_reads(edge["targets"], edge["reads"], memo=edge["memo"], **kw)
    dev = device(edge["targets"], edge["reads"], tmp_path, chunk_reads=chunk_reads, **kw)
    same(dev, spec, MODES["c_eqx_extend"])
    assert dev["info"]["chunks"] == (len(edge["reads"]) + chunk_reads - 1) // chunk_reads


@pytest.fixture(scope="module", params=[0.0, 0.05])
def generated(request, tmp_path_factory):
    """200 reads glued from one to three pieces of 30 targets of 600 to 2 500 letters (A, A+B, A+A, A+revcomp(A), A+B+A), error-free or with
    5 % substitutions; the spec of the plain run once, shared"""
    d = tmp_path_factory.mktemp("map_split_generated")
    g = S.generate(d, seed=5, n_targets=30, n_reads=200, error=request.param)
    g["dir"], g["memo"] = d, {}
    g["spec"] = S.map_reads(g["targets"], g["read_list"], memo=g["memo"])
    return g


def test_generated_set(generated, tmp_path):
    g = generated
    dev = device(g["targets"], g["read_list"], tmp_path)
    same(dev, g["spec"], {})
    assert g["spec"]["split"]["supplementary"] > 100 and g["spec"]["split"]["later_chains"] > 50


@pytest.mark.parametrize("mode", ["c_eqx", "extend", "c_eqx_extend"])
def test_generated_set_aligned_and_extended(generated, tmp_path, mode):
    """--extend alone on the whole set; with -c the first 40 reads of it (the specification aligns in plain Python, a tenth of a second a line)"""
    g = generated
    reads = g["read_list"] if mode == "extend" else g["read_list"][:40]
    memo = g["memo"] if mode == "extend" else g.setdefault("memo40", {})
    spec = S.map_reads(g["targets"], reads, memo=memo, **MODES[mode])
    same(device(g["targets"], reads, tmp_path, **MODES[mode]), spec, MODES[mode])
    assert spec["split"]["supplementary"] > 20


@pytest.mark.parametrize("chunk_reads", [1, 7, 0])
def test_chunk_sizes_give_the_same_bytes(generated, tmp_path, chunk_reads):
    g = generated
    dev = device(g["targets"], g["read_list"], tmp_path, chunk_reads=chunk_reads)
    same(dev, g["spec"], {})
    assert dev["info"]["chunks"] == ((200 + chunk_reads - 1) // chunk_reads if chunk_reads else 1)


def test_split_off_and_the_null_call_give_todays_bytes(generated, tmp_path):
    from tksm_amd import _lib
    from tksm_amd.sequence import Sequencer
    g = generated
    off = S.map_reads(g["targets"], g["read_list"], split=False, memo=g["memo"])
    dev = device(g["targets"], g["read_list"], tmp_path, split=False)
    assert dev["paf"] == off["paf"] != g["spec"]["paf"] and "split" not in dev["info"] and {k: dev["info"][k] for k in M.COUNTERS} == off["info"]
    s = Sequencer(0)
    try:
        for name, seq in g["targets"]:
            s.add_contig(name, seq)
        lib = _lib.load()
        p = _lib.MapParams(15, 10, 500, 5000, 500, 3, 40, 0, 0.8, 5, 0, 0)
        info, sinfo = _lib.MapInfo(), _lib.SplitInfo()
        out = tmp_path / "null.paf"
        rc = lib.tksmseq_map_split(s._ctx, ctypes.byref(p), None, None, None, g["reads"].encode(), str(out).encode(), ctypes.byref(info), None, None, ctypes.byref(sinfo))
        assert rc == 0 and out.read_text() == off["paf"] and sinfo.rounds == 0 and info.lines == off["info"]["lines"]
        sp = _lib.SplitParams(4, 30, 8, 0)
        rc = lib.tksmseq_map_split(s._ctx, None, None, None, ctypes.byref(sp), g["reads"].encode(), str(out).encode(), None, None, None, None)
        assert rc == 0 and out.read_text() == g["spec"]["paf"]
    finally:
        s.close()


def test_error_codes(edge, tmp_path):
    from tksm_amd import _lib
    from tksm_amd.sequence import Sequencer, TksmSeqError
    fq = M.write_fastq(os.path.join(str(tmp_path), "e.fq"), edge["reads"][:2])
    s = Sequencer(0)
    try:
        for name, seq in edge["targets"][:2]:
            s.add_contig(name, seq)
        for bad in (dict(split_chains=0), dict(split_chains=17), dict(split_overlap=-1), dict(split_segments=1), dict(split_segments=65)):
            with pytest.raises(TksmSeqError) as e:
                s.map(fq, tmp_path / "o.paf", split=True, **bad)
            assert e.value.code == _lib.EINVAL and "map: split " in str(e.value), bad
        assert not (tmp_path / "o.paf").exists()
    finally:
        s.close()


def test_module_writes_the_lines_and_logs_the_estimate(generated, tmp_path):
    g = generated
    out = tmp_path / "module.paf"
    r = subprocess.run([EXE, "map", "-r", g["ref"], "--reads", g["reads"], "-o", str(out), "--split", "--verbosity", "INFO"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-600:]
    assert out.read_text() == g["spec"]["paf"]
    J, mapped = g["spec"]["split"]["supplementary"], g["spec"]["info"]["mapped"]
    m = re.search(r"split: (\d+) junctions in (\d+) mapped reads: unsegment -p estimate ([0-9.]+)", r.stderr + r.stdout)
    assert m and (int(m.group(1)), int(m.group(2))) == (J, mapped) and abs(float(m.group(3)) - J / (mapped + J - 1)) < 1e-6
    plain = subprocess.run([EXE, "map", "-r", g["ref"], "--reads", g["reads"], "-o", str(out), "--verbosity", "INFO"], capture_output=True, text=True)
    assert plain.returncode == 0 and "junctions" not in plain.stderr + plain.stdout
    assert out.read_text() == S.map_reads(g["targets"], g["read_list"], split=False, memo=g["memo"])["paf"]
