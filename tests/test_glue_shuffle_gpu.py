"""unsegment (Glu) and shuffle (Shf) on the device (-m gpu): tksmseq_glue / tksmseq_shuffle against tests/glue_shuffle_spec.py as MDF text,
byte for byte; the glued batch sequenced --perfect against its members' reads; `tksm unsegment` and `tksm shuffle` on files against the
specification of the whole input, whatever --batch-bytes and --devices are."""
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

import glue_shuffle_spec as gs
import mdf_ops_oracle as mo

pytestmark = pytest.mark.gpu

EXE = os.path.join(ROOT, "tksm_amd", "tksm")
COMMENTS = ["CB=ACGT;", "", "Cat;", "tid=T1;CB=TTGCA;", "Cat=x;z;", "CB=.;", "z;"]
NAN = float("nan")


def _cli(*args, **kw):
    return subprocess.run([EXE, *[str(a) for a in args]], capture_output=True, text=True, timeout=600, **kw)


def _mdf(rs, n):
    """n records of 1 - 5 segments on two contigs and both strands: substitutions on some (on the batch's last interval too), literal
    segments, zero-size segments (never alone), one record in five with depth 3, the comments of COMMENTS in turn"""
    lines = []
    for i in range(n):
        lines.append(f"+m{i}\t{3 if i % 5 == 2 else 1}\t{COMMENTS[i % len(COMMENTS)]}\n")
        k_seg = 1 + int(rs.randint(0, 5))
        for k in range(k_seg):
            last = i == n - 1 and k == k_seg - 1
            if k > 0 and not last and rs.rand() < 0.1:
                st = int(rs.randint(5000, 50_000))
                lines.append(f"chr{int(rs.randint(1, 3))}\t{st}\t{st}\t{'+-'[int(rs.randint(0, 2))]}\t\n")
                continue
            if not last and rs.rand() < 0.15:
                lit = ("ACGTTGCA", "A" * int(rs.randint(1, 20)))[int(rs.randint(0, 2))]
                lines.append(f"{lit}\t0\t{len(lit)}\t{'+-'[int(rs.randint(0, 2))]}\t{'0C' if rs.rand() < 0.5 else ''}\n")
                continue
            ln, st = int(rs.randint(1, 400)), int(rs.randint(5000, 50_000))
            md = ",".join(f"{int(rs.randint(0, ln))}{'ACGT'[int(rs.randint(0, 4))]}" for _ in range(2 if last else int(rs.randint(0, 3))))
            lines.append(f"chr{int(rs.randint(1, 3))}\t{st}\t{st + ln}\t{'+-'[int(rs.randint(0, 2))]}\t{md}\n")
    return "".join(lines)


def _singles(n, comments=True):
    """n single-segment records, a comment on two in three"""
    return "".join(f"+k{i}\t1\t{('n=%d;' % i) if comments and i % 3 else ''}\nchr{1 + i % 2}\t{100 + i % 40_000}\t{150 + i % 40_000 + i % 7}\t{'+-'[i % 2]}\t{'3G' if i % 5 == 0 else ''}\n"
                   for i in range(n))


@pytest.fixture(scope="module")
def dev():
    from tksm_amd.sequence import Sequencer
    rs = np.random.RandomState(21)
    s = Sequencer(0)
    for i in range(2):
        s.add_contig(f"chr{i + 1}", rs.choice(np.frombuffer(b"ACGT", np.uint8), 60_000).tobytes().decode())
    yield s
    s.close()


@pytest.fixture(scope="module")
def sample(dev):
    """one parsed batch of 300 records (420 molecules) and its specification's molecules: read by the tests, never changed"""
    text = _mdf(np.random.RandomState(2), 300)
    b = dev.batch_from_mdf(text)
    mols = mo.stream_mdf(text, unroll=True)
    assert b.n_reads == len(mols) == 420 and mols[-1]["segments"][-1]["errors"]
    assert any(sg["start"] == sg["end"] for m in mols for sg in m["segments"]) and any(sg["chr"] == "ACGTTGCA" for m in mols for sg in m["segments"])
    yield text, mols, b
    b.free()


def _text(s, batch):
    try:
        return s.to_mdf_text(batch)
    finally:
        batch.free()


def _no_comments(text):
    return "".join((l.rsplit("\t", 1)[0] + "\t\n") if l.startswith("+") else l for l in text.splitlines(keepends=True))


# ------------------------------------------------------------------------------------------------ glue
@pytest.mark.parametrize("p", [0.0, 0.1, 0.5, 0.9, 1.0, -1.0, 2.0, NAN])
def test_glue_equals_the_spec_at_every_probability(dev, sample, p):
    _, mols, b = sample
    for seed in (42, 7):
        want = gs.glue_spec(mols, p, seed)
        out = dev.glue(b, p, seed=seed)
        assert out.n_reads == len(want)
        got = _text(dev, out)
        assert got == mo.write_mdf(want), (p, seed)
        if not p > 0.0:
            assert got == mo.write_mdf(mols)                               # the unrolled input
        if p >= 1.0:
            assert len(want) == 1 and len(want[0]["segments"]) == sum(len(m["segments"]) for m in mols) and want[0]["id"] == "m0"
        assert _text(dev, dev.glue(b, p, seed=seed, comments=False)) == _no_comments(mo.write_mdf(want))
    if p == 0.5:
        heads = [m for m in gs.glue_spec(mols, p, 42) if "Cat" in m["meta"]]
        # glued heads that carried `Cat;` and `Cat=x;` themselves
        assert any(m["meta"]["Cat"][0] == "." for m in heads) and any(m["meta"]["Cat"][0] == "x" and len(m["meta"]["Cat"]) > 1 for m in heads)


@pytest.mark.parametrize("first", [0, 1, 2**32 - 1, 2**32])
def test_glue_first_molecule_index(dev, sample, first):
    """the draws are those of first + i; molecule 0 of the call is a head whatever joins(first) says"""
    _, mols, b = sample
    seed = next(sd for sd in range(100) if first == 0 or gs.joins_np(sd, 0.5, [first])[0])
    want = gs.glue_spec(mols, 0.5, seed, first=first)
    assert want[0]["id"] == "m0" and 100 < len(want) < 320
    assert _text(dev, dev.glue(b, 0.5, seed=seed, first_molecule_index=first)) == mo.write_mdf(want)
    if first:
        assert mo.write_mdf(want) != mo.write_mdf(gs.glue_spec(mols, 0.5, seed))


def test_glue_small_batches_and_last_molecule(dev):
    one = dev.batch_from_mdf("+a\t1\tk=v;\nchr1\t10\t20\t-\t3C\n")
    for p in (0.0, 1.0):
        assert _text(dev, dev.glue(one, p)) == "+a\t1\tk=v;\nchr1\t10\t20\t-\t3C\n"
    empty = dev.batch_from_mdf("")
    out = dev.glue(empty, 0.5)
    assert out.n_reads == 0 and _text(dev, out) == ""
    one.free(); empty.free()
    # the last molecule joining, and the last molecule a head of its own; a depth-3 record alone, glued to itself
    text = _singles(5) + "+r\t3\tk=v;\nchr2\t7\t9\t+\t1A\n"
    mols = mo.stream_mdf(text, unroll=True)
    b = dev.batch_from_mdf(text)
    seen = set()
    for seed in range(40):
        want = gs.glue_spec(mols, 0.5, seed)
        seen.add(want[-1]["id"] == "r_2")
        assert _text(dev, dev.glue(b, 0.5, seed=seed)) == mo.write_mdf(want), seed
    assert seen == {True, False}
    assert _text(dev, dev.glue(b, 1.0)) == "+k0\t1\tCat=k1,k2,k3,k4,r_0,r_1,r_2;\n" + "".join(l for l in mo.write_mdf(mols).splitlines(keepends=True) if not l.startswith("+"))
    b.free()


def test_glue_chain_across_blocks_and_waves(dev):
    """p = 0.995 over 1 000 single-segment molecules: chains longer than a 128-lane block"""
    text = _singles(1000)
    mols = mo.stream_mdf(text, unroll=True)
    seed = next(sd for sd in range(50) if gs.chains(1000, 0.995, sd).max() > 128 and len(gs.chains(1000, 0.995, sd)) > 2)
    lengths = gs.chains(1000, 0.995, seed)
    assert lengths.max() > 128 and lengths.sum() == 1000
    b = dev.batch_from_mdf(text)
    want = gs.glue_spec(mols, 0.995, seed)
    assert [len(m["segments"]) for m in want] == list(lengths)
    out = dev.glue(b, 0.995, seed=seed)
    assert out.n_reads == len(lengths) and _text(dev, out) == mo.write_mdf(want)
    b.free()


def test_glue_input_without_comments(dev):
    bare = dev.batch_from_arrays(np.array([[0, 1], [1, 1], [2, 1]]), np.array([[0, 0, 10, 0], [1, 5, 9, 0], [0, 3, 4, 0]]), ids=np.array([[0, 1], [1, 1], [2, 1]]), id_pool=b"abc")
    assert _text(dev, dev.glue(bare, 0.0)) == "+a\t1\t\nchr1\t0\t10\t+\t\n+b\t1\t\nchr2\t5\t9\t+\t\n+c\t1\t\nchr1\t3\t4\t+\t\n"
    assert _text(dev, dev.glue(bare, 1.0)) == "+a\t1\tCat=b,c;\nchr1\t0\t10\t+\t\nchr2\t5\t9\t+\t\nchr1\t3\t4\t+\t\n"
    assert _text(dev, dev.glue(bare, 1.0, comments=False)) == "+a\t1\t\nchr1\t0\t10\t+\t\nchr2\t5\t9\t+\t\nchr1\t3\t4\t+\t\n"
    seed = next(sd for sd in range(50) if list(gs.chains(3, 0.5, sd)) == [1, 2])
    assert _text(dev, dev.glue(bare, 0.5, seed=seed)) == "+a\t1\t\nchr1\t0\t10\t+\t\n+b\t1\tCat=c;\nchr2\t5\t9\t+\t\nchr1\t3\t4\t+\t\n"
    bare.free()


def test_glued_batch_sequences_to_the_members_reads(dev, sample):
    """Sequencer.run(..., perfect) of the glued batch: per chain, its members' perfect reads from the unglued batch, one behind the other"""
    _, mols, _ = sample
    flat = dev.batch_from_mdf(mo.write_mdf(mols))                         # (depth 1: one record per molecule)
    seq = lambda rec: rec.split(b"\n")[1]
    own = [seq(r) for r in dev.run(flat, target="perfect", fastq=False, seed=5).records()]
    assert len(own) == len(mols) and all(own)
    for p in (0.5, 0.9):
        lengths = gs.chains(len(mols), p, 3)
        glued = dev.glue(flat, p, seed=3)
        got = [seq(r) for r in dev.run(glued, target="perfect", fastq=False, seed=5).records()]
        at, want = 0, []
        for ln in lengths:
            want.append(b"".join(own[at:at + ln]))
            at += ln
        assert got == want, p
        glued.free()
    flat.free()


# ------------------------------------------------------------------------------------------------ shuffle
def _b_values(n):
    return sorted({B for B in (0, 1, 2, 63, 64, 65, n - 1, n, n + 1) if B >= 0})


@pytest.mark.parametrize("seed", [42, 9])
@pytest.mark.parametrize("n", [0, 1, 2, 70_000])
def test_shuffle_single_segment_molecules(dev, n, seed):
    """sizes around nothing, and one at which the sorts and the scans cross their block sizes"""
    text = _singles(n)
    recs = [mo.write_mdf([m]) for m in mo.stream_mdf(text, unroll=True)]
    b = dev.batch_from_mdf(text)
    for B in _b_values(n) + ([1000] if n == 70_000 else []):
        out = dev.shuffle(b, seed=seed, buffer_size=B)
        assert out.n_reads == n
        got = _text(dev, out)
        order = gs.shuffle_order(n, seed, B)
        assert got == "".join(recs[i] for i in order), (n, B)
        if B == 1:
            assert order == list(range(n))
        elif n > 2:
            assert order != list(range(n)) and sorted(order) == list(range(n))
    if n == 70_000:
        assert _text(dev, dev.shuffle(b, seed=seed, buffer_size=1000, comments=False)) == _no_comments("".join(recs[i] for i in gs.shuffle_order(n, seed, 1000)))
    b.free()


@pytest.mark.parametrize("seed", [42, 9])
def test_shuffle_the_sample(dev, sample, seed):
    """the sample's 420 molecules -- several segments, substitutions, literals, depth-3 records, comments -- at every buffer size"""
    text, mols, b = sample
    n = len(mols)
    records = lambda t: sorted(re.split(r"(?m)^(?=\+)", t))
    for B in _b_values(n):
        want = mo.write_mdf(gs.shuffle_spec(mols, seed, B))
        got = _text(dev, dev.shuffle(b, seed=seed, buffer_size=B))
        assert got == want, B
        assert records(got) == records(mo.write_mdf(mols))               # a permutation of the unrolled input
    # comments follow their molecules: the copies of a depth-3 record share a comment entry and end up apart
    order = gs.shuffle_order(n, seed)
    ids = [mols[i]["id"] for i in order]
    assert abs(ids.index("m2_0") - ids.index("m2_1")) > 1 and mols[order[ids.index("m2_1")]]["meta"] == {"Cat": ["."]}
    assert _text(dev, dev.shuffle(b, seed=seed, comments=False)) == _no_comments(mo.write_mdf(gs.shuffle_spec(mols, seed)))
    # the shuffled batch is a batch like any other: glue takes it
    sh = dev.shuffle(b, seed=seed, buffer_size=64)
    assert _text(dev, dev.glue(sh, 0.3, seed=seed)) == mo.write_mdf(gs.glue_spec(gs.shuffle_spec(mols, seed, 64), 0.3, seed))
    sh.free()


def test_shuffle_423_molecules(dev):
    """the molecule count of the other MDF suites (300 records, one in five with depth 3, plus a depth-3 probe)"""
    text = "+probe\t3\tCB=ACGT;\nchr1\t1000\t1100\t+\t5A,50C\nchr2\t7000\t7010\t-\t\n" + _mdf(np.random.RandomState(1), 300)
    mols = mo.stream_mdf(text, unroll=True)
    n = len(mols)
    assert n == 423
    b = dev.batch_from_mdf(text)
    for seed in (42, 9):
        for B in _b_values(n):
            assert _text(dev, dev.shuffle(b, seed=seed, buffer_size=B)) == mo.write_mdf(gs.shuffle_spec(mols, seed, B)), (seed, B)
    b.free()


# ------------------------------------------------------------------------------------------------ the modules on files
@pytest.mark.parametrize("p", [0.3, 0.9])
def test_tksm_unsegment_does_not_depend_on_pieces_or_devices(dev, sample, p, tmp_path):
    text, mols, _ = sample
    src, out = tmp_path / "in.mdf", tmp_path / "out.mdf"
    src.write_text(text)
    want = mo.write_mdf(gs.glue_spec(mols, p, 13))
    for extra in (["--batch-bytes", "300"], ["--batch-bytes", "3000"], [], ["--batch-bytes", "300", "--devices", "0,0"], ["--devices", "0,0"], ["--batch-bytes", "3000", "--devices", "0"]):
        r = _cli("unsegment", "-i", src, "-o", out, "-p", p, "-s", 13, *extra)
        assert r.returncode == 0, (extra, r.stderr[-600:])
        assert out.read_text() == want, extra
    back = dev.batch_from_mdf(want)
    assert _text(dev, back) == want                                       # the output parses back to the same text


def test_tksm_unsegment_edges(tmp_path):
    (tmp_path / "empty.mdf").write_text("")
    r = _cli("unsegment", "-i", tmp_path / "empty.mdf", "-o", tmp_path / "e.mdf", "-p", "0.5")
    assert r.returncode == 0 and (tmp_path / "e.mdf").read_text() == ""
    text = _singles(200)
    (tmp_path / "in.mdf").write_text(text)
    mols = mo.stream_mdf(text, unroll=True)
    for p in ("0", "1", "1.5"):                                           # p >= 1: the whole input is one piece, and one molecule
        r = _cli("unsegment", "-i", tmp_path / "in.mdf", "-o", tmp_path / "o.mdf", "--probability", p, "--batch-bytes", "100")
        assert r.returncode == 0, r.stderr[-600:]
        assert (tmp_path / "o.mdf").read_text() == mo.write_mdf(gs.glue_spec(mols, float(p), 42)), p
    r = _cli("unsegment", "-i", tmp_path / "nope.mdf", "-o", tmp_path / "o2.mdf", "-p", "0.5")
    assert r.returncode == 1 and "Could not open file" in r.stderr


def test_tksm_shuffle_on_files(dev, sample, tmp_path):
    text, mols, _ = sample
    src, out = tmp_path / "in.mdf", tmp_path / "out.mdf"
    src.write_text(text)
    for extra, B in (([], 0), (["--buffer-size", "64"], 64), (["--buffer-size=100000", "--devices", "0,0"], 100000)):
        r = _cli("shuffle", "-i", src, "-o", out, "-s", 13, *extra)
        assert r.returncode == 0, (extra, r.stderr[-600:])
        want = mo.write_mdf(gs.shuffle_spec(mols, 13, B))
        assert out.read_text() == want, extra
        assert _text(dev, dev.batch_from_mdf(want)) == want
    (tmp_path / "empty.mdf").write_text("")
    r = _cli("shuffle", "-i", tmp_path / "empty.mdf", "-o", tmp_path / "e.mdf")
    assert r.returncode == 0 and (tmp_path / "e.mdf").read_text() == ""
