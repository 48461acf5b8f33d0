"""map -c on the device against the specification (tests/map_align_spec.py): the PAF bytes and the integer counters of both info blocks, no
tolerance.  Shapes: planted edits on both strands with secondary lines, segments around the wave width and the ring of 64 lanes, an indel
outside and inside the band, chains whose links lie at the edge of the window of 64 predecessors (tandem repeats, at band 63 and 1), chains
of dense groups with ties between predecessors of two tiles (k = 4, 5, 6), one segment near max_gap and bandwidth, dense overlapping anchors with dt or dq below k, N runs, every offset
of a packed word on the reverse strand, chunk sizes and a chunk over the alignment's budget, recycled memory, reuse of a context, error
codes, and the loop the mode is for: transcribe -> sequence -> map -c -> model-sequence."""
import ctypes
import gzip
import os
import random
import subprocess

import pytest

from conftest import ERR_MODEL, QS_MODEL, ROOT

import map_align_spec as A
import map_spec as M

pytestmark = pytest.mark.gpu

EXE = os.path.join(ROOT, "tksm_amd", "tksm")


def device(targets, reads, d, tag="dev", gz=False, sequencer=None, align=True, **params):
    """the device's PAF and counters for targets and reads given as [(name, letters)]"""
    from tksm_amd.sequence import Sequencer
    fq = M.write_fastq(os.path.join(str(d), tag + ".fq" + (".gz" if gz else "")), reads)
    out = os.path.join(str(d), tag + ".paf" + (".gz" if gz else ""))
    s = sequencer or Sequencer(0)
    try:
        if not sequencer:
            for name, seq in targets:
                s.add_contig(name, seq)
        info = s.map(fq, out, align=align, **params)
    finally:
        if not sequencer:
            s.close()
    assert not [f for f in os.listdir(str(d)) if f.endswith(".tmp")]
    return {"paf": (gzip.open(out, "rt") if gz else open(out)).read(), "info": info}


def same(dev, spec, other=False):
    assert dev["paf"] == spec["other" if other else "paf"]
    assert {k: dev["info"][k] for k in M.COUNTERS} == spec["info"]
    a = dev["info"]["align"]
    assert {k: a[k] for k in A.COUNTERS} == spec["align"]
    assert a["columns"] == a["matches"] + a["mismatches"] + a["inserted"] + a["deleted"] and a["lines"] == dev["info"]["lines"]
    assert a["align_ms"] > 0 or not a["lines"]
    for line in dev["paf"].splitlines():
        f = line.split("\t")
        t, q, n = A.cigar_spans(f[-1][5:])
        assert f[-1].startswith("cg:Z:") and t == int(f[8]) - int(f[7]) and q == int(f[3]) - int(f[2])
        assert f[-2].startswith("NM:i:") and int(f[10]) == sum(n.values()) and int(f[-2][5:]) == int(f[10]) - int(f[9])
        assert n["M"] or (int(f[9]) == n["="] and int(f[-2][5:]) == n["X"] + n["I"] + n["D"])


def check(targets, reads, d, band=63, eqx=False, memo=None, **params):
    spec = A.map_reads(targets, reads, band=band, eqx=eqx, memo=memo, **params)
    dev = device(targets, reads, d, align_band=band, eqx=eqx, **params)
    same(dev, spec)
    return dev, spec


def with_copy(g, rs):
    """the generated targets and a lightly edited copy of the first, so that its reads have a second chain"""
    return g["targets"] + [("copy", A.plant(rs, g["targets"][0][1], 0.02)[0])]


@pytest.fixture(scope="module")
def default_case(tmp_path_factory):
    """60 reads of 200 - 600 bases with 8 % planted edits on both strands, every line written (-p 0.0): computed once, shared"""
    d = tmp_path_factory.mktemp("map_align_default")
    g = A.generate(d, seed=1)
    g["targets"] = with_copy(g, random.Random(2))
    g["ref"] = M.write_fasta(os.path.join(str(d), "with_copy.fa"), g["targets"])
    g["dir"], g["out"] = d, A.map_reads(g["targets"], g["read_list"], secondary_ratio=0.0)
    return g


def test_exact_reads_give_one_run_and_no_edit(tmp_path):
    g = A.generate(tmp_path, seed=4, n_reads=30, error=0.0)
    dev, spec = check(g["targets"], g["read_list"], tmp_path)
    assert spec["info"]["mapped"] == 30
    for line in dev["paf"].splitlines():
        f = line.split("\t")
        assert f[-2] == "NM:i:0" and f[-1] == "cg:Z:%sM" % f[10] and f[9] == f[10]


def test_planted_edits_both_strands_and_secondary_lines(default_case):
    g = default_case
    dev = device(g["targets"], g["read_list"], g["dir"], secondary_ratio=0.0)
    same(dev, g["out"])
    eqx = device(g["targets"], g["read_list"], g["dir"], tag="eqx", secondary_ratio=0.0, eqx=True)
    same(eqx, g["out"], other=True)
    assert g["out"]["info"]["secondary"] > 0 and {l.split("\t")[4] for l in dev["paf"].splitlines()} == {"+", "-"}
    assert any("X" in l.split("cg:Z:")[1] for l in eqx["paf"].splitlines()) and all(c not in l.split("cg:Z:")[1] for l in dev["paf"].splitlines() for c in "=X")
    # columns 1-9 and 12 and the tp, cm and s1 tags are those of the same run without alignment
    plain = device(g["targets"], g["read_list"], g["dir"], tag="plain", align=False, secondary_ratio=0.0)
    assert "align" not in plain["info"] and plain["paf"] == g["out"]["plain"]
    for a, b in zip(dev["paf"].splitlines(), plain["paf"].splitlines()):
        fa, fb = a.split("\t"), b.split("\t")
        assert fa[:9] == fb[:9] and fa[11:15] == fb[11:15] and len(fa) == 17 and len(fb) == 15


def broken(rs, target, a, length, delete=0, insert=0):
    """target with one substitution every 10 bases over [a, a + length) (its last base included), so that no 15-mer of the stretch is left,
    and `delete` bases taken out / `insert` bases put in at its middle"""
    out = list(target)
    for x in sorted(set(list(range(a, a + length, 10)) + [a + length - 1])):
        out[x] = rs.choice([c for c in "ACGT" if c != target[x]])
    mid = a + length // 2
    out[mid:mid + delete] = [rs.choice("ACGT") for _ in range(insert)]
    return "".join(out)


SHAPES = [(32, 31), (32, 32), (33, 32), (64, 63), (64, 64), (65, 64), (65, 65), (63, 63), (63, 64), (64, 65)]


def test_segments_around_the_wave_and_the_ring(tmp_path):
    """-w 1 makes every intact 15-mer an anchor, so a stretch without one is one segment of dt = dq = its length + 15, less a deleted base
    or more an inserted one"""
    rs = random.Random(12)
    target = M.random_seq(rs, 420)
    reads = []
    for n, (dt, dq) in enumerate(SHAPES):
        read = broken(rs, target, 150, dt - 15, delete=max(dt - dq, 0), insert=max(dq - dt, 0))
        reads += [("f%d" % n, read), ("r%d" % n, M.revcomp(read))]
        one = A.map_reads([("t", target)], [reads[-2]], w=1)
        assert (dt, dq) in one["shapes"] and one["align"]["longest_segment"] == dt + dq
    dev, spec = check([("t", target)], reads, tmp_path, w=1)
    assert spec["info"]["mapped"] == 2 * len(SHAPES) and (1, 1) in spec["shapes"]


@pytest.mark.parametrize("band", [1, 2, 63])
def test_an_indel_outside_and_inside_the_band(tmp_path, band):
    rs = random.Random(13)
    target = M.random_seq(rs, 400)
    read = broken(rs, target, 150, 80, delete=40)
    dev, spec = check([("t", target)], [("f", read), ("r", M.revcomp(read))], tmp_path, band=band, w=1)
    wide = A.map_reads([("t", target)], [("f", read)], band=63, w=1)
    assert (95, 55) in spec["shapes"]
    # 40 deletions and the 9 substitutions is what the band of 63 finds or beats; a band of 1 or 2 cannot hold 40 deletions in a row
    assert wide["nm"]["f"] <= 49 and (spec["nm"]["f"] > 49) == (band < 63)


@pytest.mark.parametrize("band", [63, 1])
def test_chains_of_tandem_repeats_at_the_edge_of_the_predecessor_window(tmp_path, band):
    """M.tandem_case (what it reaches: tests/test_map.py): the chains that link at distance 63 and 64, the shorter one that the window of
    64 leaves of r = 65, and the single anchors of r = 66, each aligned"""
    case = M.tandem_case()
    dev, spec = check(case["targets"], case["reads"], tmp_path, band=band, memo=case["memo"], **case["params"])
    chain = {name: lines[0][3] for name, lines in spec["lines"].items()}
    assert spec["align"]["lines"] == 8 and M.classes_of_chain(chain["f64"])["distance_64"] > 0 and M.classes_of_chain(chain["r64"])["distance_64"] > 0
    assert 1 == chain["f66"]["cnt"] < chain["f65"]["cnt"] < chain["f64"]["cnt"] == chain["f63"]["cnt"]


def test_chains_of_dense_groups_with_ties_in_both_tiles(tmp_path):
    """A.dense_case for k = 4, 5 and 6 with --eqx: the written chains went through every kind of tie (M.CLASSES)"""
    total = dict.fromkeys(M.CLASSES, 0)
    for k in A.DENSE:
        targets, reads, params = A.dense_case(k)
        dev, spec = check(targets, reads, tmp_path, eqx=True, **params)
        for what, n in M.classes_of_lines(spec).items():
            total[what] += n
    assert all(total[what] >= 1 for what in M.CLASSES if what != "distance_64"), total


def test_one_long_segment_near_max_gap_and_bandwidth(tmp_path):
    rs = random.Random(14)
    target = M.random_seq(rs, 5600)
    read = broken(rs, target, 350, 4870, delete=500)
    dev, spec = check([("t", target)], [("f", read), ("r", M.revcomp(read))], tmp_path)
    long = [(dt, dq) for dt, dq in spec["shapes"] if dt > 4000]
    assert len(long) == 1 and 4870 < long[0][0] <= 5000 and long[0][0] - long[0][1] == 500 and spec["info"]["mapped"] == 2


def test_dense_overlapping_anchors(tmp_path):
    """-k 4 -w 1: anchors overlap, so dt < k and dq < k, and 1-base indels and homopolymers give dt != dq with dt = 1 or dq = 1"""
    rs = random.Random(15)
    targets, reads = [], []
    for t in range(6):
        seq = M.random_seq(rs, 30) + "A" * rs.randint(3, 7) + M.random_seq(rs, 30) + "CC" + M.random_seq(rs, 25)
        targets.append(("t%d" % t, seq))
        for r in range(6):
            read = A.plant(rs, seq, 0.04)[0]
            reads.append(("q%d_%d" % (t, r), read if r % 2 else M.revcomp(read)))
    dev, spec = check(targets, reads, tmp_path, k=4, w=1, min_score=10, secondary_ratio=0.0)
    shapes = spec["shapes"]
    assert spec["info"]["mapped"] >= 30
    assert any(dt < 4 and dq < 4 and dt != dq for dt, dq in shapes) and any(dt == 1 and dq > 1 for dt, dq in shapes) and any(dq == 1 and dt > 1 for dt, dq in shapes)


def test_n_runs_in_reads_and_targets(tmp_path):
    rs = random.Random(16)
    seq = M.random_seq(rs, 700)
    target = seq[:200] + "NNNNNNN" + seq[207:450] + "N" + seq[451:]
    reads = []
    for r in range(8):
        a = rs.randint(0, 100)
        piece = list(A.plant(rs, seq[a:a + 550], 0.03)[0])
        for x in (120, 121, 122, 300, 420 + r):
            piece[x] = "N"
        reads.append(("n%d" % r, "".join(piece) if r % 2 else M.revcomp("".join(piece))))
    dev, spec = check([("t", target)], reads, tmp_path, w=5, eqx=True)
    assert spec["info"]["mapped"] == 8 and spec["align"]["mismatches"] >= 8 * 5


def test_every_offset_within_a_packed_word_on_the_reverse_strand(tmp_path):
    rs = random.Random(17)
    target = M.random_seq(rs, 420)
    reads = []
    for off in range(32):
        piece = list(target[60:60 + 192 + off])
        for x in range(20 + off, len(piece), 37):
            piece[x] = rs.choice([c for c in "ACGT" if c != piece[x]])
        reads.append(("o%02d" % off, M.revcomp("".join(piece))))
    dev, spec = check([("t", target)], reads, tmp_path, eqx=True)
    assert spec["info"]["mapped"] == 32 and {l.split("\t")[4] for l in dev["paf"].splitlines()} == {"-"}


@pytest.mark.parametrize("chunk_reads", [1, 7, 64])
def test_chunk_sizes_give_the_same_bytes(default_case, tmp_path, chunk_reads):
    g = default_case
    dev = device(g["targets"], g["read_list"], tmp_path, chunk_reads=chunk_reads, secondary_ratio=0.0)
    same(dev, g["out"])
    assert dev["info"]["chunks"] == (60 + chunk_reads - 1) // chunk_reads


def test_a_chunk_over_the_alignment_budget_is_split(tmp_path):
    """5 600 copies of one read whose 486 anchors lie on each of 6 identical targets: 16.3 M anchors, below the anchor budget (2^24), but the
    33 600 lines' anchors alone take 131 MB, above what a chunk's alignment may take (128 MiB): the chunk is halved, nothing else changes"""
    rs = random.Random(8)
    t = M.random_seq(rs, 500)
    targets = [("same%02d" % i, t) for i in range(6)]
    reads = [("copy%04d" % i, t) for i in range(5600)]
    spec = A.map_reads(targets, reads, k=15, w=1, secondary_ratio=0.0)
    lines, segments = spec["align"]["lines"], spec["align"]["segments"]
    fixed = lines * (16 + 32 + 8 + 63 * 4) + segments * 8              # per line: its two records, its run offset and its 1 000 columns' words
    assert spec["info"]["anchors"] == 5600 * 486 * 6 < 1 << 24 and fixed > 128 << 20 > fixed // 2 + lines * 8
    dev = device(targets, reads, tmp_path, k=15, w=1, secondary_ratio=0.0)
    same(dev, spec)
    assert dev["info"]["chunks"] == 2 and spec["align"]["lines"] == 5600 * 6


@pytest.mark.parametrize("word", ["00000001", "ffffffff"])
def test_recycled_memory_does_not_reach_the_output(default_case, tmp_path, word):
    """the module in a child whose device allocations are filled with a word first (TKSMSEQ_POISON): the same bytes"""
    g = default_case
    out = tmp_path / "poisoned.paf"
    env = dict(os.environ, TKSMSEQ_POISON=word)
    r = subprocess.run([EXE, "map", "-r", g["ref"], "--reads", g["reads"], "-o", str(out), "-c", "-p", "0.0", "--chunk-reads", "25"], capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stderr[-600:]
    assert f"poison {word}:" in r.stderr and " 0 blocks" not in r.stderr
    assert out.read_text() == g["out"]["paf"]


def test_same_context_twice_and_after_another_module(default_case, tmp_path):
    from tksm_amd.sequence import Sequencer
    g = default_case
    s = Sequencer(0)
    try:
        for name, seq in g["targets"]:
            s.add_contig(name, seq)
        first = device(None, g["read_list"], tmp_path, tag="first", sequencer=s, secondary_ratio=0.0)
        mdf = "".join(f"+m{i}\t1\t\n{name}\t0\t{len(seq)}\t+\t\n" for i, (name, seq) in enumerate(g["targets"]))
        b = s.batch_from_mdf(mdf)
        records = s.run(b, target="perfect", fastq=True).records()
        b.free()
        assert len(records) == len(g["targets"])
        plain = device(None, g["read_list"], tmp_path, tag="between", sequencer=s, align=False, secondary_ratio=0.0)
        second = device(None, g["read_list"], tmp_path, tag="second", sequencer=s, chunk_reads=33, secondary_ratio=0.0, eqx=True)
    finally:
        s.close()
    same(first, g["out"])
    same(second, g["out"], other=True)
    assert plain["paf"] == g["out"]["plain"]


def test_error_codes_and_the_null_call(default_case, tmp_path):
    from tksm_amd import _lib
    from tksm_amd.sequence import Sequencer, TksmSeqError
    g = default_case
    s = Sequencer(0)
    try:
        for name, seq in g["targets"]:
            s.add_contig(name, seq)
        for bad in (dict(align_band=0), dict(align_band=64), dict(max_gap=65537)):
            with pytest.raises(TksmSeqError) as e:
                s.map(g["reads"], tmp_path / "o.paf", align=True, **bad)
            assert e.value.code == _lib.EINVAL and "map: " in str(e.value), bad
        assert not (tmp_path / "o.paf").exists()
        assert s.map(g["reads"], tmp_path / "gap.paf", max_gap=65537)["reads"] == 60          # without alignment max_gap has no such limit
        assert s.map(g["reads"], tmp_path / "edge.paf", align=True, max_gap=65536, align_band=1)["align"]["lines"] > 0
        # align == NULL: the bytes of tksmseq_map
        lib = _lib.load()
        p = _lib.MapParams(15, 10, 500, 5000, 500, 3, 40, 0, 0.0, 5, 0, 0)
        info = _lib.MapInfo()
        rc = lib.tksmseq_map_align(s._ctx, ctypes.byref(p), None, g["reads"].encode(), str(tmp_path / "null.paf").encode(), ctypes.byref(info), None)
        assert rc == 0 and (tmp_path / "null.paf").read_text() == g["out"]["plain"] and info.lines == g["out"]["info"]["lines"]
    finally:
        s.close()


# ------------------------------------------------------------------------------------------------ the loop this is for
def test_transcribe_sequence_map_align_model_sequence(tmp_path):
    """about 2 000 molecules: transcribe -> sequence (Badread, nanopore2020) -> tksm map -c -> tksm model-sequence, which skips no line for a
    missing cg:Z: or a foreign op and uses every primary line; abundance and model-truncation accept the same PAF"""
    from test_map_gpu import transcriptome
    from tksm_amd.sequence import Sequencer
    d = tmp_path
    rs = random.Random(78)
    contigs, gtf, spliced = transcriptome(rs)
    (d / "ann.gtf").write_text(gtf)
    (d / "ab.tsv").write_text("transcript_id\ttpm\tcell_barcode\n" + "".join(f"{tid}\t{rs.randint(1, 30)}\t.\n" for tid, _ in spliced))
    s = Sequencer(0)
    try:
        for name, seq in contigs:
            s.add_contig(name, seq)
        s.add_gtf(str(d / "ann.gtf"))
        s.set_identity(84.0, 99.0, 5.5); s.load_error_model(ERR_MODEL); s.load_qscore_model(QS_MODEL)
        plan = s.transcribe_plan(str(d / "ab.tsv"), 2000, seed=6)
        batch = plan.batch()
        records = s.run(batch, target="badread", fastq=True, compute_qual=True, seed=6).records()
        batch.free()
        plan.close()
    finally:
        s.close()
    half = len(records) // 2
    (d / "a.fq").write_bytes(b"".join(records[:half]))
    with gzip.open(d / "b.fq.gz", "wb") as f:
        f.write(b"".join(records[half:]))
    ref = M.write_fasta(d / "tx.fa", spliced)
    fqs = f"{d / 'a.fq'},{d / 'b.fq.gz'}"
    for flags, paf in (([], d / "c.paf.gz"), (["--eqx"], d / "eqx.paf")):
        r = subprocess.run([EXE, "map", "-r", ref, "--reads", fqs, "-o", str(paf), "-c", "-p", "0.0", *flags], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-600:]
        r = subprocess.run([EXE, "model-sequence", "--reference", ref, "--reads", fqs, "--alignment", str(paf), "--error-model", str(d / "e.gz"), "--qscore-model",
                            str(d / "q.gz")], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-600:]
        assert gzip.open(d / "e.gz", "rt").read().count("\n") > 10 and "overall;" in gzip.open(d / "q.gz", "rt").read()
    lines = gzip.open(d / "c.paf.gz", "rt").read().splitlines()
    primary = sum("\ttp:A:P\t" in l for l in lines)
    assert primary > 1500 and all("\tcg:Z:" in l and "\tNM:i:" in l for l in lines)
    s = Sequencer(0)
    try:
        for tid, seq in spliced:
            s.add_contig(tid, seq)
        for paf in (d / "c.paf.gz", d / "eqx.paf"):
            info = s.model_sequence([str(d / "a.fq"), str(d / "b.fq.gz")], paf, error_out=d / "e2.gz", qscore_out=d / "q2.gz")
            assert info["lines"] == len(lines) and info["used"] == primary and info["skipped_supplementary"] == len(lines) - primary
            assert info["skipped_no_cigar"] == info["skipped_cigar_op"] == info["skipped_unknown_read"] == info["skipped_unknown_target"] == 0
        s.abundance(d / "c.paf.gz", out=d / "abundance.tsv")
        s.model_truncation(d / "eqx.paf", d / "truncation.json")             # (model-truncation reads plain text)
    finally:
        s.close()
    assert (d / "abundance.tsv").read_text().count("\n") > 10 and (d / "truncation.json").stat().st_size > 0
