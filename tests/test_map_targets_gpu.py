"""map -g on the device against the specification (tests/map_targets_spec.py), no tolerance: the spliced image bit for bit (padding included)
on a fresh context, on one that built a larger set before, and in a child process whose recycled device memory reads as
TKSMSEQ_POISON=00000001; the FASTA and the --perfect reads of `transcribe`; the defining property (the PAF equals the PAF of today's map on
the written FASTA, in every mode); --genome-coords; stale and bad use.  Run as a program (the poisoned child) it writes the image of the
hand-made table to --out."""
import ctypes as C
import gzip
import os
import random
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

import map_spec as M
import map_targets_spec as T

pytestmark = pytest.mark.gpu

ANN = os.path.join(GOLDEN, "transcribe", "ann.gtf")
POISON = "00000001"
CHILD_SECONDS = 60
HIP_TROUBLE = re.compile(r"illegal memory access|Memory access fault|HSA_STATUS_ERROR|hipError|HIP error", re.I)


# ----------------------------------------------------------------------------- the hand-made table of the image test
def image_genome():
    """ga (2 000 letters) and gb (1 100): random, with an N first, last and in the middle of gb's exon [200, 250) and an N block over the word
    boundary at 288"""
    rs = random.Random(77)
    ga, gb = M.random_seq(rs, 2000), list(M.random_seq(rs, 1100))
    for g in [200, 225, 249] + list(range(280, 300)) + [1099]:
        gb[g] = "N"
    gb[600], gb[601] = "a", "n"                                                  # (lower case: read as A and as N)
    return {"ga": ga, "gb": "".join(gb)}


def image_table():
    t = []
    for n in (1, 15, 16, 17, 31, 32, 33, 64, 65):                                # exon (and target) lengths, at every start within a word
        for k, s in enumerate((0, 15, 16, 31, 32)):
            t.append(("len%d_s%d" % (n, s), [("ga", 64 + s, 64 + s + n, "+-"[(n + k) % 2])]))
    t.append(("first", [("ga", 0, 33, "+")]))
    t.append(("last", [("gb", 1100 - 65, 1100, "-")]))
    t.append(("last_plus", [("ga", 1999, 2000, "+"), ("ga", 0, 1, "-")]))
    t.append(("ones", [("ga", 300 + i, 301 + i, "+-"[i % 2]) for i in range(40)]))       # several exons in one word
    t.append(("sums", [("ga", 700, 715, "+"), ("ga", 800, 816, "-"), ("ga", 900, 901, "+"), ("ga", 1000, 1033, "-")]))   # 65 letters
    t.append(("disorder", [("ga", 500, 560, "+"), ("ga", 480, 530, "+"), ("ga", 100, 140, "-"), ("ga", 100, 140, "+")]))
    t.append(("two_contigs", [("ga", 10, 50, "+"), ("gb", 10, 50, "-")]))
    t.append(("n_plus", [("gb", 200, 250, "+")]))
    t.append(("n_minus", [("gb", 200, 250, "-")]))
    t.append(("n_block", [("gb", 270, 310, "+"), ("gb", 270, 310, "-"), ("gb", 590, 610, "-")]))
    t.append(("empty_between", [("ga", 1200, 1231, "+"), ("ga", 5, 5, "-"), ("ga", 1300, 1332, "-")]))
    t.append(("no_exon", []))
    t.append(("all_empty", [("ga", 7, 7, "+")]))
    t.append(("unknown", [("ga", 0, 10, "+"), ("gz", 0, 10, "+")]))
    t.append(("bad_end", [("gb", 1090, 1101, "+")]))
    t.append(("bad_order", [("ga", 30, 20, "+")]))
    t.append(("long", [("ga", 3, 1990, "-"), ("gb", 1, 1099, "+")]))
    return t


def larger_table():
    return [("big%d" % i, [("ga", 0, 2000, "+-"[i % 2]), ("gb", 0, 1100, "+")]) for i in range(6)]


def write_gtf(path, table):
    """transcript and exon lines, 1-based closed; a transcript's own line carries its first exon's contig"""
    with open(path, "w") as f:
        for tid, exons in table:
            c = exons[0][0] if exons else "ga"
            f.write("%s\thand\ttranscript\t1\t2\t.\t+\t.\ttranscript_id \"%s\";\n" % (c, tid))
            for c, a, b, strand in exons:
                f.write("%s\thand\texon\t%d\t%d\t.\t%s\t.\ttranscript_id \"%s\";\n" % (c, a + 1, b, strand, tid))
    return path


def device_image(s, gtf):
    """the image and the tables of the target set of `gtf` on Sequencer s (whose transcript table is replaced)"""
    s.clear_transcripts()
    s.add_gtf(gtf)
    t = s.targets()
    try:
        codes, valid = t.download()
        return dict(codes=codes, valid=valid, names=t.names, lengths=t.lengths, voff=t.voff, projectable=t.projectable, info=dict(t.info))
    finally:
        t.free()


def image_runs(d):
    """{"fresh", "recycled"}: the image of the hand-made table on a new context, and on one that built and freed a larger set first"""
    from tksm_amd.sequence import Sequencer
    small, big = write_gtf(os.path.join(str(d), "image.gtf"), image_table()), write_gtf(os.path.join(str(d), "larger.gtf"), larger_table())
    out = {}
    for how in ("fresh", "recycled"):
        s = Sequencer(0)
        try:
            for name, seq in image_genome().items():
                s.add_contig(name, seq)
            if how == "recycled":
                assert device_image(s, big)["info"]["letters"] == 6 * 3100
            out[how] = device_image(s, small)
        finally:
            s.close()
    return out


def same_image(got, want):
    assert got["names"] == want["names"] and got["lengths"] == want["lengths"] and got["voff"] == want["voff"][:-1] and got["projectable"] == want["projectable"]
    assert {k: got["info"][k] for k in T.COUNTERS} == want["info"]
    assert got["valid"].tolist() == want["valid"] and got["codes"].tolist() == want["codes"]


@pytest.fixture(scope="module")
def image_spec():
    want = T.targets(image_genome(), image_table())
    assert (want["info"]["skipped_empty"], want["info"]["skipped_unknown_contig"], want["info"]["skipped_bad_exon"]) == (2, 1, 2)
    assert set(want["lengths"]) >= {1, 31, 32, 33, 64, 65} and any("N" in s for s in want["seqs"])
    return want


def test_images_bit_for_bit(image_spec, tmp_path):
    runs = image_runs(tmp_path)
    for how in ("fresh", "recycled"):
        same_image(runs[how], image_spec)
        assert runs[how]["info"]["splice_ms"] > 0


def test_poisoned_memory_gives_the_same_image(image_spec, tmp_path):
    env = dict(os.environ, TKSMSEQ_POISON=POISON)
    r = subprocess.run(["timeout", "-k", "10", str(CHILD_SECONDS), sys.executable, os.path.abspath(__file__), "--out", str(tmp_path)], capture_output=True, text=True,
                       env=env, timeout=CHILD_SECONDS + 30)
    assert r.returncode == 0 and not HIP_TROUBLE.search(r.stderr), f"exit status {r.returncode}\n--- stdout\n{r.stdout[-2000:]}\n--- stderr\n{r.stderr[-4000:]}"
    filled = [(int(b), int(n)) for b, n in re.findall(rf"^poison {POISON}: (\d+) blocks, (\d+) bytes$", r.stderr, re.M)]
    assert len(filled) == 2 and all(b > 0 and n > 0 for b, n in filled), r.stderr[-2000:]
    z = np.load(os.path.join(str(tmp_path), "images.npz"))
    for how in ("fresh", "recycled"):
        assert z[how + "_valid"].tolist() == image_spec["valid"] and z[how + "_codes"].tolist() == image_spec["codes"], how


# ----------------------------------------------------------------------------- the fixture: ann.gtf on a seeded genome
EXTRA = [("P5", [("c1", 3000 + 200 * i, 3100 + 200 * i, "+") for i in range(5)])]     # a `+` transcript of five exons, four junctions of 100


def fixture_genome():
    rs = random.Random(2025)
    return {"c1": M.random_seq(rs, 5000), "c2": M.random_seq(rs, 4000), "c3": M.random_seq(rs, 3000)}


def draw_reads(t):
    """about 60 reads of 150 to 600 letters from the targets: half reverse-complemented, every third with 5 % substitutions, a few glued pairs"""
    rs = random.Random(8)
    reads, clean = [], set()
    seqs = [s for s in t["seqs"] if len(s) >= 150]
    for r in range(56):
        seq = seqs[r % len(seqs)]
        n = rs.randint(150, min(600, len(seq)))
        a = rs.randint(0, len(seq) - n)
        piece = seq[a:a + n]
        if r % 3 == 2:
            piece = "".join(rs.choice([x for x in "ACGT" if x != c]) if rs.random() < 0.05 else c for c in piece)
        else:
            clean.add("r%02d" % r)
        reads.append(("r%02d" % r, M.revcomp(piece) if r % 2 else piece))
    for g in range(4):
        a, b = seqs[(2 * g) % len(seqs)], seqs[(2 * g + 5) % len(seqs)]
        # (the second piece scores below 0.8 of the first: a supplementary line with --split, no secondary without)
        reads.append(("glued%d" % g, a[:330] + (M.revcomp(b[-200:]) if g % 2 else b[-200:])))
    return reads, clean


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    """the genome, ann.gtf and the extra transcript on one Sequencer with their target set, the reads, and the specification's targets"""
    from tksm_amd.sequence import Sequencer
    d = tmp_path_factory.mktemp("map_targets")
    genome = fixture_genome()
    extra = write_gtf(os.path.join(str(d), "extra.gtf"), EXTRA)
    table = T.parse([("ann", open(ANN).read()), ("extra", open(extra).read())])
    spec = T.targets(genome, table)
    assert [n for n, ex in table if not ex] == ["T7"] and "T7" not in spec["names"] and spec["info"]["skipped_empty"] == 1
    assert dict(zip(spec["names"], spec["projectable"])) == {"T1": True, "T2": False, "T3": True, "T4": True, "T5": True, "T6": True, "T8.1": False, "T9": True,
                                                            "T10": True, "T11": True, "T12": True, "P5": True}
    s = Sequencer(0)
    for name, seq in genome.items():
        s.add_contig(name, seq)
    s.add_gtf(ANN)
    s.add_gtf(extra)
    targets = s.targets()
    reads, clean = draw_reads(spec)
    fq = M.write_fastq(os.path.join(str(d), "reads.fq"), reads)
    yield dict(dir=d, genome=genome, table=table, spec=spec, s=s, targets=targets, reads=reads, clean=clean, fq=fq, memo={})
    targets.free()
    s.close()


def test_fasta_and_the_perfect_reads_of_transcribe(world, image_spec, tmp_path):
    from tksm_amd.sequence import Sequencer
    s, targets, spec = world["s"], world["targets"], world["spec"]
    same_image(dict(zip(("codes", "valid"), targets.download()), names=targets.names, lengths=targets.lengths, voff=targets.voff, projectable=targets.projectable,
                    info=targets.info), spec)
    for width, name in ((60, "t60.fa"), (0, "t0.fa"), (7, "t7.fa.gz")):
        path = os.path.join(str(tmp_path), name)
        targets.write_fasta(path, line_width=width) if width != 60 else targets.write_fasta(path)
        assert (gzip.open(path).read() if name.endswith(".gz") else open(path, "rb").read()) == T.fasta(spec, width), name
    assert not [f for f in os.listdir(str(tmp_path)) if f.endswith(".tmp")]
    # the hand-made table, its N letters among them
    t = Sequencer(0)
    try:
        for name, seq in image_genome().items():
            t.add_contig(name, seq)
        t.add_gtf(write_gtf(os.path.join(str(tmp_path), "image.gtf"), image_table()))
        ts = t.targets()
        ts.write_fasta(os.path.join(str(tmp_path), "image.fa"), line_width=33)
        ts.free()
    finally:
        t.close()
    text = open(os.path.join(str(tmp_path), "image.fa"), "rb").read()
    assert text == T.fasta(image_spec, 33) and b"N" in text
    # target t is the molecule `transcribe` emits for its transcript: one molecule per kept transcript, sequenced --perfect
    ab = "h\n" + "".join("%s\t1\tACGT\n" % name for name in spec["names"])
    p = s.transcribe_plan(None, len(spec["names"]), seed=4, text=ab, use_whole_id=True)
    b = p.batch()
    try:
        recs = s.run(b, target="perfect", fastq=True, seed=4).records()
        assert p.molecules == len(recs) == len(spec["names"]) == 12
        assert [r.decode().split("\n")[1] for r in recs] == spec["seqs"]
    finally:
        b.free()
        p.close()


MODES = {"plain": dict(), "c": dict(align=True), "c_eqx_extend": dict(align=True, eqx=True, extend=True), "split_c_extend": dict(split=True, align=True, extend=True)}


def spec_modes(mode):
    """the modes of Sequencer.map as map_split_spec.map_reads names them"""
    m = dict(MODES[mode])
    return dict(split=m.pop("split", False), **m)


@pytest.fixture(scope="module")
def on_fasta(world):
    """a second context whose reference is the FASTA the target set wrote"""
    from tksm_amd.sequence import Sequencer
    path = os.path.join(str(world["dir"]), "cdna.fa")
    world["targets"].write_fasta(path)
    s = Sequencer(0)
    for name, seq in M.read_fasta(path):
        s.add_contig(name, seq)
    yield s
    s.close()


@pytest.mark.parametrize("mode", list(MODES))
def test_defining_property(world, on_fasta, tmp_path, mode):
    a, b = os.path.join(str(tmp_path), "targets.paf"), os.path.join(str(tmp_path), "fasta.paf")
    got = world["s"].map(world["fq"], a, targets=world["targets"], **MODES[mode])
    ref = on_fasta.map(world["fq"], b, **MODES[mode])
    spec = T.map_reads(world["genome"], world["table"], world["reads"], memo=world["memo"], **spec_modes(mode))
    text = open(a).read()
    assert text == open(b).read() and text == spec["paf"]
    assert {k: got[k] for k in M.COUNTERS} == {k: ref[k] for k in M.COUNTERS} == spec["info"]
    assert got["project"] == dict.fromkeys(T.PROJECT_COUNTERS, 0) and "project" not in ref
    assert got["mapped"] >= 58 and (mode != "split_c_extend" or got["split"]["supplementary"] >= 3)
    if mode == "split_c_extend":
        c = os.path.join(str(tmp_path), "chunks.paf")
        world["s"].map(world["fq"], c, targets=world["targets"], chunk_reads=7, **MODES[mode])
        assert open(c).read() == text


def crafted_reads(spec):
    p5, t3, t8 = (spec["seqs"][spec["names"].index(n)] for n in ("P5", "T3", "T8.1"))
    return [("plus3", p5[60:340]),                                               # three junctions of a `+` transcript
            ("minus3", M.revcomp(t3[250:560])),                                  # three junctions of a descending `-` transcript
            ("exon_end", p5[20:100]),                                            # ends at an exon's last letter
            ("exon_start", p5[200:290]),                                         # starts at an exon's first letter
            ("ins", p5[30:100] + "GATTACA" + p5[100:170]),                       # an insertion at a junction
            ("del", p5[120:195] + p5[206:290]),                                  # a deletion over a junction: letters dropped on both sides
            ("mixed", t8[150:450])]                                              # the mixed-strand target: stays in transcript coordinates


@pytest.mark.parametrize("mode", ["plain", "c_eqx_extend"])
def test_genome_coords(world, tmp_path, mode):
    spec_t = world["spec"]
    reads = world["reads"] + crafted_reads(spec_t)
    fq = M.write_fastq(os.path.join(str(tmp_path), "reads.fq"), reads)
    out = os.path.join(str(tmp_path), "genome.paf")
    got = world["s"].map(fq, out, targets=world["targets"], genome_coords=True, **MODES[mode])
    spec = T.map_reads(world["genome"], world["table"], reads, genome_coords=True, memo=world["memo"], **spec_modes(mode))
    text = open(out).read()
    assert text == spec["paf"] and got["project"] == spec["project"]
    assert got["project"]["lines"] == got["lines"] == got["project"]["projected"] + got["project"]["unprojected"]
    assert got["project"]["unprojected"] >= 1 and spec["first_unprojected"] in ("T2", "T8.1")
    rows = {}
    for line in text.splitlines():
        rows.setdefault(line.split("\t")[0], []).append(line.split("\t"))
    mixed = rows["mixed"][0]
    assert mixed[5] == "T8.1" and mixed[6] == "600" and not mixed[-1].startswith("tx:Z:")
    span = {n: (ex[0][0], min(a for _, a, _, _ in ex), max(b for _, _, b, _ in ex)) for n, ex in zip(spec_t["names"], spec_t["exons"])}
    for name in sorted(world["clean"]) + ["plus3", "minus3", "exon_end", "exon_start"]:
        f = rows[name][0]
        if not f[-1].startswith("tx:Z:"):
            continue
        c, lo, hi = span[f[-1][5:]]
        assert f[5] == c and f[6] == str(len(world["genome"][c])) and lo <= int(f[7]) < int(f[8]) <= hi, name
        if mode != "plain":
            runs = T.cigar_runs(f[-2][5:])
            assert {op for _, op in runs} <= {"=", "N"} and sum(n for n, op in runs if op == "=") == int(f[1]), name
    if mode == "plain":
        return
    cg = {name: rows[name][0][-2][5:] for name in ("plus3", "minus3", "exon_end", "exon_start", "ins", "del")}
    assert cg["plus3"] == "40=100N100=100N100=100N40=" and rows["plus3"][0][4:9] == ["+", "c1", "5000", "3060", "3640"]
    assert cg["minus3"] == "60=100N100=100N100=100N50=" and rows["minus3"][0][4:9] == ["+", "c1", "5000", "1840", "2450"]
    assert cg["exon_end"] == "80=" and rows["exon_end"][0][7:9] == ["3020", "3100"] and cg["exon_start"] == "90=" and rows["exon_start"][0][7:9] == ["3400", "3490"]
    runs = T.cigar_runs(cg["ins"])
    assert [op for _, op in runs].count("N") == 1 and sum(n for n, op in runs if op == "I") - sum(n for n, op in runs if op == "D") == 7       # 147 read, 140 target letters
    runs = T.cigar_runs(cg["del"])
    assert [op for _, op in runs].count("N") == 1 and sum(n for n, op in runs if op == "D") - sum(n for n, op in runs if op == "I") == 11      # 159 read, 170 target letters


def test_stale_and_bad_use(world, tmp_path):
    from tksm_amd import _lib as L
    from tksm_amd.sequence import Sequencer, TksmSeqError
    fq, out = world["fq"], os.path.join(str(tmp_path), "o.paf")
    s = Sequencer(0)
    try:
        with pytest.raises(TksmSeqError) as e:                                   # no transcript table
            s.targets()
        assert e.value.code == L.EINVAL
        for name, seq in world["genome"].items():
            s.add_contig(name, seq)
        with pytest.raises(TksmSeqError) as e:
            s.targets()
        assert e.value.code == L.EINVAL
        s.add_gtf(ANN)
        t = s.targets()
        assert s.map(fq, out, targets=t)["mapped"] > 0
        s.add_gtf(ANN)                                                           # (nothing new, yet a new table)
        for use in (lambda: s.map(fq, out, targets=t), t.download, lambda: t.write_fasta(os.path.join(str(tmp_path), "x.fa"))):
            with pytest.raises(TksmSeqError, match="transcript table has changed") as e:
                use()
            assert e.value.code == L.EINVAL
        t.free()
        t = s.targets()
        s.add_contig("c9", "ACGT" * 50)                                          # the reference grew
        with pytest.raises(TksmSeqError, match="reference has changed") as e:
            s.map(fq, out, targets=t)
        assert e.value.code == L.EINVAL
        t.free()
        # another context's set, and genome_coords without a set (the C call itself: Python refuses earlier)
        with pytest.raises(TksmSeqError, match="another context") as e:
            s.map(fq, out, targets=world["targets"])
        assert e.value.code == L.EINVAL
        tp = L.MapTargetsParams(1, 0)
        rc = s._lib.tksmseq_map_targets(s._ctx, None, C.byref(tp), None, None, None, None, fq.encode(), out.encode(), None, None, None, None, None)
        assert rc == L.EINVAL and b"genome_coords needs a target set" in s._lib.tksmseq_last_error(s._ctx)
        assert not os.path.exists(os.path.join(str(tmp_path), "x.fa"))
    finally:
        s.close()


def _child(out):
    runs = image_runs(out)
    np.savez(os.path.join(out, "images.npz"), **{how + "_" + k: runs[how][k] for how in runs for k in ("codes", "valid")})


if __name__ == "__main__":
    _child(sys.argv[sys.argv.index("--out") + 1])
