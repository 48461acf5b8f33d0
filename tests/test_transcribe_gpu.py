"""transcribe on the device (-m gpu): tksmseq_transcribe / tksmseq_transcribe_text against the specification (tests/tsb_spec.py), text for
text, over slices that cut rows; the device-made batch against the batch parsed from the compact text; independence of the slicing at
2 M molecules and the 2^28 limit; the errors; a check that does not go through the specification (--perfect reads are the spliced
exons); `tksm transcribe` + `tksm sequence -i` against the chained `tksm sequence --transcribe-*`, byte for byte; the Python chain
plan.batch -> polya -> scb -> tag -> run.  CPU part: tests/test_transcribe.py."""
import ctypes
import gzip
import os
import subprocess

import numpy as np
import pytest

from conftest import ERR_MODEL, QS_MODEL, ROOT

import tsb_spec as ts

EXE = os.path.join(ROOT, "tksm_amd", "tksm")
pytestmark = pytest.mark.gpu
CONTIGS = [("chrA", 12_000), ("chrB", 9_000), ("chrC", 7_000)]
EXON_COUNTS = (1, 2, 63, 64, 65, 200)
BARCODES = ["ACGTACGTACGTACGT", "TTTTGGGGCCCCAAAA", "GATTACAGATTACAGA"]


def _cli(*args, timeout=600, **kw):
    return subprocess.run([EXE, *[str(a) for a in args]], capture_output=True, text=True, timeout=timeout, **kw)


def _genome(seed=17):
    rs = np.random.RandomState(seed)
    return {name: rs.choice(np.frombuffer(b"ACGT", np.uint8), n).tobytes().decode() for name, n in CONTIGS}


def _write_fasta(path, ref, width=60):
    with open(path, "w") as f:
        for name, seq in ref.items():
            f.write(f">{name} test contig\n" + "".join(seq[i:i + width] + "\n" for i in range(0, len(seq), width)))


def _make_gtf(rs, n, contigs, tag="T", counts=EXON_COUNTS, bare=0):
    """n transcripts (the last `bare` without exon lines) -> (text, {id: exon count}); exons of 10 - 39 bases, 5 - 19 apart, in file
    order along the contig for '+' transcripts and against it for '-' ones; the longest run past the end of a 7 000-base contig"""
    out, n_ex = ["# made by the test\n"], {}
    for k in range(n):
        tid = f"{tag}{k}"
        chrom = contigs[int(rs.randint(len(contigs)))]
        strand = "+-"[int(rs.randint(2))]
        ne = 0 if k >= n - bare else counts[k % len(counts)] if k < 2 * len(counts) else counts[int(rs.randint(len(counts)))]
        at = f'gene_id "G{k // 3}"; transcript_id "{tid}"; gene_biotype "protein_coding";'
        pos, exons = int(rs.randint(1, 400)), []
        for _ in range(ne):
            ln = int(rs.randint(10, 40))
            exons.append((pos, pos + ln - 1))
            pos += ln + int(rs.randint(5, 20))
        out.append(f"{chrom}\ttest\ttranscript\t{exons[0][0] if exons else 1}\t{pos}\t.\t{strand}\t.\t{at}\n")
        for a, b in (exons if strand == "+" else exons[::-1]):
            out.append(f"{chrom}\ttest\texon\t{a}\t{b}\t.\t{strand}\t.\t{at}\n")
        n_ex[tid] = ne
    return "".join(out), n_ex


def _make_abundance(rs, n_rows, n_ex, big_row=None, cbs=("ACGT", "TTGCA", ".", ""), unfound=0.07):
    """rows whose tpm is a multiple of 0.25 and whose sum is the molecule count: every count is its tpm, a carry of .25 / .5 / .75 is decided
    by the row's draw.  Nine rows in ten name a transcript of one or two exons.  Returns (text, molecule count)"""
    small = [t for t, e in n_ex.items() if e <= 2]
    large = [t for t, e in n_ex.items() if e > 2]
    values = np.array([0, 1, 7, 0.25, 0.5, 2.75])
    tpm = values[rs.choice(len(values), n_rows, p=[0.3, 0.47, 0.08, 0.05, 0.05, 0.05])]
    lines, total = ["transcript_id\ttpm\tcell\n"], 0.0
    for r in range(n_rows):
        u = rs.random_sample()
        tid = f"ghost{r}" if u < unfound else large[int(rs.randint(len(large)))] if (u > 0.97 and large) else small[int(rs.randint(len(small)))]
        v = float(tpm[r])
        if big_row is not None and r == big_row[0]:
            tid, v = next(t for t in small if n_ex[t] == 1), float(big_row[1])
        lines.append(f"{tid}.{r % 3}\t{v!r}\t{cbs[r % len(cbs)]}\n".replace("\t\n", "\n"))
        total += v
    pad = float(np.ceil(total)) - total + 3.0                             # an unfound row that makes the sum an integer
    lines.append(f"pad\t{pad!r}\tACGT\n")
    return "".join(lines), int(total + pad)


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    """the genome, a GTF of 300 transcripts (some on a contig the reference lacks), a Sequencer that holds both, and the 70 001-row plan
    with its specification -- made once, read by the tests"""
    from tksm_amd.sequence import Sequencer
    d = tmp_path_factory.mktemp("tsb")
    rs = np.random.RandomState(31)
    ref = _genome()
    gtf, n_ex = _make_gtf(rs, 300, ["chrA", "chrB", "chrC", "chrNoFasta"], bare=2)
    assert set(n_ex.values()) == set(EXON_COUNTS) | {0}
    ab, mc = _make_abundance(rs, 70_000, n_ex, big_row=(40_123, 100_000))
    (d / "ann.gtf").write_text(gtf)
    (d / "ab.tsv").write_text(ab)
    s = Sequencer(0)
    for name, seq in ref.items():
        s.add_contig(name, seq)
    s.add_gtf(d / "ann.gtf")
    s.set_identity(84.0, 99.0, 5.5)
    s.load_error_model(ERR_MODEL)
    s.load_qscore_model(QS_MODEL)
    spec = ts.tsb_spec(42, [gtf], [ab], mc)[0]
    plan = s.transcribe_plan(d / "ab.tsv", mc, seed=42)
    yield dict(dir=d, ref=ref, gtf=gtf, n_ex=n_ex, ab=ab, mc=mc, s=s, spec=spec, plan=plan)
    plan.close()
    s.close()


def _text(s, batch):
    try:
        return s.to_mdf_text(batch)
    finally:
        batch.free()


def test_kernels_match_the_specification(world):
    s, plan, spec = world["s"], world["plan"], world["spec"]
    assert spec.rows == 70_001 and (plan.rows, plan.records, plan.molecules) == (spec.rows, spec.records, spec.molecules)
    assert plan.missing == spec.missing and len(plan.missing) > 3000
    depths = set(spec.depth.tolist())
    assert {0, 1, 7, 100_000} <= depths and spec.records > 10_000                       # index digits roll over up to 9 999 -> 10 000
    assert s.transcripts_info() == {"n_transcripts": 300, "n_exons": sum(world["n_ex"].values())}
    assert plan.mdf_text() == spec.mdf_text()
    assert plan.mdf_text(9_998, 5) == spec.mdf_text(9_998, 5) and plan.mdf_text(spec.records, 3) == ""
    big = int(np.flatnonzero(spec.depth[spec.emitted] == 100_000)[0])
    b0 = int(spec.first[big])
    mid = [int(spec.first[k]) + int(spec.depth[spec.emitted[k]]) // 2 for k in range(spec.records) if spec.depth[spec.emitted[k]] == 7][:40]
    slices = [(0, None), (0, 1), (b0 + 99, 1001), (b0 - 3, 10), (b0 + 99_990, 25), (mid[0], mid[9] - mid[0]), (mid[20], 1),
              (spec.molecules - 1, 1), (spec.molecules - 1, 50), (spec.molecules, 10), (spec.molecules + 1000, 10), (5, 0)]
    for first, n in slices:
        got = _text(s, plan.batch(first, n))
        assert got == spec.unrolled_text(first, n), (first, n)
    whole = _text(s, plan.batch())
    assert whole.count("\n+") + 1 == spec.molecules
    assert f"+M{big}_99999\t1\t" in whole and f"+M{big}_100000" not in whole
    # without comments: the same molecules, an empty comment column
    assert _text(s, plan.batch(b0 - 3, 10, comments=False)) == spec.unrolled_text(b0 - 3, 10, comments=False)
    # other parameters of the plan: seed, prefix, whole ids (every row's id carries a version: nothing is found), first row index
    for kw in (dict(seed=7), dict(prefix="mol-"), dict(use_whole_id=True), dict(first_row_index=2**33 + 5), dict(weight=0.37)):
        p = s.transcribe_plan(world["dir"] / "ab.tsv", world["mc"], **{"seed": 42, **kw})
        isoforms = ts.read_gtfs([world["gtf"]])
        want = ts.TsbPlan(kw.get("seed", 42), isoforms, world["ab"], world["mc"], kw.get("weight", 1.0), kw.get("first_row_index", 0),
                          kw.get("use_whole_id", False), kw.get("prefix", "M"))
        try:
            assert (p.rows, p.records, p.molecules) == (want.rows, want.records, want.molecules), kw
            assert p.mdf_text() == want.mdf_text(), kw
            assert _text(s, p.batch(want.molecules // 2, 300)) == want.unrolled_text(want.molecules // 2, 300), kw
        finally:
            p.close()
    assert ts.TsbPlan(7, isoforms, world["ab"], world["mc"], 1.0, 0, False, "M").mdf_text() != spec.mdf_text()      # the draws matter


def test_device_batch_equals_the_batch_parsed_from_the_compact_text(world):
    s, plan = world["s"], world["plan"]
    compact = plan.mdf_text()
    assert _text(s, plan.batch()) == _text(s, s.batch_from_mdf(compact))
    bare = "".join(l.rsplit("\t", 1)[0] + "\t\n" if l.startswith("+") else l + "\n" for l in compact.split("\n")[:-1])
    assert _text(s, plan.batch(comments=False)) == _text(s, s.batch_from_mdf(bare))
    # a context without the reference: every contig is a literal, the text is the same
    from tksm_amd.sequence import Sequencer
    t = Sequencer(0)
    try:
        t.add_gtf(world["dir"] / "ann.gtf")
        p = t.transcribe_plan(None, world["mc"], seed=42, text=world["ab"])
        assert _text(t, p.batch(1000, 5000)) == world["spec"].unrolled_text(1000, 5000)
        # the reference arrives afterwards: the table is resolved again
        for name, seq in world["ref"].items():
            t.add_contig(name, seq)
        assert _text(t, p.batch(1000, 5000)) == world["spec"].unrolled_text(1000, 5000)
        p.close()
    finally:
        t.close()


def test_two_million_molecules_whole_and_in_four_pieces_and_the_call_limit(world):
    from tksm_amd.sequence import TksmSeqError
    from tksm_amd import _lib as L
    s = world["s"]
    one = [t for t, e in world["n_ex"].items() if e == 1][:8]
    ab = "h\n" + "".join(f"{one[r % 8]}\t100\tACGT\n" for r in range(20_000))
    p = s.transcribe_plan(None, 2_000_000, seed=1, text=ab)
    try:
        assert (p.records, p.molecules) == (20_000, 2_000_000)
        whole = _text(s, p.batch())
        parts = [_text(s, p.batch(k * 500_000 + (37 if k else 0), 500_000 + (37 if k == 0 else -37 if k == 3 else 0))) for k in range(4)]
        assert whole.count("\n") == 4_000_000 and "".join(parts) == whole
        with pytest.raises(TksmSeqError) as e:
            p.batch(0, 2**28 + 1)
        assert e.value.code == L.ELIMIT and "2^28" in str(e.value)
        b = p.batch(5, 2**28)                                                             # the limit itself is allowed (and clipped to the end)
        assert b.n_reads == 2_000_000 - 5
        b.free()
    finally:
        p.close()


def test_errors(world, tmp_path):
    from tksm_amd.sequence import Sequencer, TksmSeqError
    from tksm_amd import _lib as L
    t = Sequencer(0)
    try:
        with pytest.raises(TksmSeqError) as e:
            t.transcribe_plan(world["dir"] / "ab.tsv", 10)
        assert e.value.code == L.ESTATE and "no GTF" in str(e.value)
        bad = tmp_path / "bad.gtf"
        bad.write_text(world["gtf"].split("\n", 3)[1] + "\nchrA\tx\texon\t5\n")
        with pytest.raises(TksmSeqError) as e:
            t.add_gtf(bad)
        assert e.value.code == L.EINVAL and f"{bad}:2:" in str(e.value) and "9 tab-separated fields" in str(e.value)
        assert t.transcripts_info() == {"n_transcripts": 0, "n_exons": 0}              # a failed file adds nothing
        bad.write_text("chrA\tx\texon\t5\t9\t.\t+\t.\tgene_id \"g\";\n")
        with pytest.raises(TksmSeqError) as e:
            t.add_gtf(bad)
        assert e.value.code == L.EINVAL and f"{bad}:1:" in str(e.value) and "before any transcript" in str(e.value)
        bad.write_text("#\n\nchrA\tx\tgene\t5\tnine\t.\t+\t.\tgene_id \"g\";\n")
        with pytest.raises(TksmSeqError) as e:
            t.add_gtf(bad)
        assert e.value.code == L.EINVAL and f"{bad}:3:" in str(e.value)
        with pytest.raises(TksmSeqError) as e:
            t.add_gtf(tmp_path / "none.gtf")
        assert e.value.code == L.EIO
        t.add_gtf(world["dir"] / "ann.gtf")
        with pytest.raises(TksmSeqError) as e:
            t.transcribe_plan(tmp_path / "none.tsv", 10)
        assert e.value.code == L.EIO and "Could not open abundance file" in str(e.value)
        # a plan is used on the context it was made for, with the transcript table it was made with
        p = t.transcribe_plan(world["dir"] / "ab.tsv", world["mc"])
        h = ctypes.c_void_p()
        assert world["s"]._lib.tksmseq_transcribe(world["s"]._ctx, p._h, 0, 1, 0, ctypes.byref(h)) == L.ESTATE and not h.value
        t.add_gtf(world["dir"] / "ann.gtf")                                                # (nothing new, yet a new table)
        with pytest.raises(TksmSeqError) as e:
            p.batch(0, 1)
        assert e.value.code == L.ESTATE and "has changed" in str(e.value)
        p.close()
        t.clear_transcripts()
        assert t.transcripts_info() == {"n_transcripts": 0, "n_exons": 0}
    finally:
        t.close()


def _revcomp(s):
    return s.translate(str.maketrans("ACGTN", "TGCAN"))[::-1]


def test_perfect_reads_are_the_spliced_exons(world):
    """not through the specification: the sequence of every sampled read, rebuilt from the genome and the exon lines of the GTF text"""
    s, ref = world["s"], world["ref"]
    exons, cur = {}, None
    for l in world["gtf"].split("\n"):
        f = l.split("\t")
        if len(f) == 9 and f[2] == "transcript":
            cur = f[8].split('transcript_id "')[1].split('"')[0]
            exons[cur] = []
        elif len(f) == 9 and f[2] == "exon":
            exons[cur].append((f[0], int(f[3]) - 1, int(f[4]), f[6]))
    known = [t for t, ex in exons.items() if ex and all(c in ref for c, _, _, _ in ex)]
    rs = np.random.RandomState(3)
    rows = [known[int(rs.randint(len(known)))] for _ in range(400)]
    ab = "h\n" + "".join(f"{t}\t{1 + k % 3}\tACGT\n" for k, t in enumerate(rows))
    p = s.transcribe_plan(None, sum(1 + k % 3 for k in range(400)), seed=9, text=ab)
    b = p.batch()
    try:
        recs = s.run(b, target="perfect", fastq=True, seed=9).records()
        assert len(recs) == p.molecules == 799
        want = [t for k, t in enumerate(rows) for _ in range(1 + k % 3)]
        n_minus = 0
        for m in range(0, 799, 3):
            head, seq = recs[m].decode().split("\n")[:2]
            spliced = "".join(ref[c][a:e] if st == "+" else _revcomp(ref[c][a:e]) for c, a, e, st in exons[want[m]])
            assert seq == spliced, (m, want[m])
            n_minus += exons[want[m]][0][3] == "-"
            assert "molecule_id=M" in head
        assert 50 < n_minus < 220 and max(len(exons[t]) for t in want) == 200
    finally:
        b.free()
        p.close()


def test_module_route_equals_chained_route(tmp_path):
    """`tksm transcribe -o x.mdf` then `tksm sequence -i x.mdf` against `tksm sequence --transcribe-*`: the same FASTQ byte for byte, perfect
    and Badread with q-scores, whatever the batch size, the contexts in flight and the device list; two GTFs (the first wins), two abundance
    tables with weights, a GTF contig the FASTA lacks, exons past the end of a contig and transcripts without exons on both routes"""
    rs = np.random.RandomState(5)
    ref = _genome()
    fa = tmp_path / "g.fa"
    _write_fasta(fa, ref)
    g1, n1 = _make_gtf(rs, 60, ["chrA", "chrB", "chrC", "chrNoFasta"], bare=2)
    g2, n2 = _make_gtf(rs, 20, ["chrC"], tag="T", counts=(3,))                          # the same ids T0..T19 again: ignored
    g2b, n2b = _make_gtf(rs, 10, ["chrB"], tag="U", counts=(1, 2, 5))
    at = 'gene_id "GP"; transcript_id "PAST"; gene_biotype "protein_coding";'                # exons across and past the end of chrC (7 000)
    g1 += f"chrC\ttest\ttranscript\t6801\t8100\t.\t-\t.\t{at}\n" + "".join(f"chrC\ttest\texon\t{a}\t{b}\t.\t-\t.\t{at}\n" for a, b in ((8001, 8100), (6901, 7400), (6801, 6850)))
    (tmp_path / "a.gtf").write_text(g1)
    (tmp_path / "b.gtf").write_text(g2 + g2b)
    n_ex = {**n2b, **n1}
    ab1, _ = _make_abundance(rs, 900, n_ex, big_row=(17, 300), cbs=("ACGT", "TTGCA"))
    ab1 += "PAST\t40\tACGT\n"
    ab2, _ = _make_abundance(rs, 500, n_ex, cbs=("GGCC",))
    (tmp_path / "1.tsv").write_text(ab1)
    (tmp_path / "2.tsv").write_text(ab2)
    gtfs, abs_, mc = f"{tmp_path / 'a.gtf'},{tmp_path / 'b.gtf'}", [tmp_path / "1.tsv", tmp_path / "2.tsv"], 4000
    mdf = tmp_path / "x.mdf"
    r = _cli("transcribe", "-g", gtfs, "-a", abs_[0], "-a", abs_[1], "-w", "3,1", "--molecule-count", mc, "-o", mdf, "-s", 21)
    assert r.returncode == 0, r.stderr
    text = open(mdf).read()
    plans = ts.tsb_spec(21, [g1, g2 + g2b], [ab1, ab2], mc, weights=(3.0, 1.0))
    assert text == "".join(p.mdf_text() for p in plans)
    n_mol = sum(p.molecules for p in plans)
    assert 3000 < n_mol < 5000 and "chrNoFasta\t" in text and "\tCB=GGCC;tid=U" in text and ";\n+" in text and "tid=PAST;\nchrC\t8000\t8100\t-" in text
    assert r.stderr.count("is not found in the input GTFs!") == sum(len(p.missing) for p in plans) > 50
    # the batch size of the module does not matter
    r = _cli("transcribe", "--gtf", tmp_path / "a.gtf", "--gtf", tmp_path / "b.gtf", "--abundance", f"{abs_[0]},{abs_[1]}", "--weights=0.75,0.25", "--molecule-count", mc,
             "-o", tmp_path / "y.mdf", "-s", 21, "--batch-molecules", 7, "--non-coding", "--verbosity", "ERROR")
    assert r.returncode == 0 and "is not found" not in r.stderr and open(tmp_path / "y.mdf").read() == text
    tsb = ["--transcribe-gtf", gtfs, "--transcribe-abundance", abs_[0], "--transcribe-abundance", abs_[1], "--transcribe-weights", "3,1",
           "--transcribe-molecule-count", mc]
    for mode in (["--perfect"], ["-o"]):
        via_text, chained = tmp_path / "a.fastq", tmp_path / "b.fastq"
        r = _cli("sequence", "-r", fa, "-i", mdf, *mode, via_text, "-s", 21)
        assert r.returncode == 0, r.stderr
        r = _cli("sequence", "-r", fa, *tsb, *mode, chained, "-s", 21, "--transcribe-batch-molecules", 400)
        assert r.returncode == 0, r.stderr
        a = open(via_text, "rb").read()
        assert a.count(b"\n") == 4 * n_mol and open(chained, "rb").read() == a, mode
        if mode == ["-o"]:
            quals = a.split(b"\n")[3::4]
            assert any(set(q) != {ord("K")} for q in quals[:50])             # q-scores were computed
        variants = [["--transcribe-batch-molecules", 100_000], ["--transcribe-batch-molecules", 97, "--in-flight", 1],
                    ["--devices", "0,0", "--transcribe-batch-molecules", 250, "--in-flight", 2]] if mode == ["--perfect"] else \
                   [["--devices", "0,0", "--transcribe-batch-molecules", 333]]
        for extra in variants:
            r = _cli("sequence", "-r", fa, *tsb, *mode, chained, "-s", 21, *extra)
            assert r.returncode == 0, r.stderr
            assert open(chained, "rb").read() == a, (mode, extra)
    r = _cli("sequence", "-r", fa, *tsb, "--perfect", tmp_path / "c.fastq.gz", "-s", 21, "--gzip", "device")
    assert r.returncode == 0, r.stderr
    r = _cli("sequence", "-r", fa, "-i", mdf, "--perfect", tmp_path / "d.fastq", "-s", 21)
    assert gzip.open(tmp_path / "c.fastq.gz", "rb").read() == open(tmp_path / "d.fastq", "rb").read()


def test_python_chain_on_the_device(world):
    """plan.batch -> polya -> scb -> tag -> run, against the same chain from the parsed compact text; scb reads CB from the comments the
    transcribe batch carries, and refuses a batch made without them"""
    from tksm_amd.sequence import TksmSeqError
    from tksm_amd import _lib as L
    s = world["s"]
    known = [t for t, e in world["n_ex"].items() if 0 < e <= 65]
    ab = "h\n" + "".join(f"{known[k % len(known)]}\t{1 + k % 4}\t{BARCODES[k % 3]}\n" for k in range(120))
    p = s.transcribe_plan(None, sum(1 + k % 4 for k in range(120)), seed=2, text=ab)

    def chain(b):
        steps = [b]
        try:
            steps.append(s.polya(steps[-1], normal=(30.0, 5.0), seed=2))
            steps.append(s.scb(steps[-1]))
            steps.append(s.tag(steps[-1], format5="NNNNNNNN", format3="ACGT", seed=2))
            return s.to_mdf_text(steps[-1]), s.run(steps[-1], target="badread", fastq=True, seed=2).records()
        finally:
            for x in steps:
                x.free()
    try:
        text_a, recs_a = chain(p.batch())
        text_b, recs_b = chain(s.batch_from_mdf(p.mdf_text()))
        assert text_a == text_b and recs_a == recs_b and len(recs_a) == p.molecules == 300
        assert sum(l.split("\t")[0] in BARCODES for l in text_a.split("\n")) == 300      # every molecule got its barcode segment
        assert "CB=" not in text_a and "tid=" in text_a
        b = p.batch(comments=False)
        try:
            with pytest.raises(TksmSeqError) as e:
                s.scb(b)
            assert e.value.code == L.EINVAL
        finally:
            b.free()
    finally:
        p.close()
