"""filter (Flt) and concat (Mrg) on the device (-m gpu): tksmseq_filter / tksmseq_concat against tests/filter_spec.py as MDF text,
molecule for molecule; `tksm filter` on files against the device call; the README's single-cell experiment as it is drawn -- head,
Flt / Flt --negate, the barcoded half through plA -> Tag -> SCB -> Tag, Mrg, PCR -> Flp -> Tag -> Seq -- device to device and through
`tksm ...` over files joined with `cat`."""
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ERR_MODEL, GOLDEN, QS_MODEL, ROOT

import core_modules_spec as cs
import filter_spec as fs
import mdf_ops_oracle as mo

pytestmark = pytest.mark.gpu

EXE = os.path.join(ROOT, "tksm_amd", "tksm")
TSB = os.path.join(GOLDEN, "transcribe")
LIT = "ACGTTGCA"                          # a literal segment whose text serves as a `locus` name
LIT_OTHER = "ACGTTGCC"                    # same length, last letter differs
COMMENTS = ["CB=ACGT;", "CB=.;", "CB=;", "", "CB=.,X;", "tid=T1;CB=TTGCA;", "z;"]
PROBE = (1000, 1100)                      # the one chr1 segment of molecule `probe`; the random segments start at 5000 or later


def _cli(*args, **kw):
    return subprocess.run([EXE, *[str(a) for a in args]], capture_output=True, text=True, timeout=600, **kw)


def _mdf(rs, n, probe=True):
    """n records: 1 - 5 segments on two contigs and both strands, substitutions on some, literal segments (LIT among them), one record
    in five with depth 3, the comments of COMMENTS in turn"""
    lines = []
    if probe:
        lines.append(f"+probe\t3\tCB=ACGT;\nchr1\t{PROBE[0]}\t{PROBE[1]}\t+\t5A,50C\nchr2\t7000\t7010\t-\t\n")
    for i in range(n):
        lines.append(f"+m{i}\t{3 if i % 5 == 2 else 1}\t{COMMENTS[i % len(COMMENTS)]}\n")
        for k in range(1 + int(rs.randint(0, 5))):
            if rs.rand() < 0.15:
                lit = (LIT, LIT_OTHER, "A" * int(rs.randint(1, 20)))[int(rs.randint(0, 3))]
                lines.append(f"{lit}\t0\t{len(lit)}\t{'+-'[int(rs.randint(0, 2))]}\t{'0C' if rs.rand() < 0.5 else ''}\n")
                continue
            ln, st = int(rs.randint(1, 400)), int(rs.randint(5000, 50_000))
            md = ",".join(f"{int(rs.randint(0, ln))}{'ACGT'[int(rs.randint(0, 4))]}" for _ in range(int(rs.randint(0, 3))))
            lines.append(f"chr{int(rs.randint(1, 3))}\t{st}\t{st + ln}\t{'+-'[int(rs.randint(0, 2))]}\t{md}\n")
    return "".join(lines)


@pytest.fixture(scope="module")
def gs():
    from tksm_amd.sequence import Sequencer
    rs = np.random.RandomState(21)
    ref = {f"chr{i + 1}": rs.choice(np.frombuffer(b"ACGT", np.uint8), 60_000).tobytes().decode() for i in range(2)}
    s = Sequencer(0)
    for k, v in ref.items():
        s.add_contig(k, v)
    yield s, ref
    s.close()


@pytest.fixture(scope="module")
def sample(gs):
    """one parsed batch of 300 records (423 molecules) and its specification's molecules: read by the tests, never changed"""
    s, _ = gs
    text = _mdf(np.random.RandomState(1), 300)
    b = s.batch_from_mdf(text)
    yield text, mo.stream_mdf(text, unroll=True), b
    b.free()


def _text(s, batch):
    try:
        return s.to_mdf_text(batch)
    finally:
        batch.free()


def _no_comments(text):
    return "".join((l.rsplit("\t", 1)[0] + "\t\n") if l.startswith("+") else l for l in text.splitlines(keepends=True))


def _check(s, b, mols, conditions, negate=False):
    """both sides against the specification, text for text; returns the ids of the true side"""
    want_t, want_f = fs.filter_spec(mols, conditions, negate)
    t, f = s.filter(b, conditions, negate=negate)
    assert (t.n_reads, f.n_reads) == (len(want_t), len(want_f)), (conditions, negate)
    assert _text(s, t) == mo.write_mdf(want_t), (conditions, negate)
    assert _text(s, f) == mo.write_mdf(want_f), (conditions, negate)
    return [m["id"] for m in want_t]


# ------------------------------------------------------------------------------------------------ each condition kind alone
def test_info_condition(gs, sample):
    s, _ = gs
    _, mols, b = sample
    true_ids = _check(s, b, mols, ["info CB"])
    # CB=ACGT; and tid=T1;CB=TTGCA; are true; CB=.; CB=; none, CB=.,X; and a bare key are false
    assert "probe_0" in true_ids and "m0" in true_ids and "m5" in true_ids
    assert not {"m1", "m2_0", "m3", "m4", "m6"} & set(true_ids)
    assert _check(s, b, mols, ["info z"]) == []
    assert "m5" in _check(s, b, mols, ["info tid"])
    _check(s, b, mols, ["info CB"], negate=True)
    # without comments no molecule has a key; NO_COMMENTS on the output still reads the input's
    t, f = s.filter(b, ["info CB"], comments=False)
    assert _text(s, t) == _no_comments(mo.write_mdf(fs.filter_spec(mols, ["info CB"])[0]))
    assert _text(s, f) == _no_comments(mo.write_mdf(fs.filter_spec(mols, ["info CB"])[1]))
    bare = s.batch_from_arrays(np.array([[0, 1], [1, 1]]), np.array([[0, 0, 10, 0], [1, 5, 9, 0]]), ids=np.array([[0, 1], [1, 1]]), id_pool=b"ab")
    t, f = s.filter(bare, ["info CB"])
    assert (t.n_reads, f.n_reads) == (0, 2) and _text(s, t) == "" and _text(s, f) == "+a\t1\t\nchr1\t0\t10\t+\t\n+b\t1\t\nchr2\t5\t9\t+\t\n"
    bare.free()


def test_every_size_operator_at_below_and_above_a_size(gs, sample):
    s, _ = gs
    _, mols, b = sample
    size = mo.mol_size(mols[7])
    assert size > 1 and sum(mo.mol_size(m) == size for m in mols) >= 1
    for op in ("<", "<=", ">", ">=", "==", "!="):
        for v in (size - 1, size, size + 1):
            ids = _check(s, b, mols, [f"size {op}{v}"])
            assert (mols[7]["id"] in ids) == {"<": size < v, "<=": size <= v, ">": size > v, ">=": size >= v, "==": size == v, "!=": size != v}[op]
    assert len(_check(s, b, mols, ["size >=0"])) == len(mols) and _check(s, b, mols, ["size <0"]) == []
    assert _check(s, b, mols, ["size >2147483647"]) == []


def test_locus_at_every_boundary_of_the_overlap_table(gs, sample):
    """the thirteen positions of a range against the probe's chr1 segment [1000, 1100) -- on chr1, and on chr2, where the probe has
    another segment far away; the probe lands where src/interval.h:38-58 puts it, the two shared-endpoint zeros included"""
    s, _ = gs
    _, mols, b = sample
    a, e = PROBE
    table = [(a - 50, a - 10, 0), (a - 50, a, 0), (a - 50, a + 40, 40), (a - 50, e, 0), (a - 50, e + 50, 100), (a, a + 40, 40), (a, e, 100),
             (a, e + 50, 0), (a + 10, e - 10, 80), (a + 40, e, 60), (a + 40, e + 50, 60), (e, e + 50, 0), (e + 10, e + 50, 0)]
    for lo, hi, want in table:
        assert fs.overlap(a, e, lo, hi) == want
        ids = _check(s, b, mols, [f"locus chr1:{lo}-{hi}"])
        assert ("probe_0" in ids) == ("probe_2" in ids) == (want > 0), (lo, hi)
        assert "probe_1" not in _check(s, b, mols, [f"locus chr2:{lo}-{hi}"])
    for pos, hit in ((a - 1, False), (a, True), (e - 1, True), (e, False)):
        assert ("probe_1" in _check(s, b, mols, [f"locus chr1:{pos}"])) == hit, pos
    assert "probe_0" in _check(s, b, mols, ["locus chr2:7009"]) and "probe_0" not in _check(s, b, mols, ["locus chr2:7010"])


def test_locus_by_name_contigs_and_literals(gs, sample):
    s, _ = gs
    text, mols, b = sample
    assert f"\n{LIT}\t" in text and f"\n{LIT_OTHER}\t" in text
    n1, n2 = len(_check(s, b, mols, ["locus chr1"])), len(_check(s, b, mols, ["locus chr2"]))
    assert 0 < n1 < len(mols) and 0 < n2 < len(mols)
    # a name that is no contig equals a literal segment's text: by length and bytes
    n_lit = len(_check(s, b, mols, [f"locus {LIT}"]))
    assert 0 < n_lit < len(mols) and n_lit == sum(any(sg["chr"] == LIT for sg in m["segments"]) for m in mols)
    assert len(_check(s, b, mols, [f"locus {LIT_OTHER}"])) > 0
    assert _check(s, b, mols, [f"locus {LIT[:-1]}"]) == [] and _check(s, b, mols, [f"locus {LIT}A"]) == [] and _check(s, b, mols, ["locus chr3"]) == []
    assert len(_check(s, b, mols, [f"locus {LIT}:0-3"])) == n_lit and _check(s, b, mols, [f"locus {LIT}:8-20"]) == []
    assert len(_check(s, b, mols, [f"locus {LIT}:7"])) == n_lit and _check(s, b, mols, [f"locus {LIT}:0-8"]) != []


# ------------------------------------------------------------------------------------------------ conjunctions, errors
def test_conjunctions_negate_and_no_false_side(gs, sample):
    s, _ = gs
    _, mols, b = sample
    for conds in (["info CB", "size >300"], ["locus chr1", "locus chr2"], ["size >=100", "size <600", "info CB"], [f"locus {LIT}", "size !=8", "locus chr2:5000-30000"]):
        for negate in (False, True):
            ids = _check(s, b, mols, conds, negate)
            assert 0 < len(ids) < len(mols), (conds, negate)
            t, f = s.filter(b, conds, negate=negate, want_false=False)
            assert f is None and _text(s, t) == mo.write_mdf(fs.filter_spec(mols, conds, negate)[0])
    # one string is one condition; no condition at all: everything is true
    t, f = s.filter(b, "info CB")
    assert _text(s, t) == mo.write_mdf(fs.filter_spec(mols, ["info CB"])[0])
    f.free()
    t, f = s.filter(b, [])
    assert (t.n_reads, f.n_reads) == (len(mols), 0)
    t.free(); f.free()


def test_invalid_conditions_are_einval(gs, sample):
    from tksm_amd import _lib as L
    from tksm_amd.sequence import TksmSeqError
    s, _ = gs
    _, _, b = sample
    for text in ("size", "info CB x", "bogus x", "size >", "size =5", "size >x", "size >-3", "size >99999999999", "locus chr1:-5", "locus chr1:5-b"):
        with pytest.raises(TksmSeqError) as e:
            s.filter(b, ["size >5", text])
        assert e.value.code == L.EINVAL and f"Invalid condition: {text}" in str(e.value), text
    with pytest.raises(TksmSeqError) as e:
        s.merge([])
    assert e.value.code == L.EINVAL


# ------------------------------------------------------------------------------------------------ molecule counts, empty sides
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 256, 257, 1000])
def test_molecule_counts_and_empty_sides(gs, n):
    """all-true, all-false and alternating sides at the block edges (128 lanes per block: 256 / 257) and below a wave (63 / 64 / 65);
    an empty side is a batch like any other: written as empty text, taken by polyA and by concat"""
    s, _ = gs
    text = "".join(f"+k{i}\t1\t{'CB=ACGT;' if i % 2 == 0 else 'x=1;'}\nchr{1 + i % 2}\t{100 + i}\t{150 + 2 * i}\t{'+-'[i % 2]}\t{'3G' if i % 3 == 0 else ''}\n" for i in range(n))
    mols = mo.stream_mdf(text, unroll=True)
    b = s.batch_from_mdf(text)
    assert b.n_reads == n
    assert len(_check(s, b, mols, ["size >=0"])) == n                     # all true
    assert _check(s, b, mols, ["size >100000"]) == []                     # all false
    assert len(_check(s, b, mols, ["info CB"])) == (n + 1) // 2           # alternating
    assert len(_check(s, b, mols, ["info CB"], negate=True)) == n // 2
    t, f = s.filter(b, ["size >100000"])
    assert t.n_reads == 0 and s.to_mdf_text(t) == ""
    pa = s.polya(t, normal=(15.0, 7.5), seed=3)
    assert pa.n_reads == 0 and _text(s, pa) == ""
    whole = mo.write_mdf(mols)
    assert _text(s, s.merge([t, f])) == whole and _text(s, s.merge([f, t, t])) == whole and _text(s, s.merge([t])) == ""
    assert _text(s, s.merge([f])) == whole                                # one input: a copy
    t2, f2 = s.filter(t, ["info CB"])                                     # an empty batch is an input like any other
    assert (t2.n_reads, f2.n_reads) == (0, 0)
    for x in (t, f, t2, f2, b):
        x.free()


# ------------------------------------------------------------------------------------------------ partition, concat
def test_partition_then_concat_holds_the_input(gs, sample):
    s, _ = gs
    _, mols, b = sample
    t, f = s.filter(b, ["info CB", "size >150"])
    want_t, want_f = fs.filter_spec(mols, ["info CB", "size >150"])
    joined = _text(s, s.merge([t, f]))
    assert joined == mo.write_mdf(fs.concat_spec([want_t, want_f]))      # each side in input order
    records = lambda text: sorted(re.split(r"(?m)^(?=\+)", text))
    assert records(joined) == records(mo.write_mdf(mols)) and len(records(joined)) == len(mols) + 1      # the input's molecules as a multiset
    t.free(); f.free()


def test_concat_of_three_differently_edited_batches(gs, sample):
    """polyA (shared literals appended), tag with drawn literals (one per molecule) and an untouched batch: the text equals concat_spec,
    and sequencing the concatenation --perfect gives the three batches' own FASTA one after the other -- which a wrong literal,
    literal-pool or substitution re-base would break"""
    s, _ = gs
    _, mols, b = sample
    t, f = s.filter(b, ["size >200"])
    mt, mf = fs.filter_spec(mols, ["size >200"])
    b1 = s.polya(t, normal=(15.0, 7.5), seed=17)
    b2 = s.tag(f, format5="NNNNNNNN", format3="ACGTN", seed=9)
    # (untouched: the sample written with depth 1 and parsed again -- Seq names the copies of a depth > 1 record by the record, the
    # concatenation by their unrolled ids, so only ids that are already unrolled can be compared record for record)
    b3 = s.batch_from_mdf(mo.write_mdf(mols))
    spec = [cs.polya_spec(mt, 17, "normal", 15.0, 7.5, 0, 5000), cs.tag_spec(mf, 9, "NNNNNNNN", "ACGTN"), mols]
    for order in ((0, 1, 2), (2, 1, 0), (1, 1, 0)):
        parts = [(b1, b2, b3)[k] for k in order]
        cat = s.merge(parts)
        assert s.to_mdf_text(cat) == mo.write_mdf(fs.concat_spec([spec[k] for k in order])), order
        got = b"".join(s.run(cat, target="perfect", fastq=False, seed=5).records())
        own, first = [], 0
        for p in parts:
            own.append(b"".join(s.run(p, target="perfect", fastq=False, seed=5, first_read_index=first).records()))
            first += p.n_reads
        assert got == b"".join(own) and got.count(b">") == cat.n_reads, order
        cat.free()
    cat = s.merge([b1, b2], comments=False)
    assert _text(s, cat) == _no_comments(mo.write_mdf(fs.concat_spec(spec[:2])))
    # an input without comments contributes empty ones
    bare = s.batch_from_arrays(np.array([[0, 1]]), np.array([[0, 0, 10, 0]]), ids=np.array([[0, 1]]), id_pool=b"q")
    assert _text(s, s.merge([bare, b2, bare])) == "+q\t1\t\nchr1\t0\t10\t+\t\n" + mo.write_mdf(spec[1]) + "+q\t1\t\nchr1\t0\t10\t+\t\n"
    for x in (bare, b1, b2, b3, t, f):
        x.free()


def test_filtering_the_halves_equals_filtering_the_whole(gs, sample):
    s, _ = gs
    text, mols, _ = sample
    cut = text.index("\n+", len(text) // 2) + 1
    conds = ["info CB", "locus chr1"]
    halves = [s.batch_from_mdf(text[:cut]), s.batch_from_mdf(text[cut:])]
    sides = [s.filter(h, conds) for h in halves]
    want_t, want_f = fs.filter_spec(mols, conds)
    assert _text(s, s.merge([sides[0][0], sides[1][0]])) == mo.write_mdf(want_t)
    assert _text(s, s.merge([sides[0][1], sides[1][1]])) == mo.write_mdf(want_f)
    for x in halves + [y for p in sides for y in p]:
        x.free()


# ------------------------------------------------------------------------------------------------ the module on files
def test_tksm_filter_on_files_equals_the_device_call(gs, sample, tmp_path):
    s, _ = gs
    text, mols, b = sample
    src = tmp_path / "in.mdf"
    src.write_text(text)
    for k, (conds, negate) in enumerate(((["info CB"], False), (["size >=200", f"locus {LIT}"], True), (["locus chr1:5000-20000", "info CB"], False))):
        t, f = s.filter(b, conds, negate=negate)
        dev_t, dev_f = _text(s, t), _text(s, f)
        ft, ff = tmp_path / f"t{k}.mdf", tmp_path / f"f{k}.mdf"
        r = _cli("filter", "-i", src, "-t", ft, "-f", ff, "-c", ",".join(conds), *(["--negate"] if negate else []))
        assert r.returncode == 0, r.stderr[-600:]
        assert ft.read_text() == dev_t and ff.read_text() == dev_f, conds
        # small pieces over two device entries, the conditions one -c each, no false output
        r = _cli("filter", "-i", src, "--true-output", tmp_path / "alt.mdf", *[x for c in conds for x in ("-c", c)], *(["--negate=true"] if negate else []),
                 "--batch-bytes", "2000", "--devices", "0,0")
        assert r.returncode == 0 and (tmp_path / "alt.mdf").read_text() == dev_t, conds
    # an empty input makes two empty outputs
    (tmp_path / "empty.mdf").write_text("")
    r = _cli("filter", "-i", tmp_path / "empty.mdf", "-t", tmp_path / "et.mdf", "-f", tmp_path / "ef.mdf", "-c", "info CB")
    assert r.returncode == 0 and (tmp_path / "et.mdf").read_text() == "" and (tmp_path / "ef.mdf").read_text() == ""


def test_the_references_example_partitions_the_transcribe_fixture(tmp_path):
    """`-c "info CB"` with and without --negate on tests/golden/transcribe/expected_exact.mdf: the `.` and the empty barcode land on
    the false side; the two calls mirror each other"""
    src = os.path.join(TSB, "expected_exact.mdf")
    mols = mo.stream_mdf(open(src).read(), unroll=True)
    want_t, want_f = fs.filter_spec(mols, ["info CB"])
    t, f, nt, nf = (tmp_path / x for x in ("t.mdf", "f.mdf", "nt.mdf", "nf.mdf"))
    r = _cli("filter", "-i", src, "-t", t, "-f", f, "-c", "info CB")
    assert r.returncode == 0, r.stderr[-600:]
    r = _cli("filter", "-i", src, "-t", nt, "-f", nf, "-c", "info CB", "--negate")
    assert r.returncode == 0, r.stderr[-600:]
    assert t.read_text() == nf.read_text() == mo.write_mdf(want_t) and f.read_text() == nt.read_text() == mo.write_mdf(want_f)
    false_ids = [m["id"] for m in want_f]
    assert false_ids == ["M4_0", "M4_1", "M5"] and "tid=T5;" in f.read_text() and "tid=T6;" in f.read_text()      # `CB=.` (T5) and the empty barcode (T6)
    assert len(want_t) == 46 and "+M6_3\t1\tCB=GGGGCCCCAA;tid=T7;\n+M7" in t.read_text()                          # a molecule without segments moves like any other


# ------------------------------------------------------------------------------------------------ the README experiment
def test_readme_single_cell_experiment_device_and_files(tmp_path):
    """TKSM_single_cell as the README draws it.  Head: Tsb -> Trc.  Flt `info CB` / Flt `info CB --negate` split it; the barcoded half
    goes through plA -> Tag -> SCB -> Tag; Mrg joins the halves; PCR -> Flp -> Tag -> Seq.  Device to device, and the same steps
    through `tksm ...` over files joined with `cat`: the same FASTQ byte for byte (perfect, and Badread with q-scores)."""
    from tksm_amd.sequence import Sequencer
    rs = np.random.RandomState(8)
    ref = {c: rs.choice(np.frombuffer(b"ACGT", np.uint8), n).tobytes().decode() for c, n in (("c1", 5000), ("c2", 3200), ("c3", 3200))}
    fa = tmp_path / "ref.fa"
    fa.write_text("".join(f">{k}\n{v}\n" for k, v in ref.items()))
    gtf, ab = os.path.join(TSB, "ann.gtf"), os.path.join(TSB, "abund_exact.tsv")
    seed, a5, a3, umi = 13, "AATGTACTTCGTTCAGTTACGTATTGCT", "GCAATACGTAACTGAACGAAGT", "AGATCGGAAGAGCGTCGTGTAG"
    s = Sequencer(0)
    made = []                                                             # every batch, freed before the context goes

    def keep(b):
        made.append(b)
        return b
    try:
        for k, v in ref.items():
            s.add_contig(k, v)
        s.add_gtf(gtf)
        s.set_identity(84.0, 99.0, 5.5); s.load_error_model(ERR_MODEL); s.load_qscore_model(QS_MODEL)
        plan = s.transcribe_plan(ab, 60, seed=seed)
        head = keep(s.truncate(keep(plan.batch()), normal=(250.0, 80.0), seed=seed))
        t, f = map(keep, s.filter(head, ["info CB"]))
        nt = keep(s.filter(head, ["info CB"], negate=True, want_false=False)[0])
        assert (t.n_reads, f.n_reads) == (46, 3) and s.to_mdf_text(nt) == s.to_mdf_text(f) != ""
        bar = keep(s.polya(t, normal=(15.0, 7.5), seed=seed))
        bar = keep(s.tag(bar, format3="10", seed=seed))
        bar = keep(s.scb(bar))
        bar = keep(s.tag(bar, format3=umi, seed=seed))
        merged = keep(s.merge([bar, nt]))
        dev_merged = s.to_mdf_text(merged)
        last = keep(s.pcr(merged, 5, 300, preset="Taq-setting1", seed=seed))
        last = keep(s.flip(last, 0.5, seed=seed))
        last = keep(s.tag(last, format5=a5, format3=a3, seed=seed))
        dev_last, n_last = s.to_mdf_text(last), last.n_reads
        dev_perfect = b"".join(s.run(last, target="perfect", fastq=True, seed=seed).records())
        dev_bad = b"".join(s.run(last, target="badread", fastq=True, compute_qual=True, seed=seed).records())
        plan.close()
    finally:
        for b in made:
            b.free()
        s.close()
    assert dev_perfect.count(b"\n") == 4 * n_last and n_last > 100
    # the same through files
    env = dict(os.environ, TKSM_MODELS=os.path.join(ROOT, "tksm_amd", "models"))
    p = lambda name: tmp_path / name

    def run(*args):
        r = _cli(*args, env=env)
        assert r.returncode == 0, (args, r.stderr[-600:])
    run("transcribe", "-g", gtf, "-a", ab, "--molecule-count", 60, "-o", p("tsb.mdf"), "-s", seed)
    run("truncate", "-i", p("tsb.mdf"), "-o", p("head.mdf"), "--normal", "250,80", "-s", seed)
    run("filter", "-i", p("head.mdf"), "-t", p("cb.mdf"), "-c", "info CB")
    run("filter", "-i", p("head.mdf"), "-t", p("nocb.mdf"), "-c", "info CB", "--negate")
    run("polyA", "-i", p("cb.mdf"), "-o", p("pla.mdf"), "--normal=15,7.5", "-s", seed)
    run("tag", "-i", p("pla.mdf"), "-o", p("tag1.mdf"), "--format3", "10", "-s", seed)
    run("scb", "-i", p("tag1.mdf"), "-o", p("scb.mdf"))
    run("tag", "-i", p("scb.mdf"), "-o", p("tag2.mdf"), "--format3", umi, "-s", seed)
    with open(p("merged.mdf"), "wb") as out:                              # Mrg outside piped mode
        assert subprocess.run(["cat", str(p("tag2.mdf")), str(p("nocb.mdf"))], stdout=out).returncode == 0
    assert p("merged.mdf").read_text() == dev_merged
    run("pcr", "-i", p("merged.mdf"), "-o", p("pcr.mdf"), "--cycles", 5, "--molecule-count", 300, "-x", "Taq-setting1", "-s", seed)
    run("flip", "-i", p("pcr.mdf"), "-o", p("flip.mdf"), "-p", "0.5", "-s", seed)
    run("tag", "-i", p("flip.mdf"), "-o", p("last.mdf"), "--format5", a5, "--format3", a3, "-s", seed)
    assert p("last.mdf").read_text() == dev_last
    run("sequence", "-i", p("last.mdf"), "-r", fa, "--perfect", p("p.fastq"), "-s", seed)
    run("sequence", "-i", p("last.mdf"), "-r", fa, "-o", p("b.fastq"), "-s", seed, "--badread-error-model", ERR_MODEL, "--badread-qscore-model", QS_MODEL,
        "--badread-identity", "84,99,5.5")
    assert p("p.fastq").read_bytes() == dev_perfect
    assert p("b.fastq").read_bytes() == dev_bad
