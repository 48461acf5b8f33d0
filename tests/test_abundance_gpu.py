"""abundance on the device (-m gpu): `tksm abundance`, Sequencer.abundance and the C-ABI accessors against the files the reference's own
script wrote (tests/golden/abundance/) and against the numpy specification (tests/abundance_spec.py).

The gate of an abundance: relative 1e-9.  Derived, not measured: a round is three sums of non-negative terms (per transcript, the total,
per read), each within n 2^-53 of the exact sum for n terms, n < 1e5 here: 10 rounds x 3 sums x 1e5 x 1.1e-16 = 3.3e-10.  Whether the EM
map amplifies a rounding difference is not proven; the worst relative difference seen is printed by every test that gates on it.

The second half of the file stands at the thresholds of the reduction chain (chunk, block of segments, the looping total, the sorts' key
widths, the (transcript, cell) segments), and compares the device with abundance_spec.ordered_run -- the documented order of addition
-- byte for byte."""
import gzip
import json
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

import abundance_spec as A

pytestmark = pytest.mark.gpu
AB = os.path.join(GOLDEN, "abundance")
PAF = os.path.join(AB, "reads.paf")
LR = os.path.join(AB, "lr_matches.tsv")
EXE = os.path.join(ROOT, "tksm_amd", "tksm")
RUNS = {"default": ([], {}), "em0": (["-em", "0"], {"em_iterations": 0}), "em1": (["--em-iterations", "1"], {"em_iterations": 1}), "lr_br": (["-m", LR], {"lr_br": LR})}
GATE = 1e-9


@pytest.fixture(scope="module")
def S():
    from tksm_amd.sequence import Sequencer
    s = Sequencer(0)
    yield s
    s.close()


def _module(*args):
    return subprocess.run([EXE, "abundance", *[str(a) for a in args]], capture_output=True, text=True)


def _expected(name):
    return open(os.path.join(AB, f"expected_{name}.tsv")).read()


def _text(res):
    """the writer's text from the arrays Sequencer.abundance returns"""
    return "target_id\ttpm\tcell\n" + "".join(f"{n}\t{t:.3f}\t{c}\n" for n, t, c in zip(res["names"], res["tpm"], res["cells"]))


def gate(got, want, what):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape and np.isfinite(got).all(), what
    pos = want > 0
    rel = (np.abs(got[pos] - want[pos]) / want[pos]).max() if pos.any() else 0.0
    print(f"{what}: worst relative difference {rel:.3g} over {int(pos.sum())} values")
    assert rel <= GATE, what
    assert (got[~pos] == 0).all(), what


@pytest.mark.parametrize("name", list(RUNS))
def test_goldens_through_the_module(tmp_path, name):
    """`tksm abundance` reproduces the reference-written table byte for byte, plain and gzipped, with the reference's stdout lines"""
    flags, _ = RUNS[name]
    out, gz = tmp_path / "a.tsv", tmp_path / "a.tsv.gz"
    r = _module("-p", PAF, "-o", out, *flags)
    assert r.returncode == 0, r.stderr
    assert open(out).read() == _expected(name)
    lines = r.stdout.splitlines()
    assert lines[-1] == "Parsed alignments for 540 reads" and "Parsing PAF file..." in lines and "Running EM..." in lines
    assert ("Parsing LR barcode matches TSV..." in lines) == (name == "lr_br")
    r = _module("--paf", PAF, "--output", gz, *flags)
    assert r.returncode == 0, r.stderr
    assert open(gz, "rb").read(2) == b"\x1f\x8b" and gzip.open(gz, "rt").read() == _expected(name)
    assert not os.path.exists(str(out) + ".tmp") and not os.path.exists(str(gz) + ".tmp")


@pytest.mark.parametrize("name", list(RUNS))
def test_goldens_through_python_and_the_accessors(S, tmp_path, name):
    """Sequencer.abundance(out=...) writes the same bytes, and the rows the C-ABI accessors give print to the same text.  The abundance
    vector after 10 rounds against the reference's own: worst relative difference seen on the MI355X 1.21e-15 (gate 1e-9);
    over all tests of this file that gate on the specification, 8.92e-15 (the tpm of the 5 000-hit (transcript, cell) segment's input;
    4.39e-15 before the tests at the thresholds of the reduction chain)."""
    _, kw = RUNS[name]
    out = tmp_path / "a.tsv.gz"
    res = S.abundance(PAF, out=out, **kw)
    assert gzip.open(out, "rt").read() == _expected(name)
    assert _text(res) == _expected(name)
    assert res["surviving_reads"] == 540 and res["device_ms"] > 0
    if kw.get("em_iterations", 10) == 10:
        ref = json.load(open(os.path.join(AB, "expected_abundance.json")))
        want = np.array([float(ref["abundance"].get(t, "0.0")) for t in res["transcripts"]])
        gate(res["abundance"], want, f"{name}: abundance after 10 rounds vs the reference")
    spec = A.run(PAF, **kw)
    assert list(res["transcripts"]) == spec["transcripts"]
    gate(res["abundance"], spec["abundance"], f"{name}: abundance vs the specification")


# ---- synthetic inputs -----------------------------------------------------------------------------------------------------------------
def paf_text(reads):
    """reads: [(name, query length, [(transcript, target_start, matches, block length), ...])]"""
    return "".join(f"{rid}\t{ql}\t0\t{b}\t+\t{t}\t9000\t{ts}\t{ts + b}\t{m}\t{b}\t60\ttp:A:P\n" for rid, ql, recs in reads for t, ts, m, b in recs)


def random_reads(rs, n_reads, n_t, max_recs=5, one_record=False):
    reads = []
    for i in range(n_reads):
        ql = int(rs.randint(500, 3000))
        k = 1 if one_record else int(rs.randint(1, max_recs + 1))
        poor = rs.rand() < 0.1
        b = int(ql * (rs.uniform(0.2, 0.49) if poor else rs.uniform(0.6, 1.0)))
        best = int(b * rs.uniform(0.8, 0.98))
        t0 = int(rs.randint(0, n_t))
        reads.append((f"r{i}", ql, [(f"t{(t0 + 3 * j) % n_t}", int(rs.randint(0, 40)), best if j == 0 else int(best * rs.uniform(0.9, 1.0)), b - j) for j in range(k)]))
    return reads


def check_against_spec(S, tmp_path, reads, what, **kw):
    paf = tmp_path / "in.paf"
    paf.write_text(reads if isinstance(reads, str) else paf_text(reads))
    res = S.abundance(paf, keep_hits=True, **kw)
    spec = A.run(paf, **kw)
    assert list(res["transcripts"]) == spec["transcripts"] and list(res["reads"]) == spec["reads"]
    assert list(res["kept"]) == spec["kept"] and res["surviving_reads"] == len(spec["surviving"])
    assert [res["reads"][i] for i in res["surviving"]] == spec["surviving"]
    off, tid = res["hit_offsets"], res["hit_transcripts"]
    for k, rid in enumerate(spec["surviving"]):
        assert list(tid[off[k]:off[k + 1]]) == [t for t, _ in spec["hits"][rid]], rid
    if len(spec["surviving"]):
        gate(res["hit_weights"], [w for rid in spec["surviving"] for _, w in spec["hits"][rid]], f"{what}: final weights")
    gate(res["abundance"], spec["abundance"], f"{what}: abundance")
    assert list(zip(res["names"], res["cells"])) == [(n, c) for n, c, _ in spec["rows"]], what
    gate(res["tpm"], [t for _, _, t in spec["rows"]], f"{what}: tpm")
    return res, spec


@pytest.mark.parametrize("n_reads", [1, 63, 64, 65, 257])
def test_read_counts_around_the_wave_and_the_block(S, tmp_path, n_reads):
    check_against_spec(S, tmp_path, random_reads(np.random.RandomState(n_reads), n_reads, 23), f"{n_reads} reads")


def test_every_read_with_one_record_and_one_read_with_300(S, tmp_path):
    check_against_spec(S, tmp_path, random_reads(np.random.RandomState(7), 500, 40, one_record=True), "one record per read")
    rs = np.random.RandomState(8)
    reads = random_reads(rs, 200, 60)
    reads.insert(100, ("long", 2000, [(f"t{j % 90}", int(rs.randint(0, 20)), 1500 - int(rs.randint(0, 120)), 1800) for j in range(300)]))
    res, spec = check_against_spec(S, tmp_path, reads, "a read with 300 records")
    assert len(spec["hits"]["long"]) > 100


def _heavy(n_big, n_second, n_single):
    """n_big reads hit transcript `big` (n_second of them also a transcript of their own); n_single reads hit one transcript each"""
    reads = []
    for i in range(n_big):
        recs = [("big", 0, 900, 950)]
        if i % (n_big // n_second) == 0 and i // (n_big // n_second) < n_second:
            recs.insert(i % 2, (f"s{i}", 3, 880 + i % 20, 950))
        reads.append((f"b{i}", 1000, recs))
    for i in range(n_single):
        reads.insert(3 * i, (f"u{i}", 1000, [(f"u{i}", 0, 700, 800)]))
    return reads


def test_a_transcript_of_five_chunks_next_to_transcripts_with_one_hit(S, tmp_path):
    """5 000 of 6 000 hits on one transcript (five chunks of the M-step), 1 000 transcripts with one hit each"""
    from tksm_amd import _lib
    assert _lib.ABUND_CHUNK == 1024
    res, spec = check_against_spec(S, tmp_path, _heavy(5000, 500, 500), "5000 of 6000 hits on one transcript")
    assert len(res["hit_transcripts"]) == 6000 and (res["hit_transcripts"] == spec["transcripts"].index("big")).sum() == 5000


@pytest.mark.parametrize("n_big", [1024, 1025])
def test_chunk_boundary(S, tmp_path, n_big):
    """exactly one chunk, and one chunk plus one hit"""
    res, spec = check_against_spec(S, tmp_path, _heavy(n_big, 64, 10), f"{n_big} hits on one transcript")
    assert (res["hit_transcripts"] == spec["transcripts"].index("big")).sum() == n_big


def _interleave(rs, lines):
    """the lines in another interleaving: the first line of every read and the first mention of every transcript keep their places
    relative to each other, every read's lines their order; the other lines are held back by random amounts"""
    seen_r, seen_t, out, held = set(), set(), [], []
    for ln in lines:
        f = ln.split("\t")
        anchor = f[0] not in seen_r or f[5] not in seen_t
        seen_r.add(f[0]); seen_t.add(f[5])
        if not anchor and rs.rand() < 0.5:
            held.append(ln)
            continue
        mine = [h for h in held if h.split("\t")[0] == f[0]]          # a read's lines stay in order: its held lines go first
        held = [h for h in held if h.split("\t")[0] != f[0]]
        out += mine + [ln]
        while held and rs.rand() < 0.3:
            k = int(rs.randint(0, len(held)))
            first_of_read = next(i for i, h in enumerate(held) if h.split("\t")[0] == held[k].split("\t")[0])
            out.append(held.pop(first_of_read))
    return out + held


def test_determinism_across_runs_clones_and_interleavings(S, tmp_path):
    rs = np.random.RandomState(11)
    lines = paf_text(random_reads(rs, 3000, 80)).splitlines(keepends=True)
    paf = tmp_path / "a.paf"
    paf.write_text("".join(lines))
    a = S.abundance(paf)
    b = S.abundance(paf)
    assert a["abundance"].tobytes() == b["abundance"].tobytes() and a["tpm"].tobytes() == b["tpm"].tobytes()
    c = S.clone()
    try:
        d = c.abundance(paf)
    finally:
        c.close()
    assert d["abundance"].tobytes() == a["abundance"].tobytes() and list(d["names"]) == list(a["names"])
    mixed = _interleave(rs, lines)
    assert mixed != lines and sorted(mixed) == sorted(lines)
    other = tmp_path / "b.paf"
    other.write_text("".join(mixed))
    (ta, ra), (tb, rb) = A.parse_paf(other), A.parse_paf(paf)
    assert ta == tb and list(ra.items()) == list(rb.items())                  # the constraint: same reads, transcripts and records in the same orders
    e = S.abundance(other)
    assert e["abundance"].tobytes() == a["abundance"].tobytes() and e["tpm"].tobytes() == a["tpm"].tobytes() and list(e["names"]) == list(a["names"])


EDGES = {
    "ratio_95_96": [("r", 1000, [("a", 0, 100, 900), ("b", 0, 95, 900), ("c", 0, 96, 900)])],
    "ratio_19_20": [("r", 1000, [("a", 0, 20, 900), ("b", 0, 19, 900)])],
    "start_19_is_full_length": [("r", 1000, [("a", 19, 800, 900), ("b", 20, 799, 900), ("c", 5, 790, 900)])],
    "start_20_is_not": [("r", 1000, [("a", 20, 800, 900), ("b", 19, 799, 900), ("c", 300, 790, 900)])],
    "half_exactly_stays": [("r", 1000, [("a", 0, 480, 500)])],
    "half_under_is_dropped": [("r", 1001, [("a", 0, 480, 500)]), ("q", 1000, [("a", 0, 900, 950)])],
    "later_full_length_tie_wins": [("r", 1000, [("a", 50, 900, 950), ("b", 5, 900, 600), ("c", 60, 900, 950)])],
    "tie_takes_its_block_length": [("r", 1000, [("a", 50, 900, 950), ("b", 5, 900, 400)]), ("q", 1000, [("b", 0, 900, 950)])],
    "earlier_full_length_tie_stays": [("r", 1000, [("a", 5, 900, 950), ("b", 50, 900, 600)])],
    "two_hits_on_one_transcript": [("r", 1000, [("a", 0, 900, 950), ("a", 3, 890, 940), ("b", 0, 700, 800)]), ("q", 1000, [("b", 0, 900, 950)])],
    "first_record_gives_the_length": [("r", 1000, [("a", 0, 900, 950)]), ("q", 1000, [("b", 0, 900, 950)]), ("r", 5000, [("c", 0, 899, 950)])],
    "no_full_length_zero_matches_is_dropped": [("r", 1000, [("a", 50, 0, 950)]), ("q", 1000, [("b", 0, 900, 950)])],
    "every_read_dropped": [("r", 1000, [("a", 0, 100, 100)])],
}


@pytest.mark.parametrize("name", list(EDGES))
def test_planted_edge_reads_one_by_one(S, tmp_path, name):
    res, spec = check_against_spec(S, tmp_path, EDGES[name], name)
    want = {"ratio_95_96": ["a", "c"], "ratio_19_20": ["a"], "start_19_is_full_length": ["a", "c"], "start_20_is_not": ["a", "c"], "half_exactly_stays": ["a"],
            "half_under_is_dropped": None, "later_full_length_tie_wins": ["b"], "tie_takes_its_block_length": None, "earlier_full_length_tie_stays": ["a"],
            "two_hits_on_one_transcript": ["a", "a"], "first_record_gives_the_length": ["a", "c"], "no_full_length_zero_matches_is_dropped": None,
            "every_read_dropped": None}[name]
    assert bool(res["kept"][0]) == (want is not None)
    if want is not None:
        assert [res["transcripts"][t] for t in res["hit_transcripts"][res["hit_offsets"][0]:res["hit_offsets"][1]]] == want
    if name == "every_read_dropped":
        assert len(res["names"]) == 0 and res["surviving_reads"] == 0


def test_em_zero_leaves_the_uniform_split(S, tmp_path):
    res, spec = check_against_spec(S, tmp_path, random_reads(np.random.RandomState(3), 300, 20), "-em 0", em_iterations=0)
    assert all(w == 1.0 / n for k in range(len(res["surviving"])) for n in [res["hit_offsets"][k + 1] - res["hit_offsets"][k]]
               for w in res["hit_weights"][res["hit_offsets"][k]:res["hit_offsets"][k + 1]])


REFUSALS = {
    "zero_length_first_record": ("good\t100\t0\t90\t+\tt\t900\t0\t90\t90\t90\t60\nnought\t0\t0\t0\t+\tt\t900\t0\t90\t90\t90\t60\n", "nought"),
    "zero_matches_behind_the_gate": ("good\t100\t0\t90\t+\tt\t900\t0\t90\t90\t90\t60\nempty\t100\t0\t90\t+\tt\t900\t5\t95\t0\t90\t60\n", "empty"),
    "ten_columns": ("good\t100\t0\t90\t+\tt\t900\t0\t90\t90\t90\t60\nshort\t100\t0\t90\t+\tt\t900\t0\t90\t90\n", "PAF line 2"),
    "non_integer_column": ("good\t100\t0\t90\t+\tt\t900\t0\t90\t90\t90\t60\nbad\t100\t0\t90\t+\tt\t900\t0\t90\tninety\t90\t60\n", "PAF line 2"),
    "non_integer_column_3": ("good\t100\t0\t90\t+\tt\t900\t0\t90\t90\t90\t60\nbad\t100\t0\t90\t+\tt\t900\t0x\t90\t90\t90\t60\n", "PAF line 2"),
}


@pytest.mark.parametrize("name", list(REFUSALS))
def test_refusals(S, tmp_path, name):
    from tksm_amd import _lib as L
    from tksm_amd.sequence import TksmSeqError
    text, needle = REFUSALS[name]
    paf, out = tmp_path / "in.paf", tmp_path / "out.tsv"
    paf.write_text(text)
    with pytest.raises(TksmSeqError) as e:
        S.abundance(paf, out=out)
    assert e.value.code == L.EINVAL and needle in str(e.value)
    assert not out.exists()
    r = _module("-p", paf, "-o", out)
    assert r.returncode == 1 and needle in r.stderr
    assert not out.exists() and not os.path.exists(str(out) + ".tmp")


def test_more_refusals_and_an_empty_input(S, tmp_path):
    from tksm_amd import _lib as L
    from tksm_amd.sequence import TksmSeqError

    def code(**kw):
        with pytest.raises(TksmSeqError) as e:
            S.abundance(PAF, **kw)
        return e.value.code
    assert code(cb_count=4, lr_br=LR) == L.EINVAL and code(cb_count=4, cb_pattern="NNQ") == L.EINVAL and code(cb_count=4, cb_dropout=1.5) == L.EINVAL
    assert code(cb_count=4, cb_lognorm_params=(10.0, 0.0)) == L.EINVAL and code(cb_count=4, cb_pattern="") == L.EINVAL
    assert code(cb_count=1 << 31) == L.ELIMIT
    wl = tmp_path / "wl.txt"
    wl.write_text("AAAA\nCCCC\n")
    assert code(cb_count=3, cb_txt=wl) == L.EINVAL and code(cb_count=3, cb_txt=tmp_path / "none.txt") == L.EIO
    assert code(lr_br=tmp_path / "none.tsv") == L.EIO
    four = tmp_path / "four.tsv"
    four.write_text("r\t0\t1\tBC\n")
    assert code(lr_br=four) == L.EINVAL
    with pytest.raises(TksmSeqError) as e:
        S.abundance(tmp_path / "missing.paf")
    assert e.value.code == L.EIO
    empty, out = tmp_path / "empty.paf", tmp_path / "empty.tsv"
    empty.write_text("")
    res = S.abundance(empty, out=out)
    assert open(out).read() == "target_id\ttpm\tcell\n" and res["surviving_reads"] == 0 and len(res["abundance"]) == 0
    target = tmp_path / "no" / "such" / "dir" / "a.tsv"
    r = _module("-p", PAF, "-o", target)
    assert r.returncode == 1 and "cannot write" in r.stderr and not os.path.exists(os.path.dirname(str(target)))


@pytest.fixture(scope="module")
def cb_paf(tmp_path_factory):
    """20 000 reads on 30 transcripts (a tenth dropped), for the cell draws"""
    p = tmp_path_factory.mktemp("cb") / "cb.paf"
    p.write_text(paf_text(random_reads(np.random.RandomState(21), 20000, 30, max_recs=3)))
    return p


def test_cb_count_cells_equal_the_specifications_draws(S, cb_paf, tmp_path):
    """the same Philox streams: the cell of every surviving read, the rows and (far from rounding boundaries) the table's text; the share
    of reads per cell against the weights by chi-square (p > 1e-3, the level of the project's other distribution tests)"""
    from scipy.stats import chisquare
    kw = dict(cb_count=8, seed=5, cb_lognorm_params=(10.0, 1.0), cb_dropout=0.2)
    out = tmp_path / "cb.tsv"
    res = S.abundance(cb_paf, out=out, keep_hits=True, **kw)
    spec = A.run(cb_paf, **kw)
    assert list(res["read_cells"]) == spec["read_cells"] and len(spec["read_cells"]) > 17000
    assert list(zip(res["names"], res["cells"])) == [(n, c) for n, c, _ in spec["rows"]]
    gate(res["tpm"], [t for _, _, t in spec["rows"]], "--cb-count 8: tpm")
    far = all(abs((t * 1000.0) % 1.0 - 0.5) > 1e-4 for _, _, t in spec["rows"])
    assert not far or open(out).read() == spec["tsv"]
    assert set(res["cells"]) <= set(spec["barcodes"]) and "." in set(res["cells"])
    counts = np.array([sum(1 for c in res["read_cells"] if c == b) for b in spec["barcodes"]])
    assert len(set(spec["barcodes"])) == 9 and counts.sum() == len(res["read_cells"])
    p = chisquare(counts, counts.sum() * spec["weights"] / spec["weights"].sum()).pvalue
    print(f"chi-square of the reads per cell against the weights: p = {p:.4f}; counts {counts.tolist()}")
    assert p > 1e-3
    # the module: the same table
    out2 = tmp_path / "cb2.tsv"
    r = _module("-p", cb_paf, "-o", out2, "--cb-count", "8", "--random-seed", "5")
    assert r.returncode == 0 and open(out2).read() == open(out).read()
    # the draw is keyed by the read's index among the surviving reads: the first reads of a shorter file draw the same cells
    short = tmp_path / "short.paf"
    short.write_text("".join(open(cb_paf).read().splitlines(keepends=True)[:3000]))
    part = S.abundance(short, keep_hits=True, **kw)
    n = len(part["read_cells"]) - 1                                   # (the last read may have lost records to the cut)
    assert n > 1000 and list(part["read_cells"][:n]) == spec["read_cells"][:n]


def test_cb_count_dropout_and_whitelist(S, cb_paf, tmp_path):
    res = S.abundance(cb_paf, cb_count=6, seed=9, cb_dropout=0.0)
    spec = A.run(cb_paf, cb_count=6, seed=9, cb_dropout=0.0)
    assert "." not in set(res["cells"]) and list(zip(res["names"], res["cells"])) == [(n, c) for n, c, _ in spec["rows"]]
    everything = S.abundance(cb_paf, cb_count=6, seed=9, cb_dropout=1.0)
    assert set(everything["cells"]) == {"."}
    wl = tmp_path / "wl.txt.gz"
    names = [f"BC{i:03d}" for i in range(40)]
    with gzip.open(wl, "wt") as f:
        f.write("\n".join(names) + "\n")
    res = S.abundance(cb_paf, cb_count=12, seed=4, cb_txt=wl, keep_hits=True)
    spec = A.run(cb_paf, cb_count=12, seed=4, cb_txt=wl)
    assert set(res["cells"]) <= set(names) | {"."} and list(res["read_cells"]) == spec["read_cells"]
    assert list(zip(res["names"], res["cells"])) == [(n, c) for n, c, _ in spec["rows"]]
    gate(res["tpm"], [t for _, _, t in spec["rows"]], "--cb-txt: tpm")
    # a whitelist that repeats a barcode: equal strings are one cell
    twice = tmp_path / "twice.txt"
    twice.write_text("SAME\nSAME\nSAME\nSAME\n")
    res = S.abundance(cb_paf, cb_count=4, seed=4, cb_txt=twice, cb_dropout=0.0)
    spec = A.run(cb_paf, cb_count=4, seed=4, cb_txt=twice, cb_dropout=0.0)
    assert set(res["cells"]) == {"SAME"} and list(res["names"]) == [n for n, _, _ in spec["rows"]]
    gate(res["tpm"], [t for _, _, t in spec["rows"]], "one cell under four barcodes: tpm")


def test_written_table_round_trips_through_transcribe(S, tmp_path):
    """the PAF's targets are the fixture GTF's transcript ids with a version behind a dot; the plan made from the device-written table
    counts the molecules the plan made from the specification's table counts: the file is one `transcribe` reads, dot-cut ids included"""
    from tksm_amd.sequence import Sequencer
    gtf = os.path.join(GOLDEN, "transcribe", "ann.gtf")
    rs = np.random.RandomState(13)
    reads = random_reads(rs, 1500, 12, max_recs=4)
    reads = [(rid, ql, [(f"T{1 + int(t[1:])}.{1 + int(t[1:]) % 3}", ts, m, b) for t, ts, m, b in recs]) for rid, ql, recs in reads]
    paf, ours, theirs = tmp_path / "in.paf", tmp_path / "ours.tsv", tmp_path / "theirs.tsv"
    paf.write_text(paf_text(reads))
    S.abundance(paf, out=ours)
    theirs.write_text(A.run(paf)["tsv"])
    s = Sequencer(0)
    try:
        s.add_gtf(gtf)
        infos = []
        for table in (ours, theirs):
            plan = s.transcribe_plan(table, 5000, seed=3)
            infos.append(([plan.rows, plan.records, plan.molecules, list(plan.missing)], plan.mdf_text()))
            plan.close()
    finally:
        s.close()
    assert infos[0] == infos[1]
    rows, records, molecules, missing = infos[0][0]
    assert rows == 12 and records == 11 and missing == ["T8"] and 4500 <= molecules <= 5100      # (the fixture GTF knows T8 only under the id T8.1)


# ---- transcriptome-scale shapes: the thresholds of the reduction chain ------------------------------------------------------------------
# The levels of a sum: chunks of 1024 hits, the wave tree, blocks of 256 segments (k_abund_mfinish), and ONE block that loops over the
# block results once there are more than 256 of them (k_abund_mtotal), that is above 65 536 segments.
def threshold_reads(T):
    """read i hits t{i}; every third read also t{(7919 i + 1) mod T}, with fewer matches that stay above 0.95 of the best: sums and
    weights are not trivial and the hits' transcripts do not rise with the hit index"""
    return [(f"r{i}", 1000, [(f"t{i}", 0, 900, 950)] + ([(f"t{(7919 * i + 1) % T}", 3, 870 + i % 25, 950)] if i % 3 == 0 else [])) for i in range(T)]


def lr_text(cell_of_read):
    """the five-column lr-br table, third column 1"""
    return "".join(f"{rid}\t0\t1\t0\t{bc}\n" for rid, bc in cell_of_read)


def all_tpm(spec):
    """every tpm of the specification's split, the rows the writer skips included"""
    cell = dict(zip(spec["surviving"], spec["read_cells"]))
    return np.array(list(A.split(spec["hits"], cell.__getitem__).values())) * 1_000_000


@pytest.mark.parametrize("T", [255, 256, 257, 65536, 65537, 65793])
def test_transcript_counts_around_the_block_and_the_total_loop(S, tmp_path, T):
    """one block of k_abund_mfinish less one, exactly, plus one; 256 blocks (one pass of k_abund_mtotal), 257 (its loop), and 258 with
    ONE transcript in the last.  At 65 793 a block result that is dropped or counted twice moves the total by 1.5e-5 relative."""
    res, spec = check_against_spec(S, tmp_path, threshold_reads(T), f"{T} transcripts")
    assert len(res["abundance"]) == T and len(res["hit_transcripts"]) == T + (T + 2) // 3
    total = float(np.sum(res["abundance"].astype(np.longdouble)))
    print(f"{T} transcripts: the abundances add up to 1 {total - 1.0:+.3g}")
    assert abs(total - 1.0) <= 1e-12
    # the row set can be compared only when no tpm sits at the cut (0.001) or at the text's rounding boundary below it (0.0005): on the
    # specification's own values, as tests/golden/make_abundance_golden.py does
    tpm = all_tpm(spec)
    assert len(tpm) == T and min(np.abs(tpm / 0.001 - 1).min(), np.abs(tpm / 0.0005 - 1).min()) > 1e-6


def hitless_reads():
    """2 000 transcripts in order of first appearance: h0_* (300, named only by reads the 0.5 gate drops), n0_* (200), h1_0 (1), n1_*
    (199), h2_* (300: ids 700 - 999, across 768), n2_* (700), h3_* (300, the last ids of the table)"""
    reads, seen = [], []

    def hitless(run, count):
        for j in range(count):
            reads.append((f"d{run}_{j}", 1000, [(f"h{run}_{j}", 0, 390, 400), (f"h{run}_{j}", 5, 380, 400)][:1 + j % 2]))

    def named(run, count):
        for j in range(count):
            recs = [(f"n{run}_{j}", 0, 900, 950)]
            if seen and j % 3 != 1:
                recs.insert(j % 2, (seen[(31 * j + 7 * run) % len(seen)], 2, 860 + j % 40, 950))
            seen.append(f"n{run}_{j}")
            reads.append((f"r{run}_{j}", 1000, recs))
    hitless(0, 300); named(0, 200); hitless(1, 1); named(1, 199); hitless(2, 300); named(2, 700); hitless(3, 300)
    return reads


def test_runs_of_transcripts_without_a_surviving_hit(S, tmp_path):
    """the fill loops of k_abund_dense_offsets: a run of empty segments before the first hit, of one, of 300 across a block boundary, and
    behind the last hit"""
    res, spec = check_against_spec(S, tmp_path, hitless_reads(), "runs of transcripts without hits")
    names = list(res["transcripts"])
    assert len(names) == 2000
    ids = np.array([i for i, n in enumerate(names) if n.startswith("h")])
    assert ids.tolist() == list(range(300)) + [500] + list(range(700, 1000)) + list(range(1700, 2000))
    assert (res["abundance"][ids] == 0.0).all() and (np.delete(res["abundance"], ids) > 0).all()
    tpm = all_tpm(spec)                      # (150 transcripts that share every read fall to 1e-16 tpm in ten rounds: far below the cut)
    assert len(tpm) == 2000 - len(ids) and min(np.abs(tpm / 0.001 - 1).min(), np.abs(tpm / 0.0005 - 1).min()) > 1e-6
    assert not any(n.startswith("h") for n in res["names"]) and len(res["names"]) > 900
    assert not np.isin(res["hit_transcripts"], ids).any() and res["surviving_reads"] == 1099
    # the plain table and the one split by cells: the same empty transcripts
    cells = tmp_path / "cells.tsv"
    cells.write_text(lr_text((rid, f"C{i % 5}") for i, (rid, _, _) in enumerate(hitless_reads()) if i % 4))
    res, spec = check_against_spec(S, tmp_path, hitless_reads(), "runs of transcripts without hits, cells", lr_br=cells)
    assert (res["abundance"][ids] == 0.0).all() and not any(n.startswith("h") for n in res["names"]) and set(res["cells"]) == {".", "C0", "C1", "C2", "C3", "C4"}


def key_width_reads(T):
    """a dropped read names t0 .. t{T-1} first, so they are the ids 0 .. T-1; then 64 reads, the first on the highest id, the last on
    the lowest, every third with a second hit"""
    reads = [("names", 1000, [(f"t{t}", 0, 390, 400) for t in range(T)])]
    for i in range(64):
        t = T - 1 - (i * T) // 64
        reads.append((f"r{i}", 1000, [(f"t{t}", 0, 900, 950)] + ([(f"t{(t + 1) % T}", 1, 880 + i % 20, 950)] if i % 3 == 0 else [])))
    return reads


@pytest.mark.parametrize("cells", [False, True], ids=["plain", "cells"])
@pytest.mark.parametrize("T", [1, 2, 3, 4, 5, 8, 9, 16, 17])
def test_sort_key_widths(S, tmp_path, T, cells):
    """the radix sorts see bits_for(T) bits of a transcript id (32 more for the pair keys): T = 1, 2, 3 and 2^k, 2^k + 1"""
    kw = {}
    if cells:
        table = tmp_path / "cells.tsv"
        table.write_text(lr_text((f"r{i}", f"C{(5 * i) % 3}") for i in range(64)))
        kw["lr_br"] = table
    res, spec = check_against_spec(S, tmp_path, key_width_reads(T), f"{T} transcripts, {'three cells' if cells else 'plain'}", **kw)
    tid = res["hit_transcripts"]
    assert tid[0] == T - 1 and tid[res["hit_offsets"][63]] == 0 and sorted(set(tid.tolist())) == list(range(T))
    assert list(res["read_cells"]) == spec["read_cells"] and len(set(res["cells"])) == (3 if cells else 1)


def test_pair_keys_of_49_bits(S, tmp_path):
    """65 537 transcripts (17 bits) with two cells: the pair sort's end bit 32 + 17, and more than 65 536 (transcript, cell) segments.
    Ids 0 and 65 536 differ in bit 16 only (bit 48 of a pair key).  Six more reads of cell A alternate between those two transcripts, so
    a sort that does not see bit 48 leaves their keys in hit order, (0, A), (65536, A), (0, A), ..., equal keys are no longer adjacent,
    and the segments -- hence the rows -- of (0, A) and (65536, A) come in pieces."""
    reads = threshold_reads(65537)
    order = list(dict.fromkeys(t for _, _, recs in reads for t, _, _, _ in recs))          # transcripts by first appearance: their ids
    assert len(order) == 65537
    reads += [(f"x{j}", 1000, [(order[65536 * (j % 2)], 0, 900, 950)]) for j in range(6)]
    table = tmp_path / "cells.tsv"
    table.write_text(lr_text([(f"r{i}", "AC"[(i // 3) % 2]) for i in range(65537)] + [(f"x{j}", "A") for j in range(6)]))
    res, spec = check_against_spec(S, tmp_path, reads, "65537 transcripts, two cells", lr_br=table)
    assert list(res["read_cells"]) == spec["read_cells"] and set(res["cells"]) == {"A", "C"} and len(res["names"]) > 65537
    low, high = list(res["transcripts"]).index(order[0]), list(res["transcripts"]).index(order[65536])
    assert (low, high) == (0, 65536) and hits_of(res, order[0], "A") >= 3 and hits_of(res, order[65536], "A") >= 3
    assert len(set(zip(res["names"], res["cells"]))) == len(res["names"])                   # no (transcript, cell) pair in two rows
    tpm = all_tpm(spec)                                              # (the input's own condition, as above: no tpm at the cut)
    assert min(np.abs(tpm / 0.001 - 1).min(), np.abs(tpm / 0.0005 - 1).min()) > 1e-6


# ---- the (transcript, cell) path at its thresholds --------------------------------------------------------------------------------------
def segment_reads(n_big):
    """(reads, table): n_big reads of cell C0 hit `big` (every seventh also one of o0 .. o9); among them 64 cells C1 .. C64 of three reads
    each and 50 reads the table does not name (cell `.`), all on `big` and the ten others"""
    reads, table = [], []
    for i in range(n_big):
        reads.append((f"b{i}", 1000, [("big", 0, 900, 950)] + ([(f"o{i % 10}", 2, 870 + i % 25, 950)] if i % 7 == 0 else [])))
        table.append((f"b{i}", "C0"))
    others = []
    for c in range(1, 65):
        for k in range(3):
            others.append((f"x{c}_{k}", 1000, ([("big", 0, 900, 950)] if k != 1 else []) + ([(f"o{(c + k) % 10}", 1, 890 - k, 950)] if k else [])))
            table.append((f"x{c}_{k}", f"C{c}"))
    others += [(f"u{i}", 1000, [(f"o{i % 10}", 0, 899, 950), ("big", 0, 900, 950)][::1 - 2 * (i % 2)]) for i in range(50)]
    for j, r in enumerate(others):
        reads.insert(min(len(reads), 5 * j + 1), r)
    return reads, lr_text(table)


def hits_of(res, transcript, cell):
    """how many hits the (transcript, cell) segment has, from the kept hits"""
    t = list(res["transcripts"]).index(transcript)
    off, tid = res["hit_offsets"], res["hit_transcripts"]
    return sum(int((tid[off[k]:off[k + 1]] == t).sum()) for k, c in enumerate(res["read_cells"]) if c == cell)


@pytest.mark.parametrize("n_big", [1024, 1025, 5000])
def test_a_cell_segment_of_one_chunk_one_more_hit_and_five_chunks(S, tmp_path, n_big):
    reads, table = segment_reads(n_big)
    lr = tmp_path / "cells.tsv"
    lr.write_text(table)
    res, spec = check_against_spec(S, tmp_path, reads, f"(big, C0) of {n_big} hits", lr_br=lr)
    assert list(res["read_cells"]) == spec["read_cells"]
    assert hits_of(res, "big", "C0") == n_big and hits_of(res, "big", ".") == 50 and hits_of(res, "big", "C7") == 2
    assert set(res["cells"]) == {"."} | {f"C{c}" for c in range(65)}


@pytest.mark.parametrize("n_cells", [255, 256, 257])
def test_cell_segment_counts_around_the_block(S, tmp_path, n_cells):
    """one transcript, n_cells cells of one read each: n_cells segments, a block of k_abund_mfinish less one, exactly, plus one"""
    lr = tmp_path / "cells.tsv"
    lr.write_text(lr_text((f"r{i}", f"C{(i * 101) % n_cells}") for i in range(n_cells)))
    res, spec = check_against_spec(S, tmp_path, [(f"r{i}", 1000, [("one", 0, 900, 950)]) for i in range(n_cells)], f"{n_cells} cells on one transcript", lr_br=lr)
    assert len(res["names"]) == n_cells and len(set(res["cells"])) == n_cells and (res["tpm"] == (1.0 / n_cells) * 1000000.0).all()


def test_more_than_65536_cell_segments(S, tmp_path):
    """66 000 reads with a cell each on 300 transcripts: 88 000 segments, the loop of k_abund_mtotal for the split's total, rows in order
    of first appearance"""
    n = 66000
    reads = [(f"r{i}", 1000, [(f"t{i % 300}", 0, 900, 950)] + ([(f"t{(7 * i + 1) % 300}", 3, 870 + i % 25, 950)] if i % 3 == 0 else [])) for i in range(n)]
    lr = tmp_path / "cells.tsv"
    lr.write_text(lr_text((f"r{i}", f"C{(i * 7919) % n}") for i in range(n)))
    res, spec = check_against_spec(S, tmp_path, reads, "66000 cells", lr_br=lr)
    assert len(res["names"]) == len(res["hit_transcripts"]) == n + n // 3 and len(set(res["cells"])) == n
    total = float(np.sum(res["tpm"].astype(np.longdouble)))
    print(f"66000 cells: the tpm add up to 1e6 {total - 1e6:+.3g}")
    assert abs(total / 1e6 - 1.0) <= 1e-12


def test_reads_the_table_does_not_name(S, tmp_path):
    """unnamed reads share `.` on the transcripts of the named ones (segment_reads holds 50); a table that names no read of the PAF at all
    leaves one cell, and the run is the plain run bit for bit"""
    reads, _ = segment_reads(1500)
    paf, lr = tmp_path / "a.paf", tmp_path / "nobody.tsv"
    paf.write_text(paf_text(reads))
    lr.write_text(lr_text((f"elsewhere{i}", f"C{i % 4}") for i in range(100)))
    for rounds in (10, 0):
        plain, with_table = S.abundance(paf, em_iterations=rounds, keep_hits=True), S.abundance(paf, em_iterations=rounds, lr_br=lr, keep_hits=True)
        for k in ("abundance", "tpm", "hit_weights"):
            assert plain[k].tobytes() == with_table[k].tobytes(), k
        assert list(plain["names"]) == list(with_table["names"]) and set(with_table["cells"]) == {"."} and set(with_table["read_cells"]) == {"."}
    check_against_spec(S, tmp_path, reads, "a table that names no read", lr_br=lr)
    half = tmp_path / "half.tsv"
    half.write_text(lr_text((rid, f"C{i % 3}") for i, (rid, _, _) in enumerate(reads) if i % 2))
    res, spec = check_against_spec(S, tmp_path, reads, "a table that names every other read", lr_br=half)
    assert list(res["read_cells"]) == spec["read_cells"] and list(res["read_cells"]).count(".") == len(reads) - len(reads) // 2


def test_em_zero_with_cells(S, tmp_path):
    """no round: the per-transcript sum runs for the abundance vector's scale only, the rows come from the (transcript, cell) sum"""
    reads, table = segment_reads(1025)
    lr = tmp_path / "cells.tsv"
    lr.write_text(table)
    res, spec = check_against_spec(S, tmp_path, reads, "-em 0 with cells", lr_br=lr, em_iterations=0)
    off = res["hit_offsets"]
    assert all(w == 1.0 / (off[k + 1] - off[k]) for k in range(len(off) - 1) for w in res["hit_weights"][off[k]:off[k + 1]])
    assert hits_of(res, "big", "C0") == 1025 and abs(float(res["abundance"].sum()) - 1.0) <= 1e-12


def test_cb_count_with_few_barcodes_and_segments_of_several_chunks(S, tmp_path):
    """three barcodes and the dropout cell at a quarter of the reads each, 6 000 surviving reads on two transcripts: every (transcript,
    cell) segment is longer than a chunk.  Against the specification's draws, as test_cb_count_cells_equal_the_specifications_draws."""
    reads = [(f"r{i}", 1000, [("ta", 0, 900, 950)] + ([("tb", 1, 870 + i % 25, 950)] if i % 8 else [])) for i in range(6000)]
    reads[100:100] = [(f"d{i}", 1000, [("ta", 0, 390, 400)]) for i in range(40)]
    paf, out = tmp_path / "cb.paf", tmp_path / "cb.tsv"
    paf.write_text(paf_text(reads))
    kw = dict(cb_count=3, seed=11, cb_lognorm_params=(10.0, 0.05), cb_dropout=0.25)
    res = S.abundance(paf, out=out, keep_hits=True, **kw)
    spec = A.run(paf, **kw)
    assert res["surviving_reads"] == 6000 and list(res["read_cells"]) == spec["read_cells"]
    assert len(set(spec["barcodes"])) == 4 and all(hits_of(res, t, c) > 1024 for t in ("ta", "tb") for c in spec["barcodes"])
    assert list(zip(res["names"], res["cells"])) == [(n, c) for n, c, _ in spec["rows"]] and len(spec["rows"]) == 8
    gate(res["abundance"], spec["abundance"], "--cb-count 3: abundance")
    gate(res["tpm"], [t for _, _, t in spec["rows"]], "--cb-count 3: tpm")
    far = all(abs((t * 1000.0) % 1.0 - 0.5) > 1e-4 for _, _, t in spec["rows"])
    assert not far or open(out).read() == spec["tsv"]


# ---- the order of addition, bit for bit -------------------------------------------------------------------------------------------------
def same_bits(got, want, what):
    got, want = np.ascontiguousarray(got, np.float64), np.ascontiguousarray(want, np.float64)
    assert got.shape == want.shape, what
    ulps = np.abs(got.view(np.int64) - want.view(np.int64))
    print(f"{what}: {int((ulps > 0).sum())} of {ulps.size} values differ" + (f", by {int(ulps.max())} ulp at most, first at {int(np.argmax(ulps > 0))}" if ulps.any() else ""))
    assert got.tobytes() == want.tobytes(), what


ORDERED = ["random_700_transcripts", "random_700_transcripts_cells", "fixture_em0", "fixture_em1", "fixture_em10", "fixture_cells", "five_chunks",
           "65793_transcripts", "cell_segment_of_five_chunks"]


def ordered_case(name, tmp_path):
    """(PAF, lr-br table or None, rounds) of a case of the byte comparison"""
    if name.startswith("fixture"):
        return PAF, LR if name == "fixture_cells" else None, {"fixture_em0": 0, "fixture_em1": 1}.get(name, 10)
    table = None
    if name.startswith("random_700"):        # 3 000 reads of up to five records on 700 transcripts (three blocks); 40 cells over three quarters of the reads
        reads = random_reads(np.random.RandomState(5), 3000, 700)
        table = lr_text((f"r{i}", f"C{(i * 13) % 40}") for i in range(3000) if i % 4) if name.endswith("cells") else None
    elif name == "five_chunks":
        reads = _heavy(5000, 500, 500)
    elif name == "65793_transcripts":
        reads = threshold_reads(65793)
    else:
        reads, table = segment_reads(5000)
    paf, lr = tmp_path / "in.paf", tmp_path / "cells.tsv"
    paf.write_text(paf_text(reads))
    if table:
        lr.write_text(table)
    return paf, lr if table else None, 10


@pytest.mark.parametrize("name", ORDERED)
def test_the_documented_order_of_addition_gives_the_devices_bits(S, tmp_path, name):
    """abundance_spec.ordered_run adds and divides in the order DESIGN.md documents (chunks of 1024, lanes, the wave tree, chunk order,
    the block tree, the strided total, the E-step in hit order), in numpy float64: the device's abundances, final weights and tpm are
    the same bytes.  A launch geometry that changed the order of a single addition would change them."""
    paf, lr, rounds = ordered_case(name, tmp_path)
    res = S.abundance(paf, em_iterations=rounds, lr_br=lr, keep_hits=True)
    want = A.ordered_run(paf, em_iterations=rounds, lr_br=lr)
    assert list(zip(res["names"], res["cells"])) == [(n, c) for n, c, _ in want["rows"]]
    if rounds == 0:
        same_bits(res["hit_weights"], want["uniform_weights"], f"{name}: uniform weights")
    same_bits(res["abundance"], want["abundance"], f"{name}: abundance")
    same_bits(res["hit_weights"], want["hit_weights"], f"{name}: final weights")
    same_bits(res["tpm"], want["tpm"], f"{name}: tpm")
