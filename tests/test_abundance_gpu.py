"""abundance on the device (-m gpu): `tksm abundance`, Sequencer.abundance and the C-ABI accessors against the files the reference's own
script wrote (tests/golden/abundance/) and against the numpy specification (tests/abundance_spec.py).

The gate of an abundance: relative 1e-9.  Derived, not measured: a round is three sums of non-negative terms (per transcript, the total,
per read), each within n 2^-53 of the exact sum for n terms, n < 1e5 here: 10 rounds x 3 sums x 1e5 x 1.1e-16 = 3.3e-10.  Whether the EM
map amplifies a rounding difference is not proven; the worst relative difference seen is printed by every test that gates on it."""
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
    over all tests of this file that gate on the specification, 4.39e-15."""
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
