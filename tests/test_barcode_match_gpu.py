"""barcode-match on the device against the specification (tests/barcode_spec.py): the three files and the counters byte for byte, over the
word sizes, segment sizes, window edges, read counts, candidate counts around the match's candidate tile, chunk sizes and file kinds; the
round trip of molecules barcoded on the device; error codes.  All compared quantities are integers and text: there is no tolerance."""
import gzip
import json
import os
import random
import subprocess

import pytest

from conftest import ERR_MODEL, GOLDEN, QS_MODEL, ROOT

import barcode_spec as B

pytestmark = pytest.mark.gpu

EXE = os.path.join(ROOT, "tksm_amd", "tksm")
KNOWN = json.load(open(os.path.join(GOLDEN, "barcode_match_known_answers.json")))
COUNTERS = ("reads", "no_adapter", "forward", "reverse", "whitelist", "candidates", "no_barcode", "unique", "ambiguous", "pairs")
FILES = ("matches", "segments", "selected")


@pytest.fixture(scope="module")
def s():
    from tksm_amd.sequence import Sequencer
    x = Sequencer(0)
    x.set_identity(84.0, 99.0, 5.5)
    x.load_error_model(ERR_MODEL)
    x.load_qscore_model(QS_MODEL)
    rs = random.Random(2)
    x.add_contig("chrB", "".join(rs.choice("ACGT") for _ in range(30_000)))
    yield x
    x.close()


@pytest.fixture(scope="module")
def default_case(tmp_path_factory):
    """about 300 reads at the defaults, and what the specification makes of them: computed once, shared, never changed"""
    d = tmp_path_factory.mktemp("barcode_default")
    g = B.generate(d, seed=7, n_barcodes=160, n_seen=120)
    g["dir"], g["out"] = str(d), B.run(g["reads"], g["whitelist"])
    return g


def device(s, reads, whitelist, d, tag="dev", **kw):
    paths = {k: os.path.join(str(d), f"{tag}.{k}.tsv") for k in FILES}
    info = s.barcode_match(reads, whitelist, paths["matches"], segments_out=paths["segments"], selected_out=paths["selected"], **kw)
    out = {k: open(paths[k]).read() for k in FILES}
    assert not [f for f in os.listdir(str(d)) if f.endswith(".tmp")]
    out["info"] = info
    return out


def same(dev, spec):
    for k in FILES:
        assert dev[k] == spec[k], k
    assert {k: dev["info"][k] for k in COUNTERS} == spec["info"]


def check(s, d, reads, whitelist, chunk_reads=0, **params):
    spec = B.run(reads, whitelist, **params)
    dev = device(s, reads, whitelist, d, chunk_reads=chunk_reads, **params)
    same(dev, spec)
    return dev, spec


def head_fastq(path, n, out):
    lines = open(path).read().split("\n")
    with open(out, "w") as f:
        f.write("\n".join(lines[:4 * n]) + "\n")
    return out


def test_generated_data_at_the_defaults(s, default_case):
    g = default_case
    dev = device(s, g["reads"], g["whitelist"], g["dir"])
    same(dev, g["out"])
    for k in ("forward", "reverse", "adapter_at_max", "adapter_over_max", "adapter_ends_at_window", "adapter_ends_past_window", "adapter_both_ends",
              "shorter_than_adapter", "ends_inside_barcode", "ends_after_barcode", "adapter_with_n", "barcode_substitution", "barcode_insertion",
              "barcode_deletion", "barcode_at_max_errors", "barcode_over_max_errors", "barcode_with_n", "lower_case", "two_tied", "more_than_eight_tied",
              "homopolymer", "exact_at_min", "exact_below_min", "never_seen", "no_adapter"):
        assert g["classes"].get(k), k
    i = dev["info"]
    assert 250 <= i["reads"] <= 350 and i["ambiguous"] == 2 and i["no_adapter"] >= 3 and i["no_barcode"] >= 3 and i["chunks"] == 1
    assert i["device_ms"] > 0 and len(i["stage_ms"]) == 4


@pytest.mark.parametrize("L,adapter,extra", [
    (4, None, dict(max_errors=1)),
    (16, None, dict()),
    (32, None, dict()),                               # the word's top bit
    (16, "GATTACAGGCTCAAGTCCTGAACGTTAGCCAT", dict()),     # an adapter of 32: the word's top bit in the adapter pass
    (16, None, dict(pad=0)),
    (32, None, dict(pad=16)),                         # a segment of 64 letters: the packing boundary
    (8, "ACGTTGCA", dict(window=8, max_adapter_errors=1)),            # the window is the adapter's length
    (16, None, dict(window=5000)),                    # a window longer than every read
])
def test_word_sizes_segment_sizes_and_window_edges(s, tmp_path, L, adapter, extra):
    params = dict(extra)
    if adapter:
        params["adapter"] = adapter
    g = B.generate(tmp_path, seed=100 + L, L=L, n_barcodes=40, n_seen=25, **params)
    dev, spec = check(s, tmp_path, g["reads"], g["whitelist"], **params)
    assert spec["info"]["unique"] + spec["info"]["ambiguous"] > 10 and spec["info"]["forward"] > 5 and spec["info"]["reverse"] > 0
    if extra.get("pad") == 16:
        assert max(len(l.split("\t")[4]) for l in spec["segments"].splitlines()) == 64


@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_read_counts_around_a_wave(s, default_case, tmp_path, n):
    reads = head_fastq(default_case["reads"], n, str(tmp_path / "head.fq"))
    dev, spec = check(s, tmp_path, reads, default_case["whitelist"], min_exact=1)
    assert spec["info"]["reads"] == n


@pytest.mark.parametrize("n_barcodes", [1, 255, 256, 257, 513, 3000])
def test_candidate_counts_around_the_tile(s, default_case, tmp_path, n_barcodes):
    """min_exact 0 makes the whole whitelist the candidates; with these few reads a workgroup row of the match takes BM_CAND_TILE candidates,
    so 256 / 257 / 513 candidates are one full row / a row and one candidate / two rows and one"""
    from tksm_amd import _lib
    assert _lib.BM_CAND_TILE == 256
    reads = head_fastq(default_case["reads"], 70, str(tmp_path / "head.fq"))
    rs = random.Random(n_barcodes)
    wl = list(dict.fromkeys(default_case["barcodes"][:min(n_barcodes, 60)] + ["".join(rs.choice("ACGT") for _ in range(16)) for _ in range(n_barcodes)]))[:n_barcodes]
    rs.shuffle(wl)
    (tmp_path / "wl.txt").write_text("\n".join(wl) + "\n")
    dev, spec = check(s, tmp_path, reads, str(tmp_path / "wl.txt"), min_exact=0)
    assert spec["info"]["candidates"] == n_barcodes and spec["info"]["pairs"] == n_barcodes * (spec["info"]["forward"] + spec["info"]["reverse"])


@pytest.mark.parametrize("min_exact", [0, 1, 2, 1000])
def test_selection_thresholds(s, default_case, tmp_path, min_exact):
    dev, spec = check(s, tmp_path, default_case["reads"], default_case["whitelist"], min_exact=min_exact)
    if min_exact == 1000:
        i = spec["info"]
        assert spec["matches"] == "" and spec["selected"] == "" and i["candidates"] == 0 and i["no_barcode"] == i["forward"] + i["reverse"] > 0
    else:
        assert spec["info"]["candidates"] > 100


def test_revcomp_barcodes(s, tmp_path):
    g = B.generate(tmp_path, seed=21, n_barcodes=60, n_seen=40, revcomp_barcodes=True)
    dev, spec = check(s, tmp_path, g["reads"], g["whitelist"], revcomp_barcodes=True)
    assert spec["info"]["unique"] > 80
    plain = device(s, g["reads"], g["whitelist"], tmp_path, tag="plain")
    same(plain, B.run(g["reads"], g["whitelist"]))
    assert plain["info"]["unique"] < 10


def test_chunk_sizes_and_repetition_give_the_same_bytes(s, default_case, tmp_path):
    g = default_case
    first = device(s, g["reads"], g["whitelist"], tmp_path, tag="c0")
    same(first, g["out"])
    for chunk in (1, 64, 65, 0):
        again = device(s, g["reads"], g["whitelist"], tmp_path, tag=f"c{chunk}", chunk_reads=chunk)
        assert all(again[k] == first[k] for k in FILES), chunk
        assert again["info"]["chunks"] == (-(-g["n_reads"] // chunk) if chunk else 1)
    # other calls use and free device memory in between: a larger match with other parameters, and a simulation
    other = B.generate(tmp_path, seed=5, L=32, n_barcodes=300, n_seen=150, pad=16)
    device(s, other["reads"], other["whitelist"], tmp_path, tag="other", pad=16, min_exact=0)
    b = s.batch_from_mdf("".join(f"+m{i}\t1\t\nchrB\t{100 * i}\t{100 * i + 2000}\t+\t\n" for i in range(64)))
    try:
        assert len(s.run(b, target="badread", fastq=True, seed=1).records()) == 64
    finally:
        b.free()
    later = device(s, g["reads"], g["whitelist"], tmp_path, tag="later", chunk_reads=100)
    assert all(later[k] == first[k] for k in FILES)


def test_gz_inputs_two_read_files_and_gz_output(s, default_case, tmp_path):
    g = default_case
    lines = open(g["reads"]).read().split("\n")
    half = 4 * (g["n_reads"] // 2)
    with gzip.open(tmp_path / "a.fq.gz", "wt") as f:
        f.write("\n".join(lines[:half]) + "\n")
    (tmp_path / "b.fq").write_text("\n".join(lines[half:]))
    with gzip.open(tmp_path / "wl.txt.gz", "wt") as f:
        f.write(open(g["whitelist"]).read())
    reads = [str(tmp_path / "a.fq.gz"), str(tmp_path / "b.fq")]
    assert B.run(reads, str(tmp_path / "wl.txt.gz")) == g["out"]
    paths = {k: str(tmp_path / f"{k}.tsv.gz") for k in FILES}
    s.barcode_match(reads, tmp_path / "wl.txt.gz", paths["matches"], segments_out=paths["segments"], selected_out=paths["selected"])
    for k in FILES:
        assert open(paths[k], "rb").read(2) == b"\x1f\x8b" and gzip.open(paths[k], "rt").read() == g["out"][k], k


def test_reads_list_with_an_empty_entry_and_the_loaders_messages(s, tmp_path):
    """the comma list of read files as the C-ABI takes it: "a.fq,,b.fq" is the one file with both; the loader's messages word for word"""
    from tksm_amd import _lib as L
    from tksm_amd.sequence import TksmSeqError
    g = B.generate(tmp_path, seed=3, n_barcodes=8, n_seen=4)
    reads = head_fastq(g["reads"], 30, str(tmp_path / "thirty.fq"))
    lines = open(reads).read().split("\n")
    (tmp_path / "a.fq").write_text("\n".join(lines[:4 * 13]) + "\n")
    (tmp_path / "b.fq").write_text("\n".join(lines[4 * 13:]))
    one = device(s, reads, g["whitelist"], tmp_path, tag="one")
    both = device(s, [tmp_path / "a.fq", "", tmp_path / "b.fq"], g["whitelist"], tmp_path, tag="list")
    same(one, B.run(reads, g["whitelist"]))
    assert all(both[k] == one[k] for k in FILES) and one["info"]["reads"] == 30
    (tmp_path / "empty.fq").write_text("\n")
    (tmp_path / "bad.fq").write_text("@a\nACGT\n+\nIII\n")
    for reads, message in ((tmp_path / "empty.fq", f"barcode-match: no reads in {tmp_path / 'empty.fq'}"),
                           ([tmp_path / "a.fq", tmp_path / "bad.fq"], f"{tmp_path / 'bad.fq'}: FASTQ record 1: sequence and quality differ in length")):
        with pytest.raises(TksmSeqError) as e:
            s.barcode_match(reads, g["whitelist"], tmp_path / "never.tsv")
        assert e.value.code == L.EINVAL and str(e.value) == f"tksmseq error {L.EINVAL}: {message}" and not (tmp_path / "never.tsv").exists()


def test_cli_against_the_python_call_and_the_hand_counted_case(s, default_case, tmp_path):
    g = default_case
    out = {k: str(tmp_path / f"cli.{k}.tsv") for k in FILES}
    # (the allocator fills what it hands out with this word: the module's files do not depend on what its memory held)
    r = subprocess.run([EXE, "barcode-match", "--reads", g["reads"], "--whitelist", g["whitelist"], "-o", out["matches"], "--segments-out", out["segments"],
                        "--selected-out", out["selected"], "--chunk-reads", "77"], capture_output=True, text=True, env=dict(os.environ, TKSMSEQ_POISON="00000001"))
    assert r.returncode == 0, r.stderr
    assert "barcode-match: " in r.stderr and f"{g['n_reads']} reads" in r.stderr
    for k in FILES:
        assert open(out[k]).read() == g["out"][k], k
    for name in ("reads", "whitelist"):
        (tmp_path / f"known.{name}").write_text(KNOWN[name])
    dev = device(s, tmp_path / "known.reads", tmp_path / "known.whitelist", tmp_path, tag="known", **KNOWN["params"])
    same(dev, KNOWN)
    r = subprocess.run([EXE, "barcode-match", "--reads", tmp_path / "known.reads", "--whitelist", tmp_path / "known.whitelist", "-o", tmp_path / "k.tsv",
                        "--adapter", "ACGTAC", "--window=10", "--max-adapter-errors", "1", "--pad", "1", "--max-errors", "1", "--min-exact", "1"],
                       capture_output=True, text=True)
    assert r.returncode == 0 and (tmp_path / "k.tsv").read_text() == KNOWN["matches"], r.stderr
    r = subprocess.run([EXE, "barcode-match", "--reads", tmp_path / "nonesuch.fq", "--whitelist", tmp_path / "known.whitelist", "-o", tmp_path / "n.tsv"],
                       capture_output=True, text=True)
    assert r.returncode == 1 and "Error:" in r.stderr and not (tmp_path / "n.tsv").exists()


@pytest.fixture(scope="module")
def barcoded(s, tmp_path_factory):
    """molecules with CB= comments through polya -> tag (10 N) -> scb -> tag (the adapter's reverse complement) -> flip 0.5 -> tag (outer adapters)"""
    d = tmp_path_factory.mktemp("barcode_round_trip")
    rs = random.Random(17)
    rnd = lambda n: "".join(rs.choice("ACGT") for _ in range(n))
    cbs = list(dict.fromkeys(rnd(16) for _ in range(24)))
    truth = [cbs[k % len(cbs)] for k in range(96)]
    text = "".join(f"+mol{k}\t1\tCB={cb};\nchrB\t{200 * k}\t{200 * k + 300 + 3 * k}\t{'+-'[k % 2]}\t\n" for k, cb in enumerate(truth))
    steps = [s.batch_from_mdf(text)]
    steps.append(s.polya(steps[-1], normal=(30.0, 5.0), seed=3))
    steps.append(s.tag(steps[-1], format3="10", seed=3))
    steps.append(s.scb(steps[-1]))
    steps.append(s.tag(steps[-1], format3=B.revcomp(B.DEFAULT_ADAPTER), seed=4))
    steps.append(s.flip(steps[-1], 0.5, seed=5))
    steps.append(s.tag(steps[-1], format5=rnd(28), format3=rnd(28), seed=6))
    (d / "wl.txt").write_text("\n".join(cbs) + "\n")
    yield {"dir": d, "batch": steps[-1], "truth": truth, "whitelist": str(d / "wl.txt")}
    for x in steps:
        x.free()


def _fastq_of(records, path):
    with open(path, "wb") as f:
        f.write(b"".join(records))
    return [r.split(b"\n", 1)[0][1:].split()[0].decode() for r in records]


def test_round_trip_of_molecules_barcoded_on_the_device(s, barcoded):
    d = barcoded["dir"]
    names = _fastq_of(s.run(barcoded["batch"], target="perfect", fastq=True, seed=9).records(), d / "perfect.fq")
    assert len(names) == 96 == len(set(names))
    dev, spec = check(s, d, str(d / "perfect.fq"), barcoded["whitelist"], revcomp_barcodes=True)
    rows = {l.split("\t")[0]: l.split("\t") for l in dev["matches"].splitlines()}
    assert {n: (rows[n][1], rows[n][2], rows[n][4]) for n in names} == {n: ("0", "1", cb) for n, cb in zip(names, barcoded["truth"])}
    assert 20 < dev["info"]["forward"] < 76 and dev["info"]["unique"] == 96


def test_badread_reads_of_the_same_molecules(s, barcoded):
    d = barcoded["dir"]
    names = _fastq_of(s.run(barcoded["batch"], target="badread", fastq=True, seed=9).records(), d / "badread.fq")
    dev, spec = check(s, d, str(d / "badread.fq"), barcoded["whitelist"], revcomp_barcodes=True, min_exact=0)
    rows = {l.split("\t")[0]: l.split("\t") for l in dev["matches"].splitlines()}
    right = sum(1 for n, cb in zip(names, barcoded["truth"]) if n in rows and rows[n][2] == "1" and rows[n][4] == cb)
    print(f"badread reads (identity 84, 99, 5.5): {right} of {len(names)} come back with their own barcode alone at distance <= 2 (an observation, not a gate)")


def test_error_codes(s, default_case, tmp_path):
    from tksm_amd import _lib as L
    from tksm_amd.sequence import TksmSeqError
    g = default_case

    def code(reads, whitelist, **kw):
        with pytest.raises(TksmSeqError) as e:
            s.barcode_match(reads, whitelist, tmp_path / "never.tsv", **kw)
        assert not (tmp_path / "never.tsv").exists()
        return e.value.code, str(e.value)

    for text, word in (("ACGTACGTACGTACGT\nACGTACGTACGTACG\n", "line 2"), ("ACGTACGTACGTACGT\nACGTACGTACGTACGN\n", "ACGT"), ("ACG\n", "line 1"), ("\n", "empty")):
        (tmp_path / "bad.txt").write_text(text)
        c, msg = code(g["reads"], tmp_path / "bad.txt")
        assert c == L.EINVAL and word in msg, (text, msg)
    (tmp_path / "dup.txt").write_text("ACGTACGTACGTACGT\nTTTTACGTACGTACGT\n\nACGTACGTACGTACGT\n")
    c, msg = code(g["reads"], tmp_path / "dup.txt")
    assert c == L.EINVAL and "line 4" in msg and "line 1" in msg
    assert code(tmp_path / "nonesuch.fq", g["whitelist"])[0] == L.EIO
    assert code(g["reads"], tmp_path / "nonesuch.txt")[0] == L.EIO
    (tmp_path / "bad.fq").write_text("@a\nACGT\n+\nIII\n")
    assert code(tmp_path / "bad.fq", g["whitelist"])[0] == L.EINVAL
    (tmp_path / "twice.fq").write_text("@a\nACGT\n+\nIIII\n@a x\nACGT\n+\nIIII\n")
    assert code(tmp_path / "twice.fq", g["whitelist"])[0] == L.EINVAL
    (tmp_path / "empty.fq").write_text("")
    assert code(tmp_path / "empty.fq", g["whitelist"])[0] == L.EINVAL
    for kw in (dict(adapter="ACG"), dict(window=21), dict(pad=17), dict(max_adapter_errors=22), dict(max_errors=16), dict(min_exact=-1)):
        assert code(g["reads"], g["whitelist"], **kw)[0] == L.EINVAL, kw
    with pytest.raises(TksmSeqError) as e:
        s.barcode_match(g["reads"], g["whitelist"], tmp_path / "no_such_dir" / "m.tsv")
    assert e.value.code == L.EIO
