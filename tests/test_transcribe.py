"""transcribe: GTF + abundance tables to molecules (src/transcribe.cpp) -- the CPU part: the specification (tests/tsb_spec.py) against
the reference's loop restated with numpy's generator and against the committed fixture; every quirk of the reference on both; the
rounding rule; the edges of the double -> int conversion; independence of the slicing; the library's exports; the argument checks of
`tksm transcribe` and of the chained `tksm sequence --transcribe-*` (all made before a device is opened).  GPU part:
tests/test_transcribe_gpu.py."""
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

import tsb_spec as ts

EXE = os.path.join(ROOT, "tksm_amd", "tksm")
D = os.path.join(GOLDEN, "transcribe")
GTF = open(os.path.join(D, "ann.gtf")).read()
ABUND = open(os.path.join(D, "abund_exact.tsv")).read()


def _cli(*args, timeout=600, **kw):
    return subprocess.run([EXE, *[str(a) for a in args]], capture_output=True, text=True, timeout=timeout, **kw)


def _both(gtfs, abundances, molecule_count, seed=5, **kw):
    """(reference text, spec text, ids the reference warned about); the callers use inputs whose counts are integers, so both agree"""
    warn = []
    ref = ts.tsb_reference(np.random.RandomState(seed), gtfs, abundances, molecule_count, warn=warn, **kw)
    spec = ts.tsb_spec_text(seed, gtfs, abundances, molecule_count, **kw)
    return ref, spec, warn


def _line(chrom, typ, a, b, strand, attrs):
    return f"{chrom}\tt\t{typ}\t{a}\t{b}\t.\t{strand}\t.\t{attrs}\n"


# ------------------------------------------------------------------------------------------------ the fixture
def test_exact_fixture_spec_reference_and_golden_agree():
    want = open(os.path.join(D, "expected_exact.mdf")).read()
    ref, spec, warn = _both([GTF], [ABUND], 60)
    assert ref == want and spec == want
    assert warn == ["T8", "NOPE"]                                       # T8.1 exists only with its version
    heads = [l for l in want.split("\n") if l.startswith("+")]
    assert [h.split("\t")[0] for h in heads] == [f"+M{k}" for k in range(10)]
    assert "+M6\t4\tCB=GGGGCCCCAA;tid=T7;\n+M7" in want                  # T7: a molecule without segments
    assert "+M1\t1\tCB=ACGTACGTAC;tid=T2;\nc1\t100\t300\t+\t\nc3\t2950\t3000\t+\t\n" in want     # the second T2's exon, appended
    assert sum(int(h.split("\t")[1]) for h in heads) == 60 - 6 - 5        # the unfound rows count in sum_tpm, their molecules are lost
    # any other seed: no draw matters
    assert ts.tsb_spec_text(99, [GTF], [ABUND], 60) == want


# ------------------------------------------------------------------------------------------------ quirks
def test_default_depth_is_the_non_coding_switch():
    for dd in (1, -3):
        ref, spec, warn = _both([GTF], [ABUND], 60, default_depth=dd)
        assert ref == spec and "tid=T4;" not in ref and "T4" in warn       # the lncRNA gene is gone
    ref, spec, _ = _both([GTF], [ABUND], 60, default_depth=0)
    assert ref == spec and "tid=T4;" in ref
    # a line without gene_biotype is dropped as well when the switch is on
    g = _line("c", "transcript", 1, 9, "+", 'transcript_id "A";') + _line("c", "exon", 1, 9, "+", 'transcript_id "A";')
    ref, spec, warn = _both([g], ["h\nA 1 x\n"], 1, default_depth=1)
    assert ref == spec == "" and warn == ["A"]


def test_version_trimming_and_use_whole_id():
    ab = "h\nT8.1\t2\tAC\nT1.7\t2\tAC\nT1\t2\tAC\n.\t0\tAC\n"
    ref, spec, warn = _both([GTF], [ab], 6)
    assert ref == spec and warn == ["T8", ""] and ref.count("tid=T1;") == 2
    ref, spec, warn = _both([GTF], [ab], 6, use_whole_id=True)
    assert ref == spec and warn == ["T1.7", "."] and "tid=T8.1;" in ref and ref.count("tid=T1;") == 1
    assert ts.format_annot_id("a.b.c") == "a" and ts.format_annot_id(".x") == "" and ts.format_annot_id("a.b", False) == "a.b"


def test_duplicate_transcript_id_and_first_file_wins():
    g1 = (_line("c1", "transcript", 1, 50, "+", 'transcript_id "A";') + _line("c1", "exon", 1, 20, "+", 'transcript_id "A";') +
          _line("c1", "transcript", 100, 200, "-", 'transcript_id "B";') + _line("c1", "exon", 100, 200, "-", 'transcript_id "B";') +
          _line("c2", "transcript", 5, 9, "-", 'transcript_id "A";') + _line("c2", "exon", 5, 9, "-", 'transcript_id "ignored";'))
    g2 = _line("c9", "transcript", 1, 5, "+", 'transcript_id "A";') + _line("c9", "exon", 1, 5, "+", "") + \
        _line("c9", "transcript", 7, 9, "+", 'transcript_id "C";') + _line("c9", "exon", 7, 9, "+", "")
    ab = "h\nA 1 x\nB 1 x\nC 1 x\n"
    ref, spec, warn = _both([g1, g2], [ab], 3)
    assert ref == spec and not warn
    assert ref.startswith("+M0\t1\tCB=x;tid=A;\nc1\t0\t20\t+\t\nc2\t4\t9\t-\t\n+M1")      # A: first line's exon, then the duplicate's; not g2's
    assert "tid=C;\nc9\t6\t9\t+\t\n" in ref
    ref2, spec2, _ = _both([g2, g1], [ab], 3)
    assert ref2 == spec2 and ref2.startswith("+M0\t1\tCB=x;tid=A;\nc9\t0\t5\t+\t\n+M1")


def test_attribute_values_are_the_second_token():
    assert ts.gtf_line(_line("c", "exon", 1, 2, "+", 'gene_name "A B"; x  "y"; k v w;solo; "q" "r";')[:-1], "f:1")[5] == \
        {"gene_name": "A", "x": "", "k": "v", "solo": "", "q": "r"}
    g = _line("c", "transcript", 1, 9, "+", 'transcript_id "first second"; transcript_id "last one"') + _line("c", "exon", 3, 9, "x", "")
    ref, spec, _ = _both([g], ["h\nlast 2 ,\n"], 2)
    assert ref == spec == "+M0\t2\tCB=,;tid=last;\nc\t2\t9\t-\t\n"          # a strand that is not "+" is minus


def test_unfound_ids_are_warned_not_emitted_and_counted_in_the_sum():
    ab = "h\nT1 10 a\nGHOST 30 a\nT2 20 a\n"
    ref, spec, warn = _both([GTF], [ab], 60)
    assert ref == spec and warn == ["GHOST"]
    assert [l.split("\t")[:2] for l in ref.split("\n") if l.startswith("+")] == [["+M0", "10"], ["+M1", "20"]]
    p = ts.tsb_spec(5, [GTF], [ab], 60)[0]
    assert (p.rows, p.records, p.molecules, p.missing) == (3, 2, 30, ["GHOST"])


def test_cb_empty_dot_and_beg():
    ab = "h\nT1 1\nT2 1 .\n\nT5 1 AC extra columns\n   \t\nT6 x AC\n"
    ref, spec, warn = _both([GTF], [ab], 3)
    assert ref == spec and warn == ["BEG", "BEG"]
    heads = [l for l in ref.split("\n") if l.startswith("+")]
    assert heads == ["+M0\t1\tCB=;tid=T1;", "+M1\t1\tCB;tid=T2;", "+M2\t1\tCB=AC;tid=T5;"]       # T6: tpm unparsable -> 0
    assert ts.read_abundance(ab)[5] == ("T6", 0.0, "")
    # a GTF that has the id BEG makes the empty line a molecule
    g = GTF + _line("c1", "transcript", 1, 9, "+", 'transcript_id "BEG";')
    ref, spec, warn = _both([g], ["h\n\nT1 1 q\n"], 1)
    assert ref == spec and not warn and ref.startswith("+M0\t1\tCB=q;tid=T1;")      # (BEG has tpm 0: no molecule)
    for tok, want in (("1.5abc", (1.5, 3, True)), ("1e", (0.0, 2, False)), (".", (0.0, 1, False)), ("-.5E+1,", (-5.0, 6, True)), ("1e5.3", (1e5, 3, True)),
                      ("nan", (0.0, 0, False)), ("1e999", (np.finfo(np.float64).max, 5, False))):
        assert ts.parse_tpm(tok) == want, tok


def test_index_restarts_with_every_file_and_both_weight_forms():
    a1, a2 = "h\nT1 3 a\nT2 1 a\n", "h\nT5 2 b\nT6 2 b\nT10 4 b\n"
    ref, spec, _ = _both([GTF], [a1, a2], 16)                              # one weight: 1 / 2 each -> 8 molecules per file
    assert ref == spec
    assert [l.split("\t")[:2] for l in ref.split("\n") if l.startswith("+")] == [["+M0", "6"], ["+M1", "2"], ["+M0", "2"], ["+M1", "2"], ["+M2", "4"]]
    ref, spec, _ = _both([GTF], [a1, a2], 16, weights=(1.0, 3.0), prefix="mol_")     # normalised: 4 and 12
    assert ref == spec
    assert [l.split("\t")[:2] for l in ref.split("\n") if l.startswith("+")] == [["+mol_0", "3"], ["+mol_1", "1"], ["+mol_0", "3"], ["+mol_1", "3"], ["+mol_2", "6"]]
    assert ts.file_weights([2.0], 4) == [0.5] * 4 and ts.file_weights([1, 1, 2], 3) == [0.25, 0.25, 0.5]
    with pytest.raises(ValueError):
        ts.file_weights([1, 2], 3)
    plans = ts.tsb_spec(5, [GTF], [a1, a2], 16)
    assert [p.rows for p in plans] == [2, 3]


def test_undefined_inputs_are_errors_that_name_file_and_line():
    good = _line("c", "transcript", 1, 9, "+", 'transcript_id "A";')
    for bad, what in ((good + "c\tt\texon\t1\t9\t.\t+\t.\n", "bad.gtf:2: a GTF line has 9"), (good + "\n" + _line("c", "exon", "x", 9, "+", ""), "bad.gtf:3: start and end"),
                      (_line("c", "exon", 1, 9, "+", ""), "bad.gtf:1: an exon line before"), (_line("c", "gene", 0, 9, "+", ""), "bad.gtf:1: start and end"),
                      (_line("c", "gene", 1, 2**31, "+", ""), "bad.gtf:1: start and end")):
        for fn in (lambda g: ts.tsb_reference(np.random.RandomState(1), [g], ["h\n"], 1), lambda g: ts.tsb_spec(1, [g], ["h\n"], 1)):
            with pytest.raises(ValueError) as e:
                fn(("bad.gtf", bad))
            assert what in str(e.value)


# ------------------------------------------------------------------------------------------------ the count rule
def test_rounding_rule_on_50000_rows():
    """Every depth is floor(c) or floor(c) + 1, and the number X of rounded-up rows is a sum of independent Bernoulli(carry) draws: mean
    S = sum(carry), variance V = sum(carry (1 - carry)).  |X - S| <= 5 sqrt(V) for the spec and for the restated reference, and the two
    differ by at most 5 sqrt(2 V) (the difference of two independent such sums)."""
    n = 50_000
    rs = np.random.RandomState(2024)
    ids = [f"X{k}" for k in range(n)]
    gtf = "".join(_line("c", "transcript", 1, 5, "+", f'transcript_id "{t}";') for t in ids)
    tpm = rs.gamma(2.0, 3.0, n) + 0.001
    found = rs.random_sample(n) < 0.9
    ab = "h\n" + "".join(f"{t if f else 'none' + t}\t{v!r}\tB\n" for t, v, f in zip(ids, tpm.tolist(), found))
    mc = 400_000
    plan = ts.tsb_spec(42, [gtf], [ab], mc)[0]
    c, carry = plan.c, plan.carry
    assert np.array_equal(plan.found, found) and (c > 0).all()
    floor = np.floor(c).astype(np.int64)
    assert np.all(carry > 0) and np.all(carry < 1)                                     # no integer c among them
    d = plan.depth[found]
    assert np.all((d == floor[found]) | (d == floor[found] + 1)) and np.all(plan.depth[~found] == 0)
    S, V = float(carry[found].sum()), float((carry[found] * (1 - carry[found])).sum())
    x_spec = int((d == floor[found] + 1).sum())
    text = ts.tsb_reference(np.random.RandomState(77), [gtf], [ab], mc)
    by_id = {}
    for l in text.split("\n"):
        if l.startswith("+"):
            _, depth, comment = l.split("\t")
            by_id[comment.split("tid=")[1].rstrip(";")] = int(depth)
    assert not any(k.startswith("none") for k in by_id)
    d_ref = np.array([by_id.get(t, 0) for t in ids])[found]                           # (the reference writes no row whose depth is 0)
    assert np.all((d_ref == floor[found]) | (d_ref == floor[found] + 1))
    x_ref = int((d_ref == floor[found] + 1).sum())
    print(f"S = {S:.1f}, sqrt(V) = {V ** 0.5:.1f}, X spec = {x_spec}, X reference = {x_ref}")
    assert abs(x_spec - S) <= 5 * V ** 0.5
    assert abs(x_ref - S) <= 5 * V ** 0.5
    assert abs(x_spec - x_ref) <= 5 * (2 * V) ** 0.5


def test_to_int_edges_give_no_molecule():
    """NaN, -1e300 and negative counts emit nothing; +1e300 is clamped to the int range in double first (the conversion is defined, the
    count is 2^31 - 1: by the count rule a positive count is a count)"""
    # c = +-1e300 exactly: the sum is (1e300 - 1e300) + 1 = 1
    c, carry, depth = ts.counts_spec(3, [1e300, -1e300, 1.0], [True] * 3, 1.0, 1)
    assert c.tolist() == [1e300, -1e300, 1.0] and depth.tolist() == [2**31 - 1, 0, 1]
    # a NaN tpm makes the sum, and with it every count, NaN
    c, carry, depth = ts.counts_spec(3, [float("nan"), 5.0], [True, True], 1.0, 10)
    assert np.isnan(c).all() and depth.tolist() == [0, 0]
    # negative tpm next to a positive sum
    c, carry, depth = ts.counts_spec(3, [-1e300, 2e300, -0.25, -5.0], [True] * 4, 1.0, 4)
    assert depth.tolist() == [0, 8, 0, 0]
    # infinities on the way: W x tpm overflows
    c, carry, depth = ts.counts_spec(3, [-1e300, 2e300], [True, True], 1e10, 4)
    assert depth.tolist() == [0, 2**31 - 1]
    # a sum that overflows: c = x / inf = 0
    c, carry, depth = ts.counts_spec(3, [1e308, 1e308], [True, True], 1.0, 2**31 - 1)
    assert depth.tolist() == [0, 0]
    # through the text: the generator writes no record for such rows
    for bad in ("-5", "-0.25", "-1e300"):
        plan = ts.tsb_spec(1, [GTF], [f"h\nT1 {bad} a\nT2 2e300 a\n"], 4)[0]
        assert plan.depth[0] == 0 and "tid=T1;" not in plan.mdf_text() and plan.records == 1, bad
    # "nan" and "inf" are not numbers to operator>>: tpm 0, and the barcode is not read
    assert ts.read_abundance("h\nT1 nan a\nT1 inf a\n") == [("T1", 0.0, ""), ("T1", 0.0, "")]
    assert ts.to_int([float("nan"), 1e300, -1e300, 2147483647.5, -2147483648.5, -0.9, 0.9]).tolist() == [0, 2**31 - 1, -2**31, 2**31 - 1, -2**31, 0, 0]


def test_slices_of_the_unrolled_molecules_equal_the_whole():
    rs = np.random.RandomState(8)
    ids = ["T1", "T2", "T3", "T5", "T7", "T9", "nope"]
    ab = "h\n" + "".join(f"{ids[int(rs.randint(len(ids)))]}\t{[0, 1, 1, 2.5, 7, 40][int(rs.randint(6))]}\tCB{k % 3}\n" for k in range(300))
    plan = ts.tsb_spec(4, [GTF], [ab], int(sum(float(l.split()[1]) for l in ab.split("\n")[1:-1])))[0]
    whole = plan.unrolled_text()
    assert whole.count("\n+") + 1 == plan.molecules and "_39\t1\t" in whole
    import mdf_ops_oracle as mo
    assert whole == mo.write_mdf(mo.stream_mdf(plan.mdf_text(), unroll=True))          # what a module reading the compact text writes
    for cuts in ([0, 1, 2, 50, 51, 777, plan.molecules], [0, plan.molecules - 1, plan.molecules, plan.molecules + 5]):
        assert "".join(plan.unrolled_text(a, b - a) for a, b in zip(cuts, cuts[1:])) == whole
    assert "".join(plan.mdf_text(k, 7) for k in range(0, plan.records, 7)) == plan.mdf_text()
    assert plan.unrolled_text(3, 4, comments=False).count("\t1\t\n") == 4


# ------------------------------------------------------------------------------------------------ exports and argument checks
def test_transcribe_symbols_are_exported():
    from tksm_amd import _lib
    lib = _lib.load()
    for s in ("tksmseq_transcripts_add_gtf", "tksmseq_transcripts_info", "tksmseq_transcripts_clear", "tksmseq_transcribe_plan_create",
              "tksmseq_transcribe_plan_clone", "tksmseq_transcribe_plan_info", "tksmseq_transcribe_plan_missing", "tksmseq_transcribe_plan_free",
              "tksmseq_transcribe", "tksmseq_transcribe_text", "tksmseq_transcribe_main"):
        assert s in _lib.SYMBOLS and hasattr(lib, s)
    from tksm_amd.sequence import Sequencer, TranscribePlan
    assert all(hasattr(Sequencer, m) for m in ("add_gtf", "transcribe_plan")) and all(hasattr(TranscribePlan, m) for m in ("batch", "mdf_text", "close"))


def test_tksm_transcribe_argument_checks(tmp_path):
    r = _cli("transcribe", "--help")
    assert r.returncode == 0 and "usage: transcribe" in r.stdout and "--fusion-gtf" in r.stdout and "not built" in r.stdout
    r = _cli("transcribe")
    assert r.returncode == 1
    for name in ("gtf", "abundance", "output", "molecule-count"):
        assert r.stderr.count(f"Missing mandatory parameter {name}\n") == 1
    assert "usage: transcribe" in r.stdout                                    # the help follows the missing parameters
    gtf, ab, out = os.path.join(D, "ann.gtf"), os.path.join(D, "abund_exact.tsv"), tmp_path / "o.mdf"
    r = _cli("transcribe", "-g", gtf, "-a", ab, "-o", out)
    assert r.returncode == 1 and r.stderr.count("Missing mandatory parameter") == 1 and "molecule-count" in r.stderr
    r = _cli("transcribe", "-g", gtf, "-a", tmp_path / "none.tsv", "-o", out, "--molecule-count", 60)
    assert r.returncode == 1 and f"Could not open abundance file {tmp_path / 'none.tsv'}!" in r.stderr
    r = _cli("transcribe", "-g", f"{gtf},{tmp_path / 'none.gtf'}", "-a", ab, "-o", out, "--molecule-count", 60)
    assert r.returncode == 1 and f"Could not open GTF file {tmp_path / 'none.gtf'}!" in r.stderr
    r = _cli("transcribe", "-g", gtf, "-a", f"{ab},{ab},{ab}", "-w", "1,2", "-o", out, "--molecule-count", 60)
    assert r.returncode == 1 and "one weight, or one per abundance file" in r.stderr
    for fusion in ("--fusion-gtf", "--fusion-file", "--fusion-output", "--fusion-count", "--disable-deletions", "--translocation-ratio", "--expression-fallback"):
        r = _cli("transcribe", "-g", gtf, "-a", ab, "-o", out, "--molecule-count", 60, fusion, "1")
        assert r.returncode == 1 and f"Option '{fusion}' does not exist" in r.stderr, fusion
    r = _cli("transcribe", "-g", gtf, "-a", ab, "-o", out, "--molecule-count", "many")
    assert r.returncode == 1 and "malformed" in r.stderr
    r = _cli("transcribe", "-g", gtf, "-a", ab, "-o", out, "--molecule-count", 60, "--batch-molecules", 0)
    assert r.returncode == 1 and "malformed" in r.stderr
    r = _cli("transcribe", "-g", gtf, "-a", ab, "-o", out, "--molecule-count", 60, "-i", "in.mdf")
    assert r.returncode == 1 and "does not exist" in r.stderr
    assert not out.exists()                                                    # nothing was opened before the checks were over


def test_chained_sequence_argument_checks(tmp_path):
    gtf, ab, out = os.path.join(D, "ann.gtf"), os.path.join(D, "abund_exact.tsv"), tmp_path / "o.fastq"
    tsb = ["--transcribe-gtf", gtf, "--transcribe-abundance", ab, "--transcribe-molecule-count", 60]
    r = _cli("sequence", "-r", "x.fa", *tsb, "-i", "in.mdf", "--perfect", out)
    assert r.returncode == 2 and "-i/--input" in r.stderr and "--transcribe-*" in r.stderr
    r = _cli("sequence", "-r", "x.fa", *tsb, "--perfect", out, "--wgs-frag-len-dist", "normal 100 10", "--wgs-depth", 1)
    assert r.returncode == 2 and "--transcribe-*" in r.stderr and "--wgs-*" in r.stderr
    r = _cli("sequence", "-r", "x.fa", *tsb, "--perfect", out, "--pcr-cycles", 3)
    assert r.returncode == 2 and "--transcribe-*" in r.stderr and "--pcr-*" in r.stderr
    r = _cli("sequence", "-r", "x.fa", *tsb, "--perfect", out, "--truncate-normal", "100,10")
    assert r.returncode == 2 and "--transcribe-*" in r.stderr and "--truncate-*" in r.stderr
    r = _cli("sequence", "-r", "x.fa", "--transcribe-use-whole-id", "--perfect", out)
    assert r.returncode == 1
    for name in ("gtf", "abundance", "molecule-count"):
        assert r.stderr.count(f"Missing mandatory parameter {name}\n") == 1
    r = _cli("sequence", "-r", "x.fa", *tsb[:4], "--perfect", out)
    assert r.returncode == 1 and r.stderr.count("Missing mandatory parameter") == 1 and "molecule-count" in r.stderr
    r = _cli("sequence", "-r", "x.fa", "--transcribe-gtf", gtf, "--transcribe-abundance", tmp_path / "none.tsv", "--transcribe-molecule-count", 60, "--perfect", out)
    assert r.returncode == 1 and f"Could not open abundance file {tmp_path / 'none.tsv'}!" in r.stderr
    r = _cli("sequence", "-r", "x.fa", "--transcribe-gtf", tmp_path / "none.gtf", "--transcribe-abundance", ab, "--transcribe-molecule-count", 60, "--perfect", out)
    assert r.returncode == 1 and f"Could not open GTF file {tmp_path / 'none.gtf'}!" in r.stderr
    r = _cli("sequence", "-r", "x.fa", *tsb, "--transcribe-weights", "1,2,3", "--perfect", out)
    assert r.returncode == 1 and "one weight, or one per abundance file" in r.stderr
    r = _cli("sequence", "-r", "x.fa", *tsb, "--transcribe-batch-molecules", 0, "--perfect", out)
    assert r.returncode == 2 and "--transcribe-batch-molecules" in r.stderr
    r = _cli("sequence", "-r", "x.fa", *tsb, "--transcribe-molecule-count", "many", "--perfect", out)
    assert r.returncode == 2 and "--transcribe-molecule-count" in r.stderr
    r = _cli("sequence", "-r", "x.fa", *tsb, "--transcribe-fusion-gtf", "f.gtf", "--perfect", out)
    assert r.returncode == 2 and "unrecognized arguments" in r.stderr
    # without any --transcribe-* option a missing -i is what it was, and the abbreviations the other tests use still resolve
    r = _cli("sequence", "-r", "x.fa", "--perfect", out)
    assert r.returncode == 2 and "the following arguments are required: -i/--input" in r.stderr
    r = _cli("sequence", "--inp", "missing.mdf", "--perf", out, "--badread-i", "90,99,3", "--th", 2)
    assert r.returncode == 1 and "ambiguous" not in r.stderr and "unrecognized" not in r.stderr
    assert not out.exists()
    r = _cli("sequence", "--help")
    assert r.returncode == 0 and "--transcribe-gtf" in r.stdout


def test_dispatcher_knows_transcribe_and_list_is_unchanged():
    r = _cli("list")
    assert r.returncode == 0 and r.stdout == "sequence\npcr\ntruncate\npolyA\ntag\nscb\nflip\n"
    r = _cli("no-such-module")
    assert r.returncode == 1 and "`transcribe`" in r.stderr
    r = _cli("transcribe", "-h")
    assert r.returncode == 0
