"""model-sequence on the device (tksmseq_model_sequence, `tksm model-sequence`, Sequencer.model_sequence) against the plain Python statement
of its rules (tests/model_seq_spec.py): the two model files byte for byte, the counters, the chunking, the cuts, and the built pair used
by the simulator.  Shapes: about 200 drawn alignments with the generator's planted classes, and (M.shape_cases) alignments of 1, 2, 63,
64, 65, 127, 128, 129, 192 and 193 ops, first passes of 64 ops with 64, 65, 127, 128 and 129 columns, single ops of 63 to 5 000 columns, a
deletion of 3 000 and an insertion of 300 columns as op 0, 1, 63 and 64, runs of max_del and max_del + 1 deletions behind a window of more
than 29 letters; 1 to 9 alignments in all, so that the last workgroup of four waves has idle ones."""
import gzip
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

import model_seq_spec as M

pytestmark = pytest.mark.gpu
EXE = os.path.join(ROOT, "tksm_amd", "tksm")
COUNTERS = ("lines", "used", "skipped_no_cigar", "skipped_supplementary", "skipped_unknown_read", "skipped_unknown_target", "skipped_cigar_op",
            "counting_positions", "alternatives_too_long", "windows_max_del", "keys_too_long", "read_positions", "error_keys", "qscore_keys")


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    """about 200 alignments of 60 to 400 columns, among them 63, 64 and 65 columns, one of 20 000 columns, a read of 65 lines, and every
    planted class of the generator; the specification's output at the defaults is computed once"""
    d = tmp_path_factory.mktemp("model_seq")
    g = M.generate(d, seed=11, n_alignments=200, long_columns=20000)
    g["dir"] = d
    g["spec"] = {}
    return g


def spec(g, **kw):
    key = tuple(sorted(kw.items()))
    if key not in g["spec"]:
        g["spec"][key] = M.run(g["reference"], g["reads"], g["alignment"], **kw)
    return g["spec"][key]


@pytest.fixture(scope="module")
def S(data):
    from tksm_amd.sequence import Sequencer
    s = Sequencer(0)
    s.get_reference_seqs([data["reference"]])
    yield s
    s.close()


def build(S, g, tmp_path, tag="m", **kw):
    e, q = tmp_path / f"{tag}.error", tmp_path / f"{tag}.qscore"
    info = S.model_sequence(g["reads"], g["alignment"], e, q, **kw)
    return e.read_text(), q.read_text(), info


def same_counters(info, want):
    assert {k: info[k] for k in COUNTERS} == {k: want[k] for k in COUNTERS}


@pytest.mark.parametrize("min_occur", [1, 100])
def test_both_files_equal_the_specification_at_the_defaults(S, data, tmp_path, min_occur):
    e, q, info = build(S, data, tmp_path, min_occur=min_occur)
    want = spec(data, min_occur=min_occur)
    assert e == want["error"]
    assert q == want["qscore"]
    same_counters(info, want["info"])
    # every class the generator plants occurred, and the counters saw the ones they count
    for what in ("strand_plus", "strand_minus", "ops_M", "ops_=X", "insertion_first_column", "insertion_last_column", "del_run_max_del",
                 "del_run_max_del_plus_1", "alternative_K_plus_4", "alternative_K_plus_5", "reference_N", "read_N", "lower_case", "alignment_of_K",
                 "alignment_of_K_minus_1", "ends_at_contig_end", "read_with_several_lines", "tp_A_S", "no_cigar", "unknown_read", "unknown_target"):
        assert data["classes"].get(what, 0) >= 1, what
    for k in ("skipped_no_cigar", "skipped_supplementary", "skipped_unknown_read", "skipped_unknown_target", "skipped_cigar_op", "alternatives_too_long",
              "windows_max_del", "keys_too_long"):
        assert info[k] >= 1, k
    assert info["chunks"] == 1 and info["device_ms"] > 0


def test_the_hand_counted_case(tmp_path):
    """tests/golden/model_seq_known_answers.json: the expected text there was written out by hand"""
    import test_model_sequence as T
    from tksm_amd.sequence import Sequencer
    p = T.write_known(tmp_path)
    s = Sequencer(0)
    try:
        s.get_reference_seqs([p["reference"]])
        info = s.model_sequence(p["reads"], p["alignment"], tmp_path / "e", tmp_path / "q", **T.KNOWN["params"])
    finally:
        s.close()
    assert (tmp_path / "e").read_text() == T.known_error_text() and (tmp_path / "q").read_text() == T.KNOWN["qscore"]
    assert {k: info[k] for k in T.KNOWN["info"]} == T.KNOWN["info"]


@pytest.mark.parametrize("k,kq", [(3, 1), (8, 29)])
def test_other_sizes(S, data, tmp_path, k, kq):
    e, q, info = build(S, data, tmp_path, error_k=k, qscore_k=kq, min_occur=1)
    want = spec(data, error_k=k, qscore_k=kq, min_occur=1)
    assert e == want["error"] and e.count("\n") == 4 ** k
    assert q == want["qscore"]
    same_counters(info, want["info"])


def test_chunking_changes_nothing_and_runs_repeat(S, data, tmp_path):
    one = build(S, data, tmp_path, "one", min_occur=1)
    many = build(S, data, tmp_path, "many", min_occur=1, chunk_events=1000)
    again = build(S, data, tmp_path, "again", min_occur=1, chunk_events=1000)
    assert one[2]["chunks"] == 1 and many[2]["chunks"] >= 10
    assert many[:2] == one[:2] and again[:2] == many[:2]
    same_counters(many[2], one[2])
    assert many[2]["events"] == one[2]["events"]


def test_max_alignments_cuts_inside_the_file(S, data, tmp_path):
    e, q, info = build(S, data, tmp_path, max_alignments=37, min_occur=1)
    want = spec(data, max_alignments=37, min_occur=1)
    assert info["used"] == 37 and info["lines"] < spec(data, min_occur=1)["info"]["lines"]
    assert e == want["error"] and q == want["qscore"]
    same_counters(info, want["info"])


# ------------------------------------------------------------------------------------------------ shapes of k_ms_expand
@pytest.fixture(scope="module")
def shapes(tmp_path_factory):
    """M.generate_shapes (what is in it: tests/test_model_sequence.py); the specification's outputs are computed once per parameter set"""
    d = tmp_path_factory.mktemp("model_seq_shapes")
    g = M.generate_shapes(d)
    g["dir"] = d
    g["spec"] = {}
    return g


@pytest.fixture(scope="module")
def SS(shapes):
    from tksm_amd.sequence import Sequencer
    s = Sequencer(0)
    s.get_reference_seqs([shapes["reference"]])
    yield s
    s.close()


@pytest.mark.parametrize("kw", [dict(), dict(error_k=3, qscore_k=1), dict(error_k=8, qscore_k=29)], ids=["defaults", "k3_kq1", "k8_kq29"])
def test_shapes_equal_the_specification(SS, shapes, tmp_path, kw):
    e, q, info = build(SS, shapes, tmp_path, min_occur=1, **kw)
    want = spec(shapes, min_occur=1, **kw)
    assert e == want["error"] and e.count("\n") == 4 ** kw.get("error_k", 7)
    assert q == want["qscore"]
    same_counters(info, want["info"])
    assert set(shapes["shape_reads"]) == set(M.shape_cases()) and info["used"] == 20 + (2 * 9 + 1 + 2) + 2 * 30       # drawn, planted, shapes
    if kw.get("qscore_k", 9) > 1:
        assert info["windows_max_del"] >= 6 * 20 and info["keys_too_long"] >= 1


def test_shapes_in_chunks_between_and_inside_alignments(SS, shapes, tmp_path):
    e, q, info = build(SS, shapes, tmp_path, min_occur=1, chunk_events=1000)
    want = spec(shapes, min_occur=1)
    assert info["chunks"] >= 20 and e == want["error"] and q == want["qscore"]
    same_counters(info, want["info"])


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 8, 9])
def test_small_numbers_of_alignments(SS, shapes, tmp_path, n):
    """four alignments per workgroup: the last one has 3, 2, 1 or no idle waves"""
    e, q, info = build(SS, shapes, tmp_path, min_occur=1, max_alignments=n)
    want = spec(shapes, min_occur=1, max_alignments=n)
    assert info["used"] == n and e == want["error"] and q == want["qscore"]
    same_counters(info, want["info"])


@pytest.mark.parametrize("max_output", [0, 2, 3, 5, 40])
def test_max_output_keeps_the_three_one_letter_keys(S, data, tmp_path, max_output):
    _, q, _ = build(S, data, tmp_path, min_occur=1, max_output=max_output)
    assert q == spec(data, min_occur=1, max_output=max_output)["qscore"]
    keys = [ln.split(";")[0] for ln in q.splitlines()[1:]]
    assert {"=", "X", "I"} <= set(keys) and len(keys) == max(3, max_output)
    # the cut alone would have dropped X and I: they are far from the most frequent keys
    full = [ln.split(";")[0] for ln in spec(data, min_occur=1)["qscore"].splitlines()[1:]]
    if max_output in (2, 3, 5):
        assert not {"X", "I"} <= set(full[:max_output])


def test_no_insertion_column_is_refused(tmp_path):
    from tksm_amd.sequence import Sequencer, TksmSeqError
    g = M.generate(tmp_path, seed=5, n_alignments=20, extra_columns=(), group=0, no_ins=True)
    assert isinstance(M.run(g["reference"], g["reads"], g["alignment"])["qscore"], ValueError)
    s = Sequencer(0)
    try:
        s.get_reference_seqs([g["reference"]])
        with pytest.raises(TksmSeqError) as err:
            s.model_sequence(g["reads"], g["alignment"], tmp_path / "e", tmp_path / "q")
        assert err.value.code == 1 and "'I'" in str(err.value)
        assert not (tmp_path / "q").exists()
        # the error model alone does not need the key
        s.model_sequence(g["reads"], g["alignment"], tmp_path / "e", None)
        assert (tmp_path / "e").read_text() == M.run(g["reference"], g["reads"], g["alignment"])["error"]
    finally:
        s.close()


def test_reads_list_with_an_empty_entry_and_the_loaders_messages(tmp_path):
    """the comma list of read files as the C-ABI takes it: "a.fq,,b.fq" is the one file with both; the loader's messages word for word"""
    from tksm_amd.sequence import Sequencer, TksmSeqError
    g = M.generate(tmp_path, seed=5, n_alignments=20, extra_columns=(), group=0)
    lines = open(g["reads"]).read().split("\n")
    half = 4 * (len(lines) // 8)
    (tmp_path / "a.fq").write_text("\n".join(lines[:half]) + "\n")
    (tmp_path / "b.fq").write_text("\n".join(lines[half:]))
    (tmp_path / "bad.fq").write_text("@r\nACGT\n+\nII\n")
    s = Sequencer(0)
    try:
        s.get_reference_seqs([g["reference"]])
        s.model_sequence(g["reads"], g["alignment"], tmp_path / "e1", tmp_path / "q1", min_occur=1)
        s.model_sequence([tmp_path / "a.fq", "", tmp_path / "b.fq"], g["alignment"], tmp_path / "e2", tmp_path / "q2", min_occur=1)
        want = M.run(g["reference"], g["reads"], g["alignment"], min_occur=1)
        assert (tmp_path / "e1").read_text() == want["error"] and (tmp_path / "q1").read_text() == want["qscore"]
        assert (tmp_path / "e2").read_bytes() == (tmp_path / "e1").read_bytes() and (tmp_path / "q2").read_bytes() == (tmp_path / "q1").read_bytes()
        with pytest.raises(TksmSeqError) as err:
            s.model_sequence([tmp_path / "a.fq", tmp_path / "bad.fq"], g["alignment"], tmp_path / "e3", tmp_path / "q3")
        assert err.value.code == 1 and str(err.value) == f"tksmseq error 1: {tmp_path / 'bad.fq'}: FASTQ record 1: sequence and quality differ in length"
        with pytest.raises(TksmSeqError) as err:
            s.model_sequence(g["reads"], g["alignment"], None, None)
        assert err.value.code == 1 and str(err.value) == "tksmseq error 1: model-sequence: neither an error-model nor a q-score-model output"
        assert not (tmp_path / "e3").exists() and not (tmp_path / "q3").exists()
    finally:
        s.close()


def test_built_models_drive_the_simulator_like_the_oracle(tmp_path, po):
    """the existing parity route on a new model file: 32 reads of 300 bases, records byte for byte.  The reads here carry single-base
    errors at 4 %: the simulator's loader holds at most 5 bases per slot of an alternative (models.cpp), which runs of insertions next to
    deletions exceed"""
    from tksm_amd.sequence import Sequencer
    data = M.generate(tmp_path / "in", seed=3, n_alignments=150, extra_columns=(), group=0, plant=False, p_err=0.04, max_run=1)
    s = Sequencer(0)
    try:
        s.get_reference_seqs([data["reference"]])
        e, q = tmp_path / "built.error.gz", tmp_path / "built.qscore.gz"
        s.model_sequence(data["reads"], data["alignment"], e, q, min_occur=20)
        s.set_identity(88.0, 99.0, 4.0)
        s.load_error_model(str(e))
        s.load_qscore_model(str(q))
        ref = M.read_fasta(data["reference"])
        rs = np.random.RandomState(2)
        mols = []
        for i in range(32):
            st = int(rs.randint(0, 5000))
            mols.append((f"m{i}", [(f"ctg{i % 3}", st, st + 300, "+-"[i % 2], "")]))
        text = "".join(f"+{m}\t1\t\n" + "".join(f"{c}\t{a}\t{b}\t{st}\t{md}\n" for c, a, b, st, md in ivs) for m, ivs in mols)
        recs = s.run(s.batch_from_mdf(text), target="badread", fastq=True, compute_qual=True, seed=4).records()
        ident = po.Identities(88.0, 4.0, 99.0)
        em, qm = po.ErrorModel(str(e)), po.QScoreModel(str(q))
        assert em.k == 7 and qm.kmer_size == 9
        for i, (mid, ivs) in enumerate(mols):
            want, _ = po.badread_record(True, 4, i, po.splice(ref, ivs), ident, em, qm, True, mid)
            assert recs[i] == want, f"record {i} differs from the oracle"
    finally:
        s.close()


def test_command_line(S, data, tmp_path):
    e, q, _ = build(S, data, tmp_path, min_occur=1)
    args = [EXE, "model-sequence", "--reference", data["reference"], "--reads", data["reads"], "--alignment", data["alignment"], "--min_occur", "1"]
    r = subprocess.run(args + ["--error-model", tmp_path / "c.error.gz", "--qscore-model", tmp_path / "c.qscore"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert gzip.open(tmp_path / "c.error.gz", "rt").read() == e and (tmp_path / "c.qscore").read_text() == q
    assert not list(tmp_path.glob("*.tmp"))
    r = subprocess.run(args[:7] + [tmp_path / "missing.paf", "--qscore-model", tmp_path / "d.qscore"], capture_output=True, text=True)
    assert r.returncode == 1 and "missing.paf" in r.stderr and not (tmp_path / "d.qscore").exists()


def test_python_counters_equal_the_specification(S, data, tmp_path):
    info = S.model_sequence(data["reads"], data["alignment"], tmp_path / "only.error", None, max_alt=3, max_del=2)
    want = spec(data, max_alt=3, max_del=2)
    same_counters(info, want["info"])
    assert (tmp_path / "only.error").read_text() == want["error"]
    assert info["events"] >= info["read_positions"] * 6 + info["counting_positions"]      # (9 + 1) / 2 + 1 slots per read position
    assert len(info["stage_ms"]) == 4 and not (tmp_path / "only.qscore").exists()
