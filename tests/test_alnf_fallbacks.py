"""The give-up branches of the fused aligner (k_alnf / aln_fused) and the code that receives the reads it hands on.

The parity tests hold the fall-back counters at zero, so on their inputs none of this runs.  Here crafted inputs (tests/alnf_cases.py)
take each branch; every GPU test asserts (a) through Sequencer.run_diagnostics(), the per-read status and the verbose per-reason
line that the branch WAS taken, and (b) that every record and the per-read statistics of the batch equal the CPU oracle's
(oracle/tksm_oracle.c through pyoracle) for the same (seed, read index).  The reference is never a second run of the library; the
TKSMSEQ_FORCE_SLOW=1 run and the neighbours' run are controls on top of it.  DESIGN.md lists the counts one MI355X run showed."""
import functools
import json
import os
import re

import numpy as np
import pytest

import alnf_cases as ac
from conftest import GOLDEN, ERR_MODEL

SEED = 5
# FailBit (csrc/kernels.h): the bits of fallback_reasons
FAIL_QUEUE, FAIL_NOROW, FAIL_SHIFT31, FAIL_SHIFT14, FAIL_END_CELL, FAIL_WALK = 1, 2, 8, 16, 32, 64

# "fast": every alignment job in the 14-row pass, the redo list behind it, k_loop (one lane per read) receives; "fast-small": the
# full-width pass alone, k_loopw (one wave per read) receives; "small-capped": the same with a pool of 64 rows, so that a round of more
# than 64 jobs leaves waves without rows (norow); "slow": the exact wave-wide kernel for every read (the control)
VARIANTS = {
    "fast": {"TKSMSEQ_FORCE_SLOW": "0", "TKSMSEQ_SMALL_ALN": "0", "TKSMSEQ_TAIL_CUT": "0", "TKSMSEQ_WAVE_LOOP": "0", "TKSMSEQ_TAIL_WAVE": "0"},
    "fast-small": {"TKSMSEQ_FORCE_SLOW": "0", "TKSMSEQ_TAIL_WAVE": "0"},
    "small-capped": {"TKSMSEQ_FORCE_SLOW": "0", "TKSMSEQ_TAIL_WAVE": "0", "TKSMSEQ_FULL_ROWS_CAP": "64"},
    "early": {"TKSMSEQ_FORCE_SLOW": "0", "TKSMSEQ_EARLY_TAIL": "8"},
    "slow": {"TKSMSEQ_FORCE_SLOW": "1"},
}
KNOBS = sorted({k for v in VARIANTS.values() for k in v} | {"TKSMSEQ_TAIL_WCAP", "TKSMSEQ_HBM_STATE_LEN"})
NP_IDENTITY = (84.0, 99.0, 5.5)


# ------------------------------------------------------------------------------------------------ shared, computed once
@pytest.fixture(scope="session")
def models(tmp_path_factory, po):
    """{"ins" / "del" / "np": (path of the error model, its oracle form, identity (mean, max, stdev))}"""
    d = tmp_path_factory.mktemp("alnf_models")
    out = {}
    for kind in ("ins", "del"):
        p = ac.write_model(d / f"{kind}.error.gz", kind)
        out[kind] = (p, po.ErrorModel(p), ac.IDENTITY[kind])
    out["np"] = (ERR_MODEL, po.ErrorModel(ERR_MODEL), NP_IDENTITY)
    return out


@functools.lru_cache(maxsize=None)
def _case(kind, n, length, crafted=True, positions=None):
    return ac.batch(kind, n, 7, length=length, crafted=crafted, positions=positions)


_ORACLE = {}


def oracle_batch(po, models, mk, ref, mols, seed, first, key, compute_q=True):
    """[(record, FragStats)] of the batch from the oracle; computed once per `key` and left unchanged"""
    key = (mk, seed, first, compute_q) + tuple(key)
    if key not in _ORACLE:
        _, em, (mean, mx, sd) = models[mk]
        ident, qm = po.Identities(mean, sd, mx), po.QScoreModel("random")
        _ORACLE[key] = [po.badread_record(True, seed, first + i, po.splice(ref, ivs), ident, em, qm, compute_q, mid)
                        for i, (mid, ivs) in enumerate(mols)]
    return _ORACLE[key]


def golden_batch(which, pos, n):
    """read `which` of tests/golden/unbanded_reads.json at position `pos` of n ordinary reads; first read index so that it keeps its own"""
    x = json.load(open(os.path.join(GOLDEN, "unbanded_reads.json")))[which]
    ref = ac.genome()
    rs = np.random.RandomState(3)
    mols = [ac.ordinary(rs, ref, i) for i in range(n)]
    mols[pos] = (f"mol_{x['index']}", [(x["sequence"], 0, len(x["sequence"]), "+", "")])
    return ref, mols, x["index"] - pos


class Context:
    """a library context under the knobs of `variant` (read when the context is created), with the case's reference and models"""

    def __init__(self, monkeypatch, variant, models, mk, ref):
        from tksm_amd.sequence import Sequencer
        for k in KNOBS:
            monkeypatch.delenv(k, raising=False)
        for k, v in VARIANTS[variant].items():
            monkeypatch.setenv(k, v)
        monkeypatch.setenv("TKSMSEQ_VERBOSE", "1")
        path, _, (mean, mx, sd) = models[mk]
        self.s = Sequencer(0)
        for c, v in ref.items():
            self.s.add_contig(c, v)
        self.s.set_identity(mean, mx, sd)
        self.s.load_error_model(path)
        self.s.load_qscore_model("random")

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.s.close()

    def run(self, capfd, mols, seed, first, compute_q=True):
        """-> (records, integer stats, float stats, diagnostics, the verbose text)"""
        capfd.readouterr()
        res = self.s.run(self.s.batch_from_mdf(ac.mdf_text(mols)), target="badread", fastq=True, compute_qual=compute_q, seed=seed,
                         first_read_index=first, collect_stats=True)
        err = capfd.readouterr().err
        ist, dst = res.stats()
        return res.records(), ist, dst, self.s.run_diagnostics(), err


def run_gpu(monkeypatch, capfd, variant, models, mk, ref, mols, seed, first, compute_q=True):
    with Context(monkeypatch, variant, models, mk, ref) as c:
        return c.run(capfd, mols, seed, first, compute_q)


def assert_equals_oracle(recs, ist, dst, want, only=None):
    """(b): every record and the per-read statistics equal the oracle's"""
    for i, (rec, st) in enumerate(want):
        if only is not None and i not in only:
            continue
        got = tuple(int(v) for v in ist[i, :7])
        exp = (st.n_draws, st.change_count, st.n_aligns, st.frag_len, st.new_len, st.start_trim, st.end_trim)
        assert got == exp, (i, got, exp)
        assert dst[i, 0] == st.errors, (i, dst[i, 0], st.errors)
        assert recs[i] == rec, i


def per_reason(err):
    """the per-reason counts of the LAST pass of the run in the verbose text (run.cpp: finish)"""
    m = re.findall(r"per reason: queue / reservoir overflow (\d+) no pool rows (\d+) - shift>31 (\d+) shift>14 (\d+) end cell (\d+) walk (\d+) \| q-score jobs (\d+), list pass (\d+)", err)
    assert m, err[-800:]
    return dict(zip(("queue", "norow", "shift31", "shift14", "end_cell", "walk", "qjobs", "list"), map(int, m[-1])))


def passes(err):
    """how many times the device ran the batch (a slot overflow makes the host run it again with larger slots)"""
    return len(re.findall(r"\[tksmseq\] reads \d+ rounds \d+ slow-path reads", err))


# ------------------------------------------------------------------------------------------------ CPU: the cases are what they claim
def test_generators_are_deterministic(tmp_path):
    for kind in ("ins", "del"):
        assert ac.model_lines(kind) == ac.model_lines(kind) and len(ac.model_lines(kind)) == 4 ** ac.K
    a, b = ac.batch("blocks60", 65, 7, length=600), ac.batch("blocks60", 65, 7, length=600)
    assert a == b and a[2] == [0, 31, 63, 64]
    assert ac.crafted_positions(1) == [0] and ac.crafted_positions(63) == [0, 31, 62] and ac.crafted_positions(129) == [0, 31, 63, 64, 128]
    # the neighbours are the same molecules with and without the crafted reads
    c = ac.batch("blocks60", 65, 7, length=600, crafted=False)
    assert [m[1] for i, m in enumerate(a[1]) if i not in a[2]] == [m[1] for i, m in enumerate(c[1]) if i not in a[2]]
    assert all(len(ivs) == 1 and ivs[0][0] == "chr1" for _, ivs in c[1])
    import gzip
    p1, p2 = ac.write_model(tmp_path / "a.gz", "del"), ac.write_model(tmp_path / "b.gz", "del")
    assert gzip.open(p1).read() == gzip.open(p2).read()


def test_models_load_in_the_oracle_and_spare_ordinary_kmers(models):
    for kind in ("ins", "del"):
        em = models[kind][1]
        assert em.k == ac.K and em.max_alts == (4 if kind == "ins" else 3)
    n_low = sum(ac.low_complexity(k) for k in ac._kmers())
    assert n_low == 4 + 6 * (2 ** ac.K - 2)         # homopolymers + two-base k-mers: 4.7 % of all


def test_oracle_end_cell_reads_fail_the_band(po, models):
    """the long polyA-tailed literals under the deletion model: a 1000-slot window that ends inside the deleted tail has its end cell
    outside the last column's 64 rows (oracle: band_fail, then full_align); so have the three recorded reads of the nanopore2020 run"""
    ref, mols, pos = _case("tail", 129, 1300)
    want = oracle_batch(po, models, "del", ref, mols, SEED, 0, ("tail", 129, 1300))
    assert all(want[i][1].band_fail > 0 for i in pos), [want[i][1].band_fail for i in pos]
    assert sum(want[i][1].band_fail for i in range(len(mols)) if i not in pos) == 0       # the neighbours are ordinary
    for which in range(3):
        ref, mols, first = golden_batch(which, 31, 65)
        want = oracle_batch(po, models, "np", ref, mols, 42, first, ("golden", which, 31, 65))
        assert [i for i, (_, st) in enumerate(want) if st.band_fail] == [31]


def test_oracle_overflow_reads_outgrow_the_default_slot(po, models):
    ref, mols, pos = _case("repeat", 65, 600)
    want = oracle_batch(po, models, "ins", ref, mols, SEED, 0, ("repeat", 65, 600))
    for i in pos:
        st = want[i][1]
        assert st.new_len > 1.5 * st.frag_len + 64, (i, st.new_len, st.frag_len)
        assert st.ins_bases > 0.6 * st.frag_len
    # the neighbours grow, but fit
    assert all(st.new_len <= 1.5 * st.frag_len + 64 for i, (_, st) in enumerate(want) if i not in pos)


@pytest.mark.parametrize("kind,length", [("blocks24", 600), ("blocks60", 600)])
def test_oracle_shift_reads_lose_their_blocks(po, models, kind, length):
    """the shift cases: at least half of a literal's slots end deleted (its low-complexity blocks, nearly whole), no more than 45 % of
    an ordinary neighbour's; none fails the band (a large shift in the middle of a window is nothing the specification gives up on)"""
    ref, mols, pos = _case(kind, 65, length)
    want = oracle_batch(po, models, "del", ref, mols, SEED, 0, (kind, 65, length))
    for i, (_, st) in enumerate(want):
        share = st.n_del / st.frag_len
        assert (share >= 0.5) if i in pos else (share <= 0.45), (i, share)
        assert st.band_fail == 0


# ------------------------------------------------------------------------------------------------ GPU: one test per branch
def band_exits_by_receiver(err):
    """(reads that k_loop / k_loopw sent to the exact kernel at res_fail, reads that k_err sent there for a failed q-score job) of the
    last pass -- "band exit a/b" of the verbose text"""
    m = re.findall(r"band exit (\d+)/(\d+)", err)
    assert m, err[-800:]
    return int(m[-1][0]), int(m[-1][1])


def assert_receiver(variant, diag, err):
    """what every fall-back of a regular run shows, whatever its reason: counted, handed to the exact kernel by a receiver"""
    loop_exits, err_exits = band_exits_by_receiver(err)
    assert diag["fallbacks"] > 0 and diag["band_exits"] > 0 and diag["exact_kernel_reads"] > 0
    assert diag["band_exits"] == loop_exits + err_exits
    if variant == "fast":                       # the 14-row pass ran, the redo list behind it
        assert diag["jobs_14_row_rounds"] > 0 and diag["jobs_redone_full_width"] > 0
    else:                                       # every job in the full-width pass
        assert diag["jobs_14_row_rounds"] == 0 and diag["jobs_redone_full_width"] == 0 and diag["fallbacks_list_pass"] == 0
        assert diag["jobs_all_rounds"] > 0
    return loop_exits, err_exits


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["fast", "fast-small"])
def test_queue_overflow_slot_overflow_and_failed_qscore_jobs(po, models, monkeypatch, capfd, variant):
    """insertion model on repeat literals.  `bad` (queue fill) in both passes; `ovf` -> job_overflow -> the host runs the batch again
    with larger slots; q-score jobs that fail reach k_err (EXIT_BAND_ERR); a following batch of ordinary reads on the same context
    (which overflows and fails again: the model spares no read) finds no state left behind."""
    ref, mols, pos = _case("repeat", 65, 600)
    want = oracle_batch(po, models, "ins", ref, mols, SEED, 0, ("repeat", 65, 600))
    _, ordinary, _ = _case("repeat", 65, 600, False)
    want_ord = oracle_batch(po, models, "ins", ref, ordinary, SEED, 300, ("repeat-ord", 65, 600))
    with Context(monkeypatch, variant, models, "ins", ref) as c:
        recs, ist, dst, diag, err = c.run(capfd, mols, SEED, 0)
        recs2, ist2, dst2, diag2, err2 = c.run(capfd, ordinary, SEED, 300)
    print(variant, diag, per_reason(err), "passes", passes(err), "| following batch", diag2, "passes", passes(err2))
    assert passes(err) == 2                                     # ovf: the rerun
    loop_exits, err_exits = assert_receiver(variant, diag, err)
    assert diag["fallback_reasons"] & FAIL_QUEUE and per_reason(err)["queue"] > 0
    assert diag["fallbacks_qscore_jobs"] > 0 and err_exits > 0    # k_err received failed q-score jobs
    assert loop_exits > 0
    if variant == "fast":
        assert diag["fallbacks_list_pass"] > 0                    # ... and the redo list's pass gave up on some
    assert_equals_oracle(recs, ist, dst, want)
    assert_equals_oracle(recs2, ist2, dst2, want_ord)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["blocks24", "blocks60"])
@pytest.mark.parametrize("variant", ["fast", "fast-small"])
def test_window_shifts_above_14_and_above_31_rows(po, models, monkeypatch, capfd, variant, kind):
    """deletion model on block literals: a deleted block moves the window by more rows than a 14-row entry holds (redo list) and by
    more than the 64-row pass can shift its planes (exact kernel).  The oracle does not fail its band on these: status bit 16 stays
    clear, the reads still leave through the fall-back."""
    ref, mols, pos = _case(kind, 65, 600)
    want = oracle_batch(po, models, "del", ref, mols, SEED, 0, (kind, 65, 600))
    recs, ist, dst, diag, err = run_gpu(monkeypatch, capfd, variant, models, "del", ref, mols, SEED, 0)
    print(variant, kind, diag, per_reason(err))
    loop_exits, _ = assert_receiver(variant, diag, err)
    assert loop_exits > 0
    assert diag["fallback_reasons"] & FAIL_SHIFT14 and diag["fallback_reasons"] & FAIL_SHIFT31
    why = per_reason(err)
    assert why["shift14"] > 0 and why["shift31"] > 0
    if variant == "fast":
        assert diag["fallbacks_list_pass"] > 0 and why["list"] > 0
        if kind == "blocks60":          # a job that gave up in the 14-row pass itself with rows to redo: the walk / redo bit
            assert diag["fallback_reasons"] & FAIL_WALK and diag["fallback_reasons"] & FAIL_QUEUE
    assert not (ist[:, 7] & 16).any()
    assert_equals_oracle(recs, ist, dst, want)


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["fast", "fast-small"])
def test_end_cell_outside_the_band(po, models, monkeypatch, capfd, variant):
    """long polyA-tailed literals, deletion model, 129 reads: the end cell of a window lies outside its last column's rows.  The
    oracle fails its band on exactly these reads, and the run says so per read (status bit 16)."""
    ref, mols, pos = _case("tail", 129, 1300)
    want = oracle_batch(po, models, "del", ref, mols, SEED, 0, ("tail", 129, 1300))
    recs, ist, dst, diag, err = run_gpu(monkeypatch, capfd, variant, models, "del", ref, mols, SEED, 0)
    print(variant, diag, per_reason(err))
    assert assert_receiver(variant, diag, err)[0] > 0             # k_loop / k_loopw at res_fail
    assert diag["fallback_reasons"] & FAIL_END_CELL and per_reason(err)["end_cell"] > 0
    assert [i for i in range(len(mols)) if ist[i, 7] & 16] == [i for i, (_, st) in enumerate(want) if st.band_fail] == pos
    assert_equals_oracle(recs, ist, dst, want)


@pytest.mark.gpu
@pytest.mark.parametrize("which", [0, 1, 2])
@pytest.mark.parametrize("variant", ["fast", "fast-small"])
def test_recorded_unbanded_reads_among_neighbours(po, models, monkeypatch, capfd, variant, which):
    """the reads of tests/golden/unbanded_reads.json (shipped nanopore2020 model) at lane 31 of 65 ordinary reads"""
    ref, mols, first = golden_batch(which, 31, 65)
    want = oracle_batch(po, models, "np", ref, mols, 42, first, ("golden", which, 31, 65))
    recs, ist, dst, diag, err = run_gpu(monkeypatch, capfd, variant, models, "np", ref, mols, 42, first)
    print(variant, which, diag, per_reason(err))
    assert assert_receiver(variant, diag, err)[0] > 0             # k_loop / k_loopw at res_fail
    assert diag["fallback_reasons"] & FAIL_END_CELL and per_reason(err)["end_cell"] > 0
    assert [i for i in range(len(mols)) if ist[i, 7] & 16] == [31]
    assert_equals_oracle(recs, ist, dst, want)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 63, 64, 65, 129])
@pytest.mark.parametrize("variant", ["fast", "fast-small"])
def test_neighbours_of_a_lane_that_gives_up(po, models, monkeypatch, capfd, variant, n):
    """block literals at positions 0, 31, 63, 64 and last of batches of 1, 63, 64, 65 and 129 reads.  A lane that gives up, drains or
    is idle changes nothing in the jobs beside it nor in the wave-uniform loop control: every read equals the oracle, and the
    ordinary reads equal, byte for byte, those of a run in which ordinary reads stand where the literals stood (same read indices)."""
    ref, mols, pos = _case("blocks60", n, 600)
    want = oracle_batch(po, models, "del", ref, mols, SEED, 0, ("blocks60", n, 600))
    recs, ist, dst, diag, err = run_gpu(monkeypatch, capfd, variant, models, "del", ref, mols, SEED, 0)
    print(variant, n, diag, per_reason(err))
    assert pos == ac.crafted_positions(n)
    assert diag["fallbacks"] > 0 and diag["band_exits"] > 0 and diag["exact_kernel_reads"] > 0
    assert band_exits_by_receiver(err)[0] > 0
    assert diag["fallback_reasons"] & FAIL_SHIFT31
    assert_equals_oracle(recs, ist, dst, want)
    if n > 1:
        _, ctl, _ = _case("blocks60", n, 600, False)
        recs_c, ist_c, dst_c, _, _ = run_gpu(monkeypatch, capfd, variant, models, "del", ref, ctl, SEED, 0)
        for i in range(n):
            if i not in pos:
                assert recs_c[i] == recs[i] and (ist_c[i] == ist[i]).all() and (dst_c[i] == dst[i]).all(), i


@pytest.mark.gpu
@pytest.mark.parametrize("kind,n,length", [("blocks60", 65, 600), ("tail", 129, 1300)])
@pytest.mark.parametrize("variant", ["fast", "fast-small"])
def test_loop_receivers_alone_without_qscore_jobs(po, models, monkeypatch, capfd, variant, kind, n, length):
    """the same batches without q-scores.  With them, a read whose failed alignment a receiver in the error loop overlooked would still
    be caught when its q-score job fails in turn (k_err sends it to the exact kernel, which starts the read afresh); without them there
    is no second chance: the bytes are right only if k_loop ("fast") or k_loopw ("fast-small") handed the read over at res_fail."""
    ref, mols, pos = _case(kind, n, length)
    want = oracle_batch(po, models, "del", ref, mols, SEED, 0, (kind, n, length), compute_q=False)
    recs, ist, dst, diag, err = run_gpu(monkeypatch, capfd, variant, models, "del", ref, mols, SEED, 0, compute_q=False)
    print(variant, kind, diag, per_reason(err))
    loop_exits, err_exits = assert_receiver(variant, diag, err)
    assert loop_exits > 0 and err_exits == 0 and diag["fallbacks_qscore_jobs"] == 0
    assert diag["fallback_reasons"] & (FAIL_SHIFT31 if kind == "blocks60" else FAIL_END_CELL)
    assert_equals_oracle(recs, ist, dst, want)


@pytest.mark.gpu
@pytest.mark.parametrize("mk,kind,n,length", [("ins", "repeat", 65, 600), ("del", "blocks60", 65, 600), ("del", "tail", 129, 1300)])
def test_exact_kernel_for_every_read_is_the_control(po, models, monkeypatch, capfd, mk, kind, n, length):
    """TKSMSEQ_FORCE_SLOW=1 on the same batches: no rounds, no fall-backs, the same bytes"""
    ref, mols, pos = _case(kind, n, length)
    want = oracle_batch(po, models, mk, ref, mols, SEED, 0, (kind, n, length))
    recs, ist, dst, diag, err = run_gpu(monkeypatch, capfd, "slow", models, mk, ref, mols, SEED, 0)
    assert diag["rounds"] == 0 and diag["fallbacks"] == 0 and diag["jobs_all_rounds"] == 0
    assert_equals_oracle(recs, ist, dst, want)


@pytest.mark.gpu
def test_predicted_stragglers_that_fail_their_band_pass_through_the_early_slow_list(po, models, monkeypatch, capfd):
    """TKSMSEQ_EARLY_TAIL=8, 160 reads: the five polyA-tailed literals are six times as long as the median read, so they -- and no
    neighbour -- are the predicted stragglers, whose waves run beside the rounds.  Those whose band fails (the oracle says which) hand
    themselves to the exact kernel through the early reads' own slow list and k_merge_early_slow."""
    pos = (0, 31, 63, 64, 159)
    ref, mols, _ = _case("tail", 160, 2400, True, pos)
    want = oracle_batch(po, models, "del", ref, mols, SEED, 0, ("tail", 160, 2400, pos))
    failing = [i for i, (_, st) in enumerate(want) if st.band_fail]
    assert failing and set(failing) <= set(pos)
    recs, ist, dst, diag, err = run_gpu(monkeypatch, capfd, "early", models, "del", ref, mols, SEED, 0)
    print(diag, per_reason(err), failing)
    assert diag["predicted_stragglers"] == len(pos)
    assert diag["exact_kernel_reads"] >= len(failing) and diag["band_exits"] >= len(failing)
    # (k_merge_early_slow adds the reads of the early slow list to the loop receivers' count, not to k_err's)
    assert band_exits_by_receiver(err)[0] >= len(failing)
    assert [i for i in range(len(mols)) if ist[i, 7] & 16] == failing
    assert_equals_oracle(recs, ist, dst, want)


def long_ordinary(n, base_len):
    """n reads of the random genome, base_len + 10 i bases each"""
    ref = ac.genome()
    rs = np.random.RandomState(17)
    mols = []
    for i in range(n):
        st = int(rs.randint(0, len(ref["chr1"]) - base_len - 10 * n))
        mols.append((f"long{i}", [("chr1", st, st + base_len + 10 * i, "+-"[i & 1], "")]))
    return ref, mols


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["ordinary", "blocks60"])
def test_long_qscore_jobs_go_straight_to_the_redo_list(po, models, monkeypatch, capfd, case):
    """q-score jobs above 3000 slots skip the 14-row pass (straight_to_list) and are aligned by the redo list's pass.  "ordinary": eight
    reads of 3200 - 3270 bases, shipped model: every read has one such job, so at least eight jobs are redone (a 1000-slot window of the
    error loop is redone in about 2 % of the cases).  "blocks60": 3300-base block literals among short reads, deletion model: the list
    pass gives up on them (shift above 31 rows) and k_loop hands them on."""
    if case == "ordinary":
        mk, (ref, mols) = "np", long_ordinary(8, 3200)
    else:
        mk, (ref, mols, _) = "del", _case("blocks60", 8, 3300, True, (0, 3, 7))
    want = oracle_batch(po, models, mk, ref, mols, SEED, 0, ("long", case))
    recs, ist, dst, diag, err = run_gpu(monkeypatch, capfd, "fast", models, mk, ref, mols, SEED, 0)
    print(case, diag, per_reason(err))
    assert diag["jobs_14_row_rounds"] > 0
    if case == "ordinary":
        assert all(st.frag_len > 3000 for _, st in want)
        assert diag["jobs_redone_full_width"] >= len(mols)
    else:
        assert diag["jobs_redone_full_width"] > 0 and diag["fallbacks_list_pass"] > 0 and per_reason(err)["list"] > 0
        assert diag["fallback_reasons"] & FAIL_SHIFT31 and band_exits_by_receiver(err)[0] > 0
    assert_equals_oracle(recs, ist, dst, want)


@pytest.mark.gpu
@pytest.mark.parametrize("mk,kind,n", [("np", "ordinary", 129), ("del", "blocks60", 129), ("np", "ordinary", 64)])
def test_full_width_pool_without_rows_for_a_wave(po, models, monkeypatch, capfd, mk, kind, n):
    """norow.  TKSMSEQ_FULL_ROWS_CAP=64 leaves the full-width pass a pool of 64 rows while rounds of up to small_aln jobs still align
    at full width: in a round of 129 jobs at most one wave finds rows, the jobs of the others are counted as fall-backs with the
    reason bit of their own, k_loopw (k_err for a q-score job) hands their reads to the exact kernel, and every record is the oracle's.
    64 reads: every round fits the pool, the branch is not taken."""
    if kind == "ordinary":
        ref = ac.genome()
        rs = np.random.RandomState(23)
        mols = [ac.ordinary(rs, ref, i) for i in range(n)]
    else:
        ref, mols, _ = _case(kind, n, 600)
    want = oracle_batch(po, models, mk, ref, mols, SEED, 0, ("norow", kind, n))
    recs, ist, dst, diag, err = run_gpu(monkeypatch, capfd, "small-capped", models, mk, ref, mols, SEED, 0)
    why = per_reason(err)
    print(mk, kind, n, diag, why, band_exits_by_receiver(err))
    assert diag["jobs_14_row_rounds"] == 0 and diag["jobs_all_rounds"] > 0
    if n > 64:
        loop_exits, _ = assert_receiver("small-capped", diag, err)
        assert loop_exits > 0
        assert diag["fallback_reasons"] & FAIL_NOROW and why["norow"] > 0
    else:
        assert not diag["fallback_reasons"] & FAIL_NOROW and why["norow"] == 0
    assert_equals_oracle(recs, ist, dst, want)
