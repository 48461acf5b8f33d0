"""The fused aligner's forward loop at its register budget (k_alnf / aln_fused, csrc/kernels.hip): the slot codes of the next pass fetched in
mid-pass, half of them into the registers of the current pass's, the code lines stored a 16-byte piece at a time.  The cases are those of
tests/alnf_budget_spec.py and the drain-pass builders of tests/alnf_cases.py; every record of every case is compared with the CPU oracle, byte
for byte, the way tests/test_gpu_parity.py compares -- with the 14-row pass forced on (the route of a bench-size batch) and on the route a small
batch takes by itself, with the q-score round and without it, on a fresh context, on a context whose device buffers hold the data of an earlier
run of other, longer molecules, and once more (both ways) in a child process in which every byte of device memory that a buffer was not given
to keep reads as TKSMSEQ_POISON=00000001 (ctx.h; tests/test_init_images_gpu.py).  None of the ordinary cases may fall back to the exact kernel."""
import json
import os
import re
import subprocess
import sys

import pytest

import alnf_budget_spec as S
import alnf_cases as ac

DRIVER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "alnf_budget_spec.py")
POISON = "00000001"
CHILD_SECONDS = 60                          # (the in-process passes of all cases take a few seconds; every allocation waits for the device in this mode)
HIP_TROUBLE = re.compile(r"illegal memory access|Memory access fault|HSA_STATUS_ERROR|hipError|HIP error", re.I)
_ran = {}


def _device(name, route, qual, how):
    """the case's run, once"""
    key = (name, route, qual, how)
    if key not in _ran:
        _ran[key] = S.run_route(name, route, qual, how == "recycled")
    return _ran[key]


def _round16(x):
    return (x + 15) // 16 * 16


# ------------------------------------------------------------------------------------------------ CPU: the cases are what they claim
def test_the_shapes_are_the_boundaries_of_the_forward_loop(oracle_models):
    assert oracle_models["em"].k == S.K
    for name, want_l in (("windows", S.WINDOW_L), ("windows_low", [L for L in S.WINDOW_L if L >= 63]), ("random", S.RANDOM_L)):
        frag = [st.frag_len for _, st in S.oracle_records(name)]
        assert set(frag) == set(want_l), name
    assert min(S.WINDOW_L) == 1 + 2 * S.K and max(S.WINDOW_L) == S.WINDOW
    for m in (16, 32, 48, 64, 96, 128):                                  # pass boundary, reservoir refill, plane-word step
        assert {m - 1, m, m + 1} <= set(S.WINDOW_L)
    assert {999, 1000} <= set(S.WINDOW_L)                                # 999: the last line's final entry stays empty
    assert set(range(1001, 1101)) <= set(S.RANDOM_L) and sum(1500 <= L <= 1800 for L in S.RANDOM_L) >= 10
    assert [len(S.CASES[f"partial{n}"]()) for n in S.PARTIAL] == [1, 63, 64, 65]
    assert sum(len(c()) for c in S.CASES.values()) < 3000
    # the oracle never leaves its band on these reads.  With q-scores every read has one job over its whole fragment; the error loop aligns a
    # fragment with every 25th change: each of the long ones, each from 63 slots on at the low identity, none of the shortest at the default one
    for name in S.CASES:
        for q in (True, False):
            assert all(st.band_fail == 0 for _, st in S.oracle_records(name, q)), name
    assert all(st.n_aligns >= 1 for _, st in S.oracle_records("windows_low") + S.oracle_records("random"))
    assert all(st.n_aligns == 0 for _, st in S.oracle_records("windows") if st.frag_len <= 49)


def test_random_windows_start_at_odd_and_at_even_slots():
    """the slot codes are fetched from the even position at or below the window's first slot: `skip` is 0 and 1"""
    starts = S.window_starts("random")
    odd = sum(p & 1 for p in starts)
    print(f"random windows: {len(starts)}, {odd} from an odd slot")
    assert len(starts) >= 500 and odd >= 100 and len(starts) - odd >= 100
    assert S.window_starts("windows") == []                              # whole-fragment windows only


# ------------------------------------------------------------------------------------------------ GPU
@pytest.mark.gpu
@pytest.mark.parametrize("how", ["fresh", "recycled"])
@pytest.mark.parametrize("qual", [True, False], ids=["qscores", "no-qscores"])
@pytest.mark.parametrize("route", list(S.ROUTES))
@pytest.mark.parametrize("name", list(S.CASES))
def test_records_and_statistics_equal_the_oracle(name, route, qual, how):
    recs, ist, diag = _device(name, route, qual, how)
    want = S.oracle_records(name, qual)
    mols = S.CASES[name]()
    assert len(recs) == len(want) == len(mols)
    for i, (mid, _) in enumerate(mols):                                  # every read: none skipped, none sampled
        rec, st = want[i]
        got_stats = tuple(int(ist[i, j]) for j in range(7))
        assert got_stats == (st.n_draws, st.change_count, st.n_aligns, st.frag_len, st.new_len, st.start_trim, st.end_trim), (name, route, qual, how, i, mid)
        assert recs[i] == rec, (name, route, qual, how, i, mid)
    print(f"{name} {route} qscores={qual} {how}: {len(recs)} records, diagnostics {diag}")
    # as for the molecules of the same shapes in tests/test_init_images_gpu.py: none leaves the fast pipeline
    assert diag["exact_kernel_reads"] == 0 and diag["band_exits"] == 0 and diag["fallbacks"] == 0 and diag["fallback_reasons"] == 0, diag
    if route == "rows14":
        assert diag["jobs_14_row_rounds"] > 0, diag
    else:
        assert diag["jobs_14_row_rounds"] == 0 and diag["jobs_redone_full_width"] == 0, diag


@pytest.mark.gpu
@pytest.mark.parametrize("qual", [True, False], ids=["qscores", "no-qscores"])
def test_the_redone_jobs_land_on_the_full_width_list(qual):
    """14 stored rows miss about 2 % of the 1000-slot windows: those jobs are appended to the redo list and aligned again with all rows"""
    diag = _device("random", "rows14", qual, "fresh")[2]
    loop_jobs = sum(st.n_aligns for _, st in S.oracle_records("random", qual))
    jobs = diag["jobs_14_row_rounds"]
    print(f"random, 14-row pass: {jobs} jobs ({loop_jobs} re-estimations by the oracle's count), {diag['jobs_redone_full_width']} redone")
    assert jobs == diag["jobs_all_rounds"] and jobs >= loop_jobs >= 500, diag
    assert 0.005 * jobs <= diag["jobs_redone_full_width"] <= 0.06 * jobs, diag


@pytest.mark.gpu
def test_recycled_buffers_give_the_fresh_bytes_and_diagnostics():
    for name in S.CASES:
        for route in S.ROUTES:
            for qual in (True, False):
                fresh, rec = _device(name, route, qual, "fresh"), _device(name, route, qual, "recycled")
                assert fresh[0] == rec[0] and fresh[2] == rec[2], (name, route, qual)


@pytest.fixture(scope="module")
def crafted_models(tmp_path_factory, po):
    d = tmp_path_factory.mktemp("alnf_budget_models")
    return {kind: (ac.write_model(d / f"{kind}.error.gz", kind), ac.IDENTITY[kind]) for kind in ("ins", "del")}


def _crafted(po, crafted_models, mk, kind, n, length, qual):
    """(oracle's [(record, FragStats)], device's (records, statistics, diagnostics)) of a batch of tests/alnf_cases.py, 14-row pass forced on"""
    ref, mols, pos = ac.batch(kind, n, 7, length=length)
    path, (mean, mx, sd) = crafted_models[mk]
    em, qm, ident = po.ErrorModel(path), po.QScoreModel("random"), po.Identities(mean, sd, mx)
    want = [po.badread_record(True, S.SEED, i, po.splice(ref, ivs), ident, em, qm, qual, mid) for i, (mid, ivs) in enumerate(mols)]
    s = S.sequencer(S.ROUTES["rows14"], ref=ref, err=path, qs="random", identity=(mean, mx, sd))
    try:
        got = S.run_case(s, mols, qual, seed=S.SEED, first=0)
    finally:
        s.close()
    return want, got, pos


def _assert_crafted(want, got):
    recs, ist, _ = got
    assert len(recs) == len(want)
    for i, (rec, st) in enumerate(want):
        got_stats = tuple(int(ist[i, j]) for j in range(7))
        assert got_stats == (st.n_draws, st.change_count, st.n_aligns, st.frag_len, st.new_len, st.start_trim, st.end_trim), i
        assert recs[i] == rec, i


@pytest.mark.gpu
def test_drain_passes_in_mid_window_and_after_the_last_slot(po, crafted_models):
    """insertion-heavy literals (tests/alnf_cases.py, "repeat" under the insertion model) among ordinary reads.  A lane pops one column per
    iteration and a wave runs round16(its longest window) iterations with slots; the q-score job of a literal has its whole new sequence for
    columns.  A pass pushes at most 16 x 5 columns, and without a drain pass in mid-window the backlog in front of the last pass is at most
    BACKLOG_DRAIN = 20: a job with more than round16(slots) + 100 columns had a drain pass before its wave's last slot, and one with more
    columns than iterations with slots had one behind it.  Drain passes fetch no slot codes; the codes in flight must survive them."""
    want, got, pos = _crafted(po, crafted_models, "ins", "repeat", 65, 600, True)
    lmax = max(st.frag_len for _, st in want)
    grown = [i for i, (_, st) in enumerate(want) if st.new_len > _round16(lmax + 1) + 100]
    print(f"longest window {lmax} slots; columns of the literals {[want[i][1].new_len for i in pos]}; diagnostics {got[2]}")
    assert set(pos) <= set(grown)
    assert got[2]["jobs_14_row_rounds"] > 0
    _assert_crafted(want, got)


@pytest.mark.gpu
@pytest.mark.parametrize("qual", [True, False], ids=["qscores", "no-qscores"])
def test_windows_that_end_in_a_deleted_tail(po, crafted_models, qual):
    """polyA-tailed literals under the deletion model, 129 reads (two full waves and a lane): the last slots of a window push no column at all,
    its end cell leaves the last column's rows, and the reads go to the exact kernel -- as they do in tests/test_alnf_fallbacks.py, whose counts
    for this batch are above zero as well"""
    want, got, pos = _crafted(po, crafted_models, "del", "tail", 129, 1300, qual)
    print(f"diagnostics {got[2]}")
    assert all(want[i][1].band_fail > 0 for i in pos)
    assert got[2]["jobs_14_row_rounds"] > 0 and got[2]["band_exits"] >= len(pos)
    _assert_crafted(want, got)


@pytest.mark.gpu
def test_poisoned_memory_gives_the_same_bytes(tmp_path):
    """a piece stored earlier, or codes fetched later, read nothing this run did not write"""
    env = dict(os.environ, TKSMSEQ_POISON=POISON)
    r = subprocess.run(["timeout", "-k", "10", str(CHILD_SECONDS), sys.executable, DRIVER, "--out", str(tmp_path)], capture_output=True, text=True,
                       env=env, timeout=CHILD_SECONDS + 30)
    trouble = HIP_TROUBLE.search(r.stderr)
    assert r.returncode == 0 and not trouble, f"exit status {r.returncode}\n--- stdout\n{r.stdout[-2000:]}\n--- stderr\n{r.stderr[-4000:]}"
    filled = [(int(b), int(n)) for b, n in re.findall(rf"^poison {POISON}: (\d+) blocks, (\d+) bytes$", r.stderr, re.M)]
    print(f"poisoned child: {len(filled)} contexts, {sum(b for b, _ in filled)} blocks, {sum(n for _, n in filled)} bytes")
    assert len(filled) == 2 * len(S.CASES) and all(b > 0 and n > 0 for b, n in filled), r.stderr[-2000:]
    for name in S.CASES:
        want = b"".join(rec for rec, _ in S.oracle_records(name))
        for how in ("fresh", "recycled"):
            with open(os.path.join(str(tmp_path), f"{name}.{how}.bin"), "rb") as f:
                assert f.read() == want, (name, how)
        with open(os.path.join(str(tmp_path), f"{name}.diag.json")) as f:
            assert json.load(f) == _device(name, "rows14", True, "fresh")[2], name
