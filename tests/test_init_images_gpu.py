"""k_init's one-pass fragment images, k_err without the fragment bytes, the straggler kernel's window from the packed words, and
state rows that the host does not clear (-m gpu).  The cases are those of tests/init_images_spec.py; every record of every case is
compared with the CPU oracle, byte for byte, the way tests/test_gpu_parity.py compares -- on a fresh context, on a context whose device
buffers hold the data of an earlier run of other, longer molecules, and once more (both ways) in a child process in which every byte of
device memory that a buffer was not given to keep reads as TKSMSEQ_POISON=00000001 (ctx.h; tests/test_history_gpu.py)."""
import json
import os
import re
import subprocess
import sys

import pytest

import init_images_spec as S

pytestmark = pytest.mark.gpu
DRIVER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "init_images_spec.py")
POISON = "00000001"
CHILD_SECONDS = 60                          # (the in-process passes of all cases take a few seconds; every allocation waits for the device in this mode)
HIP_TROUBLE = re.compile(r"illegal memory access|Memory access fault|HSA_STATUS_ERROR|hipError|HIP error", re.I)
_ran = {}


def _device(name):
    """run_both of the case, once"""
    if name not in _ran:
        _ran[name] = S.run_both(name)
    return _ran[name]


def test_the_model_has_the_k_the_lengths_were_chosen_for(oracle_models):
    assert oracle_models["em"].k == S.K
    frag = {raw + 2 * S.K for raw in S.edge_lengths()}
    for m in (16, 64, 128, 1024):
        assert {m - 1, m, m + 1} <= frag
    assert {1 + 2 * S.K, 1000, 1001} <= frag and {1000, 1001} <= set(S.edge_lengths())


@pytest.mark.parametrize("how", ["fresh", "recycled"])
@pytest.mark.parametrize("name", list(S.CASES))
def test_records_and_statistics_equal_the_oracle(name, how):
    recs, ist, diag = _device(name)[how]
    want = S.oracle_records(name)
    mols = S.CASES[name]()
    assert len(recs) == len(want) == len(mols)
    for i, (mid, _) in enumerate(mols):
        rec, st = want[i]
        assert st.band_fail == 0
        got_stats = tuple(int(ist[i, j]) for j in range(7))
        assert got_stats == (st.n_draws, st.change_count, st.n_aligns, st.frag_len, st.new_len, st.start_trim, st.end_trim), (name, how, i, mid)
        assert recs[i] == rec, (name, how, i, mid)
    print(f"{name} {how}: {len(recs)} records, diagnostics {diag}")
    # none of these molecules leaves the fast pipeline but those with an N, which never enter it
    n_exact = sum(mid in S.N_MOLECULES for mid, _ in mols) if name == "segments" else 0
    assert diag["exact_kernel_reads"] == n_exact and diag["band_exits"] == 0 and diag["fallbacks"] == 0, diag


def test_recycled_buffers_give_the_fresh_bytes_and_diagnostics():
    for name in S.CASES:
        got = _device(name)
        assert got["fresh"][0] == got["recycled"][0], name
        assert got["fresh"][2] == got["recycled"][2], name


def test_the_straggler_kernel_took_the_small_batch_over():
    """after round 0 the whole batch fits the straggler kernel (ctx.h tail_wave): round 1 runs every remaining visit of every read, alignments
    included, then come the q-score round and the last visits -- whereas a read's regular visits are a round each"""
    recs, ist, diag = _device("stragglers")["fresh"]
    most = max(st.n_aligns for _, st in S.oracle_records("stragglers"))
    frag = [st.frag_len for _, st in S.oracle_records("stragglers")]
    print(f"stragglers: rounds {diag['rounds']}, most re-estimations of a read {most}, fragments {frag}")
    assert min(frag) <= 1000 < max(frag) and sum(f <= 1000 for f in frag) >= 3 and sum(f > 1000 for f in frag) >= 3
    assert most >= 10 and diag["rounds"] <= 4, diag
    assert diag["predicted_stragglers"] == 0


@pytest.mark.parametrize("name", ["lengths_regular", "ragged_regular"])
def test_the_regular_cases_stayed_in_the_regular_rounds(name):
    """a round per visit of the read with the most of them, with the 14-row alignment pass"""
    diag = _device(name)["fresh"][2]
    most = max(st.n_aligns for _, st in S.oracle_records(name))
    print(f"{name}: rounds {diag['rounds']}, most re-estimations of a read {most}")
    assert most >= 10 and diag["rounds"] >= most and diag["jobs_14_row_rounds"] > 0, diag


def test_the_predicted_stragglers_ran_on_their_own_stream():
    recs, ist, diag = _device("early")["fresh"]
    assert len(recs) >= 16 * S.EARLY_TAIL
    print(f"early: {diag}")
    assert 1 <= diag["predicted_stragglers"] <= S.EARLY_TAIL, diag


def test_poisoned_memory_gives_the_same_bytes(tmp_path):
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
            assert json.load(f) == _device(name)["fresh"][2], name
