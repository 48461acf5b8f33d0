"""One context over several Badread runs: what the run scheduler (csrc/run.cpp) owns besides the records -- its exit paths, the
buffers that grow from run to run and are reused, the timing ticks, and the places of the diagnostics.  The kernels themselves are
pinned against the oracle in test_gpu_parity.py; here every comparison is bytes against bytes of the same batch on a fresh context."""
import math
import re

import numpy as np
import pytest

from conftest import ERR_MODEL, QS_MODEL

pytestmark = pytest.mark.gpu
SEED = 77


def _genome():
    rs = np.random.RandomState(41)
    ref = {}
    for name, size in (("chr1", 200_000), ("chr2", 200_000), ("chr3", 120_000)):
        seq = rs.choice(np.frombuffer(b"ACGT", np.uint8), size).tobytes()
        if name == "chr1":                   # an N run: reads that touch it take the exact kernel, on the side streams
            seq = seq[:5000] + b"N" * 300 + seq[5300:]
        ref[name] = seq
    return ref


REF = _genome()


def _mdf(seed, n, mean_len):
    """molecules as test_gpu_parity._make_molecules builds them (1-3 intervals, either strand, some substitutions, a literal
    now and then); every seventh one that draws chr1 starts next to its N run"""
    rs = np.random.RandomState(seed)
    names = list(REF)
    out = []
    for i in range(n):
        total = max(40, int(rs.normal(mean_len, mean_len * 0.2)))
        k = int(rs.randint(1, 4))
        out.append(f"+mol{i}\t1\t\n")
        for _ in range(k):
            ln = total // k
            c = names[rs.randint(len(names))]
            st = int(rs.randint(4800, 5400)) if (i % 7 == 0 and c == "chr1") else int(rs.randint(0, len(REF[c]) - ln))
            mods = "" if rs.rand() < 0.8 else f"{rs.randint(ln)}{'ACGTN'[rs.randint(5)]}"
            out.append(f"{c}\t{st}\t{st + ln}\t{'+-'[rs.randint(2)]}\t{mods}\n")
        if i % 5 == 0:
            out.append(f"{'A' * int(rs.randint(5, 40))}\t0\t40\t+\t\n")
    return "".join(out)


TEXT = {"r64": _mdf(1, 64, 300), "r32": _mdf(2, 32, 300), "r2000": _mdf(3, 2000, 1000), "long": "+long\t1\t\nchr3\t0\t100200\t+\t\n"}
_fresh = {}


def _seqr():
    from tksm_amd.sequence import Sequencer
    s = Sequencer(0)
    for name, seq in REF.items():
        s.add_contig(name, seq)
    s.set_identity(84.0, 99.0, 5.5)
    s.load_error_model(ERR_MODEL)
    s.load_qscore_model(QS_MODEL)
    return s


def _run(s, name):
    return s.run(s.batch_from_mdf(TEXT[name]), target="badread", fastq=True, compute_qual=True, seed=SEED)


def _fresh_bytes(name):
    """the batch's records from a context that has run nothing else (default knobs), computed once"""
    if name not in _fresh:
        s = _seqr()
        _fresh[name] = _run(s, name).download()[0]
        s.close()
    return _fresh[name]


@pytest.mark.parametrize("regular_rounds_only", [False, True])
def test_a_refused_run_leaves_the_context_usable(monkeypatch, regular_rounds_only):
    import torch
    from tksm_amd import _lib
    from tksm_amd.sequence import TksmSeqError
    if regular_rounds_only:
        monkeypatch.setenv("TKSMSEQ_TAIL_WAVE", "0"); monkeypatch.setenv("TKSMSEQ_EARLY_TAIL", "0")
    s = _seqr()
    first = _run(s, "r64").download()[0]
    small = torch.empty(16, dtype=torch.uint8, device="cuda")
    s.set_output_buffer(small.data_ptr(), 16)
    with pytest.raises(TksmSeqError) as e:
        _run(s, "r64")
    assert e.value.code == _lib.ENOMEM and "output buffer too small" in str(e.value)
    s.set_output_buffer(0, 0)
    with pytest.raises(TksmSeqError) as e:
        _run(s, "long")
    assert e.value.code == _lib.ELIMIT and "exceeds the limit" in str(e.value)
    again = _run(s, "r64").download()[0]
    exact = s.run_diagnostics()["exact_kernel_reads"]
    s.close()
    assert exact > 0                         # the N run sent reads to the exact kernel on a side stream
    assert len(first) > 64 * 2 * 200
    assert again == first
    assert first == _fresh_bytes("r64")


def test_buffers_grow_and_are_reused():
    """one range, then about 32 ranges (the page-locked round buffers and the device buffers regrow), then one range again"""
    s = _seqr()
    got = [_run(s, name).download()[0] for name in ("r32", "r2000", "r32")]
    s.close()
    assert got[0] == got[2]
    assert got[0] == _fresh_bytes("r32") and got[2] == _fresh_bytes("r32")
    assert got[1] == _fresh_bytes("r2000")


def test_timing_does_not_change_results():
    s = _seqr()
    s.set_timing(True)
    on = _run(s, "r2000")
    rec_on, ms_on = on.download()[0], list(on.kernel_ms)
    s.set_timing(False)
    off = _run(s, "r2000")
    rec_off, ms_off = off.download()[0], list(off.kernel_ms)
    s.close()
    print(f"timing on: kernel_ms {ms_on}; k_loop + k_alnf + k_job = {ms_on[5] + ms_on[6] + ms_on[7]:.3f} ms of {ms_on[1]:.3f} ms")
    assert rec_on == rec_off and rec_off == _fresh_bytes("r2000")
    assert len(ms_off) == 8 and all(v == 0 for v in ms_off)
    assert len(ms_on) == 8 and all(math.isfinite(v) and v >= 0 for v in ms_on)
    assert ms_on[4] > 0 and ms_on[1] > 0


def test_diagnostics_keep_their_positions(monkeypatch, capfd):
    monkeypatch.setenv("TKSMSEQ_VERBOSE", "1")
    s = _seqr()
    b = s.batch_from_mdf(TEXT["r2000"])
    capfd.readouterr()
    s.run(b, target="badread", fastq=True, compute_qual=True, seed=SEED)
    err = capfd.readouterr().err
    d = s.run_diagnostics()
    s.close()
    slow = re.search(r"slow-path reads (\d+)", err)
    assert slow, err[-600:]
    print(d)
    assert d["rounds"] >= 1
    assert d["jobs_all_rounds"] >= d["jobs_14_row_rounds"]
    assert d["fallbacks"] == 0
    assert d["exact_kernel_reads"] > 0                          # the N run: the side streams were in use
    assert d["exact_kernel_reads"] == int(slow.group(1))
