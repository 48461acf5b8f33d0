"""Molecules for the forward loop of the fused aligner at its register budget (k_alnf / aln_fused, csrc/kernels.hip), and the driver that
runs them (tests/test_alnf_budget_gpu.py; pytest does not collect this file).

The 14-row pass fits 112 registers because (a) the next pass's slot codes are fetched after iteration 7 of the 16, their first half into
the registers of the half the current pass has just used up, and (b) a 16-byte piece of a code line is stored as soon as its four entries
exist.  What can go wrong with that lies at the pass boundary (16 slots), at the reservoir refill (32), at the plane-word
step (64), in the last line of a window (whose second half stays empty), in windows that start at an odd position (the codes are fetched
from the even one below: `skip` 1), in drain passes (which fetch nothing and must leave the codes in flight alone) and in the lanes of a
partial wave (which write the spare line).  The cases put windows on both sides of each of these.

Everything here is a function of constants, so the test rebuilds the inputs (and the oracle's records) without a GPU.  As a script,

    python tests/alnf_budget_spec.py --out DIR

runs every case with the 14-row pass forced on, on a fresh context and again on a context that has just run DIRTY, and writes the records
to DIR/<case>.<fresh|recycled>.bin and the diagnostics of the fresh run to DIR/<case>.diag.json -- the test starts it once with
TKSMSEQ_POISON=00000001 (ctx.h: every byte of device memory a buffer has not been given to keep reads as that word)."""
import argparse
import functools
import json
import os
import sys

import numpy as np

K = 7                                      # k of the nanopore2020 error model (the test asserts it)
SEED = 977
FIRST = 5                                  # first read index of every run
IDENTITY = (84.0, 99.0, 5.5)               # mean, max, stdev
GENOME_SIZE = 60_000
ST_ALNPOS = 4                              # the generator stream of the window positions (oracle/tksm_oracle.c)
WINDOW = 1000                              # slots of an alignment window: a longer fragment gets a random window of that many

# slot counts L = raw length + 2 K of the whole-fragment windows: a single base, the pass boundary (16), the reservoir refill (32), the plane-word
# step (64), lines whose second half stays empty, and the longest window there is
WINDOW_L = (1 + 2 * K, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65, 95, 96, 97, 127, 128, 129, 999, 1000)
RANDOM_L = tuple(range(1001, 1101)) + (1500, 1501, 1533, 1564, 1600, 1616, 1647, 1700, 1711, 1750, 1799, 1800)
PARTIAL = (1, 63, 64, 65)


@functools.lru_cache(None)
def genome():
    rs = np.random.RandomState(2203)
    return {"g": rs.choice(np.frombuffer(b"ACGT", np.uint8), GENOME_SIZE).tobytes().decode()}


def _iv(start, length, strand="+"):
    return ("g", start, start + length, strand, "")


def case_windows():
    """three fragments of every length of WINDOW_L, from different places and both strands"""
    ls = sorted(set(WINDOW_L))
    return [(f"w{L}_{j}", [_iv(400 + 1013 * j + 53 * i, L - 2 * K, "+-"[(i + j) & 1])]) for i, L in enumerate(ls) for j in range(3)]


def case_windows_low():
    """the same from 63 slots on at a low identity (LOW_IDENTITY): a re-estimation job comes with every 25th change, so at the default identity
    the error loop aligns no fragment this short, and only the q-score job (whose window is always the whole fragment) sees these lengths"""
    ls = sorted(L for L in set(WINDOW_L) if L >= 63)
    return [(f"v{L}_{j}", [_iv(900 + 1013 * j + 59 * i, L - 2 * K, "+-"[(i + j) & 1])]) for i, L in enumerate(ls) for j in range(3)]


def case_random():
    """fragments longer than a window: every re-estimation aligns a random 1000-slot window, from odd and even positions"""
    return [(f"r{L}", [_iv(700 + 431 * i, L - 2 * K, "+-"[i & 1])]) for i, L in enumerate(RANDOM_L)]


def case_partial(n):
    """n ordinary reads of 300 .. 500 bases: a last wave with 1, 63, 64 of its 64 lanes in use, and a second wave with one"""
    rs = np.random.RandomState(100 + n)
    return [(f"p{n}_{i}", [_iv(int(rs.randint(0, GENOME_SIZE - 600)), int(rs.randint(300, 501)), "+-"[i & 1])]) for i in range(n)]


LOW_IDENTITY = (55.0, 60.0, 1.0)
CASES = {"windows": case_windows, "windows_low": case_windows_low, "random": case_random, **{f"partial{n}": functools.partial(case_partial, n) for n in PARTIAL}}
CASE_IDENTITY = {"windows_low": LOW_IDENTITY}                # (every other case: IDENTITY)
# knobs read when the context is created.  "rows14": every alignment job of every round in the 14-row pass, the redo list behind it, k_loop a lane per
# read to the end -- what the bulk of a bench-size batch takes; "small": what a batch this small takes by itself (the full-width pass alone, then the
# straggler kernel)
ROUTES = {"rows14": {"TKSMSEQ_TAIL_WAVE": "0", "TKSMSEQ_WAVE_LOOP": "0", "TKSMSEQ_SMALL_ALN": "0", "TKSMSEQ_TAIL_CUT": "0"}, "small": {}}


def dirty():
    """what runs first on the context of a `recycled` pass: other and longer molecules than any case's"""
    rs = np.random.RandomState(6)
    return [(f"d{i}", [_iv(int(rs.randint(0, GENOME_SIZE - 4000)), int(rs.randint(2000, 3900)), "+-"[i % 2])]) for i in range(150)]


def mdf_text(mols):
    return "".join(f"+{m}\t1\t\n" + "".join(f"{c}\t{a}\t{b}\t{st}\t{md}\n" for c, a, b, st, md in ivs) for m, ivs in mols)


@functools.lru_cache(None)
def _oracle_models(err, qs):
    import pyoracle as po
    return po.ErrorModel(err), po.QScoreModel(qs)


@functools.lru_cache(None)
def oracle_records(name, compute_qual=True):
    """[(record, FragStats)] of the case by the CPU oracle"""
    import pyoracle as po
    from conftest import ERR_MODEL, QS_MODEL
    em, qm = _oracle_models(ERR_MODEL, QS_MODEL)
    mean, mx, sd = CASE_IDENTITY.get(name, IDENTITY)
    ident = po.Identities(mean, sd, mx)
    return [po.badread_record(True, SEED, FIRST + i, po.splice(genome(), ivs), ident, em, qm, compute_qual, mid) for i, (mid, ivs) in enumerate(CASES[name]())]


def window_starts(name):
    """the first slot of every random window of the case's error loops (tksm_oracle.c: pos = mulhi32(draw, L - 1000 + 1), a draw per re-estimation)"""
    import pyoracle as po
    out = []
    for i, (_, st) in enumerate(oracle_records(name)):
        if st.frag_len > WINDOW:
            out += [(po.philox(SEED, FIRST + i, ST_ALNPOS, a)[0] * (st.frag_len - WINDOW + 1)) >> 32 for a in range(st.n_aligns)]
    return out


# ------------------------------------------------------------------------------------------------ on the device
def sequencer(env, ref=None, err=None, qs=None, identity=IDENTITY):
    """a context with the reference and the models (default: the genome, nanopore2020); `env`: knobs that are read when it is created"""
    from conftest import ERR_MODEL, QS_MODEL
    from tksm_amd.sequence import Sequencer
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        s = Sequencer(0)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    for name, seq in (ref or genome()).items():
        s.add_contig(name, seq)
    s.set_identity(identity[0], identity[1], identity[2])
    s.load_error_model(err or ERR_MODEL)
    s.load_qscore_model(qs or QS_MODEL)
    return s


def run_case(s, mols, compute_qual=True, seed=SEED, first=FIRST):
    """(records, per-read integer statistics, diagnostics) of one run"""
    res = s.run(s.batch_from_mdf(mdf_text(mols)), target="badread", fastq=True, compute_qual=compute_qual, seed=seed, first_read_index=first, collect_stats=True)
    return res.records(), res.stats()[0].copy(), s.run_diagnostics()


def run_route(name, route, compute_qual=True, recycled=False):
    s = sequencer(ROUTES[route], identity=CASE_IDENTITY.get(name, IDENTITY))
    try:
        if recycled:
            run_case(s, dirty())
        return run_case(s, CASES[name](), compute_qual)
    finally:
        s.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    for name in CASES:
        print(f"case {name}", file=sys.stderr, flush=True)
        for how in ("fresh", "recycled"):
            recs, _, diag = run_route(name, "rows14", True, how == "recycled")
            with open(os.path.join(a.out, f"{name}.{how}.bin"), "wb") as f:
                f.write(b"".join(recs))
            if how == "fresh":
                with open(os.path.join(a.out, f"{name}.diag.json"), "w") as f:
                    json.dump(diag, f)


if __name__ == "__main__":
    import torch  # noqa: F401  (its ROCm runtime is loaded before libtksmseq.so, as in tests/conftest.py)
    main()
