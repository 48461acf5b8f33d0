"""Molecules for the edges of k_init's one-pass image builder, and the driver that runs them (tests/test_init_images_gpu.py; pytest
does not collect this file).

k_init turns the spliced fragment of a read (L = raw length + 2 k letters in LDS) into three device images in one pass, 16 letters per
lane and trip: the packed words of st_frag2 (16 bases each), the slot codes of st_nb (64-position blocks, the rest of the read's row
zeroed by the same pass -- the host clears none of it) and the {lo, hi} plane pairs of st_fplanes (64 positions each, four lanes
combine their pieces).  k_err reads a slot's symbols from its code alone, and the straggler kernel k_loopw<true> unpacks its alignment
window from st_frag2.  The cases put fragment lengths on both sides of every one of those boundaries, every kind of segment the splice
knows, the straggler kernel on both sides of the 1000-base window rule and on its own stream from round 0, and run all of it inside
device buffers that hold an earlier, longer run's data.

Everything here is a function of constants, so the test rebuilds the inputs (and the oracle's records) without a GPU.  As a script,

    python tests/init_images_spec.py --out DIR

runs every case on a fresh context and again on a context that has just run DIRTY, and writes the records to DIR/<case>.<fresh|recycled>.bin
and the diagnostics of the fresh run to DIR/<case>.diag.json -- the test starts it once with TKSMSEQ_POISON=00000001 (ctx.h: every byte
of device memory a buffer has not been given to keep reads as that word), which is fixed when the library is loaded."""
import argparse
import functools
import json
import os
import sys

import numpy as np

K = 7                                      # k of the nanopore2020 error model (the test asserts it)
SEED = 4242
FIRST = 31                                 # first read index of every run
IDENTITY = (84.0, 99.0, 5.5)               # mean, max, stdev
GENOME_SIZE = 40_000
LOWER = (3000, 3400)                       # a lower-case stretch of the contig


@functools.lru_cache(None)
def genome():
    rs = np.random.RandomState(1201)
    seq = rs.choice(np.frombuffer(b"ACGT", np.uint8), GENOME_SIZE).tobytes()
    return {"g": (seq[:LOWER[0]] + seq[LOWER[0]:LOWER[1]].lower() + seq[LOWER[1]:]).decode()}


def _iv(start, length, strand="+", mods=""):
    return ("g", start, start + length, strand, mods)


def _lit(seq, strand="+"):
    return (seq, 0, len(seq), strand, "")


def edge_lengths():
    """raw lengths whose fragment length L = raw + 2 K is -1 / 0 / +1 around multiples of 16 (a packed word, a lane's trip) and of 64 (a
    block of slot codes, a plane pair, a wave's trip), from a single base upward; L = 1000 / 1001 and raw = 1000 / 1001 (the window rule)"""
    frag = {1 + 2 * K, 2 + 2 * K, 3 + 2 * K}
    for m in (16, 32, 48, 64, 80, 128, 192, 256, 512, 1024):
        frag |= {m - 1, m, m + 1}
    frag |= {1000, 1001, 1000 + 2 * K, 1001 + 2 * K}
    return sorted(f - 2 * K for f in frag if f - 2 * K >= 1)


def case_lengths():
    return [(f"len{raw}", [_iv(5000 + 37 * i, raw, "+-"[i & 1])]) for i, raw in enumerate(edge_lengths())]


def case_ragged():
    """one 3 kb molecule among 40-base ones and a few of 500: ragged rows, several LDS buckets of the last visit"""
    mols = [(f"s{i}", [_iv(9000 + 11 * i, 40, "+-"[i % 2])]) for i in range(30)]
    mols.insert(7, ("long3k", [_iv(12000, 3000)]))
    mols += [(f"m{i}", [_iv(20000 + 501 * i, 500 + i, "-+"[i % 2])]) for i in range(6)]
    return mols


N_MOLECULES = ("n_mid", "n_last", "n_first_minus")       # molecules of case_segments with an N: the exact kernel's


def case_segments():
    """every kind of segment: minus-strand intervals, literals (alone, in front, in between, at the end, on the minus strand),
    a substitution at the first and at the last base of an interval on either strand, an N in the middle and an N as the very last base,
    intervals inside and across the lower-case stretch"""
    lo = LOWER[0]
    return [
        ("minus3", [_iv(700, 130, "-"), _iv(15000, 63, "-"), _iv(1000, 77, "-")]),
        ("lit_only", [_lit("ACGTTGCAAGGCTTAACCGGTTACGATCGATCGGATATTACGCA")]),
        ("lit_front", [_lit("TTTTTTTTTTTTTTTTTTTTTTTT"), _iv(2000, 200)]),
        ("lit_between", [_iv(2100, 100, "-"), _lit("ACGTACGTAC"), _iv(2300, 139)]),
        ("lit_end_minus", [_iv(2500, 150), _lit("AAAAAAAAAAAAAAAAAAAAAAAAAAAAAACCG", "-")]),
        ("mod_first_plus", [_iv(6000, 120, "+", "0T")]),
        ("mod_last_plus", [_iv(6200, 120, "+", "119A")]),
        ("mod_first_minus", [_iv(6400, 121, "-", "0C")]),
        ("mod_last_minus", [_iv(6600, 121, "-", "120G")]),
        ("mod_both_two_ivs", [_iv(6800, 50, "+", "0G,49C"), _iv(7000, 64, "-", "0A,63T")]),
        ("n_mid", [_iv(7200, 300, "+", "150N")]),
        ("n_last", [_iv(7600, 113), _iv(7800, 100, "+", "99N")]),
        ("n_first_minus", [_iv(8000, 200, "-", "199N")]),
        ("lower_inside", [_iv(lo + 20, 300)]),
        ("lower_across", [_iv(lo - 90, 250, "-"), _iv(LOWER[1] - 40, 100)]),
    ]


def case_stragglers():
    """a batch small enough that every read finishes in the straggler kernel after its first round: fragments on both sides of 1000
    (whole-fragment windows, random 1000-base windows), windows that start at every offset inside a packed word"""
    raws = [300, 640, 985, 986, 987, 990, 1000, 1100, 1500, 2047, 2600, 3100]
    return [(f"t{raw}", [_iv(21000 + 97 * i, raw, "+-"[i % 2])]) for i, raw in enumerate(raws)]


EARLY_TAIL = 8                             # TKSMSEQ_EARLY_TAIL of the case below: a batch of >= 16 x that many reads may have predicted stragglers


def case_early():
    """16 x EARLY_TAIL + 12 short reads and six long ones: the long ones need > 4 x the median read's visits, so they get their straggler
    waves at round 0 on a stream of their own"""
    rs = np.random.RandomState(77)
    mols = [(f"e{i}", [_iv(int(rs.randint(0, 30000)), int(rs.randint(150, 330)), "+-"[i % 2])]) for i in range(16 * EARLY_TAIL + 12)]
    mols += [(f"L{i}", [_iv(1000 + 3001 * i, 3400 + 211 * i, "-+"[i % 2])]) for i in range(6)]
    return mols


# batches this small go to the straggler kernel after round 0; the `_regular` cases keep the same molecules in the regular rounds to the
# end, as the bulk of a large batch is (k_loop a lane per read, k_alnf with 14 stored rows and its full-width pass, k_err per length bucket)
REGULAR = {"TKSMSEQ_TAIL_WAVE": "0", "TKSMSEQ_WAVE_LOOP": "0", "TKSMSEQ_SMALL_ALN": "0", "TKSMSEQ_TAIL_CUT": "0"}
CASES = {"lengths": case_lengths, "ragged": case_ragged, "segments": case_segments, "stragglers": case_stragglers, "early": case_early,
         "lengths_regular": case_lengths, "ragged_regular": case_ragged}
ENV = {"early": {"TKSMSEQ_EARLY_TAIL": str(EARLY_TAIL)}, "lengths_regular": REGULAR, "ragged_regular": REGULAR}     # knobs read when the context is created


def dirty():
    """what runs first on the context of a `recycled` pass: other and longer molecules than any case's, more of them than most"""
    rs = np.random.RandomState(5)
    return [(f"d{i}", [_iv(int(rs.randint(0, GENOME_SIZE - 4000)), int(rs.randint(3200, 3900)), "+-"[i % 2])]) for i in range(48)]


def mdf_text(mols):
    return "".join(f"+{m}\t1\t\n" + "".join(f"{c}\t{a}\t{b}\t{st}\t{md}\n" for c, a, b, st, md in ivs) for m, ivs in mols)


@functools.lru_cache(None)
def oracle_records(name):
    """[(record, FragStats)] of the case by the CPU oracle"""
    import pyoracle as po
    from conftest import ERR_MODEL, QS_MODEL
    em, qm = _oracle_models(ERR_MODEL, QS_MODEL)
    ident = po.Identities(IDENTITY[0], IDENTITY[2], IDENTITY[1])
    return [po.badread_record(True, SEED, FIRST + i, po.splice(genome(), ivs), ident, em, qm, True, mid) for i, (mid, ivs) in enumerate(CASES[name]())]


@functools.lru_cache(None)
def _oracle_models(err, qs):
    import pyoracle as po
    return po.ErrorModel(err), po.QScoreModel(qs)


# ------------------------------------------------------------------------------------------------ on the device
def sequencer(env=None):
    """a context with the genome and the nanopore2020 models; `env`: knobs that are read when it is created"""
    from conftest import ERR_MODEL, QS_MODEL
    from tksm_amd.sequence import Sequencer
    old = {k: os.environ.get(k) for k in (env or {})}
    os.environ.update(env or {})
    try:
        s = Sequencer(0)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    for name, seq in genome().items():
        s.add_contig(name, seq)
    s.set_identity(IDENTITY[0], IDENTITY[1], IDENTITY[2])
    s.load_error_model(ERR_MODEL)
    s.load_qscore_model(QS_MODEL)
    return s


def run_case(s, mols):
    """(records, per-read integer statistics, diagnostics) of one run"""
    res = s.run(s.batch_from_mdf(mdf_text(mols)), target="badread", fastq=True, compute_qual=True, seed=SEED, first_read_index=FIRST, collect_stats=True)
    return res.records(), res.stats()[0].copy(), s.run_diagnostics()


def run_both(name):
    """the case on a fresh context, and on a context whose buffers hold DIRTY's run: {"fresh": ..., "recycled": ...} as run_case gives them"""
    out = {}
    for how in ("fresh", "recycled"):
        s = sequencer(ENV.get(name))
        try:
            if how == "recycled":
                run_case(s, dirty())
            out[how] = run_case(s, CASES[name]())
        finally:
            s.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    for name in CASES:
        print(f"case {name}", file=sys.stderr, flush=True)
        got = run_both(name)
        for how, (recs, _, diag) in got.items():
            with open(os.path.join(a.out, f"{name}.{how}.bin"), "wb") as f:
                f.write(b"".join(recs))
        with open(os.path.join(a.out, f"{name}.diag.json"), "w") as f:
            json.dump(got["fresh"][2], f)


if __name__ == "__main__":
    import torch  # noqa: F401  (its ROCm runtime is loaded before libtksmseq.so, as in tests/conftest.py)
    main()
