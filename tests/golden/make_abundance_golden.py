#!/usr/bin/env python3
"""Fixtures of the abundance tests (tests/test_abundance.py, tests/test_abundance_gpu.py), WRITTEN BY THE REFERENCE'S OWN SCRIPT.

Writes into tests/golden/abundance/:
    reads.paf                 about 600 synthetic reads on 100 transcripts (lognormal weights): 60 % with 2 - 5 records on neighbouring
                              transcripts, a tenth with a poor best hit (dropped), about 60 records moved away from their read's other lines,
                              and the edge reads planted by hand (EDGE below)
    lr_matches.tsv            five columns; some lines with column 3 != 1, one read listed twice, some reads absent
    expected_default.tsv      py/transcript_abundance.py main() with -em 10
    expected_em0.tsv          ... -em 0
    expected_em1.tsv          ... -em 1
    expected_lr_br.tsv        ... -em 10 -m lr_matches.tsv
    expected_abundance.json   {transcript: repr(abundance)} after 10 rounds, by the script's own functions
The seed is the first from 20261018 on for which no expected tpm lies within 1e-6 of a %.3f rounding boundary or of the 0.001 cut: a
different order of summation moves a tpm by about 1e-10, so the files can be compared as text.
Run on the build machine only (it imports the reference's py/transcript_abundance.py, which needs tqdm):
    python tests/golden/make_abundance_golden.py
No reference source text is copied; the outputs are data."""
import importlib.util
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import REF  # noqa: E402

OUT = os.path.join(HERE, "abundance")
N_T = 100


def tname(t):
    return f"ENST{t:05d}.{1 + t % 4}"


def line(rid, qlen, t, tstart, nmatch, blen, strand="+"):
    tlen = 4000
    return f"{rid}\t{qlen}\t0\t{blen}\t{strand}\t{t}\t{tlen}\t{tstart}\t{min(tlen, tstart + blen)}\t{nmatch}\t{blen}\t60\ttp:A:P\n"


# the edge reads: (read, query length, [(transcript, target_start, matches, block length), ...])
EDGE = [
    ("edge_ratio_95_96", 1000, [(3, 0, 100, 900), (4, 0, 95, 900), (5, 0, 96, 900)]),           # 95/100 is no hit, 96/100 is
    ("edge_ratio_19_20", 1000, [(6, 0, 20, 900), (7, 0, 19, 900)]),                              # 19/20 is no hit
    ("edge_start_19_best", 1000, [(8, 19, 800, 900), (9, 20, 799, 900), (10, 5, 790, 900)]),     # 19 is full length, 20 is not
    ("edge_start_20_best", 1000, [(11, 20, 800, 900), (12, 19, 799, 900), (13, 300, 790, 900)]),
    ("edge_half_exactly", 1000, [(14, 0, 480, 500)]),                                            # 0.5 stays
    ("edge_half_under", 1001, [(15, 0, 480, 500)]),                                              # just under: dropped
    ("edge_tie_later_full", 1000, [(16, 50, 900, 950), (17, 5, 900, 600), (18, 60, 900, 950)]),  # the later full-length tie wins; 16 and 18 are no hits
    ("edge_tie_drops", 1000, [(19, 50, 900, 950), (20, 5, 900, 400)]),                           # ... and its block length decides: dropped
    ("edge_same_transcript", 1000, [(21, 0, 900, 950), (21, 3, 890, 940), (22, 0, 700, 800)]),   # two hits on one transcript stay two
    ("edge_first_length", 1000, [(23, 0, 900, 950)]),                                            # (its moved second line says 5000: the first counts)
]
ONLY_DROPPED = "ENSTDROP.1"                                # only dropped reads map here: no row


def synthetic(rs, n_reads=600):
    weights = rs.lognormal(0.0, 1.2, N_T)
    weights /= weights.sum()
    lines, moved = [], []
    for i in range(n_reads):
        rid = f"read{i:05d}"
        qlen = int(np.clip(rs.lognormal(7.0, 0.4), 400, 3000))
        t0 = int(rs.choice(N_T, p=weights))
        k = 1 if rs.rand() < 0.4 else int(rs.randint(2, 6))
        poor = rs.rand() < 0.1
        frac = rs.uniform(0.1, 0.45) if poor else rs.uniform(0.7, 1.0)
        blen = max(20, int(qlen * frac))
        best = max(10, int(blen * rs.uniform(0.85, 0.98)))
        recs = []
        for j in range(k):
            t = tname((t0 + j) % N_T) if not (poor and j == 0 and i % 7 == 0) else ONLY_DROPPED
            m = best if j == 0 else max(1, int(best * rs.uniform(0.90, 1.0)))
            ts = int(rs.randint(0, 20)) if rs.rand() < 0.7 else int(rs.randint(20, 300))
            recs.append(line(rid, qlen, t, ts, m, max(20, blen - int(rs.randint(0, 30))), "+-"[int(rs.rand() < 0.5)]))
        order = rs.permutation(k)
        for j, o in enumerate(order):
            (moved if (k > 1 and j > 0 and rs.rand() < 0.06) else lines).append(recs[o])
    for rid, qlen, recs in EDGE:
        at = int(rs.randint(0, len(lines)))
        lines[at:at] = [line(rid, qlen, tname(t), ts, m, b) for t, ts, m, b in recs]
    for rec in moved:                                        # away from their read's other lines (anywhere later or earlier)
        lines.insert(int(rs.randint(0, len(lines) + 1)), rec)
    lines.append(line("edge_first_length", 5000, tname(24), 0, 10, 950))
    return lines, len(moved) + 1


def lr_matches(rs, paf_lines):
    reads = list(dict.fromkeys(ln.split("\t")[0] for ln in paf_lines))
    bcs = ["ACGTACGTACGT", "TTGCATTGCATT", "GGGGCCCCAAAA", "CATGCATGCATG", "TTTTTTTTTTTT", "ACACACACACAC"]
    out = []
    for i, r in enumerate(reads):
        u = rs.rand()
        if u < 0.2:
            continue                                         # absent: cell "."
        c = "1" if u < 0.9 else "02"[int(rs.rand() < 0.5)]
        out.append(f"{r}\t{i}\t{c}\t{int(rs.randint(0, 3))}\t{bcs[int(rs.randint(0, len(bcs)))]}\n")
    twice = reads[5]
    out.insert(3, f"{twice}\t0\t1\t0\t{bcs[0]}\n")
    out.append(f"{twice}\t0\t1\t0\t{bcs[1]}\n")                # the later line wins
    out.append(f"{reads[6]}\t0\t0\t0\t{bcs[2]}\n")             # column 3 != 1 after a 1 line: ignored
    return out


def main():
    os.makedirs(OUT, exist_ok=True)
    spec = importlib.util.spec_from_file_location("ref_transcript_abundance", os.path.join(REF, "py", "transcript_abundance.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    paf, lr = os.path.join(OUT, "reads.paf"), os.path.join(OUT, "lr_matches.tsv")
    runs = {"expected_default.tsv": ["-em", "10"], "expected_em0.tsv": ["-em", "0"], "expected_em1.tsv": ["-em", "1"], "expected_lr_br.tsv": ["-em", "10", "-m", lr]}
    seed = 20261018
    while True:
        rs = np.random.RandomState(seed)
        lines, n_moved = synthetic(rs)
        open(paf, "w").write("".join(lines))
        open(lr, "w").write("".join(lr_matches(rs, lines)))
        # the margin of every tpm the four runs print, from the reference's own functions (the files hold three decimals only)
        tid_to_tname, alignments = mod.parse_paf(paf)
        margin = 1.0
        rid_to_bc = mod.parse_lr_bc_matches(lr)
        for rounds, cells in ((10, None), (0, None), (1, None), (10, rid_to_bc)):
            comp = mod.get_compatibility(alignments)
            for _ in range(rounds):
                mod.update_compatibility(comp, mod.calculate_abundance(comp))
            for a in mod.calculate_split_abundance(comp, cells if cells is not None else mod.defaultdict(lambda: ".")).values():
                tpm = a * 1_000_000
                margin = min(margin, abs(tpm - 0.001), abs((tpm * 1000.0) % 1.0 - 0.5) / 1000.0)
        if margin > 1e-6:
            break
        print(f"seed {seed}: a tpm {margin:.3g} from a boundary, next seed")
        seed += 1
    print(f"seed {seed}: {len(alignments)} reads, {len(lines)} lines ({n_moved} moved), closest tpm {margin:.3g} from a boundary")
    for name, extra in runs.items():
        argv = sys.argv
        sys.argv = ["transcript_abundance.py", "-p", paf, "-o", os.path.join(OUT, name)] + extra
        try:
            mod.main()                           # the reference's own main()
        finally:
            sys.argv = argv
        print("wrote", name)
    comp = mod.get_compatibility(alignments)
    for _ in range(10):
        abundance = mod.calculate_abundance(comp)
        mod.update_compatibility(comp, abundance)
    json.dump({"seed": seed, "surviving_reads": len(comp), "abundance": {tid_to_tname[t]: repr(float(a)) for t, a in abundance.items()}},
              open(os.path.join(OUT, "expected_abundance.json"), "w"), indent=1)
    print("wrote expected_abundance.json")


if __name__ == "__main__":
    main()
