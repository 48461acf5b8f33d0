#!/usr/bin/env python3
"""Fixtures of the model-truncation tests (tests/test_kde_build.py, tests/test_kde_build_gpu.py), WRITTEN BY THE REFERENCE'S OWN SCRIPT.

Writes into tests/golden/kde_build/:
    reads.paf                 1 500 synthetic primary mappings (both strands, a fifth with truncation 0, some cut at one end only, so
                              end ratios of exactly 0 and 1 occur) plus secondary (tp:A:S) lines, which the reader must skip
    model_default.json        py/truncate_kde.py main() with -b 120 --grid-end 3000
    model_lengths.json        ... --model-lengths
    model_end_ratio.json      ... --end-ratio 0.3
Run on the build machine only (it imports the reference's py/truncate_kde.py, which needs scikit-learn, the way make_kde_golden.py does):
    python tests/golden/make_kde_build_golden.py
No reference source text is copied; the outputs are data."""
import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import REF  # noqa: E402

OUT = os.path.join(HERE, "kde_build")
SETTINGS = {"model_default.json": [], "model_lengths.json": ["--model-lengths"], "model_end_ratio.json": ["--end-ratio", "0.3"]}
COMMON = ["-b", "120", "--grid-start", "0", "--grid-end", "3000", "--grid-step", "100", "-t", "1"]


def synthetic_paf(path, rs, n=1500):
    with open(path, "w") as f:
        for i in range(n):
            tlen = int(np.clip(rs.lognormal(7.0, 0.45), 300, 2900))
            trunc = int(min(tlen - 100, rs.gamma(1.6, 140.0))) if rs.rand() < 0.8 else 0
            share = rs.beta(0.7, 0.5) if rs.rand() < 0.85 else float(rs.rand() < 0.5)      # some reads cut at one end only
            at_end = int(round(trunc * share))
            strand = "+-"[int(rs.rand() < 0.5)]
            if strand == "+":
                tstart, tend = trunc - at_end, tlen - at_end
            else:
                tstart, tend = at_end, tlen - (trunc - at_end)
            alen = tend - tstart
            f.write(f"r{i}\t{alen}\t0\t{alen}\t{strand}\tt{i % 200}\t{tlen}\t{tstart}\t{tend}\t{alen}\t{alen}\t60\ttp:A:P\tcm:i:{i % 9}\n")
            if i % 6 == 0:                       # a secondary mapping: no tp:A:P
                f.write(f"r{i}\t100\t0\t100\t+\tt0\t{tlen}\t0\t100\t100\t100\t0\ttp:A:S\n")


def main():
    os.makedirs(OUT, exist_ok=True)
    paf = os.path.join(OUT, "reads.paf")
    synthetic_paf(paf, np.random.RandomState(20261018))
    spec = importlib.util.spec_from_file_location("ref_truncate_kde", os.path.join(REF, "py", "truncate_kde.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    for name, extra in SETTINGS.items():
        argv = sys.argv
        sys.argv = ["truncate_kde.py", "-i", paf, "-o", os.path.join(OUT, name)] + COMMON + extra
        try:
            mod.main()                           # the reference's own main(): KDE on the grid, printModelJson
        finally:
            sys.argv = argv
        print("wrote", name)


if __name__ == "__main__":
    main()
