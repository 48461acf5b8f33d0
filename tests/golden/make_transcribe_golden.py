#!/usr/bin/env python3
"""Fixture of the transcribe tests (tests/test_transcribe.py): the expected output for the hand-written inputs in tests/golden/transcribe/.

    ann.gtf              12 transcripts on 3 contigs, both strands; exon counts 1, 2 and 9; a non-coding gene; the id T2 twice; T7 without
                         exons; gene / CDS / UTR / stop_codon lines, '#' comments, attributes with and without gene_name
    abund_exact.tsv      integer tpm values whose sum, 60, is the --molecule-count: every count is an integer, every carry 0, and the
                         output depends on no random draw
    expected_exact.mdf   written here by tsb_reference (tests/tsb_spec.py), the line-by-line restatement of src/transcribe.cpp:119-198
The reference itself cannot be built (its extern/ is absent), so the restatement is the yardstick, as for random-wgs.
    python tests/golden/make_transcribe_golden.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
from tsb_spec import tsb_reference  # noqa: E402

D = os.path.join(HERE, "transcribe")
MOLECULE_COUNT = 60

if __name__ == "__main__":
    gtf = open(os.path.join(D, "ann.gtf")).read()
    ab = open(os.path.join(D, "abund_exact.tsv")).read()
    text = tsb_reference(np.random.RandomState(0), [gtf], [ab], MOLECULE_COUNT)
    with open(os.path.join(D, "expected_exact.mdf"), "w") as f:
        f.write(text)
    print(f"{sum(l.startswith('+') for l in text.splitlines())} records, {len(text)} bytes")
