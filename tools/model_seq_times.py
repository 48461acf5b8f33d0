#!/usr/bin/env python3
"""model-sequence: where the time goes on a large synthetic input (profiles/model_seq_times.log).

  python tools/model_seq_times.py [--alignments 200000] [--columns 1000] [--spec-alignments 2000] [--out profiles/model_seq_times.log]

Makes the input with the generator of tests/model_seq_spec.py (alignments of about --columns columns), runs Sequencer.model_sequence
once and records the module's wall time split into reading, upload, device (HIP events, per stage) and writing, and the events per
second.  For scale only, the plain Python specification runs on the first --spec-alignments alignments of the same file: it is an
unoptimised restatement of the rules, not a baseline.  One machine, one run."""
import argparse
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--alignments", type=int, default=200000)
    ap.add_argument("--columns", type=int, default=1000)
    ap.add_argument("--spec-alignments", type=int, default=2000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "model_seq_times.log"))
    a = ap.parse_args()
    import torch  # noqa: F401  (its ROCm runtime has to be loaded before libtksmseq.so)
    import model_seq_spec as M
    from tksm_amd.sequence import Sequencer
    lines = []

    def say(text=""):
        print(text, flush=True)
        lines.append(text)

    with tempfile.TemporaryDirectory() as d:
        t0 = time.time()
        g = M.generate(d, seed=1, n_alignments=a.alignments, col_lo=a.columns * 9 // 10, col_hi=a.columns * 11 // 10, extra_columns=(), group=0,
                       contig_len=1 << 20, n_contigs=8, progress=lambda i: print(f"  generated {i} alignments", flush=True))
        size = sum(os.path.getsize(g[k]) for k in ("reference", "reads", "alignment"))
        say(f"model-sequence: times on the input of tools/model_seq_times.py (the generator of tests/model_seq_spec.py, seed 1): {a.alignments} alignments of about "
            f"{a.columns} columns, {size / 1e6:.0f} MB of FASTA + FASTQ + PAF (made in {time.time() - t0:.0f} s).  One machine, one run.")
        say()
        s = Sequencer(0)
        s.get_reference_seqs([g["reference"]])
        t0 = time.time()
        info = s.model_sequence(g["reads"], g["alignment"], os.path.join(d, "e.model.gz"), os.path.join(d, "q.model.gz"))
        wall = time.time() - t0
        s.close()
        say("== device (MI355X, 1 GPU; Sequencer.model_sequence at the defaults: K = 7, Kq = 9, both files gzipped) ==")
        say(f"wall {wall:.2f} s: reading and parsing {info['read_ms'] / 1e3:.2f} s, uploads and offsets {info['upload_ms'] / 1e3:.2f} s, device {info['device_ms'] / 1e3:.3f} s, "
            f"formatting and writing {info['write_ms'] / 1e3:.2f} s")
        st = info["stage_ms"]
        say(f"device by HIP events, {info['chunks']} chunk(s): columns {st[0]:.1f} ms, events {st[1]:.1f} ms, sort + reduce + merge {st[2]:.1f} ms (its host waits included), "
            f"select {st[3]:.1f} ms")
        say(f"{info['used']} alignments used, {info['events']} events ({info['counting_positions']} counting positions, {info['read_positions']} read positions), "
            f"{info['error_keys']} + {info['qscore_keys']} distinct keys")
        say(f"events per second: {info['events'] / (info['device_ms'] / 1e3):.3g} of device time, {info['events'] / wall:.3g} of wall time")
        say()
        t0 = time.time()
        M.run(g["reference"], g["reads"], g["alignment"], max_alignments=a.spec_alignments)
        spec_s = time.time() - t0
        say(f"== for scale: the plain Python specification on the first {a.spec_alignments} alignments of the same file ==")
        say(f"wall {spec_s:.1f} s (reading the whole FASTQ included).  An unoptimised restatement of the rules, NOT a baseline: there is no earlier implementation "
            f"of these rules to compare a time against.")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
