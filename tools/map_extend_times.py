#!/usr/bin/env python3
"""map --extend: what the end extension costs on a generated transcriptome (profiles/map_extend_times.log).

  python tools/map_extend_times.py [--transcripts 20000] [--reads 200000] [--parent-tree DIR] [--out profiles/map_extend_times.log]

The input is that of tools/map_times.py (seed 1): --transcripts random transcripts of 600 to 2 500 bases, every tenth sharing its first half
with the one before it, and --reads reads that are substrings of at least 200 bases on a random strand with 5 % substitutions.  Runs
Sequencer.map four times on one context, once each: map, map --extend, map -c, map -c --extend, all at the defaults, and records every
call's wall time, its device stages by HIP events, and the counters of the extension with its cells per second.  As an observation, what
the extension is for: the bases a primary line on the read's own transcript stops short of the read's true ends, with and without it.
--parent-tree DIR: a checkout of the parent commit, built, beside this one; a child process imports tksm_amd from there and runs map and
map -c on the same files, and its times go next to this build's.  One machine, one run."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

RC = bytes.maketrans(b"ACGT", b"TGCA")
STAGES = ("sketch", "index", "seed", "chain", "select")


def generate(d, n_transcripts, n_reads):
    """tools/map_times.py's input: (fasta path, fastq path, [(transcript, start, end)] of every read, transcript bases, read bases)"""
    import numpy as np
    rs = np.random.default_rng(1)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    tx = []
    for i in range(n_transcripts):
        seq = acgt[rs.integers(0, 4, int(rs.integers(600, 2501)))].tobytes()
        if i % 10 == 9:
            seq = tx[-1][: len(tx[-1]) // 2] + seq[len(seq) // 2:]
        tx.append(seq)
    fa, fq = os.path.join(d, "tx.fa"), os.path.join(d, "reads.fq")
    with open(fa, "wb") as f:
        for i, seq in enumerate(tx):
            f.write(b">tx%06d\n" % i + seq + b"\n")
    origin = rs.integers(0, n_transcripts, n_reads)
    truth, total = [], 0
    with open(fq, "wb") as f:
        for r, t in enumerate(origin):
            seq = tx[t]
            n = int(rs.integers(200, len(seq) + 1))
            b = int(rs.integers(0, len(seq) - n + 1))
            piece = np.frombuffer(seq[b:b + n], np.uint8).copy()
            hit = rs.random(n) < 0.05
            piece[hit] = acgt[(np.searchsorted(acgt, piece[hit]) + rs.integers(1, 4, int(hit.sum()))) % 4]
            piece = piece.tobytes()
            if rs.random() < 0.5:
                piece = piece.translate(RC)[::-1]
            total += n
            truth.append((int(t), b, b + n))
            f.write(b"@r%07d\n" % r + piece + b"\n+\n" + b"I" * n + b"\n")
    return fa, fq, truth, sum(map(len, tx)), total


def run_calls(tree, fa, fq, d, calls):
    """{name: (wall seconds, info)} of Sequencer.map under every keyword set of `calls`, on one context of the build in `tree`"""
    sys.path.insert(0, tree)
    import torch  # noqa: F401  (its ROCm runtime has to be loaded before libtksmseq.so)
    from tksm_amd.sequence import Sequencer
    s = Sequencer(0)
    s.get_reference_seqs([fa])
    out = {}
    for name, kw in calls:
        t0 = time.time()
        info = s.map(fq, os.path.join(d, name + ".paf"), **kw)
        out[name] = (time.time() - t0, info)
    s.close()
    return out


def short_of_the_ends(paf, truth):
    """the sorted (tstart - a) + (b - tend) of the primary lines on the read's own transcript"""
    out = []
    for line in open(paf):
        f = line.split("\t")
        t, a, b = truth[int(f[0][1:])]
        if f[12] == "tp:A:P" and int(f[5][2:]) == t:
            out.append((int(f[7]) - a) + (b - int(f[8])))
    return sorted(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--transcripts", type=int, default=20000)
    ap.add_argument("--reads", type=int, default=200000)
    ap.add_argument("--parent-tree", default=None, help="a built checkout of the parent commit: its map and map -c times on the same files")
    ap.add_argument("--base-only", nargs=3, metavar=("TREE", "FASTA", "FASTQ"), default=None, help="(the child of --parent-tree) map and map -c of TREE's build as one JSON line")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "map_extend_times.log"))
    a = ap.parse_args()
    if a.base_only:
        tree, fa, fq = a.base_only
        with tempfile.TemporaryDirectory() as d:
            got = run_calls(tree, fa, fq, d, (("map", {}), ("map_c", dict(align=True))))
        print(json.dumps({k: [w, i] for k, (w, i) in got.items()}))
        return
    lines = []

    def say(text=""):
        print(text, flush=True)
        lines.append(text)

    def row(name, wall, i):
        extra = (f", align {i['align']['align_ms']:.1f} ms" if "align" in i else "") + (f", extend {i['extend']['extend_ms']:.1f} ms" if "extend" in i else "")
        say(f"{name:<22} wall {wall:6.2f} s: read {i['read_ms'] / 1e3:.2f} s, upload {i['upload_ms'] / 1e3:.2f} s, write {i['write_ms'] / 1e3:.2f} s; device " +
            ", ".join(f"{n} {ms:.1f}" for n, ms in zip(STAGES, i["stage_ms"])) + f" ms = {i['device_ms']:.1f} ms{extra}; {i['chunks']} chunk(s), {i['lines']} lines")

    with tempfile.TemporaryDirectory() as d:
        t0 = time.time()
        fa, fq, truth, tx_bases, read_bases = generate(d, a.transcripts, a.reads)
        say(f"map --extend: times on the input of tools/map_times.py (seed 1): {a.transcripts} transcripts of 600 to 2500 bases ({tx_bases} bases, every tenth an isoform of "
            f"the one before), {a.reads} reads of 200 bases to a whole transcript ({read_bases} bases, 5 % substitutions, both strands), {os.path.getsize(fq) >> 20} MB of "
            f"FASTQ (made in {time.time() - t0:.0f} s).  One machine, one run; every call once, in this order, on one context.")
        say()
        calls = (("map", {}), ("map --extend", dict(extend=True)), ("map -c", dict(align=True)), ("map -c --extend", dict(align=True, extend=True)))
        got = run_calls(ROOT, fa, fq, d, calls)
        say("== this build (MI355X, 1 GPU; Sequencer.map at the defaults: k 15, w 10, band 63, ext band 31, drop 40, max 2000) ==")
        for name, _ in calls:
            row(name, *got[name])
        say()
        for name in ("map --extend", "map -c --extend"):
            x = got[name][1]["extend"]
            say(f"{name}: {x['lines']} lines, {x['ends_moved']} of {2 * x['lines']} ends moved (the longest by {x['longest']} anti-diagonals), {x['target_gained']} target and "
                f"{x['read_gained']} read letters gained, {x['matches']} matches; first pass {x['antidiagonals']} anti-diagonals, {x['cells']} allowed cells; "
                f"{x['extend_ms']:.1f} ms by HIP events{' with the second pass, its traceback and its runs' if 'align' in got[name][1] else ''}: "
                f"{x['cells'] / max(1e-9, x['extend_ms'] / 1e3):.3g} first-pass cells per second of the stage")
        al = got["map -c"][1]["align"]
        say(f"for scale, the alignment of the same lines: {al['cells']} allowed cells in {al['align_ms']:.1f} ms, {al['cells'] / max(1e-9, al['align_ms'] / 1e3):.3g} cells per second")
        say()
        before, after = short_of_the_ends(os.path.join(d, "map.paf"), truth), short_of_the_ends(os.path.join(d, "map --extend.paf"), truth)

        def stats(v):
            return f"mean {sum(v) / len(v):.2f}, median {v[len(v) // 2]}, p90 {v[len(v) * 9 // 10]}, max {v[-1]}, min {v[0]}"
        say("== observation: (tstart - a) + (b - tend) of the primary lines on the read's own transcript, (a, b) the read's true interval ==")
        say(f"chains alone ({len(before)} lines): {stats(before)}")
        say(f"with --extend ({len(after)} lines): {stats(after)}")
        if a.parent_tree:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--base-only", os.path.abspath(a.parent_tree), fa, fq], capture_output=True, text=True)
            say()
            if r.returncode:
                say(f"the parent's build in {a.parent_tree} did not run: {r.stderr[-300:]}")
            else:
                say("== the parent commit's build, a child process on the same machine in the same run, the same files, after the calls above ==")
                for name, (wall, info) in json.loads(r.stdout.strip().splitlines()[-1]).items():
                    row({"map": "parent map", "map_c": "parent map -c"}[name], wall, info)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
