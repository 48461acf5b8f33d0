#!/usr/bin/env python3
"""map --split: what the option costs and what it finds (profiles/map_split_times.log).

  python tools/map_split_times.py [--transcripts 20000] [--reads 200000] [--runs 5] [--glue 0.2] [--parent-tree DIR] [--out profiles/map_split_times.log]

Three parts, one machine:
1. `map` without --split against the parent commit.  The input is that of tools/map_times.py (seed 1).  --parent-tree DIR is a checkout of
   the parent commit, built, beside this one: a child process imports tksm_amd from there and runs map, map -c and map -c --extend --runs
   times each on one context; so does a child process of this build, and both once more, in turn.  The minimum, median and maximum of the
   parent's 2 x --runs wall times are its run-to-run spread, and this build's medians stand beside it.
2. What --split adds.  The reads of part 1 glued as `unsegment` glues molecules: a read takes the next one with probability --glue, at most
   three to a read.  map and map --split once each: wall, device stages, the counters of tksmseq_split_info.  Then the same with the reads
   ordered by transcript before gluing, which is what `transcribe` -> `unsegment` without a `shuffle` gives: most junctions then join
   two pieces of one transcript, and the later rounds of a group have work.
3. As an observation: the share of glue junctions recovered and the logged estimate of `unsegment -p` beside --glue, on error-free reads,
   on the 5 % reads of part 2 and on Badread reads (identity 84 / 99 / 5.5) of whole transcripts.  The reads are glued as text after
   sequencing.  A junction counts as recovered when the two pieces beside it each have a tp:A:P line on their own transcript that covers
   more than half of the piece."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from map_extend_times import STAGES, generate  # noqa: E402

BASE_CALLS = (("map", {}), ("map -c", dict(align=True)), ("map -c --extend", dict(align=True, extend=True)))


def run_calls(tree, fa, fq, d, calls, runs=1):
    """{name: [(wall seconds, info)] * runs} of Sequencer.map under every keyword set of `calls`, on one context of the build in `tree`"""
    sys.path.insert(0, tree)
    import torch  # noqa: F401  (its ROCm runtime has to be loaded before libtksmseq.so)
    from tksm_amd.sequence import Sequencer
    s = Sequencer(0)
    s.get_reference_seqs([fa])
    out = {name: [] for name, _ in calls}
    for _ in range(runs):
        for name, kw in calls:
            t0 = time.time()
            info = s.map(fq, os.path.join(d, name.replace(" ", "_") + ".paf"), **kw)
            out[name].append((time.time() - t0, info))
    s.close()
    return out


def glue(fq_in, fq_out, truth, p, seed=2, grouped=False):
    """the reads of fq_in glued: a read takes the next with probability p, three at the most.  [[(transcript, q0, q1)] per glued read].
    grouped: the reads ordered by their transcript first, as `transcribe` writes its molecules, so that neighbours are mostly of one"""
    import random
    rs = random.Random(seed)
    pieces, out, at = [], [], 0
    with open(fq_in, "rb") as f, open(fq_out, "wb") as g:
        rows = f.read().split(b"\n")
        seqs = [rows[i + 1] for i in range(0, len(rows) - 3, 4)]
        if grouped:
            order = sorted(range(len(seqs)), key=lambda i: truth[i][0])
            seqs, truth = [seqs[i] for i in order], [truth[i] for i in order]
        while at < len(seqs):
            n = 1
            while n < 3 and at + n < len(seqs) and rs.random() < p:
                n += 1
            text, parts, q = b"".join(seqs[at:at + n]), [], 0
            for i in range(at, at + n):
                parts.append((truth[i][0], q, q + len(seqs[i])))
                q += len(seqs[i])
            g.write(b"@g%07d\n" % len(out) + text + b"\n+\n" + b"I" * len(text) + b"\n")
            out.append(parts)
            at += n
    return out


def junctions(paf, parts):
    """(junctions, junctions recovered) of a PAF over glued reads"""
    found = [set() for _ in parts]
    for line in open(paf):
        f = line.split("\t")
        if f[12] != "tp:A:P":
            continue
        r, t, a, b = int(f[0][1:]), int(f[5][2:]), int(f[2]), int(f[3])
        for i, (pt, q0, q1) in enumerate(parts[r]):
            if pt == t and 2 * max(0, min(b, q1) - max(a, q0)) > q1 - q0:
                found[r].add(i)
    total = sum(len(p) - 1 for p in parts)
    got = sum(i in found[r] and i + 1 in found[r] for r, p in enumerate(parts) for i in range(len(p) - 1))
    return total, got


def badread_reads(d, fa, n_molecules, seed=7):
    """Badread reads (identity 84 / 99 / 5.5) of whole transcripts drawn from `fa`: (fastq path, [(transcript, 0, length)])"""
    import random
    from tksm_amd.sequence import Sequencer
    models = os.path.join(ROOT, "tksm_amd", "models", "badread")
    names, lens = [], []
    for line in open(fa):
        if line.startswith(">"):
            names.append(line[1:].strip())
        else:
            lens.append(len(line.strip()))
    rs = random.Random(seed)
    pick = [rs.randrange(len(names)) for _ in range(n_molecules)]
    s = Sequencer(0)
    s.get_reference_seqs([fa])
    s.set_identity(84.0, 99.0, 5.5)
    s.load_error_model(os.path.join(models, "nanopore2020.error.gz"))
    s.load_qscore_model(os.path.join(models, "nanopore2020.qscore.gz"))
    b = s.batch_from_mdf("".join(f"+m{i}\t1\t\n{names[t]}\t0\t{lens[t]}\t+\t\n" for i, t in enumerate(pick)))
    records = s.run(b, target="badread", fastq=True, compute_qual=True, seed=seed).records()
    b.free()
    s.close()
    fq = os.path.join(d, "badread.fq")
    with open(fq, "wb") as f:
        for i, rec in enumerate(records):
            rows = bytes(rec).split(b"\n")
            f.write(b"@r%07d\n" % i + rows[1] + b"\n+\n" + rows[3] + b"\n")
    return fq, [(t, 0, lens[t]) for t in pick]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--transcripts", type=int, default=20000)
    ap.add_argument("--reads", type=int, default=200000)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--glue", type=float, default=0.2)
    ap.add_argument("--badread-molecules", type=int, default=20000)
    ap.add_argument("--parent-tree", default=None, help="a built checkout of the parent commit: its map, map -c and map -c --extend times on the same files")
    ap.add_argument("--base-only", nargs=4, metavar=("TREE", "FASTA", "FASTQ", "RUNS"), default=None, help="(the child of --parent-tree) the base calls of TREE's build as one JSON line")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "map_split_times.log"))
    a = ap.parse_args()
    if a.base_only:
        tree, fa, fq, runs = a.base_only
        with tempfile.TemporaryDirectory() as d:
            got = run_calls(tree, fa, fq, d, BASE_CALLS, int(runs))
        print(json.dumps({k: [[w, i] for w, i in v] for k, v in got.items()}))
        return
    lines = []

    def say(text=""):
        print(text, flush=True)
        lines.append(text)

    def flush():
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")

    def spread(name, runs):
        walls, dev = sorted(w for w, _ in runs), sorted(i["device_ms"] + i.get("align", {}).get("align_ms", 0) + i.get("extend", {}).get("extend_ms", 0) for _, i in runs)
        say(f"{name:<28} wall s: min {walls[0]:.3f}, median {statistics.median(walls):.3f}, max {walls[-1]:.3f}; device ms (stages + align + extend): min {dev[0]:.1f}, "
            f"median {statistics.median(dev):.1f}, max {dev[-1]:.1f}; host ms, medians: read {statistics.median(i['read_ms'] for _, i in runs):.0f}, "
            f"upload {statistics.median(i['upload_ms'] for _, i in runs):.0f}, write {statistics.median(i['write_ms'] for _, i in runs):.0f}; {runs[0][1]['lines']} lines")

    def row(name, wall, i):
        extra = f"; split {i['split']['split_ms']:.1f} ms (chain with all rounds + selection)" if "split" in i else ""
        say(f"{name:<22} wall {wall:6.2f} s: read {i['read_ms'] / 1e3:.2f} s, upload {i['upload_ms'] / 1e3:.2f} s, write {i['write_ms'] / 1e3:.2f} s; device " +
            ", ".join(f"{n} {ms:.1f}" for n, ms in zip(STAGES, i["stage_ms"])) + f" ms = {i['device_ms']:.1f} ms{extra}; {i['chunks']} chunk(s), {i['mapped']} mapped, {i['lines']} lines")

    def observe(name, tree_dir, fa, fq, parts):
        got = run_calls(ROOT, fa, fq, tree_dir, (("obs", dict(split=True)),))["obs"][0][1]
        total, found = junctions(os.path.join(tree_dir, "obs.paf"), parts)
        J, M = got["split"]["supplementary"], got["mapped"]
        say(f"{name}: {len(parts)} reads, {total} junctions, {found} recovered ({100.0 * found / max(1, total):.1f} %); {J} supplementary lines in {M} mapped reads: "
            f"unsegment -p estimate {J / max(1, M + J - 1):.4f} beside {a.glue} used to glue (a third piece is never glued on, so the glued share is a little below it)")

    with tempfile.TemporaryDirectory() as d:
        t0 = time.time()
        fa, fq, truth, tx_bases, read_bases = generate(d, a.transcripts, a.reads)
        say(f"map --split: times on the input of tools/map_times.py (seed 1): {a.transcripts} transcripts ({tx_bases} bases), {a.reads} reads ({read_bases} bases, 5 % "
            f"substitutions, both strands) (made in {time.time() - t0:.0f} s).  One machine, one session.")
        say()
        # both builds from child processes of their own, in turn (parent, this, parent, this), so that neither has the warmer files or the
        # longer-lived process; the runs of a build's two children are pooled
        trees = ([("parent", os.path.abspath(a.parent_tree))] if a.parent_tree else []) + [("this build", ROOT)]
        pooled = {label: {} for label, _ in trees}
        for turn in range(2):
            for label, tree in trees:
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--base-only", tree, fa, fq, str(a.runs)], capture_output=True, text=True)
                if r.returncode:
                    raise SystemExit(f"the build in {tree} did not run: {r.stderr[-300:]}")
                for name, runs in json.loads(r.stdout.strip().splitlines()[-1]).items():
                    pooled[label].setdefault(name, []).extend(runs)
        for label, _ in trees:
            say(f"== {label}{' (the parent commit, built beside this one)' if label == 'parent' else ' without --split'}: two child processes of {a.runs} runs each, in turn with "
                f"the other build's; {2 * a.runs} runs pooled ==")
            for name, _ in BASE_CALLS:
                spread(name, pooled[label][name])
            say()
        flush()
        say()
        glued = os.path.join(d, "glued.fq")
        parts = glue(fq, glued, truth, a.glue)
        share = sum(len(p) > 1 for p in parts) / len(parts)
        say(f"== what --split adds: the same reads glued with p = {a.glue}, at most three to a read: {len(parts)} reads, {100 * share:.1f} % of them glued from 2 or 3 ==")
        calls = (("map", {}), ("map --split", dict(split=True)), ("map -c --extend --split", dict(align=True, extend=True, split=True)))
        got = run_calls(ROOT, fa, glued, d, calls)
        for name, _ in calls:
            row(name, *got[name][0])
        for name in ("map --split", "map -c --extend --split"):
            x = got[name][0][1]["split"]
            say(f"{name}: {x['split_reads']} reads split, {x['supplementary']} supplementary lines, {x['rounds']} rounds in {got[name][0][1]['chained_groups']} chained groups, "
                f"{x['later_chains']} kept chains of later rounds, {x['rejected_overlap']} candidates refused for overlap")
        flush()
        say()
        grouped = os.path.join(d, "grouped.fq")
        gparts = glue(fq, grouped, truth, a.glue, grouped=True)
        same = sum(x[0] == y[0] for p in gparts for x, y in zip(p, p[1:]))
        say(f"== the same, the reads ordered by transcript before gluing (as `transcribe` writes molecules, no `shuffle`): {len(gparts)} reads, "
            f"{same} of {sum(len(p) - 1 for p in gparts)} junctions between two reads of one transcript ==")
        calls = (("map", {}), ("map --split", dict(split=True)))
        got = run_calls(ROOT, fa, grouped, d, calls)
        for name, _ in calls:
            row(name, *got[name][0])
        x = got["map --split"][0][1]["split"]
        say(f"map --split: {x['split_reads']} reads split, {x['supplementary']} supplementary lines, {x['rounds']} rounds in {got['map --split'][0][1]['chained_groups']} chained groups, "
            f"{x['later_chains']} kept chains of later rounds, {x['rejected_overlap']} candidates refused for overlap")
        flush()
        say()
        say("== observation: junctions recovered and the estimate of unsegment -p (map --split at the defaults) ==")
        observe("5 % substitutions", d, fa, glued, parts)
        observe("5 % substitutions, ordered by transcript", d, fa, grouped, gparts)
        import numpy as np  # noqa: F401
        exact = os.path.join(d, "exact.fq")
        tx = [l.strip() for l in open(fa, "rb") if not l.startswith(b">")]
        rc = bytes.maketrans(b"ACGT", b"TGCA")
        with open(exact, "wb") as f:
            for r, (t, b, e) in enumerate(truth):
                piece = tx[t][b:e] if r % 2 else tx[t][b:e].translate(rc)[::-1]
                f.write(b"@r%07d\n" % r + piece + b"\n+\n" + b"I" * len(piece) + b"\n")
        exact_glued = os.path.join(d, "exact_glued.fq")
        observe("error-free", d, fa, exact_glued, glue(exact, exact_glued, truth, a.glue))
        flush()
        bfq, btruth = badread_reads(d, fa, a.badread_molecules)        # (what was measured so far is in the file already: a failure here ends the run with its error)
        bglued = os.path.join(d, "badread_glued.fq")
        observe("Badread 84 / 99 / 5.5, whole transcripts", d, fa, bglued, glue(bfq, bglued, btruth, a.glue))
    flush()


if __name__ == "__main__":
    main()
