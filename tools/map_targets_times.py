#!/usr/bin/env python3
"""map -g: what the splice costs, what map -g costs beside map -r on the written FASTA, and map without -g against the parent commit
(profiles/map_targets_times.log).

  python tools/map_targets_times.py [--transcripts 20000] [--reads 200000] [--runs 5] [--parent-tree DIR] [--out profiles/map_targets_times.log]

The input is that of tools/map_times.py (seed 1): its transcripts and its reads.  For -g a genome and a GTF are made around those
transcripts: each is cut into 1 to 12 exons with introns of 50 to 500 letters between them, every other one on the `-` strand (its exons
in descending file order), 1 000 transcripts to a contig -- so that the spliced targets are the transcripts themselves and the same reads
serve every part.  One machine, one session; every figure says whether it is one run or a median.
1. Splice.  Sequencer.targets() ten times: splice_ms (HIP events: the genome's validity and the splice kernel), letters per second, and the
   bytes the two kernels must move beside what that is per second.  The comparison is with that traffic, not with a target figure.
2. map -g beside map -r <the FASTA of --targets-out> on the same reads: wall and stages, and whether the two PAFs are the same bytes.
3. No regression: map, map -c and map -c --extend without -g, this build and the parent commit's (--parent-tree DIR, a built checkout)
   from child processes in turn, 2 x --runs runs each, and whether both builds write the same bytes."""
import argparse
import hashlib
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from map_extend_times import RC, STAGES, generate  # noqa: E402

BASE_CALLS = (("map", {}), ("map -c", dict(align=True)), ("map -c --extend", dict(align=True, extend=True)))


def sha(path):
    return hashlib.sha256(open(path, "rb").read()).hexdigest()[:16]


def run_calls(tree, fa, fq, d, calls, runs=1):
    """{name: [(wall seconds, info, digest of the PAF)] * runs} of Sequencer.map under every keyword set of `calls`, on one context of the
    build in `tree` whose reference is `fa`"""
    sys.path.insert(0, tree)
    import torch  # noqa: F401  (its ROCm runtime has to be loaded before libtksmseq.so)
    from tksm_amd.sequence import Sequencer
    s = Sequencer(0)
    s.get_reference_seqs([fa])
    out = {name: [] for name, _ in calls}
    for _ in range(runs):
        for name, kw in calls:
            paf = os.path.join(d, name.replace(" ", "_") + ".paf")
            t0 = time.time()
            info = s.map(fq, paf, **kw)
            out[name].append((time.time() - t0, info, sha(paf)))
    s.close()
    return out


def genome_around(fa, d, per_contig=1000, seed=3):
    """a genome and a GTF whose spliced targets are the transcripts of `fa`: (contigs [(name, letters)], gtf path, exons, genome letters)"""
    import numpy as np
    rs = np.random.default_rng(seed)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    tx = [l.strip() for l in open(fa, "rb") if not l.startswith(b">")]
    contigs, gtf, n_exons, at, parts, name = [], [], 0, 0, [], None

    def close():
        if parts:
            contigs.append((name, b"".join(parts).decode()))

    for i, seq in enumerate(tx):
        if i % per_contig == 0:
            close()
            name, parts, at = "chr%02d" % (i // per_contig), [], 0
        n = int(rs.integers(1, 13))
        cuts = [0] + sorted(int(x) for x in rs.choice(np.arange(1, len(seq)), n - 1, replace=False)) + [len(seq)]
        pieces = [seq[a:b] for a, b in zip(cuts, cuts[1:])]
        minus = i % 2 == 1
        rows = []
        for p in (pieces[::-1] if minus else pieces):                            # in genome order
            intron = acgt[rs.integers(0, 4, int(rs.integers(50, 501)))].tobytes()
            parts += [intron, p.translate(RC)[::-1] if minus else p]
            at += len(intron)
            rows.append((at, at + len(p)))
            at += len(p)
        tid = "tx%06d" % i
        gtf.append('%s\tgen\ttranscript\t%d\t%d\t.\t%s\t.\ttranscript_id "%s";' % (name, rows[0][0] + 1, rows[-1][1], "+-"[minus], tid))
        for a, b in (rows[::-1] if minus else rows):                             # in file order: a `-` transcript descends
            gtf.append('%s\tgen\texon\t%d\t%d\t.\t%s\t.\ttranscript_id "%s";' % (name, a + 1, b, "+-"[minus], tid))
        n_exons += n
    close()
    path = os.path.join(d, "genes.gtf")
    with open(path, "w") as f:
        f.write("\n".join(gtf) + "\n")
    return contigs, path, n_exons, sum(len(s) for _, s in contigs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--transcripts", type=int, default=20000)
    ap.add_argument("--reads", type=int, default=200000)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--parent-tree", default=None, help="a built checkout of the parent commit: its map, map -c and map -c --extend on the same files")
    ap.add_argument("--base-only", nargs=4, metavar=("TREE", "FASTA", "FASTQ", "RUNS"), default=None, help="(the child of part 3) the base calls of TREE's build as one JSON line")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "map_targets_times.log"))
    a = ap.parse_args()
    if a.base_only:
        tree, fa, fq, runs = a.base_only
        with tempfile.TemporaryDirectory() as d:
            got = run_calls(tree, fa, fq, d, BASE_CALLS, int(runs))
        print(json.dumps({k: [[w, i, h] for w, i, h in v] for k, v in got.items()}))
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
        walls, dev = sorted(w for w, _, _ in runs), sorted(i["device_ms"] + i.get("align", {}).get("align_ms", 0) + i.get("extend", {}).get("extend_ms", 0) for _, i, _ in runs)
        say(f"{name:<18} wall s: min {walls[0]:.3f}, median {statistics.median(walls):.3f}, max {walls[-1]:.3f}; device ms (stages + align + extend): min {dev[0]:.1f}, "
            f"median {statistics.median(dev):.1f}, max {dev[-1]:.1f}; host ms, medians: read {statistics.median(i['read_ms'] for _, i, _ in runs):.0f}, "
            f"upload {statistics.median(i['upload_ms'] for _, i, _ in runs):.0f}, write {statistics.median(i['write_ms'] for _, i, _ in runs):.0f}; {runs[0][1]['lines']} lines")
        return statistics.median(walls), statistics.median(dev), (walls[0], walls[-1]), (dev[0], dev[-1])

    def row(name, runs):
        """medians of the runs of one call"""
        med = lambda f: statistics.median(f(w, i) for w, i in runs)  # noqa: E731
        say(f"{name:<34} wall {med(lambda w, i: w):6.3f} s: read {med(lambda w, i: i['read_ms']) / 1e3:.2f} s, upload {med(lambda w, i: i['upload_ms']) / 1e3:.2f} s, "
            f"write {med(lambda w, i: i['write_ms']) / 1e3:.2f} s; device " + ", ".join(f"{n} {statistics.median(i['stage_ms'][k] for _, i in runs):.1f}" for k, n in enumerate(STAGES)) +
            f" ms = {med(lambda w, i: i['device_ms']):.1f} ms; {runs[0][1]['chunks']} chunk(s), {runs[0][1]['mapped']} mapped, {runs[0][1]['lines']} lines")

    with tempfile.TemporaryDirectory() as d:
        import torch  # noqa: F401  (its ROCm runtime has to be loaded before libtksmseq.so)
        from tksm_amd.sequence import Sequencer
        t0 = time.time()
        fa, fq, truth, tx_bases, read_bases = generate(d, a.transcripts, a.reads)
        contigs, gtf, n_exons, genome_letters = genome_around(fa, d)
        say(f"map -g: times on the input of tools/map_times.py (seed 1): {a.transcripts} transcripts ({tx_bases} bases), {a.reads} reads ({read_bases} bases, 5 % substitutions, "
            f"both strands); around the transcripts a genome of {len(contigs)} contigs ({genome_letters} letters) and a GTF of {n_exons} exons, 1 to 12 a transcript, every other "
            f"transcript on the - strand (made in {time.time() - t0:.0f} s).  One machine, one session.")
        say()

        # ---- 1. the splice
        s = Sequencer(0)
        for name, seq in contigs:
            s.add_contig(name, seq)
        s.add_gtf(gtf)
        ms, info = [], None
        for _ in range(11):
            t = s.targets()
            info = t.info
            ms.append(info["splice_ms"])
            t.free()
        first, ms = ms[0], sorted(ms[1:])
        med = statistics.median(ms)
        g_vwords = sum((len(seq) + 4095) // 4096 * 4096 for _, seq in contigs) // 32
        must = g_vwords * 4 + info["letters"] * 3 // 8 + info["image_vwords"] * 12 + info["exons"] * 16
        say("== splice: Sequencer.targets() eleven times on one context, the first apart, then the median of ten ==")
        say(f"{info['targets']} targets of {info['letters']} letters in {info['exons']} exons ({info['projectable']} projectable; skipped {info['skipped_empty']} + "
            f"{info['skipped_unknown_contig']} + {info['skipped_bad_exon']}); image {info['image_vwords'] * 12} bytes")
        say(f"splice_ms (HIP events: the genome's validity words and the splice kernel): first {first:.3f}, then min {ms[0]:.3f}, median {med:.3f}, max {ms[-1]:.3f} ms (median of ten)")
        say(f"{info['letters'] / (med / 1e3):.3g} target letters per second; bytes the two kernels must move: {g_vwords * 4} genome validity written + "
            f"{info['letters'] * 3 // 8} exon letters read (codes and validity) + {info['image_vwords'] * 12} image written + {info['exons'] * 16} exon tuples = {must} bytes, "
            f"{must / (med / 1e3) / 1e9:.1f} GB/s at the median (the table look-ups of a lane, cached, are not counted)")
        say()
        flush()

        # ---- 2. map -g beside map -r <written FASTA>
        t = s.targets()
        cdna = os.path.join(d, "cdna.fa")
        t0 = time.time()
        t.write_fasta(cdna)
        t_fasta = time.time() - t0
        r = Sequencer(0)
        r.get_reference_seqs([cdna])
        say(f"== map -g beside map -r <the FASTA of --targets-out> (written in {t_fasta:.2f} s, one run; {os.path.getsize(cdna)} bytes), the same reads; medians of {a.runs} runs, "
            "the two contexts in turn ==")
        same = (b"".join(l.strip() for l in open(cdna, "rb") if not l.startswith(b">")) == b"".join(l.strip() for l in open(fa, "rb") if not l.startswith(b">")))
        say(f"the written FASTA holds the letters of the transcripts the genome was made around: {same}")
        for name, kw in BASE_CALLS:
            g_runs, r_runs = [], []
            for _ in range(a.runs):
                t0 = time.time()
                gi = s.map(fq, os.path.join(d, "g.paf"), targets=t, **kw)
                g_runs.append((time.time() - t0, gi))
                t0 = time.time()
                ri = r.map(fq, os.path.join(d, "r.paf"), **kw)
                r_runs.append((time.time() - t0, ri))
            row(name + " -g", g_runs)
            row(name + " -r cdna.fa", r_runs)
            say(f"{name}: the two PAFs are the same bytes: {sha(os.path.join(d, 'g.paf')) == sha(os.path.join(d, 'r.paf'))}")
        t0 = time.time()
        gi = s.map(fq, os.path.join(d, "gc.paf"), targets=t, genome_coords=True, align=True)
        say(f"map -c -g --genome-coords (one run): wall {time.time() - t0:.3f} s, write {gi['write_ms'] / 1e3:.2f} s; {gi['project']}")
        t.free()
        r.close()
        s.close()
        say()
        flush()

        # ---- 3. no regression without -g: both builds from child processes of their own, in turn (parent, this, parent, this)
        trees = ([("parent", os.path.abspath(a.parent_tree))] if a.parent_tree else []) + [("this build", ROOT)]
        pooled = {label: {} for label, _ in trees}
        for turn in range(2):
            for label, tree in trees:
                c = subprocess.run([sys.executable, os.path.abspath(__file__), "--base-only", tree, fa, fq, str(a.runs)], capture_output=True, text=True)
                if c.returncode:
                    raise SystemExit(f"the build in {tree} did not run: {c.stderr[-300:]}")
                for name, runs in json.loads(c.stdout.strip().splitlines()[-1]).items():
                    pooled[label].setdefault(name, []).extend(runs)
        stats = {}
        for label, _ in trees:
            say(f"== {label}{' (the parent commit, built beside this one)' if label == 'parent' else ''} without -g, -r tx.fa: two child processes of {a.runs} runs each, in turn "
                f"with the other build's; {2 * a.runs} runs pooled ==")
            for name, _ in BASE_CALLS:
                stats[label, name] = spread(name, pooled[label][name])
            say()
        if a.parent_tree:
            for name, _ in BASE_CALLS:
                wall, dev, _, _ = stats["this build", name]
                _, _, pw, pd = stats["parent", name]
                digests = {h for label, _ in trees for _, _, h in pooled[label][name]}
                say(f"{name:<18} this build's device median {dev:.1f} ms {'lies inside' if pd[0] <= dev <= pd[1] else 'lies OUTSIDE'} the parent's min-max {pd[0]:.1f} .. {pd[1]:.1f} ms; "
                    f"wall median {wall:.3f} s beside the parent's {pw[0]:.3f} .. {pw[1]:.3f} s; all {sum(len(pooled[label][name]) for label, _ in trees)} PAFs of both builds "
                    f"are the same bytes: {len(digests) == 1}")
    flush()


if __name__ == "__main__":
    main()
