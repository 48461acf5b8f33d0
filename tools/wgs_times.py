"""Rates of random-wgs (tksmseq_wgs, `tksm sequence --wgs-*`) on one device.

    python tools/wgs_times.py [n=2000000] [reps=5] [stream_molecules=4000000]

1. tksmseq_wgs device to device on n candidates: the call timed whole -- plan, scans, cut, write and batch finalisation (read lengths,
   sort by length) -- best of `reps`, as molecules/s.
2. The streaming rate of `tksm sequence --wgs-*` into /dev/null against the same molecules read from MDF text with -i (written by
   `tksm random-wgs` first): three runs each, interleaved, the CLI's own stage clocks (TKSMSEQ_STATS_FILE); medians, and the text
   route's spread (max - min) / median.
3. A synthetic reference with a few percent of N runs: the share of fragments that take the exact wave-wide kernel (they touch a
   non-ACGT byte) and Badread reads/s with and without the N runs.
"""
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
EXE = os.path.join(ROOT, "tksm_amd", "tksm")
MODELS = os.path.join(ROOT, "tksm_amd", "models", "badread")


def genome(n_contigs, length, n_share=0.0, run=5000, seed=1):
    rs = np.random.RandomState(seed)
    ref = {}
    for i in range(n_contigs):
        b = rs.choice(np.frombuffer(b"ACGT", np.uint8), length)
        for st in rs.randint(0, length - run, int(n_share * length / run)):
            b[st:st + run] = ord("N")
        ref[f"chr{i + 1}"] = b
    return ref


def write_fasta(path, ref):
    with open(path, "wb") as f, open(path + ".fai", "w") as fai:
        off = 0
        for name, b in ref.items():
            head = f">{name}\n".encode()
            f.write(head)
            off += len(head)
            fai.write(f"{name}\t{len(b)}\t{off}\t{len(b)}\t{len(b) + 1}\n")
            f.write(b.tobytes() + b"\n")
            off += len(b) + 1


def cli_stream(args, stats):
    env = dict(os.environ, TKSMSEQ_STATS_FILE=stats)
    t = time.perf_counter()
    r = subprocess.run([EXE, "sequence", *args], capture_output=True, text=True, env=env)
    wall = time.perf_counter() - t
    if r.returncode:
        raise SystemExit(r.stderr)
    st = json.load(open(stats))
    return st["reads"] / st["stream_s"] / 1e6, st, wall


def main():
    import torch  # noqa: F401  (the ROCm runtime torch bundles, loaded first as everywhere in the project)
    from tksm_amd.sequence import Sequencer
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 2_000_000
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    n_stream = int(sys.argv[3]) if len(sys.argv) > 3 else 4_000_000

    # 1. the generator alone
    s = Sequencer(0)
    for i in range(24):
        s.declare_contig(f"chr{i + 1}", 130_000_000 - 4_000_000 * i)
    for name, dist, a, b in (("normal 8000 3000", "normal", 8000.0, 3000.0), ("lognormal 8.5 0.7", "lognormal", 8.5, 0.7), ("exponential 0.0002", "exponential", 0.0002, 0.0)):
        best, mols = None, 0
        for _ in range(reps):
            s.synchronize()
            t = time.perf_counter()
            out, st = s.wgs(dist, a, b, base_count=10**15, n_candidates=n)
            dt = time.perf_counter() - t
            mols = out.n_reads
            out.free()
            best = dt if best is None else min(best, dt)
        print(f"tksmseq_wgs {name:20s} {n} candidates -> {mols} molecules  {best * 1e3:9.2f} ms  {mols / best / 1e6:8.1f} M molecules/s", flush=True)
    s.close()

    # 2. streaming: chained against the same molecules from MDF text
    with tempfile.TemporaryDirectory() as d:
        fa, mdf, stats = os.path.join(d, "g.fa"), os.path.join(d, "x.mdf"), os.path.join(d, "stats.json")
        write_fasta(fa, genome(8, 4_000_000))
        dist, mean = "normal 300 60", 300
        bases = n_stream * mean
        r = subprocess.run([EXE, "random-wgs", "-r", fa, "--frag-len-dist", dist, "--base-count", str(bases), "-o", mdf], capture_output=True, text=True)
        if r.returncode:
            raise SystemExit(r.stderr)
        print(f"streaming: {dist}, {bases} bases; MDF text {os.path.getsize(mdf) / 1e6:.0f} MB", flush=True)
        text_args = ["-r", fa, "-i", mdf, "--perfect", "/dev/null"]
        wgs_args = ["-r", fa, "--wgs-frag-len-dist", dist, "--wgs-base-count", str(bases), "--wgs-batch-molecules", "1000000", "--perfect", "/dev/null"]
        rates = {"text": [], "chained": []}
        for k in range(3):
            for what, args in (("text", text_args), ("chained", wgs_args)):
                rate, st, wall = cli_stream(args, stats)
                rates[what].append(rate)
                print(f"run {k} {what:8s} wall {wall:.2f} s; stream {st['stream_s']:.4f} s = {rate:.2f} M reads/s; reads {st['reads']}; batches {st['batches']}; summed stage seconds: "
                      f"read {st['read_count_s']}, parse / make {st['parse_s']}, run {st['run_s']}, device copy {st['device_copy_s']}, d2h wait {st['d2h_wait_s']}", flush=True)
        mt, mc = float(np.median(rates["text"])), float(np.median(rates["chained"]))
        spread = (max(rates["text"]) - min(rates["text"])) / mt
        print(f"median text {mt:.2f} M reads/s (spread {100 * spread:.1f} %), median chained {mc:.2f} M reads/s: chained / text = {mc / mt:.3f}; "
              f"gate chained >= text x (1 - spread) = {mt * (1 - spread):.2f}: {'ok' if mc >= mt * (1 - spread) else 'MISSED'}", flush=True)

    # 3. N runs: share of fragments for the exact kernel, Badread reads/s
    for share in (0.0, 0.03):
        s = Sequencer(0)
        for name, b in genome(4, 5_000_000, share, seed=2).items():
            s.add_contig(name, b.tobytes())
        s.set_identity(84.0, 99.0, 5.5)
        s.load_error_model(os.path.join(MODELS, "nanopore2020.error.gz"))
        s.load_qscore_model(os.path.join(MODELS, "nanopore2020.qscore.gz"))
        batch, st = s.wgs("normal", 3000.0, 1000.0, base_count=10**15, n_candidates=100_000)
        best = None
        for _ in range(3):
            s.synchronize()
            t = time.perf_counter()
            s.run(batch, target="badread", fastq=True, compute_qual=True, seed=9)
            s.synchronize()
            dt = time.perf_counter() - t
            best = dt if best is None else min(best, dt)
        diag = s.run_diagnostics()
        print(f"N share {100 * share:.0f} %: {batch.n_reads} fragments (normal 3000 1000), {diag['exact_kernel_reads']} through the exact kernel "
              f"({100.0 * diag['exact_kernel_reads'] / batch.n_reads:.2f} %), Badread {best * 1e3:.1f} ms = {batch.n_reads / best / 1e3:.1f} k reads/s", flush=True)
        batch.free()
        s.close()


if __name__ == "__main__":
    main()
