"""Rates of transcribe (tksmseq_transcribe, `tksm transcribe`, `tksm sequence --transcribe-*`) on one device.

    python tools/tsb_times.py [molecules=4000000] [reps=5]

1. The host side: seconds of the GTF reader on ~200 k lines (20 000 transcripts of 1 - 15 exons) and of a plan over an abundance table of
   `molecules` rows -- the call as a whole, the device's share of it by HIP events (count, size, four scans), the rest (read, parse,
   join, copies) by difference.
2. The device side for an scRNA-like table (mean depth about 1, about 8 exons per transcript): tksmseq_transcribe over all molecules in
   calls of 1 M, the write kernel by HIP events, summed; best of `reps`; the bytes the kernel writes (intervals, reads, ids, id bytes,
   dup words) per second next to it.
3. The streaming rate of `tksm sequence --transcribe-* --perfect /dev/null` against the same molecules read with -i from the file `tksm
   transcribe` wrote: three runs each, interleaved, the CLI's own stage clocks (TKSMSEQ_STATS_FILE); medians, the text route's spread
   (max - min) / median, and the gate: the chained median is not below the text median by more than that spread.
4. The same with a table of mean depth ~50 (the compact text is small then, and the gain shrinks).
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


def genome(n_contigs, length, seed=1):
    rs = np.random.RandomState(seed)
    return {f"chr{i + 1}": rs.choice(np.frombuffer(b"ACGT", np.uint8), length) for i in range(n_contigs)}


def write_fasta(path, ref):
    with open(path, "wb") as f:
        for name, b in ref.items():
            f.write(f">{name}\n".encode() + b.tobytes() + b"\n")


def write_gtf(path, n_tx, contigs, length, seed=2):
    """n_tx transcripts of 1 - 15 exons (8 on average) of 20 - 59 bases, with gene, CDS and UTR lines around them: ~210 k lines for 20 000"""
    rs = np.random.RandomState(seed)
    lines, n_exons = [], 0
    for t in range(n_tx):
        c, strand = contigs[t % len(contigs)], "+-"[t & 1]
        ne = int(rs.randint(1, 16))
        pos = int(rs.randint(1, length - 16 * 400))
        at = f'gene_id "ENSG{t // 2:011d}"; gene_version "3"; transcript_id "ENST{t:011d}"; gene_name "G{t // 2}"; gene_biotype "protein_coding";'
        if t % 2 == 0:
            lines.append(f"{c}\tsim\tgene\t{pos}\t{pos + 16 * 400}\t.\t{strand}\t.\t{at}\n")
        lines.append(f"{c}\tsim\ttranscript\t{pos}\t{pos + 16 * 400}\t.\t{strand}\t.\t{at}\n")
        for e in range(ne):
            ln = int(rs.randint(20, 60))
            lines.append(f"{c}\tsim\texon\t{pos}\t{pos + ln - 1}\t.\t{strand}\t.\t{at} exon_number \"{e + 1}\";\n")
            if e == 0:
                lines.append(f"{c}\tsim\tCDS\t{pos}\t{pos + ln - 1}\t.\t{strand}\t0\t{at}\n")
            pos += ln + int(rs.randint(50, 300))
        n_exons += ne
    with open(path, "w") as f:
        f.write("".join(lines))
    return len(lines), n_exons


def write_abundance(path, n_rows, n_tx, seed=3):
    rs = np.random.RandomState(seed)
    tx = rs.randint(0, n_tx, n_rows)
    tpm = rs.gamma(0.7, 3.0, n_rows)
    cb = rs.randint(0, 5000, n_rows)
    with open(path, "w") as f:
        f.write("target_id\ttpm\tcell\n")
        for a in range(0, n_rows, 500_000):
            f.write("".join(f"ENST{t:011d}.{t % 7}\t{v:.6f}\tCB{c:014d}\n" for t, v, c in zip(tx[a:a + 500_000].tolist(), tpm[a:a + 500_000].tolist(), cb[a:a + 500_000].tolist())))


def cli_stream(args, stats):
    env = dict(os.environ, TKSMSEQ_STATS_FILE=stats)
    t = time.perf_counter()
    r = subprocess.run([EXE, "sequence", *args], capture_output=True, text=True, env=env)
    wall = time.perf_counter() - t
    if r.returncode:
        raise SystemExit(r.stderr[-2000:])
    st = json.load(open(stats))
    return st["reads"] / st["stream_s"] / 1e6, st, wall


def stream_compare(d, fa, gtf, ab, mc, what):
    mdf, stats = os.path.join(d, "x.mdf"), os.path.join(d, "stats.json")
    t = time.perf_counter()
    r = subprocess.run([EXE, "transcribe", "-g", gtf, "-a", ab, "--molecule-count", str(mc), "-o", mdf, "--verbosity", "ERROR"], capture_output=True, text=True)
    if r.returncode:
        raise SystemExit(r.stderr[-2000:])
    print(f"{what}: `tksm transcribe` {time.perf_counter() - t:.2f} s wall; compact MDF {os.path.getsize(mdf) / 1e6:.0f} MB", flush=True)
    text_args = ["-r", fa, "-i", mdf, "--perfect", "/dev/null", "--verbosity", "ERROR"]
    tsb_args = ["-r", fa, "--transcribe-gtf", gtf, "--transcribe-abundance", ab, "--transcribe-molecule-count", str(mc), "--transcribe-batch-molecules", "1000000",
                "--perfect", "/dev/null", "--verbosity", "ERROR"]
    rates = {"text": [], "chained": []}
    for k in range(3):
        for route, args in (("text", text_args), ("chained", tsb_args)):
            rate, st, wall = cli_stream(args, stats)
            rates[route].append(rate)
            print(f"{what} run {k} {route:8s} wall {wall:.2f} s (set-up {st['setup_s']:.2f} s); stream {st['stream_s']:.4f} s = {rate:.2f} M reads/s; reads {st['reads']}; batches "
                  f"{st['batches']}; summed stage seconds: read {st['read_count_s']}, parse / make {st['parse_s']}, run {st['run_s']}, device copy {st['device_copy_s']}, "
                  f"d2h wait {st['d2h_wait_s']}", flush=True)
    mt, mcn = float(np.median(rates["text"])), float(np.median(rates["chained"]))
    spread = (max(rates["text"]) - min(rates["text"])) / mt
    print(f"{what}: median text {mt:.2f} M reads/s (spread {100 * spread:.1f} %), median chained {mcn:.2f} M reads/s: chained / text = {mcn / mt:.3f}; "
          f"gate chained >= text x (1 - spread) = {mt * (1 - spread):.2f}: {'ok' if mcn >= mt * (1 - spread) else 'MISSED'}", flush=True)
    os.remove(mdf)


def main():
    import torch  # noqa: F401  (the ROCm runtime torch bundles, loaded first as everywhere in the project)
    from tksm_amd.sequence import Sequencer
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 4_000_000
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    n_tx, n_contigs, length = 20_000, 8, 4_000_000
    with tempfile.TemporaryDirectory() as d:
        fa, gtf, ab, ab50 = (os.path.join(d, x) for x in ("g.fa", "ann.gtf", "ab.tsv", "ab50.tsv"))
        ref = genome(n_contigs, length)
        write_fasta(fa, ref)
        n_lines, n_exons = write_gtf(gtf, n_tx, list(ref), length)
        write_abundance(ab, n, n_tx)
        write_abundance(ab50, n // 50, n_tx, seed=4)
        print(f"GTF {n_lines} lines ({os.path.getsize(gtf) / 1e6:.0f} MB), {n_tx} transcripts, {n_exons} exons; abundance {n} rows ({os.path.getsize(ab) / 1e6:.0f} MB)", flush=True)

        s = Sequencer(0)
        for name, b in ref.items():
            s.add_contig(name, b.tobytes())
        s.set_timing(True)
        best = None
        for _ in range(3):
            s.clear_transcripts()
            t = time.perf_counter()
            s.add_gtf(gtf)
            dt = time.perf_counter() - t
            best = dt if best is None else min(best, dt)
        print(f"GTF reader: {best:.3f} s ({n_lines / best / 1e6:.2f} M lines/s), {s.transcripts_info()}", flush=True)
        plan = None
        for k in range(2):
            if plan is not None:
                plan.close()
            s.synchronize()
            t = time.perf_counter()
            plan = s.transcribe_plan(ab, n, seed=42)
            dt = time.perf_counter() - t
            dev_ms = s.transcribe_device_ms()[0]
            print(f"plan {k}: {plan.rows} rows -> {plan.records} records, {plan.molecules} molecules, {len(plan.missing)} missing: {dt:.3f} s in all, device (count, size, 4 scans) "
                  f"{dev_ms:.3f} ms, host (read, parse, join, copies) {dt - dev_ms / 1e3:.3f} s = {plan.rows / (dt - dev_ms / 1e3) / 1e6:.2f} M rows/s", flush=True)
        step = 1_000_000
        best_ms, best_wall, written = None, None, 0
        for _ in range(reps):
            ms, written = 0.0, 0
            s.synchronize()
            t = time.perf_counter()
            for first in range(0, plan.molecules, step):
                b = plan.batch(first, step, comments=False)
                ms += s.transcribe_device_ms()[1]
                written += 16 * b.n_intervals + 20 * b.n_reads + b.n_reads * (1 + len(str(plan.records)))      # (id bytes: an upper estimate)
                b.free()
            wall = time.perf_counter() - t
            best_ms = ms if best_ms is None else min(best_ms, ms)
            best_wall = wall if best_wall is None else min(best_wall, wall)
        print(f"tksmseq_transcribe {plan.molecules} molecules in calls of {step}: write kernel {best_ms:.3f} ms = {plan.molecules / best_ms / 1e3:.0f} M molecules/s, "
              f"~{written / 1e6:.0f} MB written = {written / best_ms / 1e6:.0f} GB/s; the calls as a whole (with the batch finalisation) {best_wall * 1e3:.1f} ms = "
              f"{plan.molecules / best_wall / 1e6:.1f} M molecules/s", flush=True)
        plan.close()
        s.close()

        stream_compare(d, fa, gtf, ab, n, "depth ~1")
        stream_compare(d, fa, gtf, ab50, n, "depth ~50")


if __name__ == "__main__":
    main()
