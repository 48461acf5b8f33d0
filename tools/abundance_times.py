"""Times of abundance on a synthetic PAF: 2 M reads, 5 M records, 100 k transcripts (seeded; lognormal transcript weights, 1 - 5 records per
read on neighbouring transcripts, a tenth of the reads with a poor best hit).

    python tools/abundance_times.py gen PAF [reads=2000000] [transcripts=100000] [seed=1]
    python tools/abundance_times.py device PAF [reps=3]         # on the GPU: device time by HIP events, wall time of the library call and of `tksm abundance`
    python tools/abundance_times.py reference PAF SCRIPT        # SCRIPT: the reference's py/transcript_abundance.py; wall time of its main()

`device` prints the device time of compatibility + index + 10 rounds + split (tksmseq_abundance_device_ms), the wall time of
Sequencer.abundance and of the whole module, and the share of the module's wall time that is not device time (reading and parsing the PAF,
interning names, the uploads, writing the table)."""
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def generate(path, n_reads=2_000_000, n_t=100_000, seed=1):
    rs = np.random.RandomState(seed)
    w = rs.lognormal(0.0, 1.5, n_t)
    t0 = rs.choice(n_t, n_reads, p=w / w.sum())
    k = rs.choice([1, 2, 3, 4, 5], n_reads, p=[0.3, 0.2, 0.2, 0.15, 0.15])          # mean 2.65; trimmed below to 2.5 per read
    k[np.cumsum(k) > int(2.5 * n_reads)] = 1
    qlen = np.clip(rs.lognormal(7.0, 0.4, n_reads), 400, 6000).astype(np.int64)
    poor = rs.rand(n_reads) < 0.1
    blen = np.maximum(20, (qlen * np.where(poor, rs.uniform(0.1, 0.45, n_reads), rs.uniform(0.7, 1.0, n_reads))).astype(np.int64))
    best = np.maximum(10, (blen * rs.uniform(0.85, 0.98, n_reads)).astype(np.int64))
    n_rec = 0
    with open(path, "w") as f:
        for lo in range(0, n_reads, 100_000):
            hi = min(n_reads, lo + 100_000)
            out = []
            for i in range(lo, hi):
                for j in range(k[i]):
                    m = best[i] if j == 0 else int(best[i] * (0.90 + 0.1 * ((i * 7 + j * 13) % 97) / 97.0))
                    ts = (i * 31 + j * 17) % 29 if (i + j) % 10 < 7 else 20 + (i * 13 + j) % 280
                    out.append(f"read{i}\t{qlen[i]}\t0\t{blen[i]}\t+\tENST{(t0[i] + j) % n_t:08d}.1\t9000\t{ts}\t{ts + blen[i]}\t{m}\t{blen[i]}\t60\ttp:A:P\n")
                n_rec += int(k[i])
            f.write("".join(out))
    print(f"{path}: {n_reads} reads, {n_rec} records, {n_t} transcripts, {os.path.getsize(path) / 1e6:.0f} MB (seed {seed})", flush=True)


def device(path, reps=3):
    import torch  # noqa: F401  (the ROCm runtime torch bundles, loaded first as everywhere in the project)
    from tksm_amd.sequence import Sequencer
    s = Sequencer(0)
    small = path + ".head"
    with open(path) as f, open(small, "w") as g:
        for _ in range(1000):
            g.write(f.readline())
    s.abundance(small)                                            # (first launch: code object load)
    os.remove(small)
    best_ms, best_wall, rows, surviving = None, None, 0, 0
    for _ in range(reps):
        t = time.perf_counter()
        r = s.abundance(path)
        wall = time.perf_counter() - t
        rows, surviving = len(r["names"]), r["surviving_reads"]
        best_ms = r["device_ms"] if best_ms is None else min(best_ms, r["device_ms"])
        best_wall = wall if best_wall is None else min(best_wall, wall)
    # a cross-check of the event times: 100 rounds instead of 10, device and wall; the differences are 90 rounds by both clocks
    t = time.perf_counter()
    r100 = s.abundance(path, em_iterations=100)
    wall100 = time.perf_counter() - t
    s.close()
    print(f"100 rounds: device {r100['device_ms']:.2f} ms, wall {wall100:.2f} s; 90 rounds more cost {r100['device_ms'] - best_ms:.2f} ms by the events "
          f"and {1e3 * (wall100 - best_wall):.0f} ms by the wall clock (which also holds the scatter of the host part)", flush=True)
    print(f"Sequencer.abundance: device {best_ms:.2f} ms (compatibility + index + 10 rounds + split, HIP events), wall {best_wall:.2f} s "
          f"(best of {reps}; {surviving} surviving reads, {rows} rows)", flush=True)
    out = path + ".abundance.tsv"
    t = time.perf_counter()
    subprocess.run([os.path.join(ROOT, "tksm_amd", "tksm"), "abundance", "-p", path, "-o", out, "--verbosity", "OFF"], check=True, stdout=subprocess.DEVNULL)
    wall = time.perf_counter() - t
    os.remove(out)
    print(f"tksm abundance: wall {wall:.2f} s for the whole module (process start, context, PAF, device, table); device share {100 * best_ms / 1e3 / wall:.1f} %, "
          f"host share (reading and parsing the PAF, names, uploads, writing) {100 * (1 - best_ms / 1e3 / wall):.1f} %", flush=True)


def reference(path, script):
    import importlib.util
    spec = importlib.util.spec_from_file_location("ref_transcript_abundance", script)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    out = path + ".reference.tsv"
    argv = sys.argv
    sys.argv = ["transcript_abundance.py", "-p", path, "-o", out]
    t = time.perf_counter()
    try:
        mod.main()
    finally:
        sys.argv = argv
    wall = time.perf_counter() - t
    rows = sum(1 for _ in open(out)) - 1
    os.remove(out)
    print(f"reference main(): wall {wall:.2f} s ({rows} rows)", flush=True)


if __name__ == "__main__":
    mode, path = sys.argv[1], sys.argv[2]
    if mode == "gen":
        generate(path, *[int(v) for v in sys.argv[3:6]])
    elif mode == "device":
        device(path, *[int(v) for v in sys.argv[3:4]])
    elif mode == "reference":
        reference(path, sys.argv[3])
    else:
        sys.exit(__doc__)
