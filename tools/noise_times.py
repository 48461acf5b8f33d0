"""Device-to-device rates of tail-noise (tksmseq_append_noise) at about 2 M molecules of about 1 kb in 1 - 3 segments, next to the
project's yardstick for a segment edit, measured in the same run.

    python tools/noise_times.py [n=2000000] [reps=5]

Each call is timed whole -- plan, count, scans, write and batch finalisation (read lengths, sort by length) -- on one context; the best
of `reps` is printed as molecules/s, and for the palindromic mode the substitutions the hairpins wrote per second as well (copied and
new ones: the growth of the batch's substitution table over the time of the call).  The yardstick is a flip with p = 0: the generic edit alone, no draws used.
The input is parsed from MDF text once (not timed).
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def mdf(n, seed=1):
    rs = np.random.RandomState(seed)
    st = rs.randint(0, 58_000, n)
    ln = rs.randint(500, 1500, n)
    nseg = rs.randint(1, 4, n)
    out = []
    for i in range(n):
        out.append(f"+m{i}\t1\ttid=T{i % 977};\n")
        for k in range(nseg[i]):
            out.append(f"chr{1 + ((i + k) & 1)}\t{st[i]}\t{st[i] + ln[i] // nseg[i]}\t{'+-'[(i + k) & 1]}\t{k}G\n")
    return "".join(out)


def main():
    import torch  # noqa: F401  (the ROCm runtime torch bundles, loaded first as everywhere in the project)
    from tksm_amd.sequence import Sequencer
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 2_000_000
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    s = Sequencer(0)
    rs = np.random.RandomState(2)
    for c in ("chr1", "chr2"):
        s.add_contig(c, rs.choice(np.frombuffer(b"ACGT", np.uint8), 60_000).tobytes().decode())
    t0 = time.perf_counter()
    b = s.batch_from_mdf(mdf(n))
    print(f"input: {b.n_reads} molecules, {b.n_intervals} segments, {b.n_mods} substitutions (made and parsed in {time.perf_counter() - t0:.1f} s)", flush=True)
    ops = [
        ("flip 0 (generic edit alone)", lambda: s.flip(b, 0.0)),
        ("random normal,50,10", lambda: s.append_noise(b, "normal", 50.0, 10.0)),
        ("palindromic normal,500,150 rate 0", lambda: s.append_noise(b, "normal", 500.0, 150.0, palindromic=True, error_rate=0.0)),
        ("palindromic normal,500,150 rate 0.5", lambda: s.append_noise(b, "normal", 500.0, 150.0, palindromic=True, error_rate=0.5)),
    ]
    for name, f in ops:
        best, grown = None, 0
        for _ in range(reps):
            s.synchronize()
            t = time.perf_counter()
            out = f()
            dt = time.perf_counter() - t
            grown = out.n_mods - b.n_mods
            out.free()
            best = dt if best is None else min(best, dt)
        subs = f"  {grown / best / 1e6:9.1f} M hairpin substitutions/s ({grown} written, copied and new)" if grown else ""
        print(f"{name:38s} {best * 1e3:9.2f} ms  {b.n_reads / best / 1e6:8.1f} M molecules/s{subs}", flush=True)
    b.free()
    s.close()


if __name__ == "__main__":
    main()
