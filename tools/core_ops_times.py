"""Device-to-device rates of the segment edits polyA, tag, scb and flip (tksmseq_polya / _tag / _scb / _flip) at about 2 M molecules.

    python tools/core_ops_times.py [n=2000000] [reps=5]

Each call is timed whole -- plan, count, scans, write and batch finalisation (read lengths, sort by length) -- on one context; the
best of `reps` is printed as molecules/s.  scb's host share (parsing the comments, de-duplicating the barcodes, re-serialising
the comments) is scb's time minus that of a flip with p = 0, which runs the same generic edit with no host pass.  The input is
parsed from MDF text once (not timed).
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def mdf(n, seed=1):
    rs = np.random.RandomState(seed)
    st = rs.randint(0, 59_000, n)
    ln = rs.randint(200, 1500, n)
    bc = rs.randint(0, 20_000, n)
    nseg = rs.randint(1, 4, n)
    out = []
    for i in range(n):
        out.append(f"+m{i}\t1\tCB=B{bc[i]:05d}ACGTACG;tid=T{i % 977};\n")
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
    print(f"input: {b.n_reads} molecules, {b.n_intervals} segments (made and parsed in {time.perf_counter() - t0:.1f} s)", flush=True)
    ops = [
        ("polyA normal 15,7.5", lambda: s.polya(b, normal=(15.0, 7.5))),
        ("polyA gamma 0.5,30", lambda: s.polya(b, gamma=(0.5, 30.0))),
        ("polyA poisson 4", lambda: s.polya(b, poisson=4.0)),
        ("polyA poisson 60", lambda: s.polya(b, poisson=60.0)),
        ("polyA weibull 1.5,20", lambda: s.polya(b, weibull=(1.5, 20.0))),
        ("tag -3 10 (UMI)", lambda: s.tag(b, format3="10")),
        ("tag -5 28 nt -3 22 nt adapters", lambda: s.tag(b, format5="AATGTACTTCGTTCAGTTACGTATTGCT", format3="GCAATACGTAACTGAACGAAGT")),
        ("scb", lambda: s.scb(b)),
        ("scb, no comments out", lambda: s.scb(b, comments=False)),
        ("flip 0.5", lambda: s.flip(b, 0.5)),
        ("flip 0 (generic edit alone)", lambda: s.flip(b, 0.0)),
    ]
    for name, f in ops:
        best = None
        for _ in range(reps):
            s.synchronize()
            t = time.perf_counter()
            out = f()
            dt = time.perf_counter() - t
            out.free()
            best = dt if best is None else min(best, dt)
        print(f"{name:34s} {best * 1e3:9.2f} ms  {b.n_reads / best / 1e6:8.1f} M molecules/s", flush=True)
    b.free()
    s.close()


if __name__ == "__main__":
    main()
