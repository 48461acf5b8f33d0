"""Times of model-truncation's device work on synthetic alignments, default 100 x 100 grid (0 - 10 000, step 100), bandwidth 100.

    python tools/kde_times.py [sizes=200000,10000000] [reps=5] [cv_samples=20000,100000]

tksmseq_kde_grid is timed whole -- upload of the samples, both kernels, download of the grid -- best of `reps`, and printed with its
arithmetic: 2 N gx gy flop in the matrix product, N (gx + gy) exponentials, and the share of the MI355X's 78.6 TFLOP/s fp64 matrix peak the
product reaches over the time of the call.  The bandwidth search (tksmseq_kde_cv_bandwidth) runs once per entry of `cv_samples` on the first size:
3 repeats x cv_samples^2 x 2/3 distances for the minimum, and ten exponentials each for the sums -- quadratic, so an entry predicted
from the one before it to take more than 400 s is skipped and said so.
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
FP64_MATRIX_PEAK = 78.6e12


def sample(n, seed=1):
    rs = np.random.RandomState(seed)
    tlen = np.clip(rs.lognormal(7.4, 0.6, n), 300, 9900).astype(np.int64)
    trunc = np.minimum(tlen - 100, rs.gamma(1.6, 180.0, n)).astype(np.int64) * (rs.rand(n) < 0.8)
    return np.stack([trunc, tlen], axis=1).astype(np.float64)


def main():
    import torch  # noqa: F401  (the ROCm runtime torch bundles, loaded first as everywhere in the project)
    from tksm_amd.sequence import Sequencer
    sizes = [int(v) for v in (sys.argv[1] if len(sys.argv) > 1 else "200000,10000000").split(",")]
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    cv_samples = [int(v) for v in (sys.argv[3] if len(sys.argv) > 3 else "20000,100000").split(",") if int(v)]
    s = Sequencer(0)
    idx = np.arange(0, 10001, 100)
    c = ((idx[:-1] + idx[1:]) // 2).astype(np.float64)
    s.kde_grid(sample(1000), c, c, 100.0)                         # (first launch: code object load)
    first = None
    for n in sizes:
        xy = sample(n)
        first = xy if first is None else first
        best = None
        for _ in range(reps):
            t = time.perf_counter()
            s.kde_grid(xy, c, c, 100.0)
            dt = time.perf_counter() - t
            best = dt if best is None else min(best, dt)
        flop, exps = 2.0 * n * len(c) * len(c), float(n) * 2 * len(c)
        print(f"kde_grid N={n:9d} grid {len(c)}x{len(c)}: {best * 1e3:9.2f} ms  {flop / best / 1e12:6.2f} TFLOP/s fp64 ({100 * flop / best / FP64_MATRIX_PEAK:5.1f} % of the matrix peak), "
              f"{exps / best / 1e9:7.2f} G exponentials/s ({flop:.3g} flop, {exps:.3g} exponentials)", flush=True)
    per_pair = None
    for m in cv_samples:
        if per_pair is not None and per_pair * m * m > 400.0:
            print(f"kde_cv_bandwidth cv_samples={m}: skipped, predicted {per_pair * m * m:.0f} s", flush=True)
            continue
        t = time.perf_counter()
        bw, scores = s.kde_cv_bandwidth(first, seed=42, cv_samples=m)
        dt = time.perf_counter() - t
        per_pair = dt / (float(m) * m)
        exps = 3 * (2.0 / 3.0) * m * m * 10
        print(f"kde_cv_bandwidth N={len(first)} cv_samples={m}: {dt:8.2f} s  bandwidth {bw:g}  {exps / dt / 1e9:7.2f} G exponentials/s ({exps:.3g} exponentials)", flush=True)
    s.close()


if __name__ == "__main__":
    main()
