"""Specification of model-truncation: the KDE truncation model built from a PAF (TEST INFRASTRUCTURE ONLY, numpy only).

A plain restatement of py/truncate_kde.py:
  * `read_paf`            the pairs and end ratios of the primary alignments (:158-206), default mode and --model-lengths;
  * `grid_axes`           index labels and cell centres of the square grid (:252-267);
  * `kde_grid_spec`       the EXACT Gaussian KDE with scikit-learn's normalisation 1 / (N 2 pi h^2), in the linear domain, P[i][j] for
                          (px[i], py[j]).  The Gaussian is separable, so the grid is the matrix product A^T B with
                          A[n][i] = exp(-(x_n - px_i)^2 / 2h^2), B[n][j] = exp(-(y_n - py_j)^2 / 2h^2) -- what the HIP kernel k_kde_grid computes;
  * `end_histogram`       np.histogram(end_ratios, bins=np.arange(0, 1.01, 0.01)) (:310);
  * `model_json`          the list printModelJson dumps (:298-320);
  * `cv_bandwidth_spec`   the bandwidth search (:223-242) made reproducible: the three subsamples are drawn WITH replacement from Philox
                          keyed by (seed, draw, ST_KDE_CV, repeat) instead of np.random; three contiguous folds as KFold(3) cuts them;
                          score = mean over folds of sum over the test fold of the exact log density of the train folds; the repeat's
                          bandwidth is the first maximum over 50, 150, ..., 950; the result is the median of the three.
The scikit-learn tree the reference scores with is approximate; the specification is the exact density."""
import math

import numpy as np

from core_modules_spec import philox_np
from wgs_spec import _umul64hi

ST_KDE_CV = 48
BANDWIDTHS = np.arange(50, 1000, 100).astype(np.float64)


# ------------------------------------------------------------------------------------------------ PAF
def read_paf(path, model_lengths=False):
    """(xy float64[N][2], end_ratios list) of the lines that contain tp:A:P.  Default: x = truncation length = tstart + (tlen - tend),
    y = tlen (the reference's variable names are swapped at :341-344: the truncation length is the first coordinate); an end ratio
    when the truncation is above 0.  model_lengths: x = tlen, y = tend - tstart; an end ratio when tlen - alen != 0."""
    xs, ys, ratios = [], [], []
    with open(path) as f:
        for line in f:
            if "tp:A:P" not in line:
                continue
            col = line.rstrip("\n").split("\t")
            strand, tlen, tstart, tend = col[4], int(col[6]), int(col[7]), int(col[8])
            if model_lengths:
                alen = tend - tstart
                trunc = tlen - alen
                xs.append(tlen); ys.append(alen)
                if trunc == 0:
                    continue
            else:
                trunc = tstart + (tlen - tend)
                xs.append(trunc); ys.append(tlen)
                if not trunc > 0:
                    continue
            ratios.append(((tlen - tend) if strand == "+" else tstart) / trunc)
    return np.array([xs, ys], np.float64).T.reshape(-1, 2), ratios


# ------------------------------------------------------------------------------------------------ grid
def grid_axes(grid_start, grid_end, grid_step):
    """(idx, centres): idx = arange(start, end + 1, step), centres[k] = (idx[k] + idx[k + 1]) // 2"""
    idx = np.arange(grid_start, grid_end + 1, grid_step)
    if len(idx) < 2:
        raise ValueError("the grid needs at least two indices")
    return idx, (idx[:-1] + idx[1:]) // 2


def kde_grid_spec(xy, px, py, h, block=4096):
    xy = np.asarray(xy, np.float64).reshape(-1, 2)
    px, py = np.asarray(px, np.float64), np.asarray(py, np.float64)
    n = len(xy)
    if n == 0 or not (h > 0) or not math.isfinite(h):
        raise ValueError("kde grid: empty sample or bad bandwidth")
    inv_h = 1.0 / h
    acc = np.zeros((len(px), len(py)))
    with np.errstate(under="ignore"):
        for a in range(0, n, block):
            u = (xy[a:a + block, 0:1] - px[None, :]) * inv_h
            v = (xy[a:a + block, 1:2] - py[None, :]) * inv_h
            acc += np.exp(-0.5 * (u * u)).T @ np.exp(-0.5 * (v * v))
    return acc * (1.0 / (n * (2.0 * math.pi * h * h)))


def kde_grid_bruteforce(xy, px, py, h):
    """the same cell by cell as a log-sum-exp (independent of the separable form; small inputs only)"""
    xy = np.asarray(xy, np.float64).reshape(-1, 2)
    out = np.empty((len(px), len(py)))
    for i, cx in enumerate(px):
        for j, cy in enumerate(py):
            e = -((xy[:, 0] - cx) ** 2 + (xy[:, 1] - cy) ** 2) / (2.0 * h * h)
            m = e.max()
            out[i, j] = math.exp(m + math.log(np.exp(e - m).sum()) - math.log(len(xy) * 2.0 * math.pi * h * h))
    return out


# ------------------------------------------------------------------------------------------------ model JSON
def end_histogram(ratios, end_ratio=-1):
    if end_ratio != -1:
        ratios = [end_ratio] * len(ratios)
    counts, edges = np.histogram(ratios, bins=np.arange(0, 1.01, 0.01))
    return [int(c) for c in counts], list(edges[1:])


def model_json(P, idx, ratios, end_ratio=-1):
    counts, labels = end_histogram(ratios, end_ratio)
    return [{"name": "KDE_mtx", "shape": list(P.shape), "data": list(P.T.flatten()), "labels": [int(a) for a in list(idx[1:]) + list(idx[1:])]},
            {"name": "end_mtx", "shape": [len(counts)], "data": counts, "labels": labels}]


def model_spec(paf, bandwidth=100.0, grid_start=0, grid_end=10000, grid_step=100, model_lengths=False, end_ratio=-1, seed=42, cv_samples=100000):
    xy, ratios = read_paf(paf, model_lengths)
    if bandwidth <= 0:
        bandwidth = cv_bandwidth_spec(xy, seed, cv_samples)[0]
    idx, c = grid_axes(grid_start, grid_end, grid_step)
    return model_json(kde_grid_spec(xy, c, c, bandwidth), idx, ratios, end_ratio)


# ------------------------------------------------------------------------------------------------ bandwidth search
def cv_draw(n, seed, cv_samples, repeat):
    """indices of repeat's subsample: umul64hi(x << 32 | y, n) with (x, y) the first two words of philox(seed, t, ST_KDE_CV, repeat)"""
    w = philox_np(seed, np.arange(cv_samples, dtype=np.uint64), ST_KDE_CV, repeat)
    return _umul64hi((w[0] << np.uint64(32)) | w[1], n).astype(np.int64)


def fold_bounds(n):
    """KFold(3) without shuffling: contiguous folds, the first n % 3 of them one longer"""
    sizes = [n // 3 + (1 if f < n % 3 else 0) for f in range(3)]
    return np.concatenate([[0], np.cumsum(sizes)])


def log_density_sums(test, train, bandwidths=BANDWIDTHS):
    """sum over the test points of the exact log density of `train`, per bandwidth: log-sum-exp shifted by the largest exponent of a test
    point, -d2min / 2h^2 (the same d2min for every bandwidth)"""
    d2 = np.empty((len(test), len(train)))
    for a in range(0, len(test), 256):
        dx = test[a:a + 256, 0:1] - train[None, :, 0]
        dy = test[a:a + 256, 1:2] - train[None, :, 1]
        d2[a:a + 256] = dx * dx + dy * dy
    d2min = d2.min(axis=1)
    rel = d2 - d2min[:, None]
    out = np.empty(len(bandwidths))
    with np.errstate(under="ignore"):
        for k, h in enumerate(bandwidths):
            c = 1.0 / (2.0 * h * h)
            s = np.exp(-(rel * c)).sum(axis=1)
            out[k] = (np.log(s) - d2min * c).sum() - len(test) * math.log(len(train) * (2.0 * math.pi * h * h))
    return out


def cv_bandwidth_spec(xy, seed=42, cv_samples=100000, with_folds=False):
    """(bandwidth, scores[3][10]) -- scores[r][k]: mean over the three folds; with_folds: also fold_scores[3][3][10] and the draws"""
    xy = np.asarray(xy, np.float64).reshape(-1, 2)
    scores, folds, draws, best = np.empty((3, len(BANDWIDTHS))), np.empty((3, 3, len(BANDWIDTHS))), [], []
    b = fold_bounds(cv_samples)
    for r in range(3):
        idx = cv_draw(len(xy), seed, cv_samples, r)
        pts = xy[idx]
        draws.append(idx)
        for f in range(3):
            test = pts[b[f]:b[f + 1]]
            train = np.concatenate([pts[:b[f]], pts[b[f + 1]:]])
            folds[r, f] = log_density_sums(test, train)
        scores[r] = (folds[r, 0] + folds[r, 1] + folds[r, 2]) / 3.0
        best.append(BANDWIDTHS[int(np.argmax(scores[r]))])
    bw = float(np.median(best))
    return (bw, scores, folds, draws) if with_folds else (bw, scores)
