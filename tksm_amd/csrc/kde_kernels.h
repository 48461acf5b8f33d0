// kde_kernels.h -- device side of model-truncation (py/truncate_kde.py): the Gaussian KDE of a 2-D sample on a grid of points as one
// fp64 matrix product, and the distance / shifted-sum passes of the cross-validated bandwidth search.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace tk {

constexpr uint32_t KDE_MAX_AXIS = 4096;            // grid points per axis
constexpr uint64_t KDE_CHUNK = 4096;               // samples per partial grid; doubled until the partials fit (kde_chunk_size)
constexpr uint64_t KDE_PARTIAL_BYTES = 1ull << 30; // all partial grids of one call
constexpr uint64_t KDE_MAX_CHUNKS = 1024;
constexpr int KDE_TILE_BLOCK = 128;                // axis points of one workgroup's block of 8 x 8 MFMA tiles
constexpr int KDE_N_BW = 10;                       // bandwidths of the search: 50, 150, ..., 950 (np.arange(50, 1000, 100))
constexpr uint32_t KDE_CV_SLAB = 8192;             // train points per launch of the search's kernels

// samples per chunk: a function of (n, gx, gy) only, so the same input gives the same partial sums -- and bytes -- on every device
inline uint64_t kde_chunk_size(uint64_t n, uint32_t gx, uint32_t gy) {
    uint64_t chunk = KDE_CHUNK;
    const uint64_t grid_bytes = (uint64_t)gx * gy * 8;
    for (;;) {
        const uint64_t n_chunks = (n + chunk - 1) / chunk;
        if (n_chunks <= 1 || (n_chunks <= KDE_MAX_CHUNKS && n_chunks * grid_bytes <= KDE_PARTIAL_BYTES)) return chunk;
        chunk *= 2;
    }
}

// partial[c][i][j] = sum over the samples of chunk c of exp(-((x - px[i]) inv_h)^2 / 2) exp(-((y - py[j]) inv_h)^2 / 2)
hipError_t launch_kde_grid(const double* xy, uint64_t n, const double* px, uint32_t gx, const double* py, uint32_t gy, double inv_h, uint64_t chunk,
                           double* partial, hipStream_t s);
// out[i][j] = scale x the partials added in chunk order
hipError_t launch_kde_sum(const double* partial, uint64_t n_chunks, uint64_t cells, double scale, double* out, hipStream_t s);

// bandwidth search on pts[n][2] cut into three contiguous folds at b1, b2: for test point t, over the train points u of [u0, u1) outside
// t's fold, d2min[t] = min |t - u|^2 (carried across calls; u0 == 0 starts it) ...
hipError_t launch_kde_cv_min(const double* pts, uint32_t n, uint32_t b1, uint32_t b2, uint32_t u0, uint32_t u1, double* d2min, hipStream_t s);
// ... and sums[t][k] += exp(-(|t - u|^2 - d2min[t]) c[k]) in the order of u, c[k] = 1 / 2 h_k^2
struct KdeCvScales { double c[KDE_N_BW]; };
hipError_t launch_kde_cv_sum(const double* pts, uint32_t n, uint32_t b1, uint32_t b2, uint32_t u0, uint32_t u1, const double* d2min, KdeCvScales sc,
                             double* sums, hipStream_t s);

}  // namespace tk
