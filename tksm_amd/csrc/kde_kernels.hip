// kde_kernels.hip -- the KDE truncation model on the device (gfx950).
//
// Reference behaviour restated (file:line into vpc-ccg/tksm):
//   ComputeKDELikelihoods   py/truncate_kde.py:245-287   KernelDensity(bandwidth).fit(samples).score_samples(grid centres), exp'ed
//   CV_KDE_bandwidth        py/truncate_kde.py:223-242   GridSearchCV(KernelDensity(), bandwidth in 50 .. 950, cv = 3) on a subsample
// The Gaussian kernel is separable, so the density of every grid point is one matrix product over the samples:
//   P[i][j] = 1 / (N 2 pi h^2) sum_n A[n][i] B[n][j],  A[n][i] = exp(-(x_n - px_i)^2 / 2h^2),  B[n][j] = exp(-(y_n - py_j)^2 / 2h^2)
// -- N (gx + gy) exponentials and a gx x gy x N fp64 GEMM on v_mfma_f64_16x16x4_f64.  No floating-point atomics anywhere: every chunk of
// samples writes a partial grid, and a second kernel adds the partials in chunk order, so the same input gives the same bytes.
#include "kde_kernels.h"

namespace tk {

typedef double kde_d4 __attribute__((ext_vector_type(4)));

constexpr int KDE_KS = 16;                         // samples per LDS step (four MFMA k-steps)
constexpr int KDE_LDS_ROW = KDE_TILE_BLOCK + 16;   // doubles per LDS row (1152 B = 128 modulo the banks' 256 B): the two k-rows of a half-wave never share a bank
constexpr int KDE_TILES = KDE_TILE_BLOCK / 16;     // 8 x 8 tiles per workgroup, tile rows w and w + 4 on wave w

// One workgroup (4 waves) = one chunk of samples x one block of 128 x 128 grid points.  Per step of 16 samples every thread computes the
// factors of ONE axis point (threads 0..127: A of px, 128..255: B of py) into LDS -- each factor once per (sample, axis point) of the block --
// and every wave then feeds its 2 x 8 tiles from there: lane l supplies A[i = l & 15][k = l >> 4] and B[k = l >> 4][j = l & 15]; the f64
// result tile has column l & 15 on the lane and rows (l >> 4) + 4 r in its four registers.  Axis points beyond gx / gy and samples beyond the
// chunk's end get the factor 0, which adds exactly 0.
__global__ __launch_bounds__(256) void k_kde_grid(const double* __restrict__ xy, uint64_t n, const double* __restrict__ px, uint32_t gx,
                                                  const double* __restrict__ py, uint32_t gy, double inv_h, uint64_t chunk, uint32_t nbj,
                                                  double* __restrict__ partial) {
    __shared__ double sm[2][KDE_KS][KDE_LDS_ROW];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t bi = blockIdx.y / nbj, bj = blockIdx.y % nbj;
    const uint32_t i0 = bi * KDE_TILE_BLOCK, j0 = bj * KDE_TILE_BLOCK;
    const uint32_t nti = min((uint32_t)KDE_TILES, (gx - i0 + 15u) / 16u), ntj = min((uint32_t)KDE_TILES, (gy - j0 + 15u) / 16u);
    const uint64_t cbeg = (uint64_t)blockIdx.x * chunk, cend = min(n, cbeg + chunk);
    // this thread's axis point
    const uint32_t axis = tid >> 7, c = tid & 127u;
    const uint32_t gi = (axis ? j0 : i0) + c;
    const bool valid = gi < (axis ? gy : gx);
    const double p = valid ? (axis ? py[gi] : px[gi]) : 0.0;

    kde_d4 acc[2][KDE_TILES];
#pragma unroll
    for (int r = 0; r < 2; r++)
#pragma unroll
        for (int t = 0; t < KDE_TILES; t++) acc[r][t] = kde_d4{0.0, 0.0, 0.0, 0.0};

    for (uint64_t s0 = cbeg; s0 < cend; s0 += KDE_KS) {
#pragma unroll 4
        for (int k = 0; k < KDE_KS; k++) {
            const uint64_t s = s0 + (uint64_t)k;
            double f = 0.0;
            if (valid && s < cend) {
                const double u = (xy[2 * s + axis] - p) * inv_h;
                f = exp(-0.5 * (u * u));
            }
            sm[axis][k][c] = f;
        }
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < KDE_KS / 4; kk++) {
            const int row = kk * 4 + (int)(lane >> 4);
            double a[2], b[KDE_TILES];
#pragma unroll
            for (int r = 0; r < 2; r++) a[r] = sm[0][row][(wave + 4u * r) * 16u + (lane & 15u)];
#pragma unroll
            for (int t = 0; t < KDE_TILES; t++) b[t] = sm[1][row][t * 16 + (lane & 15u)];
#pragma unroll
            for (int r = 0; r < 2; r++) {
                if (wave + 4u * r < nti) {
#pragma unroll
                    for (int t = 0; t < KDE_TILES; t++)
                        if ((uint32_t)t < ntj) acc[r][t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[r], b[t], acc[r][t], 0, 0, 0);
                }
            }
        }
        __syncthreads();
    }
    double* out = partial + (uint64_t)blockIdx.x * gx * gy;
#pragma unroll
    for (int r = 0; r < 2; r++)
#pragma unroll
        for (int t = 0; t < KDE_TILES; t++) {
            const uint32_t j = j0 + (uint32_t)t * 16u + (lane & 15u);
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const uint32_t i = i0 + (wave + 4u * r) * 16u + (lane >> 4) + 4u * q;
                if (i < gx && j < gy) out[(uint64_t)i * gy + j] = acc[r][t][q];
            }
        }
}

__global__ __launch_bounds__(256) void k_kde_sum(const double* __restrict__ partial, uint64_t n_chunks, uint64_t cells, double scale,
                                                 double* __restrict__ out) {
    const uint64_t cidx = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (cidx >= cells) return;
    double t = 0.0;
    for (uint64_t ch = 0; ch < n_chunks; ch++) t += partial[ch * cells + cidx];
    out[cidx] = t * scale;
}

// ---- bandwidth search: one lane per test point, the train points streamed through LDS 256 at a time
__global__ __launch_bounds__(256) void k_kde_cv_min(const double* __restrict__ pts, uint32_t n, uint32_t b1, uint32_t b2, uint32_t u0, uint32_t u1,
                                                    double* __restrict__ d2min) {
    __shared__ double sx[256], sy[256];
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    const bool live = t < n;
    const double x = live ? pts[2ull * t] : 0.0, y = live ? pts[2ull * t + 1] : 0.0;
    const uint32_t fb = t < b1 ? 0u : t < b2 ? b1 : b2, fe = t < b1 ? b1 : t < b2 ? b2 : n;     // t's own fold: never a train point
    double m = (u0 == 0u || !live) ? __builtin_huge_val() : d2min[t];
    for (uint32_t base = u0; base < u1; base += 256u) {
        const uint32_t u = base + threadIdx.x;
        if (u < u1) { sx[threadIdx.x] = pts[2ull * u]; sy[threadIdx.x] = pts[2ull * u + 1]; }
        __syncthreads();
        const uint32_t cnt = min(256u, u1 - base);
        for (uint32_t q = 0; q < cnt; q++) {
            const uint32_t v = base + q;
            const double dx = x - sx[q], dy = y - sy[q];
            const double d2 = dx * dx + dy * dy;
            if ((v < fb || v >= fe) && d2 < m) m = d2;
        }
        __syncthreads();
    }
    if (live) d2min[t] = m;
}

__global__ __launch_bounds__(256) void k_kde_cv_sum(const double* __restrict__ pts, uint32_t n, uint32_t b1, uint32_t b2, uint32_t u0, uint32_t u1,
                                                    const double* __restrict__ d2min, KdeCvScales sc, double* __restrict__ sums) {
    __shared__ double sx[256], sy[256];
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    const bool live = t < n;
    const double x = live ? pts[2ull * t] : 0.0, y = live ? pts[2ull * t + 1] : 0.0;
    const uint32_t fb = t < b1 ? 0u : t < b2 ? b1 : b2, fe = t < b1 ? b1 : t < b2 ? b2 : n;
    const double m = live ? d2min[t] : 0.0;
    double acc[KDE_N_BW];
#pragma unroll
    for (int k = 0; k < KDE_N_BW; k++) acc[k] = (u0 == 0u || !live) ? 0.0 : sums[(uint64_t)t * KDE_N_BW + k];
    for (uint32_t base = u0; base < u1; base += 256u) {
        const uint32_t u = base + threadIdx.x;
        if (u < u1) { sx[threadIdx.x] = pts[2ull * u]; sy[threadIdx.x] = pts[2ull * u + 1]; }
        __syncthreads();
        const uint32_t cnt = min(256u, u1 - base);
        for (uint32_t q = 0; q < cnt; q++) {
            const uint32_t v = base + q;
            if (v < fb || v >= fe) {
                const double dx = x - sx[q], dy = y - sy[q];
                const double rel = (dx * dx + dy * dy) - m;
#pragma unroll
                for (int k = 0; k < KDE_N_BW; k++) acc[k] += exp(-(rel * sc.c[k]));
            }
        }
        __syncthreads();
    }
    if (live) {
#pragma unroll
        for (int k = 0; k < KDE_N_BW; k++) sums[(uint64_t)t * KDE_N_BW + k] = acc[k];
    }
}

static hipError_t launched() { return hipGetLastError(); }

hipError_t launch_kde_grid(const double* xy, uint64_t n, const double* px, uint32_t gx, const double* py, uint32_t gy, double inv_h, uint64_t chunk,
                           double* partial, hipStream_t s) {
    const uint32_t nbi = (gx + KDE_TILE_BLOCK - 1) / KDE_TILE_BLOCK, nbj = (gy + KDE_TILE_BLOCK - 1) / KDE_TILE_BLOCK;
    const uint64_t n_chunks = (n + chunk - 1) / chunk;
    hipLaunchKernelGGL(k_kde_grid, dim3((uint32_t)n_chunks, nbi * nbj), dim3(256), 0, s, xy, n, px, gx, py, gy, inv_h, chunk, nbj, partial);
    return launched();
}

hipError_t launch_kde_sum(const double* partial, uint64_t n_chunks, uint64_t cells, double scale, double* out, hipStream_t s) {
    hipLaunchKernelGGL(k_kde_sum, dim3((uint32_t)((cells + 255) / 256)), dim3(256), 0, s, partial, n_chunks, cells, scale, out);
    return launched();
}

hipError_t launch_kde_cv_min(const double* pts, uint32_t n, uint32_t b1, uint32_t b2, uint32_t u0, uint32_t u1, double* d2min, hipStream_t s) {
    hipLaunchKernelGGL(k_kde_cv_min, dim3((n + 255u) / 256u), dim3(256), 0, s, pts, n, b1, b2, u0, u1, d2min);
    return launched();
}

hipError_t launch_kde_cv_sum(const double* pts, uint32_t n, uint32_t b1, uint32_t b2, uint32_t u0, uint32_t u1, const double* d2min, KdeCvScales sc,
                             double* sums, hipStream_t s) {
    hipLaunchKernelGGL(k_kde_cv_sum, dim3((n + 255u) / 256u), dim3(256), 0, s, pts, n, b1, b2, u0, u1, d2min, sc, sums);
    return launched();
}

}  // namespace tk
