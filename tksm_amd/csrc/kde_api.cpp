// kde_api.cpp -- C-ABI of model-truncation: tksmseq_kde_grid, tksmseq_kde_cv_bandwidth, tksmseq_model_truncation (include/tksmseq.h).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "ctx.h"
#include "kde_host.h"
#include "kde_kernels.h"
#include "tool_run.h"

namespace {

constexpr double KDE_TWO_PI = 6.283185307179586;
constexpr double KDE_MAX_COORD = 1e150;            // squares of differences stay finite

// the counter-based draw of the kernels (mdf_kernels.hip philox_mol): the first two words of Philox4x32-10 keyed by (seed, g, stream, n)
enum { ST_KDE_CV = 48 };
void philox_xy(uint64_t seed, uint64_t g, uint32_t stream, uint32_t n, uint32_t& x, uint32_t& y) {
    uint32_t c0 = (uint32_t)g, c1 = (uint32_t)(g >> 32), c2 = stream, c3 = n, k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
    for (int r = 0; r < 10; r++) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c0 = n0; c1 = (uint32_t)p1; c2 = n2; c3 = (uint32_t)p0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    x = c0; y = c1;
}

bool finite_coords(const double* v, uint64_t n) {
    for (uint64_t i = 0; i < n; i++) if (!(std::fabs(v[i]) <= KDE_MAX_COORD)) return false;
    return true;
}

int check_bandwidth(tksmseq_ctx* ctx, double h) {
    if (!(h > 0.0) || !std::isfinite(h) || !std::isfinite(1.0 / h) || !(h * h > 0.0) || !std::isfinite(h * h)) {
        ctx->err = "kde: the bandwidth must be positive and finite"; return TKSMSEQ_EINVAL;
    }
    return TKSMSEQ_OK;
}

}  // namespace

extern "C" int tksmseq_kde_grid(tksmseq_ctx* ctx, const double* xy, uint64_t n, const double* px, uint32_t gx, const double* py, uint32_t gy,
                                double bandwidth, double* out) {
    if (!ctx) return TKSMSEQ_EINVAL;
    if (!xy || !px || !py || !out) { ctx->err = "kde grid: null argument"; return TKSMSEQ_EINVAL; }
    if (int rc = check_bandwidth(ctx, bandwidth)) return rc;
    if (!n) { ctx->err = "kde grid: the sample is empty"; return TKSMSEQ_EINVAL; }
    if (!gx || !gy) { ctx->err = "kde grid: an axis has no points"; return TKSMSEQ_EINVAL; }
    if (gx > tk::KDE_MAX_AXIS || gy > tk::KDE_MAX_AXIS) { ctx->err = "kde grid: more than 4096 points on an axis"; return TKSMSEQ_ELIMIT; }
    if (n >= (1ull << 31)) { ctx->err = "kde grid: 2^31 samples or more"; return TKSMSEQ_ELIMIT; }
    if (!finite_coords(xy, 2 * n) || !finite_coords(px, gx) || !finite_coords(py, gy)) { ctx->err = "kde grid: coordinates must be finite (at most 1e150)"; return TKSMSEQ_EINVAL; }
    const uint64_t cells = (uint64_t)gx * gy, chunk = tk::kde_chunk_size(n, gx, gy), n_chunks = (n + chunk - 1) / chunk;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    TmpBuf d_xy(s), d_px(s), d_py(s), d_partial(s), d_out(s);
    HIPCHK(ctx, upload(d_xy, xy, 2 * n, s));
    HIPCHK(ctx, upload(d_px, px, gx, s));
    HIPCHK(ctx, upload(d_py, py, gy, s));
    HIPCHK(ctx, d_partial.ensure(n_chunks * cells * 8));
    HIPCHK(ctx, d_out.ensure(cells * 8));
    HIPCHK(ctx, tk::launch_kde_grid(d_xy.as<double>(), n, d_px.as<double>(), gx, d_py.as<double>(), gy, 1.0 / bandwidth, chunk, d_partial.as<double>(), s));
    const double scale = 1.0 / ((double)n * (KDE_TWO_PI * bandwidth * bandwidth));
    HIPCHK(ctx, tk::launch_kde_sum(d_partial.as<double>(), n_chunks, cells, scale, d_out.as<double>(), s));
    HIPCHK(ctx, download(out, d_out, cells, s));
    HIPCHK(ctx, hipStreamSynchronize(s));
    return TKSMSEQ_OK;
}

extern "C" int tksmseq_kde_cv_bandwidth(tksmseq_ctx* ctx, const double* xy, uint64_t n, uint64_t seed, uint64_t cv_samples, double* bandwidth,
                                        double* scores) {
    if (!ctx) return TKSMSEQ_EINVAL;
    if (!xy || !bandwidth) { ctx->err = "kde bandwidth search: null argument"; return TKSMSEQ_EINVAL; }
    if (!n) { ctx->err = "kde bandwidth search: the sample is empty"; return TKSMSEQ_EINVAL; }
    if (cv_samples < 3) { ctx->err = "kde bandwidth search: three folds need at least 3 samples"; return TKSMSEQ_EINVAL; }
    if (n >= (1ull << 31)) { ctx->err = "kde bandwidth search: 2^31 samples or more"; return TKSMSEQ_ELIMIT; }
    if (cv_samples > (1ull << 24)) { ctx->err = "kde bandwidth search: more than 2^24 cross-validation samples"; return TKSMSEQ_ELIMIT; }
    if (!finite_coords(xy, 2 * n)) { ctx->err = "kde bandwidth search: coordinates must be finite (at most 1e150)"; return TKSMSEQ_EINVAL; }
    const uint32_t m = (uint32_t)cv_samples;
    uint32_t fb[4] = {0, 0, 0, m};                                      // KFold(3): the first m % 3 folds are one longer
    for (uint32_t f = 0; f < 2; f++) fb[f + 1] = fb[f] + m / 3 + (f < m % 3 ? 1u : 0u);
    tk::KdeCvScales sc;
    double hs[tk::KDE_N_BW];
    for (int k = 0; k < tk::KDE_N_BW; k++) { hs[k] = 50.0 + 100.0 * k; sc.c[k] = 1.0 / (2.0 * hs[k] * hs[k]); }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    TmpBuf d_pts(s), d_min(s), d_sums(s);
    HIPCHK(ctx, d_pts.ensure((size_t)m * 16));
    HIPCHK(ctx, d_min.ensure((size_t)m * 8));
    HIPCHK(ctx, d_sums.ensure((size_t)m * 8 * tk::KDE_N_BW));
    std::vector<double> pts((size_t)m * 2), h_min(m), h_sums((size_t)m * tk::KDE_N_BW);
    double best[3];
    for (uint32_t r = 0; r < 3; r++) {
        for (uint32_t t = 0; t < m; t++) {
            uint32_t x, y;
            philox_xy(seed, t, ST_KDE_CV, r, x, y);
            const uint64_t i = (uint64_t)(((unsigned __int128)(((uint64_t)x << 32) | y) * (unsigned __int128)n) >> 64);
            pts[2 * (size_t)t] = xy[2 * i]; pts[2 * (size_t)t + 1] = xy[2 * i + 1];
        }
        HIPCHK(ctx, hipMemcpyAsync(d_pts.p, pts.data(), (size_t)m * 16, hipMemcpyHostToDevice, s));
        for (uint32_t u0 = 0; u0 < m; u0 += tk::KDE_CV_SLAB)
            HIPCHK(ctx, tk::launch_kde_cv_min(d_pts.as<double>(), m, fb[1], fb[2], u0, std::min(m, u0 + tk::KDE_CV_SLAB), d_min.as<double>(), s));
        for (uint32_t u0 = 0; u0 < m; u0 += tk::KDE_CV_SLAB)
            HIPCHK(ctx, tk::launch_kde_cv_sum(d_pts.as<double>(), m, fb[1], fb[2], u0, std::min(m, u0 + tk::KDE_CV_SLAB), d_min.as<double>(), sc, d_sums.as<double>(), s));
        HIPCHK(ctx, download(h_min.data(), d_min, m, s));
        HIPCHK(ctx, download(h_sums.data(), d_sums, (size_t)m * tk::KDE_N_BW, s));
        HIPCHK(ctx, hipStreamSynchronize(s));
        // the score of a fold and bandwidth: its test points in order, then the normalisation; the mean over the folds in fold order
        double mean[tk::KDE_N_BW];
        for (int k = 0; k < tk::KDE_N_BW; k++) {
            double fold[3];
            for (uint32_t f = 0; f < 3; f++) {
                const uint32_t n_test = fb[f + 1] - fb[f], n_train = m - n_test;
                double acc = 0.0;
                for (uint32_t t = fb[f]; t < fb[f + 1]; t++) acc += std::log(h_sums[(size_t)t * tk::KDE_N_BW + k]) - h_min[t] * sc.c[k];
                fold[f] = acc - (double)n_test * std::log((double)n_train * (KDE_TWO_PI * hs[k] * hs[k]));
            }
            mean[k] = (fold[0] + fold[1] + fold[2]) / 3.0;
            if (scores) scores[r * tk::KDE_N_BW + k] = mean[k];
        }
        int arg = 0;
        for (int k = 1; k < tk::KDE_N_BW; k++) if (mean[k] > mean[arg]) arg = k;       // the first maximum
        best[r] = hs[arg];
    }
    std::sort(best, best + 3);
    *bandwidth = best[1];
    return TKSMSEQ_OK;
}

int tkh::kde_build_model(tksmseq_ctx* ctx, const tksmseq_kde_model_params* p, const char* paf_path, const char* out_path, KdeBuildInfo* info) {
    if (!ctx) return TKSMSEQ_EINVAL;
    if (!p || !paf_path || !out_path) { ctx->err = "model-truncation: null argument"; return TKSMSEQ_EINVAL; }
    if (p->end_ratio != -1.0 && !(p->end_ratio >= 0.0 && p->end_ratio <= 1.0)) { ctx->err = "model-truncation: the end ratio must be -1 or within [0, 1]"; return TKSMSEQ_EINVAL; }
    std::vector<long long> idx;
    std::vector<double> centres;
    // (the limit first: counted without building the axis, so a grid far beyond it is ELIMIT as documented, not a failed axis)
    if (p->grid_step > 0 && p->grid_end >= p->grid_start &&
        ((unsigned long long)p->grid_end - (unsigned long long)p->grid_start) / (unsigned long long)p->grid_step > tk::KDE_MAX_AXIS) {
        ctx->err = "model-truncation: more than 4096 grid cells on an axis"; return TKSMSEQ_ELIMIT;
    }
    if (!kde_grid_axes(p->grid_start, p->grid_end, p->grid_step, idx, centres)) { ctx->err = "model-truncation: the grid needs at least two indices (and a positive step)"; return TKSMSEQ_EINVAL; }
    PafSample sample;
    if (!read_paf_sample(paf_path, p->model_lengths != 0, sample, ctx->err)) return ctx->err.compare(0, 8, "PAF line") == 0 ? TKSMSEQ_EINVAL : TKSMSEQ_EIO;
    const uint64_t n = sample.xy.size() / 2;
    if (!n) { ctx->err = std::string("model-truncation: no primary alignment (tp:A:P) in ") + paf_path; return TKSMSEQ_EINVAL; }
    KdeBuildInfo local;
    KdeBuildInfo& I = info ? *info : local;
    I = KdeBuildInfo();
    I.n_pairs = n; I.n_ratios = sample.ratios.size();
    I.bandwidth = p->bandwidth;
    if (!(p->bandwidth > 0.0)) {
        if (int rc = tksmseq_kde_cv_bandwidth(ctx, sample.xy.data(), n, p->seed, p->cv_samples, &I.bandwidth, I.scores)) return rc;
        I.searched = true;
    }
    const uint32_t g = (uint32_t)centres.size();
    std::vector<double> P((size_t)g * g);
    if (int rc = tksmseq_kde_grid(ctx, sample.xy.data(), n, centres.data(), g, centres.data(), g, I.bandwidth, P.data())) return rc;
    if (p->end_ratio != -1.0) std::fill(sample.ratios.begin(), sample.ratios.end(), p->end_ratio);
    std::vector<long long> counts;
    std::vector<double> labels;
    end_histogram(sample.ratios, counts, labels);
    if (!write_trc_model_json(out_path, P, idx, counts, labels, ctx->err)) return TKSMSEQ_EIO;
    return TKSMSEQ_OK;
}

extern "C" int tksmseq_model_truncation(tksmseq_ctx* ctx, const tksmseq_kde_model_params* params, const char* paf_path, const char* out_path) {
    return tkh::kde_build_model(ctx, params, paf_path, out_path, nullptr);
}
