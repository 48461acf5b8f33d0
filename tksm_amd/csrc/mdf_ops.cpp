// mdf_ops.cpp -- host side of the transforms that edit molecules, one batch in and one batch out, upstream of Seq (BASELINE config 5):
//   tksmseq_pcr            src/pcr.cpp:22-89, :138 (presets), :215-229 (whole input in memory, at most 2 x target templates)
//   tksmseq_truncate       src/truncate.cpp:23-65, :77-227, :322-351, :362-404
//   tksmseq_polya / _tag / _scb / _flip   src/polyA.cpp:133-148, src/tag.cpp:70-113, src/scb.cpp:57-80, src/interval.h:908-920
//   tksmseq_append_noise   src/append_noise.cpp:83-128 (tail-noise: a random literal or a hairpin behind every molecule)
//   tksmseq_mutate         a variant table applied to every segment (the table format of src/mutate.cpp:157-181; the transform is this build's own)
// and finalize_device_batch, which every transform ends with.  The moves (filter, concat, glue, shuffle) are in mdf_move.cpp, the sources
// (random-wgs, transcribe) in mdf_make.cpp, the MDF writer in mdf_text.cpp; mdf_batch.h has what they share.
// The molecule tables stay on the device from one transform to the next and into tksmseq_run; only sizes, per-read lengths
// (which the host needs to size and order a Seq batch) and, for the comments of truncate, the input's segments come back.
#include <atomic>
#include <cmath>
#include <cstring>
#include <unordered_map>

#include "mdf_batch.h"
#include "mut_host.h"

// lengths (python-slice clamped, as Seq sees them), their maximum and sum, and the order sorted by length: what
// batch_from_host computes on the host for an uploaded batch
int finalize_device_batch(tksmseq_ctx* ctx, tksmseq_batch* b) {
    const uint64_t n = b->n_reads;
    b->raw_len.assign(n, 0); b->order.resize(n); b->max_raw = 0; b->total_raw = 0;
    b->splice_len.clear(); b->tail_on = false; b->cache_k = -1;
    HIPCHK(ctx, b->d_order.ensure(n * 4 + 64));
    if (!n) { HIPCHK(ctx, hipStreamSynchronize(ctx->stream)); return TKSMSEQ_OK; }      // (the callers' copies from stack / local buffers have run)
    HIPCHK(ctx, ctx->w_rawlen.ensure(n * 4 + 16));
    HIPCHK(ctx, ctx->w_slotcap.ensure(n * 8 + 16));
    HIPCHK(ctx, ctx->w_status.ensure(n * 4 + 16));
    const tk::RefView R{ctx->d_packed.as<uint32_t>(), ctx->d_blocktab.as<uint32_t>(), ctx->d_pool.as<uint8_t>(), ctx->d_contigs.as<uint64_t>(),
                        (uint32_t)ctx->contig_names.size()};
    HIPCHK(ctx, tk::launch_read_lengths(view_of(b), R, 0, 1, 1, 0, nullptr, ctx->w_rawlen.as<uint32_t>(), ctx->w_slotcap.as<uint64_t>(),
                                        ctx->w_status.as<uint32_t>(), ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(b->raw_len.data(), ctx->w_rawlen.p, n * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    for (uint64_t r = 0; r < n; r++) { b->max_raw = std::max(b->max_raw, b->raw_len[r]); b->total_raw += b->raw_len[r]; b->order[r] = (uint32_t)r; }
    order_by_length(b->raw_len, b->order);
    HIPCHK(ctx, hipMemcpyAsync(b->d_order.p, b->order.data(), n * 4, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return TKSMSEQ_OK;
}

extern "C" {

int tksmseq_pcr_preset(const char* name, double* error_rate, double* efficiency) {
    // Cha & Thilly 1993 as listed in src/pcr.cpp:136-140
    static const struct { const char* n; double er, ef; } P[] = {
        {"Taq-setting1", 2 * std::pow(0.1, 4), 0.88}, {"Taq-setting2", 7.2 * std::pow(0.1, 5), 0.36}, {"Klenow", 1.3 * std::pow(0.1, 4), 0.80},
        {"T7", 3.4 * std::pow(0.1, 5), 0.90},          {"T4", 3.0 * std::pow(0.1, 6), 0.56},          {"Vent", 4.5 * std::pow(0.1, 5), 0.70}};
    if (!name) return TKSMSEQ_EINVAL;
    for (auto& p : P)
        if (!strcmp(p.n, name)) { if (error_rate) *error_rate = p.er; if (efficiency) *efficiency = p.ef; return TKSMSEQ_OK; }
    return TKSMSEQ_EINVAL;
}

// the kernel parameters of a call whose subsample keeps n_kept templates: the drop ratio and the copy-probability tables
static int pcr_tables(tksmseq_ctx* ctx, const tksmseq_pcr_params* p, uint64_t n_kept, tk::PcrParams& P) {
    P = tk::PcrParams{};
    P.seed = p->seed; P.cycles = p->cycles; P.efficiency = p->efficiency; P.rate = (4 * p->error_rate) / 3;
    // drop ratio (src/pcr.cpp:68-76) of the whole input, then the probabilities that a subtree of copies emits nothing
    const double expected_after = std::pow(1 + p->efficiency, p->cycles) * (double)n_kept;
    P.drop = expected_after > 0.0 ? (double)p->target_count / expected_after : 0.0;
    if (P.drop > 1.0) P.drop = 1.0;
    const int c = p->cycles;
    P.A[c] = 1.0; P.A[c + 1] = 1.0;
    // The kernels divide by 1 - q[t] and 1 - A[t].  Both are differences of numbers near 1, so the absolute rounding error of the tables
    // becomes a RELATIVE error of those divisors that grows as the drop ratio shrinks (1 - q[cycles - 1] is the drop ratio itself); at a
    // drop ratio near 2^-53 the divisors round to 0, pm / (1 - A[t]) is 0 / 0 and no copy is ever written.  A running bound of the
    // absolute error goes along with the recursion (standard model: every operation is exact up to a factor 1 +- u, u = 2^-53; eq, eA
    // bound |computed - exact| of q[t], A[t]), and a call whose divisors are not known to PCR_TABLE_REL_ERR = 2^-24 is refused.  A copy's
    // path takes at most 2 x 56 decisions, so every expected count is then off by less than 112 x 2^-24 = 6.7e-6 of itself: one standard
    // deviation of a count of 2.2e10 written copies (BASELINE config 5 writes 2e8).  The 32-bit uniforms the decisions are compared with
    // quantise a probability p to 2^-32 / p of itself already, 7.7e-5 at config 5's drop ratio: far coarser.  ("PCR".)
    // The ratios are taken against the COMPUTED divisors: with a ratio r the true relative error is at most r / (1 - r), r to 24 bits here.
    // (Efficiency 0, or a drop ratio of 0 -- no templates, or a molecule count of 0: nothing is written, which is what the walk gives.)
    const double u = 0x1p-53;
    double eA = 0.0, rel = 0.0;
    for (int t = c - 1; t >= 0; t--) {
        P.q[t] = (1.0 - P.drop) * P.A[t + 1];
        P.A[t] = P.A[t + 1] * (1.0 - P.efficiency * (1.0 - P.q[t]));
        const double eq = eA + 2.0 * u;                                 // 1 - drop: u; the product with A[t + 1] <= 1: eA + u
        const double x = 1.0 - P.q[t], ex = eq + u * x;
        const double y = P.efficiency * x, ey = P.efficiency * ex + u * y;
        const double z = 1.0 - y, ez = ey + u * std::fabs(z);
        eA = eA * std::fabs(z) + (P.A[t + 1] + eA) * ez + u * P.A[t];
        const double a = 1.0 - P.A[t];
        if (P.efficiency > 0.0 && P.drop > 0.0) rel = std::max(rel, std::max(x > 0.0 ? ex / x : INFINITY, a > 0.0 ? (eA + u * a) / a : INFINITY));
    }
    P.q[c] = 1.0;
    if (!(rel <= tk::PCR_TABLE_REL_ERR)) {
        char msg[320];
        snprintf(msg, sizeof msg, "PCR: %d cycles at efficiency %g on %llu templates give a drop ratio of %.3g, which the copy-probability tables do not "
                 "resolve (relative error bound %.3g, limit 2^-24): fewer cycles, or a larger molecule count", c, p->efficiency, (unsigned long long)n_kept, P.drop, rel);
        ctx->err = msg;
        return TKSMSEQ_ELIMIT;
    }
    return TKSMSEQ_OK;
}

// The templates of a PCR call and its kernel parameters, in PROCESSING ORDER.  Templates: every (depth-unrolled) molecule in input order,
// or 2 x target of them when there are more (src/pcr.cpp:217-220 shuffles and cuts: a uniformly random ordered subset; here: the
// 2 x target molecules with the smallest Philox keys, in key order); of those, positions [template_begin, template_end) of that order
// when the caller asks for a slice.  keep empty = every molecule, in input order.
static int pcr_setup(tksmseq_ctx* ctx, const tksmseq_batch* in, const tksmseq_pcr_params* p, std::vector<uint32_t>& keep, uint64_t& n_local, tk::PcrParams& P) {
    if (p->cycles < 0 || p->cycles > tk::PCR_MAX_CYCLES) { ctx->err = "PCR: between 0 and " + std::to_string(tk::PCR_MAX_CYCLES) + " cycles are supported"; return TKSMSEQ_ELIMIT; }
    if (!(p->efficiency >= 0.0) || !(p->error_rate >= 0.0)) { ctx->err = "PCR: efficiency and error rate must be non-negative"; return TKSMSEQ_EINVAL; }
    const uint64_t n = in->n_reads;
    const bool sliced = p->template_begin != 0 || p->template_end != 0;
    if (sliced && (p->template_begin > p->template_end || p->template_end > n)) { ctx->err = "PCR: template slice outside the batch"; return TKSMSEQ_EINVAL; }
    keep.clear();
    uint64_t n_kept = n;
    if (n > 2 * p->target_count) {
        n_kept = 2 * p->target_count;
        std::vector<std::pair<uint64_t, uint32_t>> key(n);
        for (uint64_t u = 0; u < n; u++) { const Ph4h w = philox_host(p->seed, (uint32_t)u, 0u, 16u, 0u); key[u] = {((uint64_t)w.x << 32) | w.y, (uint32_t)u}; }
        // std::shuffle + resize (src/pcr.cpp:217-220) = a uniformly random ORDERED subset: the 2 x target molecules with the smallest
        // keys, in the order of their keys -- the order in which their copies are written
        std::nth_element(key.begin(), key.begin() + (ptrdiff_t)n_kept, key.end());
        std::sort(key.begin(), key.begin() + (ptrdiff_t)n_kept);
        keep.resize(n_kept);
        for (uint64_t i = 0; i < n_kept; i++) keep[i] = key[i].second;
    }
    n_local = n_kept;
    if (sliced) {
        if (keep.empty()) {
            if (p->template_begin != 0 || p->template_end != n) { keep.resize(p->template_end - p->template_begin); for (size_t i = 0; i < keep.size(); i++) keep[i] = (uint32_t)(p->template_begin + i); }
        } else {
            // (a slice is a range of POSITIONS in the processing order: with the subsample that is the order of the keys)
            const uint64_t lo = std::min<uint64_t>(p->template_begin, n_kept), hi = std::min<uint64_t>(p->template_end, n_kept);
            keep = std::vector<uint32_t>(keep.begin() + (ptrdiff_t)lo, keep.begin() + (ptrdiff_t)hi);
        }
        n_local = (keep.empty() && p->template_begin == 0 && p->template_end == n) ? n : keep.size();
        if (n_local == 0) keep.assign(1, 0u);                     // (an empty slice: a list that is not "every molecule")
    }
    return pcr_tables(ctx, p, n_kept, P);
}

int tksmseq_pcr_template_counts(tksmseq_ctx* ctx, const tksmseq_batch* in, const tksmseq_pcr_params* p, uint64_t* counts) {
    if (!ctx || !in || !p || (!counts && in->n_reads)) return TKSMSEQ_EINVAL;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    std::vector<uint32_t> keep;
    uint64_t n_kept = 0;
    tk::PcrParams P{};
    tksmseq_pcr_params whole = *p;
    whole.template_begin = whole.template_end = 0;
    int rc = pcr_setup(ctx, in, &whole, keep, n_kept, P);
    if (rc) return rc;
    TmpBuf d_keep(s), d_cnt(s), d_status(s);
    if (!keep.empty() && (rc = upload(ctx, d_keep, keep.data(), n_kept * 4))) return rc;
    const tk::MolView M = mol_view(in, keep.empty() ? nullptr : d_keep.as<uint32_t>(), n_kept);
    HIPCHK(ctx, d_cnt.ensure(n_kept * 8 + 16));
    HIPCHK(ctx, d_status.ensure(64));
    HIPCHK(ctx, hipMemsetAsync(d_status.p, 0, 64, s));
    HIPCHK(ctx, tk::launch_pcr_count(M, P, d_cnt.as<uint64_t>(), d_status.as<uint32_t>(), s));
    std::vector<uint64_t> h(n_kept);
    uint32_t st = 0;
    if (n_kept) HIPCHK(ctx, hipMemcpyAsync(h.data(), d_cnt.p, n_kept * 8, hipMemcpyDeviceToHost, s));
    HIPCHK(ctx, hipMemcpyAsync(&st, d_status.p, 4, hipMemcpyDeviceToHost, s));
    HIPCHK(ctx, hipStreamSynchronize(s));
    if (st & 1u) { ctx->err = "PCR: more than " + std::to_string(tk::PCR_MAX_MUT) + " substitutions per copy (error rate x molecule length) are not supported"; return TKSMSEQ_ELIMIT; }
    std::fill(counts, counts + in->n_reads, 0ull);
    for (uint64_t i = 0; i < n_kept; i++) counts[i] = h[i];          // by position in the processing order (beyond n_kept: 0)
    return TKSMSEQ_OK;
}

// comments follow the template (re-serialised the way the reference's reader / writer pair does); node_mol: the template of every copy (device)
static int pcr_comments(tksmseq_ctx* ctx, const tksmseq_batch* in, const DevBuf& node_mol, uint64_t n_nodes, OutBatch& b) {
    std::vector<uint32_t> mol(n_nodes);
    HIPCHK(ctx, hipMemcpyAsync(mol.data(), node_mol.p, n_nodes * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    b->h_comments.reserve(2 * n_nodes);
    for (uint64_t j = 0; j < n_nodes; j++) {
        const uint32_t u = mol[j];
        if (j && u == mol[j - 1]) {                                   // (a further copy of the same template: its entry again)
            const size_t k = b->h_comments.size();
            const uint32_t off = b->h_comments[k - 2], len = b->h_comments[k - 1];
            b->h_comments.push_back(off); b->h_comments.push_back(len);
            continue;
        }
        const int rc = append_comment(ctx, b.get(), normalize_comment(in->h_comment_pool.data() + in->h_comments[2 * (size_t)u], in->h_comments[2 * (size_t)u + 1], {}),
                                      "PCR", "use template slices");
        if (rc) return rc;
    }
    return TKSMSEQ_OK;
}

int tksmseq_pcr(tksmseq_ctx* ctx, const tksmseq_batch* in, const tksmseq_pcr_params* p, tksmseq_batch** out) {
    if (!ctx || !in || !p || !out) return TKSMSEQ_EINVAL;
    *out = nullptr;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    std::vector<uint32_t> keep;
    uint64_t n_kept = 0;
    tk::PcrParams P{};
    int rc = pcr_setup(ctx, in, p, keep, n_kept, P);
    if (rc) return rc;
    OutBatch b(ctx);
    TmpBuf d_keep(s), d_cnt(s), d_off(s), d_status(s), n_mol(s), n_mask(s);
    if (!keep.empty() && (rc = upload(ctx, d_keep, keep.data(), n_kept * 4))) return rc;
    const tk::MolView M = mol_view(in, keep.empty() ? nullptr : d_keep.as<uint32_t>(), n_kept);
    HIPCHK(ctx, d_cnt.ensure(n_kept * 8 + 16));
    HIPCHK(ctx, d_status.ensure(64));
    HIPCHK(ctx, hipMemsetAsync(d_status.p, 0, 64, s));
    HIPCHK(ctx, tk::launch_pcr_count(M, P, d_cnt.as<uint64_t>(), d_status.as<uint32_t>(), s));
    uint64_t n_nodes = 0;
    if ((rc = scan_to(ctx, d_cnt, d_off, n_kept, &n_nodes))) return rc;
    uint32_t st = 0;
    HIPCHK(ctx, hipMemcpy(&st, d_status.p, 4, hipMemcpyDeviceToHost));
    if (st & 1u) { ctx->err = "PCR: more than " + std::to_string(tk::PCR_MAX_MUT) + " substitutions per copy (error rate x molecule length) are not supported"; return TKSMSEQ_ELIMIT; }
    if ((rc = b.limits(n_nodes, "PCR: ", "split the input"))) return rc;          // (before anything is sized by it)
    HIPCHK(ctx, n_mol.ensure(n_nodes * 4 + 16));
    HIPCHK(ctx, n_mask.ensure(n_nodes * 8 + 16));
    tk::MolCounts C{};
    if ((rc = b.counts(n_nodes, C))) return rc;
    HIPCHK(ctx, tk::launch_pcr_list(M, P, d_off.as<uint64_t>(), n_mol.as<uint32_t>(), n_mask.as<uint64_t>(), C, s));
    if ((rc = b.place(n_nodes, n_nodes, "PCR: ")) || (rc = b.literals(in))) return rc;
    HIPCHK(ctx, tk::launch_pcr_write(M, P, n_nodes, n_mol.as<uint32_t>(), n_mask.as<uint64_t>(), b.offsets(), b.tables(), s));
    if (!in->h_comments.empty() && !(p->flags & TKSMSEQ_MOL_NO_COMMENTS) && (rc = pcr_comments(ctx, in, n_mol, n_nodes, b))) return rc;
    return b.finish(out);
}
// ---- truncate --------------------------------------------------------------------------------------------------------------------
struct TrcModelBufs {
    TmpBuf x, y, cdf, rn, sl, sc;
    explicit TrcModelBufs(hipStream_t s) : x(s), y(s), cdf(s), rn(s), sl(s), sc(s) {}
};

// the kernel parameters of a call; KDE mode: the model file read and uploaded into d, tm its host copy, which lives until the stream has drained
static int trc_params(tksmseq_ctx* ctx, const tksmseq_trc_params* p, TrcModelHost& tm, TrcModelBufs& d, tk::TrcParams& T) {
    T = tk::TrcParams{};
    T.seed = p->seed; T.mode = p->mode; T.mu = p->mu; T.sigma = p->sigma; T.min_len = 100;      // truncate()'s default min_val
    T.always_end = p->always_end ? 1 : 0; T.models_length = p->kde_models_length ? 1 : 0;
    if (p->mode != TKSMSEQ_TRC_KDE) {
        if (p->mode != TKSMSEQ_TRC_NORMAL && p->mode != TKSMSEQ_TRC_LOGNORMAL) { ctx->err = "truncate: unknown mode"; return TKSMSEQ_EINVAL; }
        if (!std::isfinite(p->mu) || !std::isfinite(p->sigma)) { ctx->err = "truncate: mu and sigma must be finite"; return TKSMSEQ_EINVAL; }
        return TKSMSEQ_OK;
    }
    if (!p->kde_model_path) { ctx->err = "truncate: the KDE mode needs a model file"; return TKSMSEQ_EINVAL; }
    if (!load_trc_model(p->kde_model_path, tm, ctx->err)) return TKSMSEQ_EIO;
    if (!p->always_end && !tm.have_sider) { ctx->err = "truncate: the model has no end_mtx (use --always-end)"; return TKSMSEQ_EINVAL; }
    T.nx = (int)tm.xlab.size(); T.ny = (int)tm.ylab.size(); T.have_sider = tm.have_sider ? 1 : 0; T.ns = (int)tm.slab.size();
    int rc;
    if ((rc = upload(ctx, d.x, tm.xlab.data(), tm.xlab.size() * 8)) || (rc = upload(ctx, d.y, tm.ylab.data(), tm.ylab.size() * 8)) ||
        (rc = upload(ctx, d.cdf, tm.cdf.data(), tm.cdf.size() * 8)) || (rc = upload(ctx, d.rn, tm.row_n.data(), tm.row_n.size() * 4)) ||
        (rc = upload(ctx, d.sl, tm.slab.data(), tm.slab.size() * 8)) || (rc = upload(ctx, d.sc, tm.scdf.data(), tm.scdf.size() * 8))) return rc;
    T.xlab = d.x.as<long long>(); T.ylab = d.y.as<long long>(); T.cdf = d.cdf.as<double>(); T.row_n = d.rn.as<int>();
    T.slab = d.sl.as<double>(); T.scdf = d.sc.as<double>();
    return TKSMSEQ_OK;
}

// truncated=chr:start-end,... for what was cut away from molecule r (src/truncate.cpp:54-60), appended to `extra`.  H: the input's tables
// with SEGMENTS fetched; kf / kt: what k_trc_plan wrote for r (the kept part [w0, w1) of its bases, bit 31: cut at that end)
static void truncated_pieces(const tksmseq_ctx* ctx, const HostTables& H, uint64_t r, uint32_t kf, uint32_t kt, std::vector<std::pair<std::string, std::string>>& extra) {
    const auto &reads = H.reads, &ivs = H.ivs;
    auto chr_of = [&](uint32_t c) -> std::string { std::string name; H.append_contig(ctx, c, name); return name; };
    const int w0 = (int)(kf & 0x7fffffffu), w1 = (int)(kt & 0x7fffffffu);
    const bool cut5 = kf >> 31, cut3 = kt >> 31;
    const uint32_t ib = reads[2 * r], ic = reads[2 * r + 1];
    auto piece = [&](const uint32_t* iv, long long a, long long bb) { extra.push_back({"truncated", chr_of(iv[0]) + ":" + std::to_string(a) + "-" + std::to_string(bb)}); };
    if (cut3) {
        // 3' cut in segment order: the cut segment's removed part, then the dropped segments (src/truncate.cpp:41-58)
        int c = 0; bool found = false;
        for (uint32_t i = 0; i < ic; i++) {
            const uint32_t* iv = ivs.data() + 4 * (size_t)(ib + i);
            const int sz = iv[2] > iv[1] ? (int)(iv[2] - iv[1]) : 0;
            if (!found && c + sz >= w1) {
                const int keepn = w1 - c;
                if (iv[3] >> 31) piece(iv, iv[1], (long long)iv[2] - keepn); else piece(iv, (long long)iv[1] + keepn, iv[2]);
                found = true;
            } else if (found) piece(iv, iv[1], iv[2]);
            c += sz;
        }
    }
    if (cut5) {
        // 5' cut = the same on the flipped molecule (after the first cut): segments from the last kept one backwards
        int cend = 0; std::vector<std::pair<uint32_t, int>> segs;      // (interval index, start coordinate) of the once-truncated molecule
        { int c = 0; for (uint32_t i = 0; i < ic; i++) { const uint32_t* iv = ivs.data() + 4 * (size_t)(ib + i); const int sz = iv[2] > iv[1] ? (int)(iv[2] - iv[1]) : 0; if (c < w1 || (sz == 0 && !cut3)) segs.push_back({i, c}); c += sz; } cend = std::min(c, w1); }
        const int L2 = cend - w0;
        int c = 0; bool found = false;                                   // c: bases of the flipped molecule before the segment
        for (size_t q = segs.size(); q-- > 0;) {
            const uint32_t* iv = ivs.data() + 4 * (size_t)(ib + segs[q].first);
            long long st = iv[1], en = iv[2];
            int sz = en > st ? (int)(en - st) : 0;
            const bool minus = iv[3] >> 31;
            if (segs[q].second + sz > w1) {                              // already cut at its 3' side
                const int keepn = w1 - segs[q].second;
                if (minus) st = en - keepn; else en = st + keepn;
                sz = keepn;
            }
            if (!found && c + sz >= L2) {
                const int keepn = L2 - c;
                // the flipped segment has the opposite strand: flipped plus (original minus) keeps [st, st + keep)
                if (minus) piece(iv, st + keepn, en); else piece(iv, st, en - keepn);
                found = true;
            } else if (found) piece(iv, st, en);
            c += sz;
        }
    }
}

// comments: the template's, plus truncated=... and (KDE mode) TR=<length>,<3' share> (src/truncate.cpp:343).  Needs the input tables and
// the plan (kf, kt, tl, ts: device arrays of k_trc_plan) on the host.
static int trc_comments(tksmseq_ctx* ctx, const tksmseq_batch* in, bool kde, const DevBuf& kf, const DevBuf& kt, const DevBuf& tl, const DevBuf& ts, OutBatch& b) {
    hipStream_t s = ctx->stream;
    const uint64_t n = in->n_reads;
    HostTables H;
    std::vector<uint32_t> hkf(n), hkt(n);
    std::vector<double> htl(n), hts(n);
    HIPCHK(ctx, hipMemcpyAsync(hkf.data(), kf.p, n * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(ctx, hipMemcpyAsync(hkt.data(), kt.p, n * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(ctx, hipMemcpyAsync(htl.data(), tl.p, n * 8, hipMemcpyDeviceToHost, s));
    HIPCHK(ctx, hipMemcpyAsync(hts.data(), ts.p, n * 8, hipMemcpyDeviceToHost, s));
    int rc = H.fetch(ctx, in, HostTables::SEGMENTS);                    // (drains the stream: the four copies above as well)
    if (rc) return rc;
    for (uint64_t r = 0; r < n; r++) {
        std::vector<std::pair<std::string, std::string>> extra;
        truncated_pieces(ctx, H, r, hkf[r], hkt[r], extra);
        if (kde) {
            char sr[32]; snprintf(sr, sizeof sr, "%.2f", hts[r]);
            extra.push_back({"TR", fmt_double(htl[r]) + "," + sr});
        }
        if ((rc = append_comment(ctx, b.get(), normalize_comment(in->h_comment_pool.data() + in->h_comments[2 * r], in->h_comments[2 * r + 1], extra), "truncate"))) return rc;
    }
    return TKSMSEQ_OK;
}

int tksmseq_truncate(tksmseq_ctx* ctx, const tksmseq_batch* in, const tksmseq_trc_params* p, tksmseq_batch** out) {
    if (!ctx || !in || !p || !out) return TKSMSEQ_EINVAL;
    *out = nullptr;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const uint64_t n = in->n_reads;
    tk::TrcParams T{};
    TrcModelHost tm;
    TrcModelBufs model(s);
    int rc = trc_params(ctx, p, tm, model, T);
    if (rc) return rc;
    const tk::MolView M = mol_view(in);
    OutBatch b(ctx);
    TmpBuf kf(s), kt(s), tl(s), ts(s);
    HIPCHK(ctx, kf.ensure(n * 4 + 16)); HIPCHK(ctx, kt.ensure(n * 4 + 16));
    HIPCHK(ctx, tl.ensure(n * 8 + 16)); HIPCHK(ctx, ts.ensure(n * 8 + 16));
    tk::MolCounts C{};
    if ((rc = b.counts(n, C))) return rc;
    HIPCHK(ctx, tk::launch_trc_plan(M, T, p->first_molecule_index, kf.as<uint32_t>(), kt.as<uint32_t>(), tl.as<double>(), ts.as<double>(), C, s));
    // (a truncated batch is no larger than its input, so the limits cannot trip here: checked all the same, like every other output)
    if ((rc = b.place(n, n, "truncate: ")) || (rc = b.literals(in))) return rc;
    HIPCHK(ctx, tk::launch_trc_write(M, kf.as<uint32_t>(), kt.as<uint32_t>(), b.offsets(), b.tables(), s));
    if (!in->h_comments.empty() && !(p->flags & TKSMSEQ_MOL_NO_COMMENTS) && (rc = trc_comments(ctx, in, p->mode == TKSMSEQ_TRC_KDE, kf, kt, tl, ts, b))) return rc;
    return b.finish(out);
}

// ---- segment edits: polyA, tag, scb, flip ----------------------------------------------------------------------------------------
// count, scan, allocate, write: every molecule of `in` (unrolled) with literal pre[r] in front of and post[r] behind its segments, which
// are reversed and strand-toggled where flip[r] (device arrays; null: none of that kind).  b's literal table is already complete, and
// the caller's host tables must live until b.finish(), which drains the stream.
// pal: the palindromic tail noise of tksmseq_append_noise, whose kernels add a hairpin behind each molecule to the counts and to the tables.
struct PalHook { tk::NoiseParams P; uint64_t first; const uint4* plan; };
static int edit_apply(tksmseq_ctx* ctx, const tksmseq_batch* in, const uint32_t* pre, const uint32_t* post, const uint8_t* flip, OutBatch& b,
                      const PalHook* pal = nullptr) {
    hipStream_t s = ctx->stream;
    const uint64_t n = in->n_reads;
    const tk::MolView M = mol_view(in);
    tk::MolCounts C{};
    int rc;
    if ((rc = b.counts(n, C))) return rc;
    HIPCHK(ctx, tk::launch_edit_count(M, pre, post, C, s));
    if (pal) HIPCHK(ctx, tk::launch_pal_count(M, pal->P, pal->first, pal->plan, C, s));
    if ((rc = b.place(n, n, ""))) return rc;
    HIPCHK(ctx, tk::launch_edit_write(M, pre, post, flip, b->literals.as<uint64_t>(), b.offsets(), b.tables(), s));
    if (pal) HIPCHK(ctx, tk::launch_pal_write(M, pal->P, pal->first, pal->plan, b.offsets(), b.tables(), s));
    return TKSMSEQ_OK;
}

// comments unchanged (the writer re-serialises them, normalize_comment)
static void edit_comments(const tksmseq_batch* in, OutBatch& b, int32_t flags) {
    if (flags & TKSMSEQ_MOL_NO_COMMENTS) return;
    b->h_comments = in->h_comments; b->h_comment_pool = in->h_comment_pool;
}

int tksmseq_polya(tksmseq_ctx* ctx, const tksmseq_batch* in, const tksmseq_polya_params* p, tksmseq_batch** out) {
    if (!ctx || !in || !p || !out) return TKSMSEQ_EINVAL;
    *out = nullptr;
    // validate_arguments (src/polyA.cpp:61-118), plus the parameters std:: leaves undefined
    if (p->dist < TKSMSEQ_PLA_GAMMA || p->dist > TKSMSEQ_PLA_NORMAL) { ctx->err = "polyA: unknown distribution"; return TKSMSEQ_EINVAL; }
    if (p->min_length < 0) { ctx->err = "Minimum length of polyA cannot be negative"; return TKSMSEQ_EINVAL; }
    if (p->max_length < 0) { ctx->err = "Maximum length of polyA cannot be negative"; return TKSMSEQ_EINVAL; }
    if (p->min_length > p->max_length) { ctx->err = "Minimum length of polyA cannot be greater than maximum length of polyA"; return TKSMSEQ_EINVAL; }
    const bool two = p->dist != TKSMSEQ_PLA_POISSON;
    if (!std::isfinite(p->a) || (two && !std::isfinite(p->b))) { ctx->err = "polyA: distribution parameters must be finite"; return TKSMSEQ_EINVAL; }
    if ((p->dist != TKSMSEQ_PLA_NORMAL && !(p->a > 0.0)) || (two && !(p->b > 0.0))) {
        ctx->err = p->dist == TKSMSEQ_PLA_NORMAL ? "polyA: sigma must be positive" : "polyA: distribution parameters must be positive";
        return TKSMSEQ_EINVAL;
    }
    if (p->max_length > (1 << 20)) { ctx->err = "polyA: --max-length above 1048576 is not supported"; return TKSMSEQ_ELIMIT; }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const uint64_t n = in->n_reads, L = (uint64_t)p->max_length;
    OutBatch b(ctx);
    int rc = b.literals(in, L, L);
    if (rc) return rc;
    // literal b.lit_base + k is "A" x (k + 1): all of them at the start of one run of max_length 'A's
    std::vector<uint64_t> ent(2 * L);
    for (uint64_t k = 0; k < L; k++) { ent[2 * k] = b.pool_base; ent[2 * k + 1] = k + 1; }
    if (L) {
        HIPCHK(ctx, hipMemcpyAsync(b->literals.as<uint64_t>() + 2ull * b.lit_base, ent.data(), L * 16, hipMemcpyHostToDevice, s));
        HIPCHK(ctx, hipMemsetAsync(b->litpool.as<uint8_t>() + b.pool_base, 'A', L, s));
    }
    TmpBuf d_post(s);
    HIPCHK(ctx, d_post.ensure(n * 4 + 16));
    tk::PlaParams P{p->seed, p->dist, p->a, p->b, p->min_length, p->max_length, b.lit_base};
    HIPCHK(ctx, tk::launch_pla_plan(n, P, p->first_molecule_index, d_post.as<uint32_t>(), s));
    if ((rc = edit_apply(ctx, in, nullptr, d_post.as<uint32_t>(), nullptr, b))) return rc;
    edit_comments(in, b, p->flags);
    return b.finish(out);
}

// fmt2seq's table (src/util.h:62-80): number of choices of a letter, 0 if the table does not know it
static int iupac_choices(char c) {
    switch (c) {
        case 'A': case 'G': case 'T': case 'C': case 'U': return 1;
        case 'R': case 'Y': case 'K': case 'M': case 'S': case 'W': return 2;
        case 'B': case 'D': case 'H': case 'V': return 3;
        case 'N': return 4;
        default: return 0;
    }
}

int tksmseq_tag(tksmseq_ctx* ctx, const tksmseq_batch* in, const tksmseq_tag_params* p, tksmseq_batch** out) {
    if (!ctx || !in || !p || !out) return TKSMSEQ_EINVAL;
    *out = nullptr;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const uint64_t n = in->n_reads;
    std::string fmt[2];
    bool amb[2] = {false, false};
    for (int e = 0; e < 2; e++) {
        const char* f = e == 0 ? p->format5 : p->format3;
        for (; f && *f; f++) { const int k = iupac_choices(*f); if (k) { fmt[e] += *f; amb[e] |= k > 1; } }
        if (fmt[e].size() > (1u << 20)) { ctx->err = "tag: formats longer than 1048576 letters are not supported"; return TKSMSEQ_ELIMIT; }
    }
    // new literals: a shared one per adapter (no ambiguous letter), one per molecule per ambiguous format
    uint64_t n_new = 0, bytes = 0;
    for (int e = 0; e < 2; e++)
        if (!fmt[e].empty()) { n_new += amb[e] ? n : 1; bytes += (amb[e] ? n : 1) * fmt[e].size(); }
    OutBatch b(ctx);
    int rc = b.literals(in, n_new, bytes);
    if (rc) return rc;
    TmpBuf d_fmt[2] = {TmpBuf(s), TmpBuf(s)}, d_pre(s), d_post(s);
    tk::TagParams T{};
    T.seed = p->seed;
    uint64_t li = b.lit_base, off = b.pool_base;
    uint64_t ent[2][2];
    for (int e = 0; e < 2; e++) {
        tk::TagEnd& E = T.end[e];
        E.len = (int)fmt[e].size(); E.shared = tk::EDIT_NONE;
        if (fmt[e].empty()) continue;
        if ((rc = upload(ctx, d_fmt[e], fmt[e].data(), fmt[e].size()))) return rc;
        E.fmt = d_fmt[e].as<uint8_t>();
        if (amb[e]) { E.lit_base = (uint32_t)li; E.pool_base = off; li += n; off += n * fmt[e].size(); continue; }
        E.shared = (uint32_t)li;
        ent[e][0] = off; ent[e][1] = fmt[e].size();
        HIPCHK(ctx, hipMemcpyAsync(b->literals.as<uint64_t>() + 2 * li, ent[e], 16, hipMemcpyHostToDevice, s));
        HIPCHK(ctx, hipMemcpyAsync(b->litpool.as<uint8_t>() + off, fmt[e].data(), fmt[e].size(), hipMemcpyHostToDevice, s));
        li += 1; off += fmt[e].size();
    }
    HIPCHK(ctx, d_pre.ensure(n * 4 + 16));
    HIPCHK(ctx, d_post.ensure(n * 4 + 16));
    HIPCHK(ctx, tk::launch_tag_plan(n, T, p->first_molecule_index, d_pre.as<uint32_t>(), d_post.as<uint32_t>(), b->literals.as<uint64_t>(),
                                    b->litpool.as<uint8_t>(), s));
    if ((rc = edit_apply(ctx, in, d_pre.as<uint32_t>(), d_post.as<uint32_t>(), nullptr, b))) return rc;
    edit_comments(in, b, p->flags);
    return b.finish(out);
}

// id of molecule r as the writer prints it (with the unroll suffix), for error messages
static std::string molecule_id(tksmseq_ctx* ctx, const tksmseq_batch* in, uint64_t r) {
    HostTables H;
    if (H.fetch(ctx, in, HostTables::IDS)) return "#" + std::to_string(r);
    return written_id(H, in, r);
}

int tksmseq_scb(tksmseq_ctx* ctx, const tksmseq_batch* in, const tksmseq_scb_params* p, tksmseq_batch** out) {
    if (!ctx || !in || !p || !out) return TKSMSEQ_EINVAL;
    *out = nullptr;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const uint64_t n = in->n_reads;
    if (n && in->h_comments.empty()) { ctx->err = "scb: the batch carries no header comments (CB barcodes)"; return TKSMSEQ_EINVAL; }
    // the host resolves the barcodes (get_comment("CB")[0]) in one pass and de-duplicates them into literals
    OutBatch b(ctx);
    const bool want_comments = !(p->flags & TKSMSEQ_MOL_NO_COMMENTS);
    std::vector<uint32_t> post(n);
    std::unordered_map<std::string, uint32_t> index;
    std::vector<uint64_t> ent;
    std::string bytes;
    if (want_comments) b->h_comments.reserve(2 * n);
    for (uint64_t r = 0; r < n; r++) {
        Meta meta = parse_meta(in->h_comment_pool.data() + in->h_comments[2 * r], in->h_comments[2 * r + 1]);
        auto it = meta.find("CB");
        if (it == meta.end() || it->second.empty()) { ctx->err = "scb: molecule " + molecule_id(ctx, in, r) + " has no CB comment"; return TKSMSEQ_EINVAL; }
        const std::string& bc = it->second[0];
        if (bc == ".") post[r] = tk::EDIT_NONE;
        else {
            auto f = index.find(bc);
            if (f == index.end()) {
                f = index.emplace(bc, (uint32_t)index.size()).first;
                ent.push_back(bytes.size()); ent.push_back(bc.size());
                bytes += bc;
            }
            post[r] = f->second;
        }
        if (want_comments) {
            if (!p->keep_meta_barcodes) meta.erase(it);
            const int rc = append_comment(ctx, b.get(), dump_meta(meta), "scb");
            if (rc) return rc;
        }
    }
    int rc = b.literals(in, index.size(), bytes.size());
    if (rc) return rc;
    for (uint64_t r = 0; r < n; r++) if (post[r] != tk::EDIT_NONE) post[r] += b.lit_base;
    for (size_t k = 0; k < ent.size(); k += 2) ent[k] += b.pool_base;
    if (!ent.empty()) {
        HIPCHK(ctx, hipMemcpyAsync(b->literals.as<uint64_t>() + 2ull * b.lit_base, ent.data(), ent.size() * 8, hipMemcpyHostToDevice, s));
        HIPCHK(ctx, hipMemcpyAsync(b->litpool.as<uint8_t>() + b.pool_base, bytes.data(), bytes.size(), hipMemcpyHostToDevice, s));
    }
    TmpBuf d_post(s);
    if ((rc = upload(ctx, d_post, post.data(), n * 4))) return rc;
    if ((rc = edit_apply(ctx, in, nullptr, d_post.as<uint32_t>(), nullptr, b))) return rc;
    return b.finish(out);
}

int tksmseq_flip(tksmseq_ctx* ctx, const tksmseq_batch* in, const tksmseq_flip_params* p, tksmseq_batch** out) {
    if (!ctx || !in || !p || !out) return TKSMSEQ_EINVAL;
    *out = nullptr;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const uint64_t n = in->n_reads;
    OutBatch b(ctx);
    int rc = b.literals(in);
    if (rc) return rc;
    TmpBuf d_flip(s);
    HIPCHK(ctx, d_flip.ensure(n + 16));
    HIPCHK(ctx, tk::launch_flip_plan(n, p->seed, p->flip_probability, p->first_molecule_index, d_flip.as<uint8_t>(), s));
    if ((rc = edit_apply(ctx, in, nullptr, nullptr, d_flip.as<uint8_t>(), b))) return rc;
    edit_comments(in, b, p->flags);
    return b.finish(out);
}

// ---- tail-noise ------------------------------------------------------------------------------------------------------------------
int tksmseq_append_noise(tksmseq_ctx* ctx, const tksmseq_batch* in, const tksmseq_noise_params* p, tksmseq_batch** out) {
    if (!ctx || !in || !p || !out) return TKSMSEQ_EINVAL;
    *out = nullptr;
    // what the reference leaves undefined (an empty alphabet: uniform_int_distribution(0, -1); sigma <= 0) or exits on (the name)
    if (p->dist != TKSMSEQ_NOISE_NORMAL && p->dist != TKSMSEQ_NOISE_LOGNORMAL) { ctx->err = "Distribution not implemented!"; return TKSMSEQ_EINVAL; }
    if (!p->alphabet || !*p->alphabet) { ctx->err = "tail-noise: the alphabet is empty"; return TKSMSEQ_EINVAL; }
    if (!std::isfinite(p->mu) || !std::isfinite(p->sigma) || !(p->sigma > 0.0)) { ctx->err = "tail-noise: mu must be finite, sigma finite and positive"; return TKSMSEQ_EINVAL; }
    if (std::isnan(p->error_rate)) { ctx->err = "tail-noise: the error rate is not a number"; return TKSMSEQ_EINVAL; }
    const size_t k = strlen(p->alphabet);
    if (k > (size_t)tk::NOISE_MAX_LEN) { ctx->err = "tail-noise: alphabets longer than 1048576 letters are not supported"; return TKSMSEQ_ELIMIT; }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const uint64_t n = in->n_reads;
    TmpBuf d_alpha(s), d_plan(s), d_len(s), d_nblk(s), d_off(s), d_over(s), d_post(s);
    int rc = upload(ctx, d_alpha, p->alphabet, k);
    if (rc) return rc;
    const tk::NoiseParams P{p->seed, p->dist == TKSMSEQ_NOISE_LOGNORMAL ? tk::NOISE_LOGNORMAL : tk::NOISE_NORMAL, p->mu, p->sigma, p->error_rate,
                            d_alpha.as<uint8_t>(), (uint32_t)k};
    const tk::MolView M = mol_view(in);
    OutBatch b(ctx);
    if (p->palindromic) {
        if ((rc = b.literals(in))) return rc;
        HIPCHK(ctx, d_plan.ensure(n * 16 + 16));
        HIPCHK(ctx, tk::launch_noise_plan(M, P, p->first_molecule_index, nullptr, nullptr, nullptr, d_plan.as<uint4>(), s));
        const PalHook pal{P, p->first_molecule_index, d_plan.as<uint4>()};
        if ((rc = edit_apply(ctx, in, nullptr, nullptr, nullptr, b, &pal))) return rc;
    } else {
        HIPCHK(ctx, d_len.ensure(n * 4 + 16));
        HIPCHK(ctx, d_nblk.ensure(n * 8 + 16));
        HIPCHK(ctx, d_over.ensure(64));
        HIPCHK(ctx, hipMemsetAsync(d_over.p, 0xff, 8, s));
        HIPCHK(ctx, tk::launch_noise_plan(M, P, p->first_molecule_index, d_len.as<uint32_t>(), d_nblk.as<uint64_t>(), d_over.as<unsigned long long>(), nullptr, s));
        uint64_t n_blocks = 0;
        if ((rc = scan_to(ctx, d_nblk, d_off, n, &n_blocks))) return rc;
        unsigned long long over = ~0ull;
        HIPCHK(ctx, hipMemcpy(&over, d_over.p, 8, hipMemcpyDeviceToHost));
        if (over != ~0ull) {
            ctx->err = "tail-noise: the noise length drawn for molecule " + molecule_id(ctx, in, over) + " is above 1048576 (not supported)";
            return TKSMSEQ_ELIMIT;
        }
        if (n_blocks >= (1ull << 30)) { ctx->err = "tail-noise: more than 4 GB of noise letters in one batch (split the input)"; return TKSMSEQ_ELIMIT; }
        if ((rc = b.literals(in, n, 4 * n_blocks))) return rc;
        HIPCHK(ctx, d_post.ensure(n * 4 + 16));
        if (n) {
            HIPCHK(ctx, hipMemsetAsync(d_post.p, 0xff, n * 4, s));                                   // EDIT_NONE
            HIPCHK(ctx, hipMemsetAsync(b->literals.as<uint64_t>() + 2ull * b.lit_base, 0, n * 16, s));   // (molecules without noise: an empty entry nobody names)
        }
        HIPCHK(ctx, tk::launch_noise_fill(n, n_blocks, P, p->first_molecule_index, d_len.as<uint32_t>(), d_off.as<uint64_t>(), b.lit_base, b.pool_base,
                                          b->literals.as<uint64_t>(), b->litpool.as<uint8_t>(), d_post.as<uint32_t>(), s));
        if ((rc = edit_apply(ctx, in, nullptr, d_post.as<uint32_t>(), nullptr, b))) return rc;
    }
    edit_comments(in, b, p->flags);
    return b.finish(out);
}

// ---- mutate ----------------------------------------------------------------------------------------------------------------------
// A variant table in its normal form (mut_host.h), on the host; immutable once loaded, so any number of contexts may use it.
struct tksmseq_variants { mut::Variants v; };

// the table as k_mut_count / k_mut_write read it, the context's contigs resolved against the table's names
static int mut_table(tksmseq_ctx* ctx, const mut::Variants& T, tk::MutView& V) {
    hipStream_t s = ctx->stream;
    if (ctx->mut_serial != T.serial || ctx->mut_ref_version != ctx->ref_version) {
        std::vector<uint32_t> ref_ctg(ctx->contig_names.size()), name_off{0};
        for (size_t i = 0; i < ref_ctg.size(); i++) { const int k = T.find(ctx->contig_names[i].data(), ctx->contig_names[i].size()); ref_ctg[i] = k >= 0 ? (uint32_t)k : tk::MUT_NONE; }
        std::string names;
        for (auto& n : T.names) {
            if (names.size() + n.size() >= 0xffffffffull) { ctx->err = "mutate: more than 4 GB of contig names in the variant table"; return TKSMSEQ_ELIMIT; }
            names += n; name_off.push_back((uint32_t)names.size());
        }
        HIPCHK(ctx, hipStreamSynchronize(s));                           // (nothing queued may still read the table that goes)
        ctx->mut_serial = 0;
        const struct { DevBuf& d; const void* p; size_t bytes; } up[] = {
            {ctx->d_mut_refctg, ref_ctg.data(), ref_ctg.size() * 4},         {ctx->d_mut_nameoff, name_off.data(), name_off.size() * 4},
            {ctx->d_mut_names, names.data(), names.size()},                  {ctx->d_mut_delfirst, T.del_first.data(), T.del_first.size() * 4},
            {ctx->d_mut_ptfirst, T.pt_first.data(), T.pt_first.size() * 4},  {ctx->d_mut_delfrom, T.del_from.data(), T.del_from.size() * 4},
            {ctx->d_mut_delto, T.del_to.data(), T.del_to.size() * 4},        {ctx->d_mut_ptpos, T.pt_pos.data(), T.pt_pos.size() * 4},
            {ctx->d_mut_ptinfo, T.pt_info.data(), T.pt_info.size() * 8},     {ctx->d_mut_insent, T.ins_ent.data(), T.ins_ent.size() * 8},
            {ctx->d_mut_inspool, T.ins_pool.data(), T.ins_pool.size()}};
        for (auto& u : up) { const int rc = upload(ctx, u.d, u.p, u.bytes); if (rc) return rc; }
        HIPCHK(ctx, hipStreamSynchronize(s));                           // (the host vectors above go)
        ctx->mut_serial = T.serial; ctx->mut_ref_version = ctx->ref_version;
    }
    V = tk::MutView{(uint32_t)T.names.size(), (uint32_t)ctx->contig_names.size(), (uint32_t)T.n_insertions_kept(), ctx->d_mut_refctg.as<uint32_t>(),
                    ctx->d_mut_nameoff.as<uint32_t>(), ctx->d_mut_names.as<uint8_t>(), ctx->d_mut_delfirst.as<uint32_t>(), ctx->d_mut_ptfirst.as<uint32_t>(),
                    ctx->d_mut_delfrom.as<uint32_t>(), ctx->d_mut_delto.as<uint32_t>(), ctx->d_mut_ptpos.as<uint32_t>(), ctx->d_mut_ptinfo.as<uint64_t>(),
                    ctx->d_mut_insent.as<uint64_t>()};
    return TKSMSEQ_OK;
}

int tksmseq_variants_load(tksmseq_ctx* ctx, const char* path, const char* text, uint64_t len, tksmseq_variants** out) {
    if (!out || (!path && !text && len)) return TKSMSEQ_EINVAL;
    *out = nullptr;
    static std::atomic<uint64_t> serial{0};
    std::unique_ptr<tksmseq_variants> v(new tksmseq_variants());
    std::string err;
    bool limit = false, io = false;
    const bool ok = path ? mut::read_variants(path, v->v, err, limit, io) : mut::parse_variants(text, len, "<text>", v->v, err, limit);
    if (!ok) {
        if (ctx) ctx->err = err; else set_contextless_error(err);
        return io ? TKSMSEQ_EIO : limit ? TKSMSEQ_ELIMIT : TKSMSEQ_EINVAL;
    }
    v->v.serial = ++serial;
    *out = v.release();
    return TKSMSEQ_OK;
}

int tksmseq_variants_info(const tksmseq_variants* v, uint64_t* rows, uint64_t* snvs, uint64_t* insertions, uint64_t* deletions, uint64_t* deleted_ranges,
                          uint64_t* dropped_points) {
    if (!v) return TKSMSEQ_EINVAL;
    if (rows) *rows = v->v.rows;
    if (snvs) *snvs = v->v.snvs;
    if (insertions) *insertions = v->v.insertions;
    if (deletions) *deletions = v->v.deletions;
    if (deleted_ranges) *deleted_ranges = v->v.deleted_ranges;
    if (dropped_points) *dropped_points = v->v.dropped_points;
    return TKSMSEQ_OK;
}

void tksmseq_variants_free(tksmseq_variants* v) { delete v; }

int tksmseq_mutate(tksmseq_ctx* ctx, const tksmseq_batch* in, const tksmseq_variants* v, const tksmseq_mutate_params* p, tksmseq_batch** out) {
    if (!ctx || !in || !v || !p || !out) return TKSMSEQ_EINVAL;
    *out = nullptr;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const mut::Variants& T = v->v;
    tk::MutView V{};
    int rc = mut_table(ctx, T, V);
    if (rc) return rc;
    const uint64_t n = in->n_reads;
    // the output's literals: the input's, then one entry per kept insertion of the table, shared by all molecules
    OutBatch b(ctx);
    if ((rc = b.literals(in, T.n_insertions_kept(), T.ins_pool.size()))) return rc;
    if (!T.ins_pool.empty()) HIPCHK(ctx, hipMemcpyAsync(b->litpool.as<uint8_t>() + b.pool_base, ctx->d_mut_inspool.p, T.ins_pool.size(), hipMemcpyDeviceToDevice, s));
    TmpBuf lit_ctg(s);
    HIPCHK(ctx, lit_ctg.ensure(in->n_literals * 4 + 16));
    const tk::MolView M = mol_view(in);
    HIPCHK(ctx, tk::launch_mut_resolve(M.B, V, lit_ctg.as<uint32_t>(), b->literals.as<uint64_t>(), b.lit_base, b.pool_base, s));
    tk::MolCounts C{};
    if ((rc = b.counts(n, C))) return rc;
    HIPCHK(ctx, tk::launch_mut_count(M, V, lit_ctg.as<uint32_t>(), C, s));
    if ((rc = b.place(n, n, "mutate: "))) return rc;
    HIPCHK(ctx, tk::launch_mut_write(M, V, lit_ctg.as<uint32_t>(), b.lit_base, b.offsets(), b.tables(), s));
    edit_comments(in, b, p->flags);
    return b.finish(out);
}

}  // extern "C"
