// abund_api.cpp -- C-ABI of abundance: tksmseq_abundance and its result accessors (include/tksmseq.h).  The host reads and interns
// (abund_host.cpp); from get_compatibility on everything runs on the device (abund_kernels.hip).
#include <cmath>
#include <cstring>
#include <string>
#include <unordered_map>
#include <vector>

#include "abund_host.h"
#include "abund_kernels.h"
#include "ctx.h"
#include "tool_run.h"

struct tksmseq_abundance_result {
    std::vector<std::string> tnames, rnames, cells;
    std::vector<uint8_t> kept;                           // [reads]
    std::vector<tkh::AbundRow> rows;                     // the rows the writer prints, in its order
    std::vector<double> abundance;                       // [transcripts]
    std::vector<uint32_t> surv_read, surv_cell, hit_off, hit_tid;
    std::vector<double> hit_w;
    bool have_hits = false;
    uint64_t n_hits = 0;
    float device_ms = 0.f;
    std::string tsv;
};

namespace {

constexpr uint64_t ABUND_LIMIT = 1ull << 31;

int bits_for(uint64_t n_values) { int b = 1; while (b < 64 && (1ull << b) < n_values) b++; return b; }      // bits that tell n_values values apart (not map_api.cpp's bit_length)

// a segmented sum over perm: the chunk list (made once per index) and the buffers of a round
struct SegSum {
    TmpBuf chunk_off, chunk_seg, partial, sum, block_part, total;
    uint32_t n_seg = 0, n_chunks = 0;
    explicit SegSum(hipStream_t s) : chunk_off(s), chunk_seg(s), partial(s), sum(s), block_part(s), total(s) {}
    int build(tksmseq_ctx* ctx, const uint32_t* off, uint32_t segs) {
        hipStream_t s = ctx->stream;
        n_seg = segs;
        TmpBuf counts(s);
        HIPCHK(ctx, counts.ensure(((size_t)n_seg + 1) * 8));
        HIPCHK(ctx, chunk_off.ensure(((size_t)n_seg + 1) * 8));
        HIPCHK(ctx, tk::launch_abund_chunk_counts(off, n_seg, counts.as<uint64_t>(), s));
        if (int rc = scan_u64(ctx, counts.as<uint64_t>(), chunk_off.as<uint64_t>(), n_seg)) return rc;
        uint64_t nc = 0;
        if (int rc = fetch_u64(ctx, chunk_off.as<uint64_t>() + n_seg, nc)) return rc;
        if (nc >= (1ull << 32)) { ctx->err = "abundance: 2^32 chunks or more"; return TKSMSEQ_ELIMIT; }
        n_chunks = (uint32_t)nc;
        HIPCHK(ctx, chunk_seg.ensure(((size_t)n_chunks + 1) * 4));
        HIPCHK(ctx, partial.ensure(((size_t)n_chunks + 1) * 8));
        HIPCHK(ctx, sum.ensure(((size_t)n_seg + 1) * 8));
        HIPCHK(ctx, block_part.ensure(((size_t)n_seg / 256 + 2) * 8));
        HIPCHK(ctx, total.ensure(8));
        HIPCHK(ctx, tk::launch_abund_chunk_map(chunk_off.as<uint64_t>(), n_seg, chunk_seg.as<uint32_t>(), s));
        return TKSMSEQ_OK;
    }
    int run(tksmseq_ctx* ctx, const double* w, const uint32_t* perm, const uint32_t* off) {
        hipStream_t s = ctx->stream;
        HIPCHK(ctx, tk::launch_abund_msum(w, perm, off, chunk_off.as<uint64_t>(), chunk_seg.as<uint32_t>(), n_chunks, partial.as<double>(), s));
        HIPCHK(ctx, tk::launch_abund_mfinish(partial.as<double>(), chunk_off.as<uint64_t>(), n_seg, sum.as<double>(), block_part.as<double>(), total.as<double>(), s));
        return TKSMSEQ_OK;
    }
};

// the argument checks of parse_args (:121-138)
int check_params(tksmseq_ctx* ctx, const tksmseq_abundance_params* p) {
    if (!tkh::abund_check_args(p->cb_count, p->lr_br_path, p->cb_pattern, p->cb_txt_path, p->cb_dropout, p->cb_mu, p->cb_sigma, ctx->err)) return TKSMSEQ_EINVAL;
    if (p->cb_count > 0 && (uint64_t)p->cb_count >= ABUND_LIMIT) { ctx->err = "abundance: 2^31 cell barcodes or more"; return TKSMSEQ_ELIMIT; }
    return TKSMSEQ_OK;
}

}  // namespace

extern "C" int tksmseq_abundance(tksmseq_ctx* ctx, const tksmseq_abundance_params* p, const char* paf_path, tksmseq_abundance_result** out) {
    if (!ctx) return TKSMSEQ_EINVAL;
    if (!p || !paf_path || !out) { ctx->err = "abundance: null argument"; return TKSMSEQ_EINVAL; }
    *out = nullptr;
    if (int rc = check_params(ctx, p)) return rc;
    std::unique_ptr<tksmseq_abundance_result> R(new tksmseq_abundance_result());
    R->cells.push_back(".");
    std::unordered_map<std::string, uint32_t> cell_index{{".", 0u}};
    auto cell_id = [&](const std::string& name) {
        auto it = cell_index.emplace(name, (uint32_t)R->cells.size());
        if (it.second) R->cells.push_back(name);
        return it.first->second;
    };
    const bool cb_mode = p->cb_count > 0, lr_mode = !cb_mode && p->lr_br_path && *p->lr_br_path;
    std::vector<uint32_t> cell_of;                       // --cb-count: barcode index -> cell (the last entry: the dropout cell ".")
    std::vector<double> cdf;
    std::unordered_map<std::string, std::string> lr;
    std::string text;
    if (cb_mode) {
        const uint32_t count = (uint32_t)p->cb_count;
        std::vector<std::string> barcodes;
        if (p->cb_txt_path && *p->cb_txt_path) {
            if (!tkh::abund_read_file(p->cb_txt_path, text, ctx->err)) return TKSMSEQ_EIO;
            std::vector<std::string> list;
            tkh::parse_whitelist(text.data(), text.size(), list);
            if (list.size() < count) { ctx->err = "abundance: the whitelist " + std::string(p->cb_txt_path) + " has fewer barcodes than --cb-count"; return TKSMSEQ_EINVAL; }
            tkh::barcodes_from_whitelist(list, count, p->seed, barcodes);
        } else tkh::barcodes_from_pattern(p->cb_pattern, count, p->seed, barcodes);
        for (auto& b : barcodes) cell_of.push_back(cell_id(b));
        cell_of.push_back(0u);
        tkh::cell_cdf(count, p->seed, p->cb_mu, p->cb_sigma, p->cb_dropout, cdf);
        if (!std::isfinite(cdf.back()) || !(cdf.back() > 0.0)) { ctx->err = "abundance: the cell weights of --cb-lognorm-params overflow (or are all 0)"; return TKSMSEQ_EINVAL; }
    } else if (lr_mode) {
        if (!tkh::abund_read_file(p->lr_br_path, text, ctx->err)) return TKSMSEQ_EIO;
        if (!tkh::parse_lr_br(text.data(), text.size(), lr, ctx->err)) return TKSMSEQ_EINVAL;
    }
    tkh::AbundInput in;
    {
        if (!tkh::abund_read_file(paf_path, text, ctx->err)) return TKSMSEQ_EIO;
        bool limit = false;
        if (!tkh::parse_paf_abund(text.data(), text.size(), in, ctx->err, &limit)) return limit ? TKSMSEQ_ELIMIT : TKSMSEQ_EINVAL;
        std::string().swap(text);
    }
    const uint64_t n_reads64 = in.rnames.size(), n_rec64 = in.tid.size(), T64 = in.tnames.size();
    if (n_reads64 >= ABUND_LIMIT || n_rec64 >= ABUND_LIMIT || T64 >= ABUND_LIMIT) { ctx->err = "abundance: 2^31 reads, records or transcripts or more"; return TKSMSEQ_ELIMIT; }
    const uint32_t n_reads = (uint32_t)n_reads64, n_rec = (uint32_t)n_rec64, T = (uint32_t)T64;
    std::vector<uint32_t> read_cell;
    if (lr_mode) {
        read_cell.resize(n_reads);
        for (uint32_t r = 0; r < n_reads; r++) { auto it = lr.find(in.rnames[r]); read_cell[r] = it == lr.end() ? 0u : cell_id(it->second); }
    }
    R->tnames = in.tnames;
    R->kept.assign(n_reads, 0);
    R->abundance.assign(T, 0.0);
    auto finish = [&]() {
        R->rnames.swap(in.rnames);
        tkh::abundance_tsv(R->rows, R->tnames, R->cells, R->tsv);
        // (the rows the writer skips are not rows of the result)
        std::vector<tkh::AbundRow> kept_rows;
        char num[400];
        for (const auto& r : R->rows) {
            const double tpm = r.a * 1000000.0;
            if (tpm < 0.001) continue;
            snprintf(num, sizeof num, "%.3f", tpm);
            if (strcmp(num, "0.000")) kept_rows.push_back(r);
        }
        R->rows.swap(kept_rows);
        *out = R.release();
        return TKSMSEQ_OK;
    };
    if (!n_reads) return finish();

    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    Events<2> ev;
    if (int rc = ev.create(ctx)) return rc;
    TmpBuf d_rec_off(s), d_tid(s), d_tstart(s), d_nmatch(s), d_blen(s), d_qlen(s), d_read_cell(s), d_cdf(s), d_cell_of(s);
    HIPCHK(ctx, upload(d_rec_off, in.rec_off, s));
    HIPCHK(ctx, upload(d_tid, in.tid, s));
    HIPCHK(ctx, upload(d_tstart, in.tstart, s));
    HIPCHK(ctx, upload(d_nmatch, in.nmatch, s));
    HIPCHK(ctx, upload(d_blen, in.blen, s));
    HIPCHK(ctx, upload(d_qlen, in.qlen, s));
    if (lr_mode) HIPCHK(ctx, upload(d_read_cell, read_cell, s));
    if (cb_mode) { HIPCHK(ctx, upload(d_cdf, cdf, s)); HIPCHK(ctx, upload(d_cell_of, cell_of, s)); }
    if (int rc = ev.mark(ctx, 0)) return rc;

    // ---- get_compatibility: count, scan, write
    TmpBuf d_best(s), d_packed(s), d_scanned(s), d_bad(s);
    HIPCHK(ctx, d_best.ensure((size_t)n_reads * 4));
    HIPCHK(ctx, d_packed.ensure(((size_t)n_reads + 1) * 8));
    HIPCHK(ctx, d_scanned.ensure(((size_t)n_reads + 1) * 8));
    HIPCHK(ctx, d_bad.ensure(4));
    HIPCHK(ctx, tk::launch_abund_compat(d_rec_off.as<uint32_t>(), d_tstart.as<uint32_t>(), d_nmatch.as<uint32_t>(), d_blen.as<uint32_t>(), d_qlen.as<uint32_t>(), n_reads,
                                        d_best.as<uint32_t>(), d_packed.as<uint64_t>(), d_bad.as<uint32_t>(), s));
    if (int rc = scan_u64(ctx, d_packed.as<uint64_t>(), d_scanned.as<uint64_t>(), n_reads)) return rc;
    uint64_t totals = 0; uint32_t bad = tk::ABUND_NO_READ;
    HIPCHK(ctx, hipMemcpyAsync(&totals, d_scanned.as<uint64_t>() + n_reads, 8, hipMemcpyDeviceToHost, s));
    HIPCHK(ctx, hipMemcpyAsync(&bad, d_bad.p, 4, hipMemcpyDeviceToHost, s));
    HIPCHK(ctx, hipStreamSynchronize(s));
    if (bad != tk::ABUND_NO_READ) {
        if (bad >= n_reads) { ctx->err = "abundance: the compatibility pass named a read that does not exist"; return TKSMSEQ_EDEVICE; }
        ctx->err = "abundance: read " + in.rnames[bad] + (in.qlen[bad] == 0 ? ": its first record has query length 0" : ": its best record has 0 matches and passes the aligned-fraction gate") +
                   " (the reference divides by it)";
        return TKSMSEQ_EINVAL;
    }
    const uint32_t n_surv = (uint32_t)(totals >> 32), n_hits = (uint32_t)totals;
    if (n_surv > n_reads || n_hits > n_rec) { ctx->err = "abundance: the compatibility pass counted more hits than records"; return TKSMSEQ_EDEVICE; }
    R->n_hits = n_hits;
    if (!n_hits) return finish();
    TmpBuf d_surv(s), d_hit_off(s), d_hit_tid(s), d_hit_read(s), d_w(s);
    HIPCHK(ctx, d_surv.ensure((size_t)n_surv * 4));
    HIPCHK(ctx, d_hit_off.ensure(((size_t)n_surv + 1) * 4));
    HIPCHK(ctx, d_hit_tid.ensure((size_t)n_hits * 4));
    HIPCHK(ctx, d_hit_read.ensure((size_t)n_hits * 4));
    HIPCHK(ctx, d_w.ensure((size_t)n_hits * 8));
    HIPCHK(ctx, tk::launch_abund_hits(d_rec_off.as<uint32_t>(), d_tid.as<uint32_t>(), d_tstart.as<uint32_t>(), d_nmatch.as<uint32_t>(), n_reads, d_best.as<uint32_t>(),
                                      d_packed.as<uint64_t>(), d_scanned.as<uint64_t>(), d_surv.as<uint32_t>(), d_hit_off.as<uint32_t>(), d_hit_tid.as<uint32_t>(),
                                      d_hit_read.as<uint32_t>(), d_w.as<double>(), s));

    // ---- the transposed index: the hits ordered by transcript, read order kept within one
    TmpBuf d_tkeys(s), d_perm(s), d_off(s), d_abund(s);
    HIPCHK(ctx, d_tkeys.ensure((size_t)n_hits * 4));
    HIPCHK(ctx, d_perm.ensure((size_t)n_hits * 4));
    HIPCHK(ctx, d_off.ensure(((size_t)T + 1) * 4));
    HIPCHK(ctx, d_abund.ensure((size_t)T * 8));
    if (int rc = sort_pairs<uint32_t>(ctx, tk::abund_sort_u32, d_hit_tid.as<uint32_t>(), d_tkeys.as<uint32_t>(), d_perm.as<uint32_t>(), n_hits, bits_for(T))) return rc;
    HIPCHK(ctx, tk::launch_abund_dense_offsets(d_tkeys.as<uint32_t>(), n_hits, T, d_off.as<uint32_t>(), s));
    SegSum by_t(s);
    if (int rc = by_t.build(ctx, d_off.as<uint32_t>(), T)) return rc;

    // ---- EM (:358-362): M-step, E-step
    const int rounds = std::max(0, p->em_iterations);
    for (int it = 0; it < rounds; it++) {
        if (int rc = by_t.run(ctx, d_w.as<double>(), d_perm.as<uint32_t>(), d_off.as<uint32_t>())) return rc;
        if (it + 1 == rounds) HIPCHK(ctx, tk::launch_abund_scale(by_t.sum.as<double>(), by_t.total.as<double>(), T, d_abund.as<double>(), s));
        HIPCHK(ctx, tk::launch_abund_estep(d_hit_off.as<uint32_t>(), d_hit_tid.as<uint32_t>(), n_surv, by_t.sum.as<double>(), by_t.total.as<double>(), d_w.as<double>(), s));
    }

    // ---- calculate_split_abundance (:292-302)
    const bool one_cell = !cb_mode && (!lr_mode || R->cells.size() == 1);
    TmpBuf d_cell(s), d_keys(s), d_skeys(s), d_sperm(s), d_soff(s), d_segkey(s), d_flag(s), d_fscan(s);
    SegSum by_key(s);
    SegSum* split = &by_t;
    const uint32_t* split_perm = d_perm.as<uint32_t>();
    const uint32_t* split_off = d_off.as<uint32_t>();
    uint32_t n_seg = T;
    if (one_cell || rounds == 0) {
        // one cell: the split is the M-step on the final weights, over the index that exists already
        if (int rc = by_t.run(ctx, d_w.as<double>(), d_perm.as<uint32_t>(), d_off.as<uint32_t>())) return rc;
        if (rounds == 0) HIPCHK(ctx, tk::launch_abund_scale(by_t.sum.as<double>(), by_t.total.as<double>(), T, d_abund.as<double>(), s));
    }
    if (!one_cell) {
        HIPCHK(ctx, d_cell.ensure((size_t)n_surv * 4));
        if (cb_mode) HIPCHK(ctx, tk::launch_abund_cells(p->seed, d_cdf.as<double>(), d_cell_of.as<uint32_t>(), (uint32_t)cdf.size(), n_surv, d_cell.as<uint32_t>(), s));
        else HIPCHK(ctx, tk::launch_abund_gather_cells(d_surv.as<uint32_t>(), d_read_cell.as<uint32_t>(), n_surv, d_cell.as<uint32_t>(), s));
        HIPCHK(ctx, d_keys.ensure((size_t)n_hits * 8));
        HIPCHK(ctx, d_skeys.ensure((size_t)n_hits * 8));
        HIPCHK(ctx, d_sperm.ensure((size_t)n_hits * 4));
        HIPCHK(ctx, d_soff.ensure(((size_t)n_hits + 1) * 4));
        HIPCHK(ctx, d_segkey.ensure((size_t)n_hits * 8));
        HIPCHK(ctx, d_flag.ensure(((size_t)n_hits + 1) * 8));
        HIPCHK(ctx, d_fscan.ensure(((size_t)n_hits + 1) * 8));
        HIPCHK(ctx, tk::launch_abund_keys(d_hit_tid.as<uint32_t>(), d_hit_read.as<uint32_t>(), d_cell.as<uint32_t>(), n_hits, d_keys.as<uint64_t>(), s));
        if (int rc = sort_pairs<uint64_t>(ctx, tk::abund_sort_u64, d_keys.as<uint64_t>(), d_skeys.as<uint64_t>(), d_sperm.as<uint32_t>(), n_hits, 32 + bits_for(T))) return rc;
        HIPCHK(ctx, tk::launch_abund_seg_flags(d_skeys.as<uint64_t>(), n_hits, d_flag.as<uint64_t>(), s));
        if (int rc = scan_u64(ctx, d_flag.as<uint64_t>(), d_fscan.as<uint64_t>(), n_hits)) return rc;
        uint64_t ns = 0;
        if (int rc = fetch_u64(ctx, d_fscan.as<uint64_t>() + n_hits, ns)) return rc;
        if (ns == 0 || ns > n_hits) { ctx->err = "abundance: the split counted more (transcript, cell) pairs than hits"; return TKSMSEQ_EDEVICE; }
        n_seg = (uint32_t)ns;
        HIPCHK(ctx, tk::launch_abund_seg_write(d_skeys.as<uint64_t>(), n_hits, d_flag.as<uint64_t>(), d_fscan.as<uint64_t>(), d_soff.as<uint32_t>(), d_segkey.as<uint64_t>(), s));
        if (int rc = by_key.build(ctx, d_soff.as<uint32_t>(), n_seg)) return rc;
        if (int rc = by_key.run(ctx, d_w.as<double>(), d_sperm.as<uint32_t>(), d_soff.as<uint32_t>())) return rc;
        split = &by_key; split_perm = d_sperm.as<uint32_t>(); split_off = d_soff.as<uint32_t>();
    }
    // rows in order of first appearance of the pair: by the pair's lowest hit index
    TmpBuf d_rank(s), d_rank_sorted(s), d_order(s);
    HIPCHK(ctx, d_rank.ensure((size_t)n_seg * 4));
    HIPCHK(ctx, d_rank_sorted.ensure((size_t)n_seg * 4));
    HIPCHK(ctx, d_order.ensure((size_t)n_seg * 4));
    HIPCHK(ctx, tk::launch_abund_ranks(split_perm, split_off, n_seg, d_rank.as<uint32_t>(), s));
    if (int rc = sort_pairs<uint32_t>(ctx, tk::abund_sort_u32, d_rank.as<uint32_t>(), d_rank_sorted.as<uint32_t>(), d_order.as<uint32_t>(), n_seg, 32)) return rc;
    if (int rc = ev.mark(ctx, 1)) return rc;

    std::vector<uint32_t> order, rank_sorted;
    std::vector<uint64_t> seg_key;
    std::vector<double> sums;
    double total = 0.0;
    HIPCHK(ctx, download(order, d_order, n_seg, s));
    HIPCHK(ctx, download(rank_sorted, d_rank_sorted, n_seg, s));
    HIPCHK(ctx, download(sums, split->sum, n_seg, s));
    if (!one_cell) HIPCHK(ctx, download(seg_key, d_segkey, n_seg, s));
    HIPCHK(ctx, download(&total, split->total, 1, s));
    HIPCHK(ctx, download(R->abundance, d_abund, T, s));
    HIPCHK(ctx, download(R->surv_read, d_surv, n_surv, s));
    if (p->keep_hits) {
        HIPCHK(ctx, download(R->hit_off, d_hit_off, (size_t)n_surv + 1, s));
        HIPCHK(ctx, download(R->hit_tid, d_hit_tid, n_hits, s));
        HIPCHK(ctx, download(R->hit_w, d_w, n_hits, s));
        if (!one_cell) HIPCHK(ctx, download(R->surv_cell, d_cell, n_surv, s));
        else R->surv_cell.assign(n_surv, 0u);
        R->have_hits = true;
    }
    HIPCHK(ctx, hipStreamSynchronize(s));
    if (int rc = ev.add(ctx, 0, R->device_ms)) return rc;
    for (uint32_t r : R->surv_read) if (r < n_reads) R->kept[r] = 1;
    for (uint32_t j = 0; j < n_seg && rank_sorted[j] != tk::ABUND_NO_READ; j++) {
        const uint32_t g = order[j];
        if (g >= n_seg) { ctx->err = "abundance: the row order names a row that does not exist"; return TKSMSEQ_EDEVICE; }
        tkh::AbundRow row;
        row.tid = one_cell ? g : (uint32_t)(seg_key[g] >> 32);
        row.cell = one_cell ? 0u : (uint32_t)seg_key[g];
        row.a = sums[g] / total;                                   // :301
        if (row.tid >= T || row.cell >= R->cells.size()) { ctx->err = "abundance: a row names a transcript or cell that does not exist"; return TKSMSEQ_EDEVICE; }
        R->rows.push_back(row);
    }
    return finish();
}

extern "C" int tksmseq_abundance_info(const tksmseq_abundance_result* r, uint64_t* rows, uint64_t* surviving_reads, uint64_t* reads, uint64_t* transcripts,
                                      uint64_t* hits) {
    if (!r) return TKSMSEQ_EINVAL;
    if (rows) *rows = r->rows.size();
    if (surviving_reads) *surviving_reads = r->surv_read.size();
    if (reads) *reads = r->rnames.size();
    if (transcripts) *transcripts = r->tnames.size();
    if (hits) *hits = r->n_hits;
    return TKSMSEQ_OK;
}
extern "C" int tksmseq_abundance_row(const tksmseq_abundance_result* r, uint64_t i, const char** transcript, const char** cell, double* tpm) {
    if (!r || i >= r->rows.size()) return TKSMSEQ_EINVAL;
    if (transcript) *transcript = r->tnames[r->rows[i].tid].c_str();
    if (cell) *cell = r->cells[r->rows[i].cell].c_str();
    if (tpm) *tpm = r->rows[i].a * 1000000.0;
    return TKSMSEQ_OK;
}
extern "C" int tksmseq_abundance_vector(const tksmseq_abundance_result* r, const double** abundance) {
    if (!r || !abundance) return TKSMSEQ_EINVAL;
    *abundance = r->abundance.data();
    return TKSMSEQ_OK;
}
extern "C" int tksmseq_abundance_transcript(const tksmseq_abundance_result* r, uint64_t t, const char** name) {
    if (!r || !name || t >= r->tnames.size()) return TKSMSEQ_EINVAL;
    *name = r->tnames[t].c_str();
    return TKSMSEQ_OK;
}
extern "C" int tksmseq_abundance_cell(const tksmseq_abundance_result* r, uint64_t c, const char** name) {
    if (!r || !name || c >= r->cells.size()) return TKSMSEQ_EINVAL;
    *name = r->cells[c].c_str();
    return TKSMSEQ_OK;
}
extern "C" int tksmseq_abundance_read(const tksmseq_abundance_result* r, uint64_t i, const char** name, int32_t* kept) {
    if (!r || i >= r->rnames.size()) return TKSMSEQ_EINVAL;
    if (name) *name = r->rnames[i].c_str();
    if (kept) *kept = r->kept[i];
    return TKSMSEQ_OK;
}
extern "C" int tksmseq_abundance_hits(const tksmseq_abundance_result* r, const uint32_t** surviving, const uint32_t** cell, const uint32_t** hit_offsets,
                                      const uint32_t** hit_transcript, const double** hit_weight) {
    if (!r) return TKSMSEQ_EINVAL;
    if (!r->have_hits && !r->surv_read.empty()) return TKSMSEQ_ESTATE;
    if (surviving) *surviving = r->surv_read.data();
    if (cell) *cell = r->surv_cell.data();
    if (hit_offsets) *hit_offsets = r->hit_off.data();
    if (hit_transcript) *hit_transcript = r->hit_tid.data();
    if (hit_weight) *hit_weight = r->hit_w.data();
    return TKSMSEQ_OK;
}
extern "C" int tksmseq_abundance_device_ms(const tksmseq_abundance_result* r, float* ms) {
    if (!r || !ms) return TKSMSEQ_EINVAL;
    *ms = r->device_ms;
    return TKSMSEQ_OK;
}
extern "C" int tksmseq_abundance_write(const tksmseq_abundance_result* r, const char* out_path) {
    if (!r || !out_path) return TKSMSEQ_EINVAL;
    std::string e;
    return tkh::write_abundance_file(out_path, r->tsv, e) ? TKSMSEQ_OK : TKSMSEQ_EIO;
}
extern "C" void tksmseq_abundance_free(tksmseq_abundance_result* r) { delete r; }
