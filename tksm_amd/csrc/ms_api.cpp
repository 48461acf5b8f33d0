// ms_api.cpp -- C-ABI of model-sequence: tksmseq_model_sequence (include/tksmseq.h).  The host reads and checks (ms_host.cpp); the columns,
// the events, their counting and the selection of the printed rows run on the device (ms_kernels.hip); the host formats the two files.
#include <cstring>
#include <string>
#include <vector>

#include "abund_host.h"
#include "ctx.h"
#include "ms_host.h"
#include "ms_kernels.h"
#include "tool_run.h"

namespace {

constexpr uint64_t MS_LIMIT = 1ull << 31;
static_assert(sizeof(tk::MsErrRowDev) == sizeof(tkh::MsErrRow), "the device's error-model row is the host's");
static_assert(tk::MS_ALT_SLOTS == tkh::MS_MAX_ALT, "the device's error-model row is the host's");

// a reduced table: distinct (key, sub) in ascending order with their counts
struct Table {
    TmpBuf keys, subs, counts;
    uint32_t n = 0;
    bool with_subs;
    Table(hipStream_t s, bool with_subs_) : keys(s), subs(s), counts(s), with_subs(with_subs_) {}
};

// the runs of equal (key, sub) among n items, MS_NO_EVENT dropped: out.counts = run lengths, or the sums of vals over the runs.
// A q-score key fills 63 bits and q does not fit beside it: the items are ordered by sub first, then stably by key.
int reduce(tksmseq_ctx* ctx, const uint64_t* keys, const uint32_t* subs, const uint64_t* vals, uint32_t n, int key_bits, Table& out) {
    hipStream_t s = ctx->stream;
    out.n = 0;
    if (!n) return TKSMSEQ_OK;
    TmpBuf d_skeys(s), d_perm(s), d_ssub(s), d_start(s);
    HIPCHK(ctx, d_skeys.ensure((size_t)n * 8));
    HIPCHK(ctx, d_perm.ensure((size_t)n * 4));
    if (subs) {
        TmpBuf d_perm_a(s), d_keys_a(s), d_perm_b(s);
        HIPCHK(ctx, d_perm_a.ensure((size_t)n * 4));
        HIPCHK(ctx, d_perm_b.ensure((size_t)n * 4));
        HIPCHK(ctx, d_keys_a.ensure((size_t)n * 8));
        HIPCHK(ctx, d_ssub.ensure((size_t)n * 4));
        if (int rc = sort_pairs<uint32_t>(ctx, tk::abund_sort_u32, subs, d_ssub.as<uint32_t>(), d_perm_a.as<uint32_t>(), n, 7)) return rc;
        HIPCHK(ctx, tk::launch_ms_gather_u64(keys, d_perm_a.as<uint32_t>(), n, d_keys_a.as<uint64_t>(), s));
        if (int rc = sort_pairs<uint64_t>(ctx, tk::abund_sort_u64, d_keys_a.as<uint64_t>(), d_skeys.as<uint64_t>(), d_perm_b.as<uint32_t>(), n, key_bits)) return rc;
        HIPCHK(ctx, tk::launch_ms_gather_u32(d_perm_a.as<uint32_t>(), d_perm_b.as<uint32_t>(), n, d_perm.as<uint32_t>(), s));
        HIPCHK(ctx, tk::launch_ms_gather_u32(subs, d_perm.as<uint32_t>(), n, d_ssub.as<uint32_t>(), s));
        HIPCHK(ctx, hipStreamSynchronize(s));          // (the three temporaries go back to the cache here)
    } else if (int rc = sort_pairs<uint64_t>(ctx, tk::abund_sort_u64, keys, d_skeys.as<uint64_t>(), d_perm.as<uint32_t>(), n, key_bits)) return rc;
    const uint32_t* ssub = subs ? d_ssub.as<uint32_t>() : nullptr;
    uint64_t info[2] = {};
    if (int rc = run_starts(ctx, d_skeys.as<uint64_t>(), ssub, n, d_start, info)) return rc;
    if (info[0] == 0 || info[0] > n) { ctx->err = "model-sequence: the reduce counted more runs than items"; return TKSMSEQ_EDEVICE; }
    const uint32_t runs = (uint32_t)(info[0] - (info[1] ? 1 : 0));
    HIPCHK(ctx, out.keys.ensure(std::max<size_t>(runs, 1) * 8));
    HIPCHK(ctx, out.counts.ensure(std::max<size_t>(runs, 1) * 8));
    if (out.with_subs) HIPCHK(ctx, out.subs.ensure(std::max<size_t>(runs, 1) * 4));
    HIPCHK(ctx, tk::launch_ms_run_write(d_skeys.as<uint64_t>(), ssub, d_start.as<uint32_t>(), runs, vals, d_perm.as<uint32_t>(), out.keys.as<uint64_t>(),
                                        out.with_subs ? out.subs.as<uint32_t>() : nullptr, out.counts.as<uint64_t>(), s));
    HIPCHK(ctx, hipStreamSynchronize(s));              // (the sorted items go back to the cache)
    out.n = runs;
    return TKSMSEQ_OK;
}

// acc = the reduce of acc and part laid end to end: counts add up, whatever the chunks were
int merge(tksmseq_ctx* ctx, Table& acc, const Table& part, int key_bits) {
    hipStream_t s = ctx->stream;
    if (!part.n) return TKSMSEQ_OK;
    const uint64_t n = (uint64_t)acc.n + part.n;
    if (n >= MS_LIMIT) { ctx->err = "model-sequence: 2^31 distinct keys or more"; return TKSMSEQ_ELIMIT; }
    TmpBuf d_keys(s), d_subs(s), d_counts(s);
    HIPCHK(ctx, d_keys.ensure(n * 8));
    HIPCHK(ctx, d_counts.ensure(n * 8));
    if (acc.with_subs) HIPCHK(ctx, d_subs.ensure(n * 4));
    auto cat = [&](TmpBuf& d, const TmpBuf& a, const TmpBuf& b, size_t w) -> hipError_t {
        hipError_t e = acc.n ? hipMemcpyAsync(d.p, a.p, (size_t)acc.n * w, hipMemcpyDeviceToDevice, s) : hipSuccess;
        if (e == hipSuccess) e = hipMemcpyAsync((char*)d.p + (size_t)acc.n * w, b.p, (size_t)part.n * w, hipMemcpyDeviceToDevice, s);
        return e;
    };
    HIPCHK(ctx, cat(d_keys, acc.keys, part.keys, 8));
    HIPCHK(ctx, cat(d_counts, acc.counts, part.counts, 8));
    if (acc.with_subs) HIPCHK(ctx, cat(d_subs, acc.subs, part.subs, 4));
    return reduce(ctx, d_keys.as<uint64_t>(), acc.with_subs ? d_subs.as<uint32_t>() : nullptr, d_counts.as<uint64_t>(), (uint32_t)n, key_bits, acc);
}

int check_params(tksmseq_ctx* ctx, const tksmseq_model_sequence_params* p) {
    auto bad = [&](const char* what) { ctx->err = std::string("model-sequence: ") + what; return TKSMSEQ_EINVAL; };
    if (p->error_k < 3 || p->error_k > 8) return bad("error_k must be in [3, 8]");
    if (p->qscore_k < 1 || p->qscore_k > 29 || p->qscore_k % 2 == 0) return bad("qscore_k must be odd and in [1, 29]");
    if (p->max_alt < 0 || p->max_alt > tkh::MS_MAX_ALT) return bad("max_alt must be in [0, 31]");
    if (p->max_del < 0) return bad("max_del must not be negative");
    if (p->max_alignments < 0 || p->min_occur < 0 || p->max_output < 0) return bad("max_alignments, min_occur and max_output must not be negative");
    if (p->max_output >= (int64_t)MS_LIMIT) return bad("max_output must be below 2^31");
    return TKSMSEQ_OK;
}

constexpr int ERR_BITS = 48, QS_BITS = 64;
// the state of one call: what outlives a phase
struct MsRun {
    tksmseq_ctx* ctx;
    hipStream_t s;
    const tksmseq_model_sequence_params* p;
    const int K, S;
    tksmseq_model_sequence_info info{};
    std::chrono::steady_clock::time_point t0;
    tkh::MsReads reads;
    tkh::MsAlignments al;
    uint32_t n_aln = 0;
    // per alignment: columns, read positions, reference positions, error events, and their running sums
    std::vector<tk::MsAlnDev> h_aln;
    std::vector<uint64_t> cnt[4], sum[4];
    uint64_t chunk_events = 0;
    Events<5> ev;
    TmpBuf d_aln, d_ops, d_bases, d_quals, d_cnt, d_off[4];
    Table acc_e, acc_q;
    std::vector<tkh::MsErrRow> err_rows;
    tkh::MsQRow overall, forced[3];
    std::vector<tkh::MsQRow> best;

    MsRun(tksmseq_ctx* c, const tksmseq_model_sequence_params* q)
        : ctx(c), s(c->stream), p(q), K(q->error_k), S((q->qscore_k + 1) / 2 + 1), d_aln(s), d_ops(s), d_bases(s), d_quals(s), d_cnt(s),
          d_off{TmpBuf(s), TmpBuf(s), TmpBuf(s), TmpBuf(s)}, acc_e(s, false), acc_q(s, true) {}

    // ---- the host reads
    int load(const char* reads_paths, const char* paf_path) {
        t0 = std::chrono::steady_clock::now();
        // (deliberate compatibility, not an oversight: here a limit is reported as "<path>: ...", and the reads are not counted after every file as map and barcode-match do)
        if (int rc = tkh::load_fastq_list(reads_paths, reads, ctx->err)) return rc;
        std::unordered_map<std::string, uint32_t> targets;
        std::vector<uint64_t> target_len;
        for (size_t c = 0; c < ctx->contig_names.size(); c++) { targets.emplace(ctx->contig_names[c], (uint32_t)c); target_len.push_back(ctx->contigs[2 * c + 1]); }
        std::string text;
        if (!tkh::abund_read_file(paf_path, text, ctx->err)) return TKSMSEQ_EIO;
        if (!tkh::parse_paf_ms(text.data(), text.size(), reads, targets, target_len, (uint64_t)p->max_alignments, al, ctx->err))
            return ctx->err.compare(0, 3, "PAF") ? TKSMSEQ_ELIMIT : TKSMSEQ_EINVAL;
        info.lines = al.lines; info.used = al.aln.size();
        info.skipped_no_cigar = al.no_cigar; info.skipped_supplementary = al.supplementary; info.skipped_unknown_read = al.unknown_read;
        info.skipped_unknown_target = al.unknown_target; info.skipped_cigar_op = al.cigar_op;
        if (al.aln.empty()) { ctx->err = "model-sequence: no alignment of " + std::string(paf_path) + " can be used"; return TKSMSEQ_EINVAL; }
        if (al.aln.size() >= MS_LIMIT) { ctx->err = "model-sequence: 2^31 alignments or more"; return TKSMSEQ_ELIMIT; }
        n_aln = (uint32_t)al.aln.size();
        return TKSMSEQ_OK;
    }

    // ---- the counts of every alignment, and the chunks: runs of alignments of at most chunk_events events
    int plan() {
        h_aln.resize(n_aln);
        for (auto& c : cnt) c.assign((size_t)n_aln + 1, 0);
        for (auto& c : sum) c.assign((size_t)n_aln + 1, 0);
        for (uint32_t a = 0; a < n_aln; a++) {
            const tkh::MsAln& x = al.aln[a];
            tk::MsAlnDev& d = h_aln[a];
            d.read_off = reads.off[x.read]; d.ref_g = ctx->contigs[2 * (size_t)x.tid] + x.tstart;
            d.qlen = x.qlen; d.qstart = x.qstart; d.qend = x.qend; d.strand = x.strand; d.tlen = x.tend - x.tstart; d.op_off = x.op_off; d.n_ops = x.n_ops; d.pad = 0;
            uint64_t ncol = 0;
            for (uint32_t o = 0; o < x.n_ops; o++) ncol += al.ops[x.op_off + o] >> 2;
            cnt[0][a] = ncol; cnt[1][a] = x.qend - x.qstart; cnt[2][a] = d.tlen; cnt[3][a] = d.tlen >= (uint32_t)K ? d.tlen - (uint32_t)K + 1 : 0;
            if (ncol >= (1ull << 32) || cnt[3][a] + cnt[1][a] * (uint64_t)S >= MS_LIMIT) {
                ctx->err = "model-sequence: an alignment of 2^31 events or more (read " + std::to_string(x.read) + ")";
                return TKSMSEQ_ELIMIT;
            }
            for (int k = 0; k < 4; k++) sum[k][a + 1] = sum[k][a] + cnt[k][a];
        }
        info.read_ms = ms_since(t0);

        HIPCHK(ctx, hipSetDevice(ctx->device));
        chunk_events = p->chunk_events;
        if (!chunk_events) {
            size_t free_b = 0, total_b = 0;
            HIPCHK(ctx, hipMemGetInfo(&free_b, &total_b));
            chunk_events = std::max<uint64_t>(1ull << 20, std::min<uint64_t>(free_b / 192, 1ull << 28));      // (about 100 B of temporaries per event)
        }
        chunk_events = std::min<uint64_t>(chunk_events, MS_LIMIT - 1);
        return ev.create(ctx);
    }

    // ---- uploads, and the offsets of the ragged arrays (scans of the counts)
    int upload_inputs() {
        t0 = std::chrono::steady_clock::now();
        HIPCHK(ctx, upload(d_aln, h_aln, s));
        HIPCHK(ctx, upload(d_ops, al.ops, s));
        HIPCHK(ctx, upload(d_bases, reads.bases, s));
        HIPCHK(ctx, upload(d_quals, reads.quals, s));
        for (int k = 0; k < 4; k++) {
            HIPCHK(ctx, upload(d_cnt, cnt[k], s));
            HIPCHK(ctx, d_off[k].ensure(((size_t)n_aln + 1) * 8));
            if (int rc = scan_u64(ctx, d_cnt.as<uint64_t>(), d_off[k].as<uint64_t>(), n_aln)) return rc;
            HIPCHK(ctx, hipStreamSynchronize(s));          // (d_cnt is written again for the next array)
        }
        info.upload_ms = ms_since(t0);
        return TKSMSEQ_OK;
    }

    // ---- the chunks: runs of alignments of at most chunk_events events; their events, reduced and merged into the two tables
    int chunks() {
        for (uint32_t a0 = 0; a0 < n_aln;) {
            uint32_t a1 = a0 + 1;
            auto events_to = [&](uint32_t a) { return sum[3][a] - sum[3][a0] + (sum[1][a] - sum[1][a0]) * (uint64_t)S; };
            while (a1 < n_aln && events_to(a1 + 1) <= chunk_events) a1++;
            const tk::RefView R{ctx->d_packed.as<uint32_t>(), ctx->d_blocktab.as<uint32_t>(), ctx->d_pool.as<uint8_t>(), ctx->d_contigs.as<uint64_t>(),
                                (uint32_t)(ctx->contigs.size() / 2)};
            const uint64_t n_col = sum[0][a1] - sum[0][a0], n_rp = sum[1][a1] - sum[1][a0], n_tp = sum[2][a1] - sum[2][a0], n_ee = sum[3][a1] - sum[3][a0];
            if (n_ee >= MS_LIMIT || n_rp * (uint64_t)S >= MS_LIMIT) { ctx->err = "model-sequence: a chunk of 2^31 events or more"; return TKSMSEQ_ELIMIT; }
            const tk::MsChunk C{d_off[0].as<uint64_t>(), d_off[1].as<uint64_t>(), d_off[2].as<uint64_t>(), d_off[3].as<uint64_t>(),
                                sum[0][a0], sum[1][a0], sum[2][a0], sum[3][a0], a0, a1};
            TmpBuf d_cols(s), d_rcol(s), d_tcol(s), d_ekeys(s), d_qkeys(s), d_qsubs(s);
            HIPCHK(ctx, d_cols.ensure(std::max<uint64_t>(n_col, 1)));
            HIPCHK(ctx, d_rcol.ensure(std::max<uint64_t>(n_rp, 1) * 4));
            HIPCHK(ctx, d_tcol.ensure(std::max<uint64_t>(n_tp, 1) * 4));
            HIPCHK(ctx, d_ekeys.ensure(std::max<uint64_t>(n_ee, 1) * 8));
            HIPCHK(ctx, d_qkeys.ensure(std::max<uint64_t>(n_rp * S, 1) * 8));
            HIPCHK(ctx, d_qsubs.ensure(std::max<uint64_t>(n_rp * S, 1) * 4));
            if (int rc = ev.mark(ctx, 0)) return rc;
            HIPCHK(ctx, tk::launch_ms_expand(d_aln.as<tk::MsAlnDev>(), d_ops.as<uint32_t>(), d_bases.as<uint8_t>(), R, C, d_cols.as<uint8_t>(), d_rcol.as<uint32_t>(),
                                             d_tcol.as<uint32_t>(), s));
            if (int rc = ev.mark(ctx, 1)) return rc;
            HIPCHK(ctx, tk::launch_ms_err_events(d_aln.as<tk::MsAlnDev>(), d_bases.as<uint8_t>(), R, C, d_cols.as<uint8_t>(), d_rcol.as<uint32_t>(), d_tcol.as<uint32_t>(), K,
                                                 n_ee, d_ekeys.as<uint64_t>(), s));
            HIPCHK(ctx, tk::launch_ms_qs_events(d_aln.as<tk::MsAlnDev>(), d_quals.as<uint8_t>(), C, d_cols.as<uint8_t>(), d_rcol.as<uint32_t>(), p->qscore_k,
                                                (int)std::min<int32_t>(p->max_del, 1 << 20), n_rp, d_qkeys.as<uint64_t>(), d_qsubs.as<uint32_t>(), s));
            if (int rc = ev.mark(ctx, 2)) return rc;
            {
                Table part_e(s, false), part_q(s, true);
                if (int rc = reduce(ctx, d_ekeys.as<uint64_t>(), nullptr, nullptr, (uint32_t)n_ee, ERR_BITS, part_e)) return rc;
                if (int rc = merge(ctx, acc_e, part_e, ERR_BITS)) return rc;
                if (int rc = reduce(ctx, d_qkeys.as<uint64_t>(), d_qsubs.as<uint32_t>(), nullptr, (uint32_t)(n_rp * S), QS_BITS, part_q)) return rc;
                if (int rc = merge(ctx, acc_q, part_q, QS_BITS)) return rc;
            }
            if (int rc = ev.mark(ctx, 3)) return rc;
            HIPCHK(ctx, hipStreamSynchronize(s));
            for (int k = 0; k < 3; k++) if (int rc = ev.add(ctx, k, info.stage_ms[k])) return rc;
            info.chunks++;
            info.events += n_ee + n_rp * (uint64_t)S;
            a0 = a1;
        }
        info.error_keys = acc_e.n;
        return TKSMSEQ_OK;
    }

    // ---- select: the rows the host prints.  Mark 3 opens the selection's stage; select_qscore_rows closes it with mark 4
    int select_error_rows() {
        if (int rc = ev.mark(ctx, 3)) return rc;
        err_rows.resize((size_t)1 << (2 * K));
        TmpBuf d_key2(s), d_key2s(s), d_perm(s), d_bad(s), d_rows(s);
        HIPCHK(ctx, d_key2.ensure(std::max<size_t>(acc_e.n, 1) * 8));
        HIPCHK(ctx, d_key2s.ensure(std::max<size_t>(acc_e.n, 1) * 8));
        HIPCHK(ctx, d_perm.ensure(std::max<size_t>(acc_e.n, 1) * 4));
        HIPCHK(ctx, d_bad.ensure(4));
        HIPCHK(ctx, d_rows.ensure(err_rows.size() * sizeof(tk::MsErrRowDev)));
        HIPCHK(ctx, hipMemsetAsync(d_rows.p, 0, err_rows.size() * sizeof(tk::MsErrRowDev), s));
        HIPCHK(ctx, tk::launch_ms_err_rank_keys(acc_e.keys.as<uint64_t>(), acc_e.counts.as<uint64_t>(), acc_e.n, d_key2.as<uint64_t>(), d_bad.as<uint32_t>(), s));
        if (acc_e.n)
            if (int rc = sort_pairs<uint64_t>(ctx, tk::abund_sort_u64, d_key2.as<uint64_t>(), d_key2s.as<uint64_t>(), d_perm.as<uint32_t>(), acc_e.n, 50)) return rc;
        HIPCHK(ctx, tk::launch_ms_err_select(d_key2s.as<uint64_t>(), d_perm.as<uint32_t>(), acc_e.keys.as<uint64_t>(), acc_e.counts.as<uint64_t>(), acc_e.n, K, p->max_alt,
                                             d_rows.as<tk::MsErrRowDev>(), s));
        uint32_t bad = 0;
        HIPCHK(ctx, hipMemcpyAsync(&bad, d_bad.p, 4, hipMemcpyDeviceToHost, s));
        HIPCHK(ctx, hipMemcpyAsync((void*)err_rows.data(), d_rows.p, err_rows.size() * sizeof(tk::MsErrRowDev), hipMemcpyDeviceToHost, s));
        HIPCHK(ctx, hipStreamSynchronize(s));
        if (bad) { ctx->err = "model-sequence: an alternative counted 2^32 times or more"; return TKSMSEQ_ELIMIT; }
        for (const auto& r : err_rows) { info.counting_positions += r.total; info.alternatives_too_long += r.too_long; }
        return TKSMSEQ_OK;
    }

    int select_qscore_rows() {
        forced[0].key = 1ull << 58 | (uint64_t)tk::MS_EQ << 56; forced[1].key = 1ull << 58 | (uint64_t)tk::MS_MIS << 56; forced[2].key = 1ull << 58 | (uint64_t)tk::MS_INS << 56;
        if (acc_q.n) {
            const uint32_t n = acc_q.n;
            TmpBuf d_kstart(s), d_kkey(s), d_kn(s), d_key2(s), d_key2s(s), d_perm(s), d_nqual(s), d_ids(s), d_rows(s);
            uint64_t run_info[2] = {};
            if (int rc = run_starts(ctx, acc_q.keys.as<uint64_t>(), nullptr, n, d_kstart, run_info)) return rc;
            if (run_info[0] == 0 || run_info[0] > n) { ctx->err = "model-sequence: the q-score table has more keys than entries"; return TKSMSEQ_EDEVICE; }
            const uint32_t n_keys = (uint32_t)run_info[0];
            HIPCHK(ctx, d_kkey.ensure((size_t)n_keys * 8));
            HIPCHK(ctx, d_kn.ensure((size_t)n_keys * 8));
            HIPCHK(ctx, d_key2.ensure((size_t)n_keys * 8));
            HIPCHK(ctx, d_key2s.ensure((size_t)n_keys * 8));
            HIPCHK(ctx, d_perm.ensure((size_t)n_keys * 4));
            HIPCHK(ctx, d_nqual.ensure(8));
            HIPCHK(ctx, tk::launch_ms_qs_totals(acc_q.keys.as<uint64_t>(), acc_q.subs.as<uint32_t>(), acc_q.counts.as<uint64_t>(), d_kstart.as<uint32_t>(), n_keys,
                                                (uint64_t)p->min_occur, d_kkey.as<uint64_t>(), d_kn.as<uint64_t>(), d_key2.as<uint64_t>(),
                                                (unsigned long long*)d_nqual.p, s));
            if (int rc = sort_pairs<uint64_t>(ctx, tk::abund_sort_u64, d_key2.as<uint64_t>(), d_key2s.as<uint64_t>(), d_perm.as<uint32_t>(), n_keys, 64)) return rc;
            unsigned long long n_qual = 0;
            uint64_t first_keys[4] = {~0ull, ~0ull, ~0ull, ~0ull};
            HIPCHK(ctx, hipMemcpyAsync(&n_qual, d_nqual.p, 8, hipMemcpyDeviceToHost, s));
            HIPCHK(ctx, hipMemcpyAsync(first_keys, d_kkey.p, (size_t)std::min(n_keys, 4u) * 8, hipMemcpyDeviceToHost, s));
            HIPCHK(ctx, hipStreamSynchronize(s));
            if (n_qual > n_keys) { ctx->err = "model-sequence: more qualifying keys than keys"; return TKSMSEQ_EDEVICE; }
            // the keys in ascending order start with key 0 (the overall counts) and the one-letter keys: the rows the file always has
            const uint32_t n_top = (uint32_t)std::min<uint64_t>(n_qual, (uint64_t)p->max_output);
            std::vector<uint32_t> ids((size_t)n_top + 4, 0xFFFFFFFFu);
            HIPCHK(ctx, download(ids.data(), d_perm, n_top, s));
            HIPCHK(ctx, hipStreamSynchronize(s));
            for (uint32_t g = 0; g < std::min(n_keys, 4u); g++) {
                if (first_keys[g] == 0) ids[n_top] = g;
                for (int f = 0; f < 3; f++) if (first_keys[g] == forced[f].key) ids[(size_t)n_top + 1 + f] = g;
            }
            info.qscore_keys = n_keys - (first_keys[0] == 0 ? 1 : 0);
            std::vector<tk::MsQRowDev> rows(ids.size());
            HIPCHK(ctx, upload(d_ids, ids, s));
            HIPCHK(ctx, d_rows.ensure(rows.size() * sizeof(tk::MsQRowDev)));
            HIPCHK(ctx, tk::launch_ms_qs_rows(acc_q.keys.as<uint64_t>(), acc_q.subs.as<uint32_t>(), acc_q.counts.as<uint64_t>(), d_kstart.as<uint32_t>(), d_ids.as<uint32_t>(),
                                              (uint32_t)ids.size(), n_keys, d_rows.as<tk::MsQRowDev>(), s));
            HIPCHK(ctx, download(rows.data(), d_rows, rows.size(), s));
            if (int rc = ev.mark(ctx, 4)) return rc;
            HIPCHK(ctx, hipStreamSynchronize(s));
            auto to_host = [](const tk::MsQRowDev& d, tkh::MsQRow& h) { h.key = d.key; h.n = d.n; memcpy(h.count, d.count, sizeof h.count); };
            best.resize(n_top);
            for (uint32_t j = 0; j < n_top; j++) to_host(rows[j], best[j]);
            to_host(rows[n_top], overall);
            for (int f = 0; f < 3; f++) if (ids[(size_t)n_top + 1 + f] != 0xFFFFFFFFu) to_host(rows[(size_t)n_top + 1 + f], forced[f]);
            info.read_positions = overall.n;
            info.windows_max_del = rows[n_top].count[tk::MS_SUB_MAX_DEL];
            info.keys_too_long = rows[n_top].count[tk::MS_SUB_TOO_LONG];
        } else {
            if (int rc = ev.mark(ctx, 4)) return rc;
            HIPCHK(ctx, hipStreamSynchronize(s));
        }
        if (int rc = ev.add(ctx, 3, info.stage_ms[3])) return rc;
        info.device_ms = info.stage_ms[0] + info.stage_ms[1] + info.stage_ms[2] + info.stage_ms[3];
        return TKSMSEQ_OK;
    }

    // ---- the host writes
    int write(const char* error_out, const char* qscore_out) {
        t0 = std::chrono::steady_clock::now();
        std::string text, e;
        if (qscore_out) {
            std::vector<tkh::MsQRow> rows;
            if (!tkh::qscore_select(best, forced, (uint64_t)p->max_output, rows, ctx->err)) return TKSMSEQ_EINVAL;
            tkh::qscore_model_text(overall, rows, text);
            if (!tkh::write_abundance_file(qscore_out, text, e)) { ctx->err = "model-sequence: cannot write " + std::string(qscore_out); return TKSMSEQ_EIO; }
        }
        if (error_out) {
            tkh::error_model_text(K, err_rows, text);
            if (!tkh::write_abundance_file(error_out, text, e)) { ctx->err = "model-sequence: cannot write " + std::string(error_out); return TKSMSEQ_EIO; }
        }
        info.write_ms = ms_since(t0);
        return TKSMSEQ_OK;
    }
};

}  // namespace

extern "C" int tksmseq_model_sequence(tksmseq_ctx* ctx, const tksmseq_model_sequence_params* p, const char* reads_paths, const char* paf_path, const char* error_out,
                                      const char* qscore_out, tksmseq_model_sequence_info* info_out) {
    if (!ctx) return TKSMSEQ_EINVAL;
    if (!p || !reads_paths || !paf_path) { ctx->err = "model-sequence: null argument"; return TKSMSEQ_EINVAL; }
    if (error_out && !*error_out) error_out = nullptr;
    if (qscore_out && !*qscore_out) qscore_out = nullptr;
    if (!error_out && !qscore_out) { ctx->err = "model-sequence: neither an error-model nor a q-score-model output"; return TKSMSEQ_EINVAL; }
    if (int rc = check_params(ctx, p)) return rc;
    if (ctx->contigs.empty()) { ctx->err = "model-sequence: the context has no reference"; return TKSMSEQ_ESTATE; }
    if (ctx->n_declared) { ctx->err = "model-sequence: the reference has contigs that are declared only"; return TKSMSEQ_ESTATE; }
    MsRun run(ctx, p);
    if (int rc = run.load(reads_paths, paf_path)) return rc;
    if (int rc = run.plan()) return rc;
    if (int rc = run.upload_inputs()) return rc;
    if (int rc = run.chunks()) return rc;
    if (int rc = run.select_error_rows()) return rc;
    if (int rc = run.select_qscore_rows()) return rc;
    if (int rc = run.write(error_out, qscore_out)) return rc;
    if (info_out) *info_out = run.info;
    return TKSMSEQ_OK;
}
