// bm_api.cpp -- C-ABI of barcode-match: tksmseq_barcode_match (include/tksmseq.h).  The host reads and checks (ms_host.cpp's FASTQ reader,
// bm_host.cpp), packs the two ends of every read and formats the files; the adapter alignment, the exact counts, the candidate list and the
// match of every segment against every candidate run on the device (bm_kernels.hip).
#include <cstring>
#include <string>
#include <vector>

#include "abund_host.h"
#include "bm_host.h"
#include "bm_kernels.h"
#include "ctx.h"
#include "tool_run.h"

namespace {

constexpr uint64_t BM_READ_LIMIT = 1ull << 31;
constexpr uint64_t BM_CHUNK_MAX = 1ull << 22;          // reads per chunk at most: 2 lanes per read and 32-bit lane numbers
const char* const BM_DEFAULT_ADAPTER = "CTACACGACGCTCTTCCGATCT";

int check_params(tksmseq_ctx* ctx, const tksmseq_barcode_match_params* p, const std::string& adapter) {
    auto bad = [&](const char* what) { ctx->err = std::string("barcode-match: ") + what; return TKSMSEQ_EINVAL; };
    if (!tkh::bm_is_acgt(adapter, 4, 32)) return bad("the adapter must have 4 to 32 letters of ACGT");
    if (p->window < (int32_t)adapter.size()) return bad("window must be at least the adapter's length");
    if (p->pad < 0 || p->pad > 16) return bad("pad must be in [0, 16]");
    if (p->max_adapter_errors < 0 || p->max_adapter_errors >= (int32_t)adapter.size()) return bad("max_adapter_errors must be in [0, adapter length)");
    if (p->max_errors < 0) return bad("max_errors must not be negative");
    if (p->min_exact < 0) return bad("min_exact must not be negative");
    return TKSMSEQ_OK;
}

// the state of one call: what outlives a phase
struct BmRun {
    tksmseq_ctx* ctx;
    hipStream_t s;
    const tksmseq_barcode_match_params* p;
    const std::string adapter;
    tksmseq_barcode_match_info info{};
    tkh::MsReads reads;
    tkh::BmWhitelist wl;
    std::vector<std::string> names;
    uint32_t L = 0, n_wl = 0, n_reads = 0, letters = 0, n_cand = 0;
    uint64_t chunk_reads = 0;
    tk::BmAdapter A{};
    std::vector<tk::BmSeg> segs;                                   // what the device hands back: segments, exact counts, candidates, matches
    std::vector<uint64_t> exact;
    std::vector<uint32_t> cand, res_d, res_n, res_idx;
    Events<3> ev;
    // the whitelist (keys in whitelist order; sorted, with the permutation that says whose they are), its exact counts, the candidates
    TmpBuf d_keys, d_keys_sorted, d_perm, d_exact, d_cand, d_cand_peq;

    BmRun(tksmseq_ctx* c, const tksmseq_barcode_match_params* q, const std::string& a)
        : ctx(c), s(c->stream), p(q), adapter(a), d_keys(s), d_keys_sorted(s), d_perm(s), d_exact(s), d_cand(s), d_cand_peq(s) {}

    // ---- the host reads
    int load(const char* reads_paths, const char* whitelist_path) {
        const auto t0 = std::chrono::steady_clock::now();
        const std::string list = reads_paths;
        if (int rc = tkh::load_fastq_list(list, reads, ctx->err, BM_READ_LIMIT)) {
            if (rc == TKSMSEQ_ELIMIT) ctx->err = "barcode-match: 2^31 reads or more";
            return rc;
        }
        if (!reads.size()) { ctx->err = "barcode-match: no reads in " + list; return TKSMSEQ_EINVAL; }
        std::string text, e;
        if (!tkh::abund_read_file(whitelist_path, text, ctx->err)) return TKSMSEQ_EIO;
        bool limit = false;
        if (!tkh::parse_bm_whitelist(text.data(), text.size(), p->revcomp_barcodes != 0, wl, e, &limit)) {
            ctx->err = limit ? e : std::string(whitelist_path) + ": " + e;
            return limit ? TKSMSEQ_ELIMIT : TKSMSEQ_EINVAL;
        }
        L = wl.L; n_wl = (uint32_t)wl.keys.size(); n_reads = (uint32_t)reads.size();
        if (p->max_errors >= (int32_t)L) { ctx->err = "barcode-match: max_errors must be below the barcodes' length"; return TKSMSEQ_EINVAL; }
        names = reads.names();
        uint64_t longest = 1;
        for (uint32_t r = 0; r < n_reads; r++) longest = std::max<uint64_t>(longest, reads.off[r + 1] - reads.off[r]);
        // the letters of an end that can matter: the window, and a segment that starts at its last letter
        letters = (uint32_t)std::min<uint64_t>((uint64_t)p->window + L + (uint32_t)p->pad, longest);
        info.reads = n_reads; info.whitelist = n_wl;
        info.read_ms = ms_since(t0);
        return TKSMSEQ_OK;
    }

    // ---- the device opened and the chunks sized; the whitelist: keys in whitelist order, and sorted with the permutation that says whose they are
    int sort_whitelist() {
        HIPCHK(ctx, hipSetDevice(ctx->device));
        chunk_reads = p->chunk_reads;
        if (!chunk_reads) {
            size_t free_b = 0, total_b = 0;
            HIPCHK(ctx, hipMemGetInfo(&free_b, &total_b));
            // per read: both ends (3 bits a letter), the segment, and the match's partial and final lists
            const uint64_t per_read = 2 * ((uint64_t)letters * 3 / 8 + 16) + sizeof(tk::BmSeg) + 4 * (2 + tk::BM_LIST) * 4;
            chunk_reads = std::max<uint64_t>(1ull << 16, std::min<uint64_t>(free_b / 4 / per_read, 1ull << 20));
        }
        chunk_reads = std::min<uint64_t>(chunk_reads, BM_CHUNK_MAX);
        if (int rc = ev.create(ctx)) return rc;
        const auto t0 = std::chrono::steady_clock::now();
        HIPCHK(ctx, upload(d_keys, wl.keys, s));
        HIPCHK(ctx, d_keys_sorted.ensure((size_t)n_wl * 8));
        HIPCHK(ctx, d_perm.ensure((size_t)n_wl * 4));
        HIPCHK(ctx, d_exact.ensure((size_t)n_wl * 8));
        HIPCHK(ctx, hipMemsetAsync(d_exact.p, 0, (size_t)n_wl * 8, s));
        HIPCHK(ctx, hipStreamSynchronize(s));
        info.upload_ms += ms_since(t0);
        if (int rc = ev.mark(ctx, 0)) return rc;
        if (int rc = sort_pairs<uint64_t>(ctx, tk::abund_sort_u64, d_keys.as<uint64_t>(), d_keys_sorted.as<uint64_t>(), d_perm.as<uint32_t>(), n_wl, (int)(2 * L))) return rc;
        if (int rc = ev.mark(ctx, 1)) return rc;
        HIPCHK(ctx, hipStreamSynchronize(s));
        if (int rc = ev.add(ctx, 0, info.stage_ms[1])) return rc;

        for (size_t i = 0; i < adapter.size(); i++) A.peq[tkh::bm_code((uint8_t)adapter[i])] |= 1u << i;
        A.m = (uint32_t)adapter.size(); A.window = (uint32_t)p->window; A.max_errors = (uint32_t)p->max_adapter_errors; A.pad = (uint32_t)p->pad; A.L = L;
        return TKSMSEQ_OK;
    }

    // ---- pass 1 over the chunks: the adapter, the segments, the exact counts
    int pass1() {
        segs.resize(n_reads);
        std::vector<uint32_t> h_codes, h_valid, h_len;
        TmpBuf d_codes(s), d_valid(s), d_len(s), d_seg(s);
        for (uint32_t r0 = 0; r0 < n_reads;) {
            const uint32_t r1 = (uint32_t)std::min<uint64_t>(n_reads, (uint64_t)r0 + chunk_reads), n = r1 - r0;
            const auto t0 = std::chrono::steady_clock::now();
            tkh::bm_pack_ends(reads, r0, r1, letters, h_codes, h_valid, h_len);
            HIPCHK(ctx, upload(d_codes, h_codes, s));
            HIPCHK(ctx, upload(d_valid, h_valid, s));
            HIPCHK(ctx, upload(d_len, h_len, s));
            HIPCHK(ctx, d_seg.ensure((size_t)n * sizeof(tk::BmSeg)));
            HIPCHK(ctx, hipStreamSynchronize(s));
            info.upload_ms += ms_since(t0);
            const tk::BmEnds E{d_codes.as<uint32_t>(), d_valid.as<uint32_t>(), d_len.as<uint32_t>(), n};
            if (int rc = ev.mark(ctx, 0)) return rc;
            HIPCHK(ctx, tk::launch_bm_adapter(E, A, d_seg.as<tk::BmSeg>(), s));
            if (int rc = ev.mark(ctx, 1)) return rc;
            HIPCHK(ctx, tk::launch_bm_exact(d_seg.as<tk::BmSeg>(), n, d_keys_sorted.as<uint64_t>(), d_perm.as<uint32_t>(), n_wl, L, (unsigned long long*)d_exact.p, s));
            if (int rc = ev.mark(ctx, 2)) return rc;
            HIPCHK(ctx, download(segs.data() + r0, d_seg, n, s));
            HIPCHK(ctx, hipStreamSynchronize(s));
            for (int k = 0; k < 2; k++) if (int rc = ev.add(ctx, k, info.stage_ms[k])) return rc;
            info.chunks++;
            r0 = r1;
        }
        for (const tk::BmSeg& g : segs) {
            if (!(g.meta & tk::BM_META_ADAPTER)) info.no_adapter++;
            else if (g.meta & tk::BM_META_REV) info.reverse++;
            else info.forward++;
        }
        return TKSMSEQ_OK;
    }

    // ---- the candidates, in whitelist order
    int candidates() {
        exact.resize(n_wl);
        TmpBuf d_flag(s), d_scan(s);
        HIPCHK(ctx, d_flag.ensure(((size_t)n_wl + 1) * 8));
        HIPCHK(ctx, d_scan.ensure(((size_t)n_wl + 1) * 8));
        HIPCHK(ctx, d_cand.ensure((size_t)n_wl * 4));
        HIPCHK(ctx, d_cand_peq.ensure((size_t)n_wl * sizeof(uint4)));
        if (int rc = ev.mark(ctx, 0)) return rc;
        HIPCHK(ctx, tk::launch_bm_cand_flags((const unsigned long long*)d_exact.p, n_wl, (uint64_t)p->min_exact, d_flag.as<uint64_t>(), s));
        if (int rc = scan_u64(ctx, d_flag.as<uint64_t>(), d_scan.as<uint64_t>(), n_wl)) return rc;
        HIPCHK(ctx, tk::launch_bm_cand_write(d_keys.as<uint64_t>(), d_flag.as<uint64_t>(), d_scan.as<uint64_t>(), n_wl, L, d_cand.as<uint32_t>(), d_cand_peq.as<uint4>(), s));
        if (int rc = ev.mark(ctx, 1)) return rc;
        uint64_t nc = 0;
        HIPCHK(ctx, hipMemcpyAsync(&nc, d_scan.as<uint64_t>() + n_wl, 8, hipMemcpyDeviceToHost, s));
        HIPCHK(ctx, hipMemcpyAsync(exact.data(), d_exact.p, (size_t)n_wl * 8, hipMemcpyDeviceToHost, s));
        HIPCHK(ctx, hipStreamSynchronize(s));
        if (int rc = ev.add(ctx, 0, info.stage_ms[1])) return rc;
        if (nc > n_wl) { ctx->err = "barcode-match: more candidates than whitelist lines"; return TKSMSEQ_EDEVICE; }
        HIPCHK(ctx, download(cand, d_cand, (size_t)nc, s));
        HIPCHK(ctx, hipStreamSynchronize(s));
        n_cand = (uint32_t)cand.size();
        info.candidates = n_cand;
        info.pairs = (info.forward + info.reverse) * n_cand;
        return TKSMSEQ_OK;
    }

    // ---- pass 2 over the chunks: every segment against every candidate
    int pass2() {
        res_d.assign(n_reads, (uint32_t)p->max_errors + 1u); res_n.assign(n_reads, 0u); res_idx.assign((size_t)n_reads * tk::BM_LIST, 0xFFFFFFFFu);
        if (!n_cand) return TKSMSEQ_OK;
        TmpBuf d_seg(s), d_pd(s), d_pn(s), d_pi(s), d_rd(s), d_rn(s), d_ri(s);
        for (uint32_t r0 = 0; r0 < n_reads;) {
            const uint32_t r1 = (uint32_t)std::min<uint64_t>(n_reads, (uint64_t)r0 + chunk_reads), n = r1 - r0;
            const uint32_t per_split = tk::bm_split_size(n, n_cand), n_splits = (n_cand + per_split - 1) / per_split;
            const auto t0 = std::chrono::steady_clock::now();
            HIPCHK(ctx, upload(d_seg, segs.data() + r0, n, s));
            HIPCHK(ctx, d_pd.ensure((size_t)n_splits * n * 4));
            HIPCHK(ctx, d_pn.ensure((size_t)n_splits * n * 4));
            HIPCHK(ctx, d_pi.ensure((size_t)n_splits * n * tk::BM_LIST * 4));
            HIPCHK(ctx, d_rd.ensure((size_t)n * 4));
            HIPCHK(ctx, d_rn.ensure((size_t)n * 4));
            HIPCHK(ctx, d_ri.ensure((size_t)n * tk::BM_LIST * 4));
            HIPCHK(ctx, hipStreamSynchronize(s));
            info.upload_ms += ms_since(t0);
            if (int rc = ev.mark(ctx, 0)) return rc;
            HIPCHK(ctx, tk::launch_bm_match(d_seg.as<tk::BmSeg>(), n, d_cand_peq.as<uint4>(), n_cand, per_split, L, (uint32_t)p->max_errors, d_pd.as<uint32_t>(),
                                            d_pn.as<uint32_t>(), d_pi.as<uint32_t>(), s));
            if (int rc = ev.mark(ctx, 1)) return rc;
            HIPCHK(ctx, tk::launch_bm_merge(d_pd.as<uint32_t>(), d_pn.as<uint32_t>(), d_pi.as<uint32_t>(), n, n_splits, (uint32_t)p->max_errors, d_rd.as<uint32_t>(),
                                            d_rn.as<uint32_t>(), d_ri.as<uint32_t>(), s));
            HIPCHK(ctx, download(res_d.data() + r0, d_rd, n, s));
            HIPCHK(ctx, download(res_n.data() + r0, d_rn, n, s));
            HIPCHK(ctx, download(res_idx.data() + (size_t)r0 * tk::BM_LIST, d_ri, (size_t)n * tk::BM_LIST, s));
            if (int rc = ev.mark(ctx, 2)) return rc;
            HIPCHK(ctx, hipStreamSynchronize(s));
            for (int k = 0; k < 2; k++) if (int rc = ev.add(ctx, k, info.stage_ms[2 + k])) return rc;
            r0 = r1;
        }
        return TKSMSEQ_OK;
    }

    // ---- the host writes
    int write(const char* matches_out) {
        const char* segments_out = p->segments_out && *p->segments_out ? p->segments_out : nullptr;
        const char* selected_out = p->selected_out && *p->selected_out ? p->selected_out : nullptr;
        const auto t0 = std::chrono::steady_clock::now();
        std::string matches, segments, selected, piece, e;
        for (uint32_t r = 0; r < n_reads; r++) {
            const tk::BmSeg& g = segs[r];
            if (!(g.meta & tk::BM_META_ADAPTER)) continue;
            const uint32_t da = g.meta >> 16;
            const bool rev = (g.meta & tk::BM_META_REV) != 0;
            if (segments_out) {
                tkh::bm_oriented_slice(reads, r, rev, g.start, g.meta & tk::BM_META_LEN, piece);
                segments += names[r] + '\t' + std::to_string(da) + '\t' + (rev ? '-' : '+') + '\t' + std::to_string(g.start) + '\t' + piece + '\n';
            }
            if (!res_n[r] || res_d[r] > (uint32_t)p->max_errors) { info.no_barcode++; continue; }
            if (res_n[r] == 1) info.unique++; else info.ambiguous++;
            matches += names[r] + '\t' + std::to_string(res_d[r]) + '\t' + std::to_string(res_n[r]) + '\t' + std::to_string(da) + '\t';
            for (uint32_t k = 0; k < std::min<uint32_t>(res_n[r], tk::BM_LIST); k++) {
                const uint32_t c = res_idx[(size_t)r * tk::BM_LIST + k];
                if (c >= n_cand) { ctx->err = "barcode-match: a listed candidate that does not exist"; return TKSMSEQ_EDEVICE; }
                if (k) matches += ',';
                matches += wl.text[cand[c]];
            }
            matches += '\n';
        }
        if (selected_out)
            for (uint32_t c : cand) selected += wl.text[c] + '\t' + std::to_string(exact[c]) + '\n';
        if (!tkh::write_abundance_file(matches_out, matches, e)) { ctx->err = "barcode-match: cannot write " + std::string(matches_out); return TKSMSEQ_EIO; }
        if (segments_out && !tkh::write_abundance_file(segments_out, segments, e)) { ctx->err = "barcode-match: cannot write " + std::string(segments_out); return TKSMSEQ_EIO; }
        if (selected_out && !tkh::write_abundance_file(selected_out, selected, e)) { ctx->err = "barcode-match: cannot write " + std::string(selected_out); return TKSMSEQ_EIO; }
        info.write_ms = ms_since(t0);
        return TKSMSEQ_OK;
    }
};

}  // namespace

extern "C" int tksmseq_barcode_match(tksmseq_ctx* ctx, const tksmseq_barcode_match_params* p, const char* reads_paths, const char* whitelist_path,
                                     const char* matches_out, tksmseq_barcode_match_info* info_out) {
    if (!ctx) return TKSMSEQ_EINVAL;
    if (!p || !reads_paths || !whitelist_path || !matches_out || !*matches_out) { ctx->err = "barcode-match: null argument"; return TKSMSEQ_EINVAL; }
    const std::string adapter = p->adapter && *p->adapter ? p->adapter : BM_DEFAULT_ADAPTER;
    if (int rc = check_params(ctx, p, adapter)) return rc;
    BmRun run(ctx, p, adapter);
    if (int rc = run.load(reads_paths, whitelist_path)) return rc;
    if (int rc = run.sort_whitelist()) return rc;
    if (int rc = run.pass1()) return rc;
    if (int rc = run.candidates()) return rc;
    if (int rc = run.pass2()) return rc;
    run.info.device_ms = run.info.stage_ms[0] + run.info.stage_ms[1] + run.info.stage_ms[2] + run.info.stage_ms[3];
    if (int rc = run.write(matches_out)) return rc;
    if (info_out) *info_out = run.info;
    return TKSMSEQ_OK;
}
