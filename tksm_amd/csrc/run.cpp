// run.cpp -- tksmseq_run: one batch through the kernels of kernels.hip.  RunPlan sizes the run, FastRun is the fast Badread pipeline
// (prepare, init, rounds, finish), close_run turns the per-read results into records.  No CPU fallback exists here.
#include "../../include/tksmseq.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <cstdlib>
#include <string>

#include "ctx.h"

#define TRY(call) do { const int rc_ = (call); if (rc_ != TKSMSEQ_OK) return rc_; } while (0)

static tk::BatchView batch_view(const tksmseq_batch* b) {
    return tk::BatchView{b->reads.as<uint32_t>(), b->intervals.as<uint32_t>(), b->mods.as<uint32_t>(), b->literals.as<uint64_t>(),
                         b->litpool.as<uint8_t>(), b->ids.as<uint32_t>(), b->idpool.as<uint8_t>(), b->n_reads, (uint32_t)b->n_literals};
}
static tk::RefView ref_view(const tksmseq_ctx* ctx) {
    return tk::RefView{ctx->d_packed.as<uint32_t>(), ctx->d_blocktab.as<uint32_t>(), ctx->d_pool.as<uint8_t>(),
                       ctx->d_contigs.as<uint64_t>(), (uint32_t)ctx->contig_names.size()};
}

// Tail noise (py/tksm_badread.py:335-339) lengthens the fragment before the error loop, and everything that is sized or
// ordered by length on the host follows: the lengths are drawn on the device (they depend on the run's seed and read
// indices only), read back, and the batch's lengths, maximum and sorted order are rebuilt for this run.
static int apply_tail(tksmseq_ctx* ctx, tksmseq_batch* b, const tksmseq_run_params* p) {
    const bool want = p->mode == TKSMSEQ_MODE_BADREAD && ctx->tail.enabled && b->n_reads > 0;
    const uint64_t key[4] = {p->seed, p->first_read_index, p->read_index_stride ? p->read_index_stride : 1, ctx->tail_version};
    if (want == b->tail_on && (!want || !memcmp(key, b->tail_key, sizeof(key)))) return TKSMSEQ_OK;
    if (b->splice_len.empty()) b->splice_len = b->raw_len;
    const uint64_t n = b->n_reads;
    if (want) {
        HIPCHK(ctx, b->d_tail.ensure(n * 4 + 16));
        tk::TailView T{(int)ctx->tail.lx.size(), (int)ctx->tail.ly.size(), ctx->tail.ratio, ctx->d_tail_lx.as<double>(),
                       ctx->d_tail_ly.as<double>(), ctx->d_tail_cdf.as<double>()};
        HIPCHK(ctx, tk::launch_tail_lengths(batch_view(b), ref_view(ctx), T, key[0], key[1], key[2], b->d_tail.as<uint32_t>(), ctx->stream));
        std::vector<uint32_t> tl(n);
        HIPCHK(ctx, hipMemcpyAsync(tl.data(), b->d_tail.p, n * 4, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        for (uint64_t r = 0; r < n; r++) {
            const uint64_t t = (uint64_t)b->splice_len[r] + tl[r];
            if (t > 0x7fffff00ull) { ctx->err = "molecule plus tail noise longer than 2^31 bases"; return TKSMSEQ_ELIMIT; }
            b->raw_len[r] = (uint32_t)t;
        }
    } else b->raw_len = b->splice_len;
    b->max_raw = 0;
    for (uint32_t v : b->raw_len) b->max_raw = std::max(b->max_raw, v);
    order_by_length(b->raw_len, b->order);
    HIPCHK(ctx, hipMemcpyAsync(b->d_order.p, b->order.data(), n * 4, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    b->cache_k = -1;                      // the cached scratch size was for the old lengths
    b->tail_on = want;
    memcpy(b->tail_key, key, sizeof(key));
    return TKSMSEQ_OK;
}

// ------------------------------------------------------------------------------------------- what a run needs, computed once
struct RunPlan {
    tksmseq_ctx* ctx; tksmseq_batch* b; const tksmseq_run_params* p;
    int cap_num, cap_den, cap_add;        // output slot of a read: (raw + 2 k) * num / den + add
    int vlevel;                           // TKSMSEQ_VERBOSE as tksmseq_run read it
    std::chrono::steady_clock::time_point t_entry = std::chrono::steady_clock::now();
    uint64_t n = 0;
    bool badread = false, direct = false, fast = false;
    int k = 0, lcap = 0, ncap = 0, s_lcap = 0, s_ncap = 0, wpw = 0, lds = 0, n_wgs = 0, trace_words = 0;
    tk::BatchView B{}; tk::RefView R{}; tk::ErrModelView EM{}; tk::QsModelView QM{}; tk::IdentView IM{}; tk::SimParams P{}; tk::SimBuffers O{};

    uint64_t capf(uint64_t raw) const { return ((raw + 2 * (uint64_t)k) * cap_num / cap_den + cap_add + 15) & ~15ull; }
    void mark(const char* what) const {
        if (vlevel >= 2) fprintf(stderr, "[tksmseq] run: %s at %.3f s\n", what, std::chrono::duration<double>(std::chrono::steady_clock::now() - t_entry).count());
    }

    // LDS geometry from the longest molecule of the batch, and the limits of this build
    int geometry() {
        n = b->n_reads;
        badread = p->mode == TKSMSEQ_MODE_BADREAD;
        k = badread ? ctx->em.k : 0;
        if (b->cache_k != k || b->cache_num != cap_num || b->cache_den != cap_den || b->cache_add != cap_add) {
            uint64_t t = 0;
            for (uint32_t rl : b->raw_len) t += 2 * capf(rl);
            b->cache_scratch = t; b->cache_k = k; b->cache_num = cap_num; b->cache_den = cap_den; b->cache_add = cap_add;
        }
        lcap = (int)((b->max_raw + 2 * k + 7) & ~7u);   // multiple of 8: 64-bit LDS words follow 3 * lcap bytes
        ncap = badread ? (int)capf(b->max_raw) : 4;
        direct = !badread && !ctx->force_slow && !p->collect_stats;   // --perfect: packed reference -> records, no working set
        fast = badread && !ctx->force_slow && n > 0;
        // the wave-wide kernel keeps a read's whole working set in LDS: 3 L + 4 x capacity bytes.  Longer molecules can
        // still take the fast pipeline (fragment state in HBM); only if one of them needs the wave-wide kernel (non-ACGT
        // bytes, an alignment outside the band representation) the run fails with TKSMSEQ_ELIMIT.
        s_lcap = lcap; s_ncap = ncap;
        if (badread && !ctx->force_slow && tk::simulate_lds_bytes(s_lcap, s_ncap, 1) > 160 * 1024) {
            while (s_lcap > 64 && tk::simulate_lds_bytes(s_lcap, (int)capf((uint64_t)(s_lcap - 2 * k)), 1) > 160 * 1024) s_lcap -= 64;
            s_ncap = (int)capf((uint64_t)(s_lcap - 2 * k));
        }
        wpw = tk::WAVES_PER_WG;
        while (wpw > 1 && tk::simulate_lds_bytes(s_lcap, s_ncap, wpw) > 160 * 1024) wpw >>= 1;
        lds = tk::simulate_lds_bytes(s_lcap, s_ncap, wpw);
        // Badread mode: the fast pipeline keeps one joined window (1.5 x the fragment) of a read's last visit in LDS: ~100 kb
        if (!direct && (lds > 160 * 1024 || (badread && !ctx->force_slow ? lcap > 100000 : (ncap >= 65000 || lcap >= 65000)))) {
            ctx->err = "molecule of " + std::to_string(b->max_raw) + " bases exceeds the limit of this build (Badread mode: 100 000 bases)";
            return TKSMSEQ_ELIMIT;
        }
        const int wgs_per_cu = std::min(std::min(32 / wpw, 16), std::max(1, (160 * 1024) / std::max(lds, 1)));
        n_wgs = (int)std::max<uint64_t>(1, std::min<uint64_t>((n + wpw - 1) / wpw, (uint64_t)ctx->n_cus * wgs_per_cu));
        trace_words = (s_ncap + 2) * 4;   // {up mask, left mask} u64 per column of the final alignment
        return TKSMSEQ_OK;
    }
    // the per-read work buffers, and the views of batch, reference, models and buffers that the kernels take
    int buffers() {
        hipStream_t s = ctx->stream;
        HIPCHK(ctx, ctx->w_rawlen.ensure(n * 4 + 16));
        HIPCHK(ctx, ctx->w_slotcap.ensure(n * 8 + 16));
        HIPCHK(ctx, ctx->w_slotoff.ensure((n + 1) * 8 + 16));
        HIPCHK(ctx, ctx->w_outlen.ensure(n * 4 + 16));
        HIPCHK(ctx, ctx->w_ident.ensure(n * 8 + 16));
        HIPCHK(ctx, ctx->w_reclen.ensure(n * 8 + 16));
        HIPCHK(ctx, ctx->w_recoff.ensure((n + 1) * 8 + 16));
        HIPCHK(ctx, ctx->w_status.ensure(n * 4 + 16));
        HIPCHK(ctx, ctx->w_scan.ensure(tk::scan_temp_bytes(n) + 64));
        HIPCHK(ctx, ctx->w_trace.ensure(((size_t)n_wgs * wpw + (size_t)tksmseq_ctx::N_SIDE * tksmseq_ctx::SIDE_WAVES) * trace_words * 4 + 64));
        HIPCHK(ctx, ctx->w_counter.ensure(8192));
        HIPCHK(ctx, ctx->w_sums.ensure(64));
        HIPCHK(ctx, ctx->w_scratch.ensure(b->cache_scratch + 64));
        if (p->collect_stats) {
            HIPCHK(ctx, ctx->w_istats.ensure(n * 64 + 16));
            HIPCHK(ctx, ctx->w_dstats.ensure(n * 16 + 16));
            HIPCHK(ctx, hipMemsetAsync(ctx->w_istats.p, 0, n * 64, s));
            HIPCHK(ctx, hipMemsetAsync(ctx->w_dstats.p, 0, n * 16, s));
        }
        B = batch_view(b);
        R = ref_view(ctx);
        EM = tk::ErrModelView{ctx->em.type, k, ctx->em.max_alts, ctx->em_alt0 ? 1 : 0, ctx->em_uniform ? 1 : 0, ctx->d_cdf.as<uint32_t>(), ctx->d_alts.as<uint64_t>(), ctx->d_nalts.as<uint8_t>(), ctx->d_pself.as<uint2>(), ctx->d_cdf32.as<uint32_t>(), ctx->d_pseg.as<uint4>(), ctx->d_pt0.as<uint32_t>(), ctx->d_pt0b.as<uint4>(), ctx->d_altenc.as<uint4>()};
        QM = tk::QsModelView{ctx->qm.n_slots, ctx->qm.kmer_size, ctx->d_qkeys.as<uint64_t>(), ctx->d_qoff.as<uint32_t>(),
                             ctx->d_qcnt.as<uint32_t>(), ctx->d_qcdf.as<uint32_t>(), ctx->d_qq.as<uint8_t>(), ctx->d_qent.as<uint4>(),
                             ctx->d_qpairs.as<uint2>(), ctx->d_qguide.as<uint8_t>(), ctx->qm.guide_direct ? 1 : 0};
        IM = tk::IdentView{ctx->idm.constant ? 1 : 0, ctx->idm.value, ctx->d_qtab.as<double>()};
        P.seed = p->seed; P.first_read = p->first_read_index; P.stride = p->read_index_stride ? p->read_index_stride : 1;
        P.mode = badread ? 1 : 0; P.fastq = p->fastq ? 1 : 0;
        P.quirk_perfect = (badread && p->perfect_of_badread) ? 1 : 0;
        P.compute_q = (badread && p->compute_qual && p->fastq && !P.quirk_perfect) ? 1 : 0;
#ifdef TKSM_ABLATE
        P.ablate = getenv("TKSMSEQ_ABLATE") ? atoi(getenv("TKSMSEQ_ABLATE")) : 0;     // diagnostic build only (make ablate)
#endif
        P.lcap = lcap; P.ncap = ncap; P.s_lcap = s_lcap; P.s_ncap = s_ncap; P.trace_words = trace_words; P.cap_num = cap_num; P.cap_den = cap_den; P.cap_add = cap_add;
        O.raw_len = ctx->w_rawlen.as<uint32_t>(); O.slot_off = ctx->w_slotoff.as<uint64_t>(); O.scratch = ctx->w_scratch.as<uint8_t>();
        O.out_len = ctx->w_outlen.as<uint32_t>(); O.identity = ctx->w_ident.as<double>(); O.rec_len = ctx->w_reclen.as<uint64_t>();
        O.status = ctx->w_status.as<uint32_t>(); O.trace = ctx->w_trace.as<uint32_t>();
        O.work_counter = ctx->w_counter.as<unsigned long long>();
        O.tail_len = (badread && b->tail_on) ? b->d_tail.as<uint32_t>() : nullptr;
        O.tail_chain = ctx->d_tail_chain.as<tk::TailChain>();
        if (badread) {
            // memory for the unbanded alignments of the wave-wide kernel (rare: kernels.hip, full_align_wave)
            HIPCHK(ctx, ctx->w_fullpool.ensure(ctx->full_pool_bytes));
            O.full_pool = ctx->w_fullpool.as<uint8_t>(); O.full_pool_bytes = ctx->full_pool_bytes;
            O.full_pool_used = ctx->w_counter.as<unsigned long long>() + 1023;      // zeroed with the work counters
        }
        O.istats = p->collect_stats ? ctx->w_istats.as<int32_t>() : nullptr;
        O.dstats = p->collect_stats ? ctx->w_dstats.as<double>() : nullptr;
        O.read_list = nullptr; O.n_work = n;
        return TKSMSEQ_OK;
    }
};

// ------------------------------------------------------------------------------------------- the fast Badread pipeline of one run
// k_init, then rounds of k_loop (a lane per read), k_alnf (a lane per alignment) and k_err (a wave per read: the last visit); the
// exact wave-wide kernel underneath, on side streams, for the reads that cannot take it.
struct FastRun {
    enum Kind { GAP = -1, OTHER = 0, LOOP = 1, ALN = 2, JOB = 3 };   // what ran before a timing tick: host gap; k_init, k_err, exact kernel; k_loop; k_alnf; k_job
    struct Bucket { uint32_t begin, count; int lcap, ncap, wpw; bool hbm; };   // a run of the sorted read order with its own LDS geometry
    static constexpr uint32_t EARLY_CAP = 4096;

    RunPlan& pl;
    tksmseq_ctx* const ctx; tksmseq_batch* const b; const hipStream_t s; const uint64_t n;
    tk::FastBuffers FB{};
    std::vector<uint32_t> r_ncap, r_tg;   // per job-id range: columns of its longest read, 64-byte lines of predecessor codes per job
    uint64_t jcap = 0, tot_trace = 0, tot_popd = 0, nblk = 0;
    size_t nrb = 0, round_bytes = 0, geo_off = 0, geo_bytes = 0;                // layout of h_round / h_geo (ctx.h)
    uint32_t *hprefix = nullptr, *hbase_prev = nullptr, *hbase_cur = nullptr;   // in h_geo, uploaded before every round
    tk::RangeGeo* hrg = nullptr;          // in h_geo: every range's rows in this round's (first half) and the previous round's job set
    uint32_t* cnt = nullptr;              // in h_round: the counters (tk::Counter)
    const uint32_t* hcnt = nullptr;       // in h_round: this round's job counts
    std::vector<Bucket> buckets;
    uint32_t n_side = 0, side_launches = 0;                   // reads handed to / launches of the exact kernel on the side streams
    uint32_t full_rows_fit = 0;           // FB.full_rows before TKSMSEQ_FULL_ROWS_CAP
    bool late_flushed = false, early_on = false, early_active = false, revive = false, revived = false;
    uint32_t n_early = 0, n_rounds = 0, n_deferred = 0;
    uint64_t jobs_all = 0, jobs_14 = 0;                       // alignment jobs launched (diagnostics)
    std::vector<int> kinds;               // Kind of what ran before event i of ctx->evpool

    explicit FastRun(RunPlan& plan) : pl(plan), ctx(plan.ctx), b(plan.b), s(plan.ctx->stream), n(plan.n) {
        for (HelperStream& h : ctx->side) h.used = false;
        ctx->early.used = false;
    }
    // whatever way the run is left (an error return in the middle of the rounds included), no kernel of the side streams may still be
    // running on the context's buffers when the caller reuses or frees them
    ~FastRun() {
        for (HelperStream& h : ctx->side) if (h.used) (void)h.synchronize();
        (void)ctx->early.synchronize();
    }

    // records an event on the main stream, and what ran since the one before it
    int tick(Kind kind) {
        if (!ctx->timing) return TKSMSEQ_OK;
        hipEvent_t e;
        const size_t evi = kinds.size();
        if (evi >= ctx->evpool.size()) { if (hipEventCreate(&e) != hipSuccess) { ctx->err = "event"; return TKSMSEQ_EDEVICE; } ctx->evpool.push_back(e); }
        if (hipEventRecord(ctx->evpool[evi], s) != hipSuccess) { ctx->err = "event"; return TKSMSEQ_EDEVICE; }
        kinds.push_back(kind);
        return TKSMSEQ_OK;
    }
    // sizes of everything that follows from the batch: ranges, state rows, the round's exchange, the full-width pool
    void size_ranges() {
        // job-id ranges: ~256 ranges of rs (multiple of 64) consecutive reads of the sorted order
        FB.rs = (uint32_t)((((n + 255) / 256) + 63) & ~63ull);
        FB.n_ranges = (uint32_t)((n + FB.rs - 1) / FB.rs);
        jcap = (uint64_t)FB.n_ranges * FB.rs;     // job slots (>= n)
        r_ncap.resize(FB.n_ranges); r_tg.resize(FB.n_ranges);
        for (uint32_t c = 0; c < FB.n_ranges; c++) {
            r_ncap[c] = (uint32_t)pl.capf(b->raw_len[b->order[last_pos(c)]]);
            r_tg[c] = ((r_ncap[c] + 31) & ~31u) / 16 + 1;
            tot_trace += (uint64_t)FB.rs * r_tg[c]; tot_popd += (uint64_t)FB.rs * r_ncap[c];
        }
        // ragged per-read state rows: whole 64-position blocks, the padded fragment + at least one spare block
        ctx->h_row64.resize(n + 1);
        for (uint64_t r = 0; r < n; r++) { ctx->h_row64[r] = (uint32_t)nblk; nblk += ((uint64_t)b->raw_len[r] + 2 * pl.k + 63) / 64 + 1; }
        ctx->h_row64[n] = (uint32_t)nblk;
        nrb = (size_t)FB.n_ranges * 128;                                            // bytes of one set of job counts
        round_bytes = 2 * nrb + 1024;
        geo_off = (((size_t)(FB.n_ranges + 1) * 12 + 63) & ~(size_t)63);            // range geometry behind {prefix, base_prev, base_cur}
        geo_bytes = geo_off + (size_t)FB.n_ranges * 2 * sizeof(tk::RangeGeo);
        // pool of full-width rows: as many as a round can ask for, at most 4 GB (homopolymer-rich batches need many)
        // code lines (4 iterations each; whole passes of 16 iterations, some room for drain passes), one uint4 of shift bytes per pass, a spare line
        FB.full_cl = ((((uint32_t)pl.ncap + 31) & ~31u) / 4 + 16 + 3) & ~3u;
        FB.full_tg = FB.full_cl + (FB.full_cl / 4 + 3) / 4 + 1;
        FB.full_rows = (uint32_t)std::max<uint64_t>(64, std::min<uint64_t>(jcap, (4ull << 30) / ((uint64_t)FB.full_tg * 64)) & ~63ull);
        // rounds of at most this many jobs align at full width; the diagnostic cap shrinks the pool behind that choice (never the choice), so
        // that a round can ask for more rows than there are: the waves that find none report their jobs as failures (k_alnf: norow)
        full_rows_fit = FB.full_rows;
        if (ctx->full_rows_cap) FB.full_rows = std::min(FB.full_rows, std::max(64u, ctx->full_rows_cap & ~63u));
        early_on = ctx->early_tail > 0 && ctx->tail_cut == 0 && ctx->tail_wave > 0 && tk::tail_lds_bytes(pl.lcap) <= 65536 && n >= 16ull * ctx->early_tail;
    }
    // the device and page-locked buffers at those sizes, and the kernels' view of them (FB)
    int grow_buffers() {
        if (nblk >= (1ull << 32)) { ctx->err = "batch too large (split it)"; return TKSMSEQ_ELIMIT; }
        HIPCHK(ctx, ctx->f_state.ensure(n * sizeof(tk::ReadState) + 64));
        HIPCHK(ctx, ctx->f_row64.ensure((n + 1) * 4 + 64));
        HIPCHK(ctx, ctx->f_nb.ensure(nblk * 128 + 256));
        HIPCHK(ctx, ctx->f_fplanes.ensure((nblk + 8 * n) * 16 + 256));
        HIPCHK(ctx, ctx->f_frag2.ensure((4 * nblk + 4 * n) * 4 + 1024));
        for (DevBuf& m : ctx->f_jmeta) HIPCHK(ctx, m.ensure(jcap * 16 + 64));
        HIPCHK(ctx, ctx->f_jpopd.ensure(tot_popd + 64));          // (one set: only the meta records and the counts of the previous round are read again)
        HIPCHK(ctx, ctx->f_round.ensure(round_bytes + 64));
        HIPCHK(ctx, ctx->f_geoall.ensure(geo_bytes + 64));
        HIPCHK(ctx, ctx->f_trace.ensure(tot_trace * 64 + 64));                     // predecessor codes of the first alignment pass
        HIPCHK(ctx, ctx->f_redo.ensure(jcap * 4 + 64));
        HIPCHK(ctx, ctx->f_tracefull.ensure((size_t)FB.full_rows * FB.full_tg * 64 + 64));
        HIPCHK(ctx, ctx->f_slow.ensure(n * 4 + 64));
        HIPCHK(ctx, ctx->f_defer.ensure(n * 8 + 64));
        HIPCHK(ctx, ctx->f_defercnt.ensure((size_t)FB.n_ranges * 128 + 64));
        HIPCHK(ctx, ctx->h_round.ensure(round_bytes));
        HIPCHK(ctx, ctx->h_geo.ensure(geo_bytes));
        HIPCHK(ctx, hipMemcpyAsync(ctx->f_row64.p, ctx->h_row64.data(), (n + 1) * 4, hipMemcpyHostToDevice, s));
        FB.state = ctx->f_state.as<tk::ReadState>(); FB.st_nb = ctx->f_nb.as<uint16_t>();
        FB.st_fplanes = ctx->f_fplanes.as<unsigned long long>(); FB.st_frag2 = ctx->f_frag2.as<uint32_t>(); FB.row64 = ctx->f_row64.as<uint32_t>();
        FB.trace = ctx->f_trace.p;
        FB.redo_list = ctx->f_redo.as<uint32_t>();
        FB.trace_full = ctx->f_tracefull.p; FB.counters = reinterpret_cast<uint32_t*>(ctx->f_round.as<uint8_t>() + nrb);
        FB.slow_list = ctx->f_slow.as<uint32_t>();
        // predicted stragglers (launch_early): histogram of the reads' scores, their list, what they hand to the exact kernel
        FB.early_hist = nullptr; FB.early_list = nullptr; FB.early_slow = nullptr;
        if (early_on) {
            HIPCHK(ctx, ctx->f_early.ensure(65536 + (size_t)EARLY_CAP * 12 + 64));
            FB.early_hist = ctx->f_early.as<uint32_t>();
            FB.early_list = reinterpret_cast<uint2*>(ctx->f_early.as<uint8_t>() + 65536);
            FB.early_slow = reinterpret_cast<uint32_t*>(ctx->f_early.as<uint8_t>() + 65536 + (size_t)EARLY_CAP * 8);
            HIPCHK(ctx, hipMemsetAsync(ctx->f_early.p, 0, 65536, s));
        }
        FB.defer_list = ctx->f_defer.as<uint2>(); FB.defer_cnt = ctx->f_defercnt.as<uint32_t>(); FB.defer_len = ctx->defer_len;
        HIPCHK(ctx, hipMemsetAsync(ctx->f_defercnt.p, 0, (size_t)FB.n_ranges * 128, s));
        FB.prefix = ctx->f_geoall.as<uint32_t>(); FB.base_prev = FB.prefix + (FB.n_ranges + 1); FB.base_cur = FB.prefix + 2 * (FB.n_ranges + 1);
        FB.geo_cur = reinterpret_cast<tk::RangeGeo*>(ctx->f_geoall.as<uint8_t>() + geo_off); FB.geo_prev = FB.geo_cur + FB.n_ranges;
        return TKSMSEQ_OK;
    }
    // the job set of a round: meta records double buffered, the job counts on either side of the counters in f_round
    void select_set(uint32_t round) {
        const int z = round & 1, y = z ^ 1;
        FB.job_meta = ctx->f_jmeta[z].as<uint32_t>(); FB.prev_meta = ctx->f_jmeta[y].as<uint32_t>();
        FB.prev_popd = FB.job_popd = ctx->f_jpopd.as<uint8_t>();
        FB.job_cnt = reinterpret_cast<uint32_t*>(ctx->f_round.as<uint8_t>() + (z ? nrb + 1024 : 0));
        hcnt = ctx->h_round.as<uint32_t>() + (z ? (nrb + 1024) / 4 : 0);
    }
    // geometry of every range from hbase_cur (the previous round's moves to the second half), and all of h_geo to the device
    hipError_t place_ranges() {
        uint64_t ot = 0, op = 0;
        for (uint32_t c = 0; c < FB.n_ranges; c++) {
            hrg[FB.n_ranges + c] = hrg[c];
            const uint64_t slots = hbase_cur[c + 1] - hbase_cur[c];
            tk::RangeGeo g{};
            g.trace_off = ot; g.popd_off = op;
            g.tstride = r_tg[c]; g.ncap = r_ncap[c];
            hrg[c] = g;
            ot += slots * g.tstride; op += slots * g.ncap;
        }
        return hipMemcpyAsync(ctx->f_geoall.p, ctx->h_geo.p, geo_bytes, hipMemcpyHostToDevice, s);      // {prefix, bases} go along
    }
    // the next job set: every range gets counts[32 c] slots, rounded up to whole waves and packed (a read has at most one job per round)
    hipError_t pack_ranges(const uint32_t* counts, bool clear_prefix) {
        uint32_t acc = 0;
        for (uint32_t c = 0; c < FB.n_ranges; c++) {
            hbase_prev[c] = hbase_cur[c]; hbase_cur[c] = acc; acc += (counts[(size_t)c * 32] + 63) & ~63u;
            if (clear_prefix) hprefix[c] = 0;
        }
        hbase_prev[FB.n_ranges] = hbase_cur[FB.n_ranges]; hbase_cur[FB.n_ranges] = acc;
        if (clear_prefix) hprefix[FB.n_ranges] = 0;
        return place_ranges();
    }
    // length buckets over the sorted read order: each bucket gets its own LDS geometry
    void make_buckets() {
        const uint32_t minr = b->raw_len[b->order.front()], maxr = b->raw_len[b->order.back()];
        const uint32_t step = std::max<uint32_t>(128, ((maxr - minr) / ctx->n_buckets + 63) & ~63u);
        uint64_t i0 = 0;
        while (i0 < n) {
            const uint32_t lim = (b->raw_len[b->order[i0]] / step + 1) * step;
            uint64_t i1 = i0;
            while (i1 < n && b->raw_len[b->order[i1]] < lim) i1++;
            const uint32_t mx = b->raw_len[b->order[i1 - 1]];
            Bucket bk;
            bk.begin = (uint32_t)i0; bk.count = (uint32_t)(i1 - i0);
            bk.lcap = (int)((mx + 2 * pl.k + 7) & ~7u); bk.ncap = (int)pl.capf(mx);
            bk.hbm = bk.lcap > ctx->hbm_state_len;            // long reads: fragment state edited in HBM (kernels.hip, k_err)
            bk.wpw = tk::WAVES_PER_WG;
            while (bk.wpw > 1 && tk::err_lds_bytes(bk.lcap, bk.ncap, bk.wpw, bk.hbm) > 64 * 1024) bk.wpw >>= 1;
            buckets.push_back(bk);
            i0 = i1;
        }
    }
    int prepare() {
        size_ranges();
        TRY(grow_buffers());
        select_set(0);
        // (h_geo is page-locked: the copy of a round has run by the time the host writes the next round's values -- after that round's
        // synchronisation -- so one buffer is enough)
        HIPCHK(ctx, hipStreamSynchronize(s));                                      // (an earlier run's last copy)
        memset(ctx->h_geo.p, 0, geo_bytes);
        const size_t nr1 = FB.n_ranges + 1;
        hprefix = ctx->h_geo.as<uint32_t>(); hbase_prev = hprefix + nr1; hbase_cur = hprefix + 2 * nr1;
        hrg = reinterpret_cast<tk::RangeGeo*>(ctx->h_geo.as<uint8_t>() + geo_off);
        for (uint32_t c = 0; c <= FB.n_ranges; c++) hbase_cur[c] = hbase_prev[c] = c * FB.rs;
        HIPCHK(ctx, place_ranges());
        cnt = ctx->h_round.as<uint32_t>() + nrb / 4;
        make_buckets();
        // (the state rows -- f_nb, f_frag2, f_fplanes -- are not cleared: k_init writes every read's rows whole)
        HIPCHK(ctx, hipMemsetAsync(ctx->f_round.p, 0, round_bytes, s));
        TRY(tick(GAP));
        pl.mark("buffers ready");
        return TKSMSEQ_OK;
    }
    // reads [n_side, upto) of the slow list to the exact kernel, on the next side stream (ctx.h)
    int launch_side(uint32_t upto) {
        if (upto <= n_side || side_launches + 2 >= 1024) return TKSMSEQ_OK;
        const int k2 = (int)(side_launches % tksmseq_ctx::N_SIDE);
        HelperStream& h = ctx->side[k2];
        tk::SimBuffers O2 = pl.O;
        O2.read_list = ctx->f_slow.as<uint32_t>() + n_side; O2.n_work = upto - n_side;
        O2.work_counter = ctx->w_counter.as<unsigned long long>() + 1 + side_launches;     // zeroed at the start of the run
        O2.trace = pl.O.trace + ((size_t)pl.n_wgs * pl.wpw + (size_t)k2 * tksmseq_ctx::SIDE_WAVES) * pl.trace_words;
        HIPCHK(ctx, h.fork_from(s));
        const uint64_t want = (O2.n_work + pl.wpw - 1) / pl.wpw;
        const int wgs = (int)std::max<uint64_t>(1, std::min<uint64_t>(want, (uint64_t)(tksmseq_ctx::SIDE_WAVES / pl.wpw)));
        HIPCHK(ctx, tk::launch_simulate(pl.B, pl.R, pl.EM, pl.QM, pl.IM, pl.P, O2, wgs, pl.wpw, h.stream));
        HIPCHK(ctx, h.launched());
        n_side = upto; side_launches++;
        return TKSMSEQ_OK;
    }
    // ---- predicted stragglers.  A read's visits are ~ 0.14 x length x (1 - target identity), known after k_init.  In a batch whose
    // distribution of that score has a long tail (skewed lengths), the reads at its end set the number of rounds and the length
    // of the straggler launch: the top early_tail of them -- those that need > 4 x the median read's visits -- get their waves at
    // once, on a stream of their own, and run underneath the regular rounds (which pass them by).
    int launch_early(const std::vector<uint32_t>& copies) {
        uint32_t hist[256] = {};
        for (size_t i = 0; i < copies.size(); i++) hist[i & 255] += copies[i];
        uint64_t total = 0; for (uint32_t v : hist) total += v;
        uint64_t acc = 0; int median_bin = 0;
        for (int bb = 0; bb < 256; bb++) { acc += hist[bb]; if (2 * acc >= total) { median_bin = bb; break; } }
        int min_bin = 256; uint64_t top = 0;
        while (min_bin > median_bin + 16 && top + hist[min_bin - 1] <= ctx->early_tail) { min_bin--; top += hist[min_bin]; }   // 8 bins per factor of two: 16 bins = 4 x
        if (!top) return TKSMSEQ_OK;
        n_early = (uint32_t)top;
        HIPCHK(ctx, tk::launch_mark_early(FB, b->d_order.as<uint32_t>(), n, pl.k, (uint32_t)min_bin, s));
        HIPCHK(ctx, ctx->early.fork_from(s));
        HIPCHK(ctx, tk::launch_tail_early(pl.EM, pl.P, FB, n_early, pl.lcap, ctx->tail_wcap, ctx->early.stream));
        HIPCHK(ctx, ctx->early.launched());
        early_active = true;
        return TKSMSEQ_OK;
    }
    // k_init, the first look at the counters, the first side launch and the predicted stragglers
    int init() {
        const int lcap = pl.lcap;
        HIPCHK(ctx, tk::launch_init(pl.B, pl.R, pl.EM, pl.IM, pl.P, pl.O, FB, lcap * tk::WAVES_PER_WG <= 150 * 1024 ? tk::WAVES_PER_WG : (lcap * 2 <= 150 * 1024 ? 2 : 1), s));
        TRY(tick(OTHER));
        HIPCHK(ctx, hipMemcpyAsync(cnt, FB.counters, 64, hipMemcpyDeviceToHost, s));
        std::vector<uint32_t> early_copies(early_on ? 64 * 256 : 0);
        if (early_on) HIPCHK(ctx, hipMemcpyAsync(early_copies.data(), FB.early_hist, early_copies.size() * 4, hipMemcpyDeviceToHost, s));
        HIPCHK(ctx, hipStreamSynchronize(s));
        pl.mark("fragments spliced (k_init)");
        // reads with non-ACGT bytes are known after k_init: their wave-wide kernel (latency-bound, a few waves) starts now on a side
        // stream and runs underneath the rounds ... and so does the kernel of every read that leaves the fast pipeline later (an alignment
        // the band representation cannot hold: about one read in two million): launched as soon as the host sees it (flush_side)
        TRY(launch_side(cnt[tk::CNT_SLOW]));
        if (early_on) TRY(launch_early(early_copies));
        return TKSMSEQ_OK;
    }
    // every read's error loop has ended.  With q-scores: one more alignment job per read, the whole new sequence against the whole
    // fragment (k_qjobs + k_job, then k_alnf); without: their output, in this one round
    int launch_revive() {
        if (pl.P.compute_q) HIPCHK(ctx, tk::launch_qjobs(FB, pl.k, n_deferred, s));
        else {
            const Bucket& bk = buckets.back();
            HIPCHK(ctx, tk::launch_err(pl.B, pl.EM, pl.QM, pl.P, pl.O, FB, b->d_order.as<uint32_t>(), 0, n_deferred, bk.lcap, bk.ncap, 2, 0, FB.n_ranges, bk.wpw, bk.hbm, s));
        }
        revive = false;
        return TKSMSEQ_OK;
    }
    // last visits: q-score lookups and output, one wave per q-score job; ranges are chunks of the sorted order, so a bucket is a run of ranges
    uint32_t last_pos(uint32_t c) const { return (uint32_t)std::min<uint64_t>((uint64_t)(c + 1) * FB.rs, n) - 1; }   // of range c in the sorted order
    int launch_last_visits() {
        size_t bi = 0;
        for (uint32_t c = 0, c1; c < FB.n_ranges; c = c1) {
            while (bi + 1 < buckets.size() && last_pos(c) >= buckets[bi].begin + buckets[bi].count) bi++;
            const Bucket& bk = buckets[bi];
            for (c1 = c + 1; c1 < FB.n_ranges && last_pos(c1) < bk.begin + bk.count; c1++) {}
            const uint32_t cntw = hprefix[c1] - hprefix[c];
            if (cntw) HIPCHK(ctx, tk::launch_err(pl.B, pl.EM, pl.QM, pl.P, pl.O, FB, b->d_order.as<uint32_t>(), 0, cntw, bk.lcap, bk.ncap, 1, c, c1, bk.wpw, bk.hbm, s));
        }
        return TKSMSEQ_OK;
    }
    // the error loops of all reads that are still running, one lane each (round 0: every read, in sorted order; later: the reads of
    // the previous round's jobs), then this round's jobs packed for k_alnf, one lane each
    int launch_loops() {
        const uint32_t* order = b->d_order.as<uint32_t>();
        const uint32_t left = hprefix[FB.n_ranges];
        const int lcap = pl.lcap;
        // waves of the straggler kernel the device holds at once (its LDS per wave grows with the longest fragment of the batch): it
        // takes over when every read that is left gets a wave of its own at once
        const uint64_t tail_slots = (uint64_t)ctx->n_cus * std::min<uint64_t>(16, (160u * 1024u) / tk::tail_lds_bytes(lcap));
        if (n_rounds == 0) HIPCHK(ctx, tk::launch_loop(pl.EM, pl.P, FB, order, 0, (uint32_t)n, lcap, 0, 0, 0, s));
        else if (left <= std::min<uint64_t>(ctx->tail_wave, tail_slots) && tk::tail_lds_bytes(lcap) <= 65536)    // the stragglers: every remaining visit in this launch
            HIPCHK(ctx, tk::launch_tail(pl.EM, pl.P, FB, order, 0, left, lcap, 1, 0, FB.n_ranges, ctx->tail_wcap, s));
        else if (left <= ctx->wave_loop && lcap <= 32768)        // few reads left: a wave each (latency)
            HIPCHK(ctx, tk::launch_loopw(pl.EM, pl.P, FB, order, 0, left, lcap, 1, 0, FB.n_ranges, s));
        else HIPCHK(ctx, tk::launch_loop(pl.EM, pl.P, FB, order, 0, left, lcap, 1, 0, FB.n_ranges, s));
        return tick(LOOP);
    }
    // counters + job counts of the round to the host; the prefix sums of the counts are the next round's list of reads
    int exchange() {
        HIPCHK(ctx, hipMemcpyAsync(ctx->h_round.p, ctx->f_round.p, round_bytes, hipMemcpyDeviceToHost, s));
        HIPCHK(ctx, hipStreamSynchronize(s));
        uint32_t jobs = 0;
        for (uint32_t c = 0; c < FB.n_ranges; c++) { hprefix[c] = jobs; jobs += hcnt[(size_t)c * 32]; }
        hprefix[FB.n_ranges] = cnt[tk::CNT_JOBS] = jobs;
        return TKSMSEQ_OK;
    }
    // reads that left the fast pipeline in this round: a launch of the wave-wide kernel costs the latency of its slowest read
    // (25-45 ms), so they are collected while the rounds are busy and flushed in batches (128 at a time, once more when the rounds
    // become latency-bound; what comes after that waits for the end) -- and only onto a side stream that has finished its previous
    // launch, unless a lot is waiting: many small launches in a row on one stream each cost the full latency
    int flush_side() {
        const bool late = cnt[tk::CNT_JOBS] * 16ull < n;
        const uint32_t pending = cnt[tk::CNT_SLOW] - n_side;
        const bool stream_idle = ctx->side[side_launches % tksmseq_ctx::N_SIDE].idle();
        if ((pending >= 128 && (stream_idle || pending >= 2048)) || (pending && late && !late_flushed)) TRY(launch_side(cnt[tk::CNT_SLOW]));
        late_flushed = late_flushed || late;
        return TKSMSEQ_OK;
    }
    // the regular rounds are over: wait for the early reads' kernel, take over what it left for the exact kernel, and look at the
    // counters again (deferred reads, slow list)
    int join_early() {
        if (!early_active) return TKSMSEQ_OK;
        HIPCHK(ctx, ctx->early.wait_done());
        HIPCHK(ctx, tk::launch_merge_early_slow(FB, s));
        HIPCHK(ctx, hipMemcpyAsync(cnt, FB.counters, 64, hipMemcpyDeviceToHost, s));
        HIPCHK(ctx, hipStreamSynchronize(s));
        cnt[tk::CNT_JOBS] = 0;
        early_active = false;
        return TKSMSEQ_OK;
    }
    // this round's alignment jobs: few of them with all 64 rows stored at once, many with 14 rows and a second pass over those that need more
    int align(bool qround) {
        const uint32_t jobs = cnt[tk::CNT_JOBS];
        const uint32_t n_jobs = hbase_cur[FB.n_ranges - 1] + ((hcnt[(size_t)(FB.n_ranges - 1) * 32] + 63) & ~63u);
        const bool full_only = jobs <= std::min(ctx->small_aln, full_rows_fit);
        jobs_all += jobs; if (!full_only) jobs_14 += jobs;
        HIPCHK(ctx, tk::launch_alnf(pl.P, FB, pl.O, n_jobs, full_only, qround ? 1 : 0, s));
        return tick(ALN);
    }
    // One round: the visits of the reads that are still running (regular rounds; once they are over, the deferred reads' q-score jobs
    // and last visits), the exchange with the host, the round's alignments, the next round's job set
    int rounds() {
        for (;; n_rounds++) {
            select_set(n_rounds);
            HIPCHK(ctx, tk::launch_round_reset(FB, s));                  // this round's job counts, the alignment passes' counters
            TRY(tick(GAP));
            const bool qround = revive && pl.P.compute_q;              // this round's jobs are the q-score alignments
            const bool regular = !revive && !revived;
            TRY(revive ? launch_revive() : revived ? launch_last_visits() : launch_loops());
            TRY(tick(regular ? JOB : OTHER));
            TRY(exchange());
            TRY(flush_side());
            if (cnt[tk::CNT_JOBS] == 0) {
                TRY(join_early());
                if (cnt[tk::CNT_DEFERRED] == 0 || revived) break;
                // every other read is done: job slots for the deferred reads (per-range counts), then their rounds
                revived = revive = true; n_deferred = cnt[tk::CNT_DEFERRED];
                std::vector<uint32_t> hd((size_t)FB.n_ranges * 32);
                HIPCHK(ctx, hipMemcpy(hd.data(), ctx->f_defercnt.p, hd.size() * 4, hipMemcpyDeviceToHost));
                HIPCHK(ctx, pack_ranges(hd.data(), true));
                continue;
            }
#ifdef TKSM_ABLATE
            if (pl.P.ablate >= 1 && pl.P.ablate <= 9) break;          // k_err returned early: the reads would never finish
#endif
            if (cnt[tk::CNT_JOBS] < ctx->tail_cut && cnt[tk::CNT_JOBS] * 64ull < n) {
                // tail: every further round costs a full alignment latency for a handful of reads; finish the
                // stragglers in one launch of the wave-wide kernel instead (same results: it recomputes them)
                HIPCHK(ctx, tk::launch_collect_unfinished(FB, n, s));
                HIPCHK(ctx, hipMemcpyAsync(cnt, FB.counters, 64, hipMemcpyDeviceToHost, s));
                HIPCHK(ctx, hipStreamSynchronize(s));
                break;
            }
            if (n_rounds > 100000) { ctx->err = "internal: error loop did not terminate"; return TKSMSEQ_EDEVICE; }
            TRY(tick(GAP));
            TRY(align(qround));
            HIPCHK(ctx, pack_ranges(hcnt, false));
        }
        pl.mark("rounds done");
        return TKSMSEQ_OK;
    }
    // diagnostics, the verbose texts, the side streams joined, the exact kernel for what is still on the slow list, the timing sums
    int finish(float ms[3]) {
        // (the counters came down with the last round's copy; nothing that counts has run since)
        uint32_t* d = ctx->last_diag;
        memset(d, 0, sizeof(ctx->last_diag));
        d[DIAG_ROUNDS] = n_rounds; d[DIAG_EXACT_KERNEL_READS] = cnt[tk::CNT_SLOW]; d[DIAG_PREDICTED_STRAGGLERS] = n_early;
        d[DIAG_JOBS_14_ROW_ROUNDS] = (uint32_t)std::min<uint64_t>(jobs_14, 0xffffffffu); d[DIAG_JOBS_REDONE_FULL_WIDTH] = cnt[tk::CNT_REDO_JOBS];
        d[DIAG_FALLBACKS] = cnt[tk::CNT_FAIL]; d[DIAG_FALLBACK_REASONS] = cnt[tk::CNT_FAIL_OR]; d[DIAG_FALLBACKS_QSCORE_JOBS] = cnt[tk::CNT_FAIL_QJOB];
        d[DIAG_FALLBACKS_LIST_PASS] = cnt[tk::CNT_FAIL_LIST]; d[DIAG_JOBS_ALL_ROUNDS] = (uint32_t)std::min<uint64_t>(jobs_all, 0xffffffffu);
        d[DIAG_BAND_EXITS] = cnt[tk::CNT_EXIT + tk::EXIT_BAND_LOOP] + cnt[tk::CNT_EXIT + tk::EXIT_BAND_ERR];
        if (pl.vlevel) {
            uint32_t cc[tk::CNT_WORDS];
            HIPCHK(ctx, hipMemcpy(cc, FB.counters, sizeof(cc), hipMemcpyDeviceToHost));
            const uint32_t *ex = cc + tk::CNT_EXIT, *why = cc + tk::CNT_FAIL_REASON;
            fprintf(stderr, "[tksmseq] this thread so far: %u device allocations, %.3f s in hipMalloc\n", alloc_calls(), alloc_seconds());
            fprintf(stderr, "[tksmseq] reads %llu rounds %u slow-path reads %u (band exit %u/%u, shift %u/%u), full-width redo: %u jobs in %u waves; predicted stragglers on their own stream: %u\n",
                    (unsigned long long)n, n_rounds, cnt[tk::CNT_SLOW], ex[tk::EXIT_BAND_LOOP], ex[tk::EXIT_BAND_ERR], ex[tk::EXIT_SHIFT_LOOP], ex[tk::EXIT_SHIFT_ERR], cc[tk::CNT_REDO_JOBS], cc[tk::CNT_REDO_WAVES], n_early);
            fprintf(stderr, "[tksmseq] fused alignment failures: %u, reasons or-ed 0x%x, last 0x%x (n %u, m %u)\n", cc[tk::CNT_FAIL], cc[tk::CNT_FAIL_OR], cc[tk::CNT_FAIL_LAST], cc[tk::CNT_FAIL_NM] & 0xffffu, cc[tk::CNT_FAIL_NM] >> 16);
            fprintf(stderr, "[tksmseq]   per reason: queue / reservoir overflow %u no pool rows %u - shift>31 %u shift>14 %u end cell %u walk %u | q-score jobs %u, list pass %u\n", why[tk::FAIL_QUEUE], why[tk::FAIL_NOROW], why[tk::FAIL_SHIFT31], why[tk::FAIL_SHIFT14], why[tk::FAIL_END_CELL], why[tk::FAIL_WALK], cc[tk::CNT_FAIL_QJOB], cc[tk::CNT_FAIL_LIST]);
        }
        for (HelperStream& h : ctx->side) if (h.used) HIPCHK(ctx, h.join_into(s));
        if (cnt[tk::CNT_SLOW] > n_side) {
            // reads that left the fast pipeline later (alignment outside the band representation, tail cut): byte-exact wave-wide path
            pl.O.read_list = ctx->f_slow.as<uint32_t>() + n_side; pl.O.n_work = cnt[tk::CNT_SLOW] - n_side;
            const uint64_t want = (pl.O.n_work + pl.wpw - 1) / pl.wpw;
            TRY(tick(GAP));
            HIPCHK(ctx, tk::launch_simulate(pl.B, pl.R, pl.EM, pl.QM, pl.IM, pl.P, pl.O, (int)std::max<uint64_t>(1, std::min<uint64_t>(want, (uint64_t)pl.n_wgs)), pl.wpw, s));
            TRY(tick(OTHER));
        }
        if (ctx->timing) {
            HIPCHK(ctx, hipStreamSynchronize(s));
            for (size_t i = 1; i < kinds.size(); i++) {
                float t = 0; (void)hipEventElapsedTime(&t, ctx->evpool[i - 1], ctx->evpool[i]);
                if (kinds[i] >= LOOP) ms[kinds[i] - LOOP] += t;
            }
        }
        return TKSMSEQ_OK;
    }
};

// ------------------------------------------------------------------------------------------- from per-read results to records
// molecules that need the exact wave-wide kernel (a non-ACGT byte, an alignment outside the band representation) and are longer
// than its LDS-resident working set: the same kernel with the working sets in HBM
static int rerun_in_hbm(const RunPlan& pl, const std::vector<uint32_t>& st) {
    tksmseq_ctx* ctx = pl.ctx;
    hipStream_t s = ctx->stream;
    std::vector<uint32_t> big;
    for (uint64_t i = 0; i < pl.n; i++) if (st[i] & 8) big.push_back((uint32_t)i);
    const int n_waves = (int)std::min<size_t>(big.size(), 64);
    const size_t per_wave = tk::simulate_big_bytes(pl.lcap, pl.ncap);
    HIPCHK(ctx, ctx->w_biglist.ensure(big.size() * 4 + 16));
    HIPCHK(ctx, ctx->w_bigscratch.ensure(per_wave * n_waves + 64));
    HIPCHK(ctx, ctx->w_bigtrace.ensure((size_t)n_waves * 2 * (pl.ncap + 2) * 8 + 64));
    HIPCHK(ctx, hipMemcpyAsync(ctx->w_biglist.p, big.data(), big.size() * 4, hipMemcpyHostToDevice, s));
    HIPCHK(ctx, hipMemsetAsync(ctx->w_counter.p, 0, 8, s));
    tk::SimBuffers O3 = pl.O;
    O3.read_list = ctx->w_biglist.as<uint32_t>(); O3.n_work = big.size();
    O3.work_counter = ctx->w_counter.as<unsigned long long>();
    O3.big_scratch = ctx->w_bigscratch.as<uint8_t>(); O3.big_per_wave = per_wave; O3.big_trace = ctx->w_bigtrace.as<unsigned long long>();
    HIPCHK(ctx, tk::launch_simulate_big(pl.B, pl.R, pl.EM, pl.QM, pl.IM, pl.P, O3, n_waves, s));
    if (pl.vlevel) fprintf(stderr, "[tksmseq] %zu molecules beyond the LDS-resident limit took the exact kernel with HBM working sets\n", big.size());
    return TKSMSEQ_OK;
}

// some read has status bits set: an error of the run, output slots that were too small (*overflow), or -- in the first pass --
// molecules for rerun_in_hbm, after which the sums and record offsets are taken once more (*again)
static int check_status(const RunPlan& pl, int pass, bool* again, bool* overflow) {
    tksmseq_ctx* ctx = pl.ctx;
    const uint64_t n = pl.n;
    std::vector<uint32_t> st(n);
    HIPCHK(ctx, hipMemcpy(st.data(), ctx->w_status.p, n * 4, hipMemcpyDeviceToHost));
    uint32_t any = 0; uint64_t first = 0;
    for (uint64_t i = 0; i < n; i++) if (st[i]) { if (!any) first = i; any |= st[i]; }
    if ((any & 16) && pl.vlevel) {
        std::string l;
        int shown = 0;
        for (uint64_t i = 0; i < n && shown < 16; i++) if (st[i] & 16) { l += " " + std::to_string(i); shown++; }
        fprintf(stderr, "[tksmseq] reads with an unbanded alignment (first %d):%s\n", shown, l.c_str());
    }
    if (any & 2) { ctx->err = "modification position outside its interval at read " + std::to_string(first); return TKSMSEQ_EINVAL; }
    if (any & 4) { ctx->err = "out of memory for the unbanded alignment fallback at read " + std::to_string(first) + " (TKSMSEQ_FULL_POOL_MB)"; return TKSMSEQ_ENOMEM; }
    if ((any & 8) && pass == 0 && pl.badread) { *again = true; return rerun_in_hbm(pl, st); }
    if (any & 8) {
        uint64_t f8 = 0;
        for (uint64_t i = 0; i < n; i++) if (st[i] & 8) { f8 = i; break; }
        ctx->err = "read " + std::to_string(f8) + " (" + std::to_string(pl.b->raw_len[f8]) + " bases) exceeds the limits of the exact wave-wide kernel";
        return TKSMSEQ_ELIMIT;
    }
    if (any & 1) *overflow = true;
    return TKSMSEQ_OK;
}

// record offsets and sums, the status pass, the output buffer, the records (k_perfect / k_emit), the event times
static int close_run(const RunPlan& pl, const float ms[3], tksmseq_result* res, bool* overflow) {
    tksmseq_ctx* ctx = pl.ctx;
    hipStream_t s = ctx->stream;
    const uint64_t n = pl.n;
    const bool T = ctx->timing;
    unsigned long long* sums = ctx->w_sums.as<unsigned long long>();
    unsigned long long hs[2] = {0, 0}; uint64_t total = 0;
    for (int pass = 0;; pass++) {
        HIPCHK(ctx, tk::launch_scan(ctx->w_reclen.as<uint64_t>(), ctx->w_recoff.as<uint64_t>(), n, ctx->w_scan.p, ctx->w_scan.cap, s));
        HIPCHK(ctx, tk::launch_sum_u32(ctx->w_status.as<uint32_t>(), n, sums, s));
        HIPCHK(ctx, tk::launch_sum_u32(ctx->w_outlen.as<uint32_t>(), n, sums + 1, s));
        if (T && pass == 0) HIPCHK(ctx, hipEventRecord(ctx->ev[3], s));
        HIPCHK(ctx, hipMemcpyAsync(hs, sums, 16, hipMemcpyDeviceToHost, s));
        HIPCHK(ctx, hipMemcpyAsync(&total, ctx->w_recoff.as<uint64_t>() + n, 8, hipMemcpyDeviceToHost, s));
        HIPCHK(ctx, hipStreamSynchronize(s));
        if (!hs[0]) break;
        bool again = false;
        TRY(check_status(pl, pass, &again, overflow));
        if (*overflow) return TKSMSEQ_OK;
        if (!again) break;
    }
    uint8_t* records;
    if (ctx->user_out) {
        if (total > ctx->user_out_cap) { ctx->err = "caller-provided output buffer too small: need " + std::to_string(total) + " bytes"; return TKSMSEQ_ENOMEM; }
        records = (uint8_t*)ctx->user_out;
    } else {
        HIPCHK(ctx, ctx->w_records.ensure(total + 64));
        records = ctx->w_records.as<uint8_t>();
    }
    if (pl.direct) HIPCHK(ctx, tk::launch_perfect(pl.B, pl.R, pl.P, pl.O, ctx->w_recoff.as<uint64_t>(), records, pl.b->max_raw, ctx->n_cus, s));
    else HIPCHK(ctx, tk::launch_emit(pl.B, pl.P, pl.O, ctx->w_recoff.as<uint64_t>(), records, s));
    if (T) {
        HIPCHK(ctx, hipEventRecord(ctx->ev[4], s));
        HIPCHK(ctx, hipEventSynchronize(ctx->ev[4]));
        for (int i = 0; i < 4; i++) (void)hipEventElapsedTime(&res->kernel_ms[i], ctx->ev[i], ctx->ev[i + 1]);
        (void)hipEventElapsedTime(&res->kernel_ms[4], ctx->ev[0], ctx->ev[4]);
        for (int i = 0; i < 3; i++) res->kernel_ms[5 + i] = ms[i];             // k_loop, k_alnf, k_job
    }
    res->records = records; res->record_offsets = ctx->w_recoff.p; res->records_bytes = total; res->n_reads = n;
    res->bases_in = pl.b->total_raw; res->bases_out = hs[1];
    return TKSMSEQ_OK;
}

static int run_once(tksmseq_ctx* ctx, tksmseq_batch* b, const tksmseq_run_params* p, int cap_num, int cap_den, int cap_add, int vlevel,
                    tksmseq_result* res, bool* overflow) {
    *overflow = false;
    RunPlan pl{ctx, b, p, cap_num, cap_den, cap_add, vlevel};
    TRY(pl.geometry());
    TRY(pl.buffers());
    hipStream_t s = ctx->stream;
    const bool T = ctx->timing;
    float ms[3] = {0, 0, 0};
    if (T) HIPCHK(ctx, hipEventRecord(ctx->ev[0], s));
    HIPCHK(ctx, hipMemsetAsync(ctx->w_counter.p, 0, 8192, s));
    HIPCHK(ctx, tk::launch_read_lengths(pl.B, pl.R, pl.k, cap_num, cap_den, cap_add, pl.O.tail_len, ctx->w_rawlen.as<uint32_t>(), ctx->w_slotcap.as<uint64_t>(),
                                        ctx->w_status.as<uint32_t>(), s));
    HIPCHK(ctx, tk::launch_scan(ctx->w_slotcap.as<uint64_t>(), ctx->w_slotoff.as<uint64_t>(), pl.n, ctx->w_scan.p, ctx->w_scan.cap, s));
    if (T) HIPCHK(ctx, hipEventRecord(ctx->ev[1], s));
    if (pl.direct) HIPCHK(ctx, tk::launch_perfect_lengths(pl.B, pl.R, pl.P, pl.O, s));
    else if (!pl.fast) HIPCHK(ctx, tk::launch_simulate(pl.B, pl.R, pl.EM, pl.QM, pl.IM, pl.P, pl.O, pl.n_wgs, pl.wpw, s));
    else {
        FastRun fr(pl);
        TRY(fr.prepare());
        TRY(fr.init());
        TRY(fr.rounds());
        TRY(fr.finish(ms));
    }
    if (T) HIPCHK(ctx, hipEventRecord(ctx->ev[2], s));
    return close_run(pl, ms, res, overflow);
}

extern "C" {

int tksmseq_run(tksmseq_ctx* ctx, const tksmseq_batch* batch, const tksmseq_run_params* p, tksmseq_result* result) {
    if (!ctx || !batch || !p || !result) return TKSMSEQ_EINVAL;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    memset(result, 0, sizeof(*result));
    if (p->mode != TKSMSEQ_MODE_PERFECT && p->mode != TKSMSEQ_MODE_BADREAD) { ctx->err = "unknown mode"; return TKSMSEQ_EINVAL; }
    if (p->mode == TKSMSEQ_MODE_BADREAD) {
        if (ctx->em.type < 0) { ctx->err = "no error model loaded"; return TKSMSEQ_ESTATE; }
        if (!ctx->idm.set) { ctx->err = "identity distribution not set"; return TKSMSEQ_ESTATE; }
        if (p->compute_qual && p->fastq && ctx->qm.n_slots == 0) { ctx->err = "no q-score model loaded"; return TKSMSEQ_ESTATE; }
    }
    if (ctx->n_declared) { ctx->err = "the reference holds contigs declared without bases (tksmseq_reference_declare_contig): there is nothing to sequence from"; return TKSMSEQ_ESTATE; }
    tksmseq_batch* b = const_cast<tksmseq_batch*>(batch);
    bool overflow = false;
    memset(ctx->last_diag, 0, sizeof(ctx->last_diag));
    int rc = apply_tail(ctx, b, p);
    if (rc != TKSMSEQ_OK) return rc;
    const int vlevel = verbose_level();           // TKSMSEQ_VERBOSE, read once per run
    rc = run_once(ctx, b, p, 3, 2, 64, vlevel, result, &overflow);
    if (rc == TKSMSEQ_OK && overflow) {
        // insertion-heavy reads outgrew the default 1.5x slot: rerun with the worst-case factor
        rc = run_once(ctx, b, p, 6, 1, 64, vlevel, result, &overflow);
        if (rc == TKSMSEQ_OK && overflow) { ctx->err = "internal: output slot overflow at the worst-case factor"; rc = TKSMSEQ_EDEVICE; }
    }
    if (rc == TKSMSEQ_OK) { ctx->last = *result; ctx->have_last = true; ctx->have_stats = p->collect_stats != 0; ctx->last_fastq = p->fastq != 0; }
    return rc;
}

int tksmseq_run_diagnostics(tksmseq_ctx* ctx, uint32_t* out) {
    if (!ctx || !out) return TKSMSEQ_EINVAL;
    if (!ctx->have_last) return TKSMSEQ_ESTATE;
    memcpy(out, ctx->last_diag, sizeof(ctx->last_diag));
    return TKSMSEQ_OK;
}

}  // extern "C"
