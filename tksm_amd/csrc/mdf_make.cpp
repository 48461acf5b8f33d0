// mdf_make.cpp -- host side of the transforms that are sources: no input batch, the molecules are made on the device
//   tksmseq_wgs            src/random_wgs.cpp:181-207 (fragments of the whole genome)
//   tksmseq_transcribe     src/transcribe.cpp:170-197 (abundance rows x the context's transcript table), with its plan functions
// Both know their totals before they allocate (OutBatch::place_known, mdf_batch.h): their scans are their own (rank and cut; per row).
#include <atomic>
#include <charconv>
#include <cmath>
#include <cstring>

#include "mdf_batch.h"

// ---- random-wgs ------------------------------------------------------------------------------------------------------------------
// the contig table as the kernels read it: running sums of the lengths, and the names (for the ids) in one pool
static int wgs_table(tksmseq_ctx* ctx) {
    if (ctx->wgs_version == ctx->ref_version && ctx->d_wgs_sofar.p) return TKSMSEQ_OK;
    const size_t nc = ctx->contig_names.size();
    std::vector<uint64_t> so_far(nc);
    std::vector<uint32_t> noff(nc), nlen(nc);
    std::string pool;
    uint64_t acc = 0;
    for (size_t i = 0; i < nc; i++) {
        acc += ctx->contigs[2 * i + 1];
        so_far[i] = acc; noff[i] = (uint32_t)pool.size(); nlen[i] = (uint32_t)ctx->contig_names[i].size();
        pool += ctx->contig_names[i];
        if (pool.size() >= 0xffffffffull) { ctx->err = "random-wgs: more than 4 GB of contig names"; return TKSMSEQ_ELIMIT; }
    }
    int rc;
    if ((rc = upload(ctx, ctx->d_wgs_sofar, so_far.data(), nc * 8)) || (rc = upload(ctx, ctx->d_wgs_nameoff, noff.data(), nc * 4)) ||
        (rc = upload(ctx, ctx->d_wgs_namelen, nlen.data(), nc * 4)) || (rc = upload(ctx, ctx->d_wgs_names, pool.data(), pool.size()))) return rc;
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    ctx->wgs_version = ctx->ref_version;
    return TKSMSEQ_OK;
}

// validate_arguments (src/random_wgs.cpp:118-125), plus what std:: leaves undefined, and the limits of one call
static int wgs_check(tksmseq_ctx* ctx, const tksmseq_wgs_params* p) {
    if (p->dist < TKSMSEQ_WGS_NORMAL || p->dist > TKSMSEQ_WGS_EXPONENTIAL) { ctx->err = "Invalid fragment length distribution"; return TKSMSEQ_EINVAL; }
    if (!std::isfinite(p->a) || !std::isfinite(p->b) || !(p->a > 0.0) || p->b < 0.0 || (p->dist == TKSMSEQ_WGS_UNIFORM && p->b < p->a)) {
        ctx->err = "Invalid fragment length distribution parameters"; return TKSMSEQ_EINVAL;
    }
    const size_t nc = ctx->contig_names.size();
    if (!nc || !ctx->total_bases) { ctx->err = "random-wgs: the reference has no contigs (or none with a base)"; return TKSMSEQ_ESTATE; }
    for (size_t i = 0; i < nc; i++)
        if (ctx->contigs[2 * i + 1] >= 0x80000000ull) { ctx->err = "random-wgs: contig " + ctx->contig_names[i] + " has 2^31 bases or more"; return TKSMSEQ_ELIMIT; }
    if (p->n_candidates > (1ull << 28)) { ctx->err = "random-wgs: more than 2^28 candidates in one call (split the range)"; return TKSMSEQ_ELIMIT; }
    return TKSMSEQ_OK;
}

// the temporaries of one call: the candidates' plan, the emitted ones ranked, their bases summed, their id bytes sized and scanned, the cut
struct WgsBufs {
    TmpBuf plan, flag, bases, rank, bsum, idlen, idoff, cut;
    explicit WgsBufs(hipStream_t s) : plan(s), flag(s), bases(s), rank(s), bsum(s), idlen(s), idoff(s), cut(s) {}
};

// plan, rank and cut nn > 0 candidates; h = cut[4] {molecules, bases, candidates consumed, reached}, then the totals rank[nn], bsum[nn], idoff[nn].
// Returns with the stream drained.
static int wgs_plan_cut(tksmseq_ctx* ctx, const tksmseq_wgs_params* p, uint64_t nn, WgsBufs& d, uint64_t h[8]) {
    hipStream_t s = ctx->stream;
    HIPCHK(ctx, d.plan.ensure(nn * 16 + 16));
    for (DevBuf* b : {(DevBuf*)&d.flag, (DevBuf*)&d.bases, (DevBuf*)&d.idlen}) HIPCHK(ctx, b->ensure(nn * 8 + 16));
    for (DevBuf* b : {(DevBuf*)&d.rank, (DevBuf*)&d.bsum, (DevBuf*)&d.idoff}) HIPCHK(ctx, b->ensure((nn + 1) * 8 + 16));
    HIPCHK(ctx, d.cut.ensure(64));
    HIPCHK(ctx, ctx->w_scan.ensure(tk::scan_temp_bytes(nn) + 64));
    HIPCHK(ctx, hipMemsetAsync(d.cut.p, 0, 64, s));
    const tk::WgsParams W{p->seed, p->dist, p->a, p->b, ctx->total_bases, (uint32_t)ctx->contig_names.size()};
    HIPCHK(ctx, tk::launch_wgs_plan(W, ctx->d_wgs_sofar.as<uint64_t>(), p->first_candidate, nn, d.plan.as<uint4>(), d.flag.as<uint64_t>(), d.bases.as<uint64_t>(), s));
    HIPCHK(ctx, tk::launch_scan(d.flag.as<uint64_t>(), d.rank.as<uint64_t>(), nn, ctx->w_scan.p, ctx->w_scan.cap, s));
    HIPCHK(ctx, tk::launch_scan(d.bases.as<uint64_t>(), d.bsum.as<uint64_t>(), nn, ctx->w_scan.p, ctx->w_scan.cap, s));
    HIPCHK(ctx, tk::launch_wgs_cut(nn, d.plan.as<uint4>(), d.rank.as<uint64_t>(), d.bsum.as<uint64_t>(), ctx->d_wgs_namelen.as<uint32_t>(), p->molecules_before,
                                   p->bases_before, (uint64_t)p->base_count, d.idlen.as<uint64_t>(), d.cut.as<uint64_t>(), s));
    HIPCHK(ctx, tk::launch_scan(d.idlen.as<uint64_t>(), d.idoff.as<uint64_t>(), nn, ctx->w_scan.p, ctx->w_scan.cap, s));
    HIPCHK(ctx, hipMemcpyAsync(h, d.cut.p, 32, hipMemcpyDeviceToHost, s));
    HIPCHK(ctx, hipMemcpyAsync(h + 4, d.rank.as<uint64_t>() + nn, 8, hipMemcpyDeviceToHost, s));
    HIPCHK(ctx, hipMemcpyAsync(h + 5, d.bsum.as<uint64_t>() + nn, 8, hipMemcpyDeviceToHost, s));
    HIPCHK(ctx, hipMemcpyAsync(h + 6, d.idoff.as<uint64_t>() + nn, 8, hipMemcpyDeviceToHost, s));
    HIPCHK(ctx, hipStreamSynchronize(s));
    return TKSMSEQ_OK;
}

extern "C" {

int tksmseq_wgs(tksmseq_ctx* ctx, const tksmseq_wgs_params* p, tksmseq_batch** out, tksmseq_wgs_progress* progress) {
    if (!ctx || !p || !out || !progress) return TKSMSEQ_EINVAL;
    *out = nullptr;
    memset(progress, 0, sizeof *progress);
    int rc = wgs_check(ctx, p);
    if (rc) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    if ((rc = wgs_table(ctx))) return rc;
    progress->next_candidate = p->first_candidate; progress->molecules = p->molecules_before; progress->bases = p->bases_before;
    const bool owed = p->base_count > 0 && p->bases_before < (uint64_t)p->base_count;
    progress->reached = owed ? 0 : 1;
    const uint64_t nn = owed ? p->n_candidates : 0;                     // (nothing owed: an empty batch, no candidate taken)
    WgsBufs d(s);
    uint64_t h[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (nn && (rc = wgs_plan_cut(ctx, p, nn, d, h))) return rc;
    const bool reached = h[3] != 0;
    const uint64_t n_mol = reached ? h[0] : h[4], n_bases = reached ? h[1] : h[5];
    // one segment per molecule, no substitutions, no literals
    OutBatch b(ctx);
    if ((rc = b.place_known(n_mol, n_mol, 0, h[6], "random-wgs: ", "fewer candidates per call")) || (rc = b.literals(nullptr))) return rc;
    if (n_mol)
        HIPCHK(ctx, tk::launch_wgs_write(nn, d.plan.as<uint4>(), d.rank.as<uint64_t>(), d.idlen.as<uint64_t>(), d.idoff.as<uint64_t>(), ctx->d_wgs_nameoff.as<uint32_t>(),
                                         ctx->d_wgs_namelen.as<uint32_t>(), ctx->d_wgs_names.as<uint8_t>(), p->molecules_before, b.tables(), s));
    if ((rc = b.finish(out))) return rc;
    if (nn) {
        progress->next_candidate = p->first_candidate + (reached ? h[2] : nn);
        progress->molecules = p->molecules_before + n_mol; progress->bases = p->bases_before + n_bases;
        progress->reached = reached ? 1 : 0;
    }
    return TKSMSEQ_OK;
}

}  // extern "C"

// ---- transcribe ------------------------------------------------------------------------------------------------------------------
// One abundance table joined with the context's transcript table: the rows on the host (shared by the plans cloned from one another),
// per-row counts and their scans on the device of the plan's context.
struct TsbShared {
    std::shared_ptr<const tsb::Transcripts> tx;
    tsb::Abundance ab;
    std::string prefix;
    uint64_t seed = 0, first_row = 0;
    double weight = 1.0, molecule_count = 0.0;
    // host copies of the device scans ([rows + 1]) and the emitted rows in order (a row's position here is its molecule index)
    std::vector<uint64_t> mol_first, ivl_first, id_first;
    std::vector<uint32_t> emitted;
};
struct tksmseq_tsb_plan {
    tksmseq_ctx* ctx = nullptr;
    std::shared_ptr<TsbShared> sh;
    DevBuf d_tx, d_rank, d_mol_first, d_ivl_first, d_id_first, d_prefix;
};

// the transcript table as k_tsb_write reads it, with contigs resolved against this context's reference
static int tsb_table(tksmseq_ctx* ctx) {
    if (!ctx->tsb) { ctx->err = "transcribe: no GTF has been added (tksmseq_transcripts_add_gtf)"; return TKSMSEQ_ESTATE; }
    const tsb::Transcripts& T = *ctx->tsb;
    if (ctx->tsb_dev_serial == T.serial && ctx->tsb_ref_version == ctx->ref_version) return TKSMSEQ_OK;
    std::vector<uint32_t> contig(T.contig_names.size());
    std::vector<uint64_t> lits;
    std::string pool;
    for (size_t i = 0; i < contig.size(); i++) {
        const int ci = ctx->find(T.contig_names[i]);
        if (ci >= 0) { contig[i] = (uint32_t)ci; continue; }
        contig[i] = 0x80000000u | (uint32_t)(lits.size() / 2);          // a literal: what the MDF parser makes of an unknown name
        lits.push_back(pool.size()); lits.push_back(T.contig_names[i].size());
        pool += T.contig_names[i];
    }
    const uint64_t E = T.n_exons();
    std::vector<uint32_t> ex(4 * E);
    for (uint64_t e = 0; e < E; e++) { ex[4 * e] = contig[T.ex_contig[e]]; ex[4 * e + 1] = T.ex_start[e]; ex[4 * e + 2] = T.ex_end[e]; ex[4 * e + 3] = (uint32_t)T.ex_minus[e] << 31; }
    hipStream_t s = ctx->stream;
    HIPCHK(ctx, hipStreamSynchronize(s));                               // (nothing queued may still read the table that goes)
    int rc;
    if ((rc = upload(ctx, ctx->d_tsb_first, T.exon_first.data(), T.exon_first.size() * 4)) || (rc = upload(ctx, ctx->d_tsb_exons, ex.data(), E * 16)) ||
        (rc = upload(ctx, ctx->d_tsb_lits, lits.data(), lits.size() * 8)) || (rc = upload(ctx, ctx->d_tsb_litpool, pool.data(), pool.size()))) return rc;
    HIPCHK(ctx, hipStreamSynchronize(s));
    ctx->tsb_n_lits = lits.size() / 2; ctx->tsb_lit_bytes = pool.size();
    ctx->tsb_dev_serial = T.serial; ctx->tsb_ref_version = ctx->ref_version;
    return TKSMSEQ_OK;
}

// counts and scans of plan p on its context; fills the shared host copies when they are not there yet
static int tsb_plan_device(tksmseq_tsb_plan* p) {
    tksmseq_ctx* ctx = p->ctx;
    TsbShared& S = *p->sh;
    const uint64_t R = S.ab.rows();
    HIPCHK(ctx, hipSetDevice(ctx->device));
    int rc = tsb_table(ctx);
    if (rc) return rc;
    hipStream_t s = ctx->stream;
    TmpBuf d_tpm(s), d_depth(s), d_flag(s), d_nivl(s), d_idb(s);
    HIPCHK(ctx, p->d_tx.ensure(R * 4 + 16)); HIPCHK(ctx, p->d_prefix.ensure(S.prefix.size() + 16));
    for (DevBuf* b : {&p->d_rank, &p->d_mol_first, &p->d_ivl_first, &p->d_id_first}) { HIPCHK(ctx, b->ensure((R + 1) * 8 + 16)); HIPCHK(ctx, hipMemsetAsync(b->p, 0, 8, s)); }
    if (!S.prefix.empty()) HIPCHK(ctx, hipMemcpyAsync(p->d_prefix.p, S.prefix.data(), S.prefix.size(), hipMemcpyHostToDevice, s));
    if (R) {
        HIPCHK(ctx, d_tpm.ensure(R * 8 + 16));
        for (DevBuf* b : {&d_depth, &d_flag, &d_nivl, &d_idb}) HIPCHK(ctx, b->ensure(R * 8 + 16));
        HIPCHK(ctx, ctx->w_scan.ensure(tk::scan_temp_bytes(R) + 64));
        HIPCHK(ctx, hipMemcpyAsync(p->d_tx.p, S.ab.tx.data(), R * 4, hipMemcpyHostToDevice, s));
        HIPCHK(ctx, hipMemcpyAsync(d_tpm.p, S.ab.tpm.data(), R * 8, hipMemcpyHostToDevice, s));
        const tk::TsbCount C{S.seed, S.first_row, S.weight, S.molecule_count, S.ab.sum_tpm};
        if (ctx->timing) HIPCHK(ctx, hipEventRecord(ctx->ev[0], s));
        HIPCHK(ctx, tk::launch_tsb_count(R, C, p->d_tx.as<uint32_t>(), d_tpm.as<double>(), d_depth.as<uint64_t>(), d_flag.as<uint64_t>(), s));
        HIPCHK(ctx, tk::launch_scan(d_flag.as<uint64_t>(), p->d_rank.as<uint64_t>(), R, ctx->w_scan.p, ctx->w_scan.cap, s));
        HIPCHK(ctx, tk::launch_tsb_size(R, p->d_tx.as<uint32_t>(), ctx->d_tsb_first.as<uint32_t>(), d_depth.as<uint64_t>(), p->d_rank.as<uint64_t>(), (uint32_t)S.prefix.size(),
                                        d_nivl.as<uint64_t>(), d_idb.as<uint64_t>(), s));
        HIPCHK(ctx, tk::launch_scan(d_depth.as<uint64_t>(), p->d_mol_first.as<uint64_t>(), R, ctx->w_scan.p, ctx->w_scan.cap, s));
        HIPCHK(ctx, tk::launch_scan(d_nivl.as<uint64_t>(), p->d_ivl_first.as<uint64_t>(), R, ctx->w_scan.p, ctx->w_scan.cap, s));
        HIPCHK(ctx, tk::launch_scan(d_idb.as<uint64_t>(), p->d_id_first.as<uint64_t>(), R, ctx->w_scan.p, ctx->w_scan.cap, s));
        if (ctx->timing) HIPCHK(ctx, hipEventRecord(ctx->ev[1], s));
    }
    if (S.mol_first.empty()) {
        S.mol_first.assign(R + 1, 0); S.ivl_first.assign(R + 1, 0); S.id_first.assign(R + 1, 0);
        HIPCHK(ctx, hipMemcpyAsync(S.mol_first.data(), p->d_mol_first.p, (R + 1) * 8, hipMemcpyDeviceToHost, s));
        HIPCHK(ctx, hipMemcpyAsync(S.ivl_first.data(), p->d_ivl_first.p, (R + 1) * 8, hipMemcpyDeviceToHost, s));
        HIPCHK(ctx, hipMemcpyAsync(S.id_first.data(), p->d_id_first.p, (R + 1) * 8, hipMemcpyDeviceToHost, s));
        HIPCHK(ctx, hipStreamSynchronize(s));
        for (uint64_t r = 0; r < R; r++) if (S.mol_first[r + 1] > S.mol_first[r]) S.emitted.push_back((uint32_t)r);
    } else HIPCHK(ctx, hipStreamSynchronize(s));
    ctx->tsb_plan_ms = 0.f;
    if (ctx->timing && R) HIPCHK(ctx, hipEventElapsedTime(&ctx->tsb_plan_ms, ctx->ev[0], ctx->ev[1]));
    return TKSMSEQ_OK;
}

static int ndig_host(uint64_t v) { int d = 1; while (v >= 10) { v /= 10; d++; } return d; }

// the row that molecule m (below the plan's total) of the unrolled run belongs to
static uint64_t tsb_owner(const TsbShared& S, uint64_t m) { return (uint64_t)(std::upper_bound(S.mol_first.begin(), S.mol_first.end(), m) - S.mol_first.begin()) - 1; }

// where molecule m's intervals and id bytes start in the whole run's
static void tsb_bases(const TsbShared& S, uint64_t m, uint64_t& ivl, uint64_t& idb) {
    const uint64_t R = S.ab.rows();
    if (m >= S.mol_first.back()) { ivl = S.ivl_first[R]; idb = S.id_first[R]; return; }
    const uint64_t r = tsb_owner(S, m), copy = m - S.mol_first[r];
    const uint32_t t = S.ab.tx[r];
    const uint64_t exons = S.tx->exon_first[t + 1] - S.tx->exon_first[t];
    const uint64_t id_len = S.prefix.size() + (uint64_t)ndig_host((uint64_t)(std::lower_bound(S.emitted.begin(), S.emitted.end(), (uint32_t)r) - S.emitted.begin()));
    ivl = S.ivl_first[r] + copy * exons; idb = S.id_first[r] + copy * id_len;
}

// the comments of molecules [m0, m1), m0 < m1: the copies of a row share one, so the work is per row touched, and one (offset, length) pair
// per molecule
static int tsb_comments(tksmseq_ctx* ctx, const TsbShared& S, uint64_t m0, uint64_t m1, tksmseq_batch* b) {
    const tsb::Transcripts& T = *S.tx;
    b->h_comments.reserve(2 * (m1 - m0));
    std::string c;
    for (uint64_t r = tsb_owner(S, m0), m = m0; m < m1; r++) {
        const uint64_t end = std::min(S.mol_first[r + 1], m1);
        if (end <= m) continue;
        const uint32_t t = S.ab.tx[r];
        c.clear();
        tsb::append_comment(c, S.ab.text.data() + S.ab.cb_off[r], S.ab.cb_len[r], T.id_pool.data() + T.id_off[t], T.id_len[t]);
        uint32_t off = 0;
        const int rc = comment_bytes(ctx, b, c.data(), c.size(), "transcribe", "fewer molecules per call", &off);
        if (rc) return rc;
        for (; m < end; m++) { b->h_comments.push_back(off); b->h_comments.push_back((uint32_t)c.size()); }
    }
    return TKSMSEQ_OK;
}

extern "C" {

int tksmseq_transcripts_add_gtf(tksmseq_ctx* ctx, const char* path, int skip_non_coding) {
    if (!ctx || !path) return TKSMSEQ_EINVAL;
    static std::atomic<uint64_t> serial{0};
    auto next = std::make_shared<tsb::Transcripts>(ctx->tsb ? *ctx->tsb : tsb::Transcripts());      // (plans and clones keep the table they have)
    bool io = false;
    if (!tsb::read_gtf(path, skip_non_coding != 0, *next, ctx->err, io)) return io ? TKSMSEQ_EIO : TKSMSEQ_EINVAL;
    next->serial = ++serial;
    ctx->tsb = std::move(next);
    return TKSMSEQ_OK;
}
int tksmseq_transcripts_info(const tksmseq_ctx* ctx, uint64_t* n_transcripts, uint64_t* n_exons) {
    if (!ctx) return TKSMSEQ_EINVAL;
    if (n_transcripts) *n_transcripts = ctx->tsb ? ctx->tsb->n() : 0;
    if (n_exons) *n_exons = ctx->tsb ? ctx->tsb->n_exons() : 0;
    return TKSMSEQ_OK;
}
int tksmseq_transcripts_clear(tksmseq_ctx* ctx) {
    if (!ctx) return TKSMSEQ_EINVAL;
    ctx->tsb.reset(); ctx->tsb_dev_serial = 0;
    return TKSMSEQ_OK;
}

int tksmseq_transcribe_plan_create(tksmseq_ctx* ctx, const char* abundance_path, const char* text, uint64_t len, const tksmseq_tsb_params* p, tksmseq_tsb_plan** out) {
    if (!ctx || !p || !out || (!abundance_path && !text && len)) return TKSMSEQ_EINVAL;
    *out = nullptr;
    if (!ctx->tsb) { ctx->err = "transcribe: no GTF has been added (tksmseq_transcripts_add_gtf)"; return TKSMSEQ_ESTATE; }
    if (!std::isfinite(p->weight)) { ctx->err = "transcribe: the weight of an abundance file must be finite"; return TKSMSEQ_EINVAL; }
    std::string file;
    if (abundance_path) {
        FILE* f = fopen(abundance_path, "rb");
        if (!f) { ctx->err = std::string("Could not open abundance file ") + abundance_path + "!"; return TKSMSEQ_EIO; }
        char buf[1 << 16];
        size_t n;
        while ((n = fread(buf, 1, sizeof buf, f)) > 0) file.append(buf, n);
        fclose(f);
        text = file.data(); len = file.size();
    }
    std::unique_ptr<tksmseq_tsb_plan> plan(new tksmseq_tsb_plan());
    plan->ctx = ctx;
    plan->sh = std::make_shared<TsbShared>();
    TsbShared& S = *plan->sh;
    S.tx = ctx->tsb;
    if (!tsb::parse_abundance(text, len, p->use_whole_id != 0, *S.tx, S.ab, ctx->err)) return TKSMSEQ_ELIMIT;
    S.prefix = p->prefix ? p->prefix : "M";
    if (S.prefix.size() > 4096) { ctx->err = "transcribe: a molecule prefix of more than 4096 bytes"; return TKSMSEQ_ELIMIT; }
    S.seed = p->seed; S.first_row = p->first_row_index; S.weight = p->weight; S.molecule_count = (double)p->molecule_count;
    const int rc = tsb_plan_device(plan.get());
    if (rc) return rc;
    *out = plan.release();
    return TKSMSEQ_OK;
}
int tksmseq_transcribe_plan_clone(tksmseq_ctx* ctx, const tksmseq_tsb_plan* src, tksmseq_tsb_plan** out) {
    if (!ctx || !src || !out) return TKSMSEQ_EINVAL;
    *out = nullptr;
    if (ctx->tsb != src->sh->tx) { ctx->err = "transcribe: the context does not hold the transcript table the plan was made with"; return TKSMSEQ_ESTATE; }
    std::unique_ptr<tksmseq_tsb_plan> plan(new tksmseq_tsb_plan());
    plan->ctx = ctx; plan->sh = src->sh;
    const int rc = tsb_plan_device(plan.get());
    if (rc) return rc;
    *out = plan.release();
    return TKSMSEQ_OK;
}
int tksmseq_transcribe_plan_info(const tksmseq_tsb_plan* plan, uint64_t* rows, uint64_t* records, uint64_t* molecules, uint64_t* missing) {
    if (!plan) return TKSMSEQ_EINVAL;
    const TsbShared& S = *plan->sh;
    if (rows) *rows = S.ab.rows();
    if (records) *records = S.emitted.size();
    if (molecules) *molecules = S.mol_first.back();
    if (missing) *missing = S.ab.missing_off.size();
    return TKSMSEQ_OK;
}
int tksmseq_transcribe_plan_missing(const tksmseq_tsb_plan* plan, uint64_t i, const char** id, uint64_t* len) {
    if (!plan || !id || !len || i >= plan->sh->ab.missing_off.size()) return TKSMSEQ_EINVAL;
    const tsb::Abundance& A = plan->sh->ab;
    *id = A.missing_off[i] == 0xffffffffu ? "BEG" : A.text.data() + A.missing_off[i];
    *len = A.missing_len[i];
    return TKSMSEQ_OK;
}
void tksmseq_transcribe_plan_free(tksmseq_tsb_plan* plan) {
    if (!plan) return;
    if (plan->ctx) { (void)hipSetDevice(plan->ctx->device); (void)hipStreamSynchronize(plan->ctx->stream); }
    delete plan;
}

int tksmseq_transcribe(tksmseq_ctx* ctx, const tksmseq_tsb_plan* plan, uint64_t first_molecule, uint64_t n_molecules, int32_t flags, tksmseq_batch** out) {
    if (!ctx || !plan || !out) return TKSMSEQ_EINVAL;
    *out = nullptr;
    if (n_molecules > (1ull << 28)) { ctx->err = "transcribe: more than 2^28 molecules in one call (split the range)"; return TKSMSEQ_ELIMIT; }
    const TsbShared& S = *plan->sh;
    if (plan->ctx != ctx) { ctx->err = "transcribe: the plan belongs to another context (tksmseq_transcribe_plan_clone makes one for this context)"; return TKSMSEQ_ESTATE; }
    if (ctx->tsb != S.tx) { ctx->err = "transcribe: the transcript table has changed since the plan was made"; return TKSMSEQ_ESTATE; }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    int rc = tsb_table(ctx);                                            // (the reference may have changed: contigs are resolved again)
    if (rc) return rc;
    hipStream_t s = ctx->stream;
    const uint64_t R = S.ab.rows(), total = S.mol_first.back();
    const uint64_t m0 = std::min(first_molecule, total), n = std::min(n_molecules, total - m0), m1 = m0 + n;
    uint64_t ivl0 = 0, id0 = 0, ivl1 = 0, id1 = 0;
    if (n) { tsb_bases(S, m0, ivl0, id0); tsb_bases(S, m1, ivl1, id1); }
    OutBatch b(ctx);
    if ((rc = b.place_known(n, ivl1 - ivl0, 0, id1 - id0, "transcribe: ", "fewer molecules per call")) || (rc = b.literals(nullptr, ctx->tsb_n_lits, ctx->tsb_lit_bytes))) return rc;
    if (ctx->tsb_n_lits) HIPCHK(ctx, hipMemcpyAsync(b->literals.p, ctx->d_tsb_lits.p, ctx->tsb_n_lits * 16, hipMemcpyDeviceToDevice, s));
    if (ctx->tsb_lit_bytes) HIPCHK(ctx, hipMemcpyAsync(b->litpool.p, ctx->d_tsb_litpool.p, ctx->tsb_lit_bytes, hipMemcpyDeviceToDevice, s));
    HIPCHK(ctx, b->d_dup.ensure(n * 4 + 16));
    if (n) {
        const tk::TsbPlanView V{R, plan->d_tx.as<uint32_t>(), plan->d_mol_first.as<uint64_t>(), plan->d_rank.as<uint64_t>(), plan->d_ivl_first.as<uint64_t>(),
                                plan->d_id_first.as<uint64_t>(), ctx->d_tsb_first.as<uint32_t>(), ctx->d_tsb_exons.as<uint4>(), plan->d_prefix.as<uint8_t>(), (uint32_t)S.prefix.size()};
        if (ctx->timing) HIPCHK(ctx, hipEventRecord(ctx->ev[0], s));
        HIPCHK(ctx, tk::launch_tsb_write(V, m0, n, ivl0, ivl1 - ivl0, id0, b.tables(), b->d_dup.as<uint32_t>(), s));
        if (ctx->timing) HIPCHK(ctx, hipEventRecord(ctx->ev[1], s));
        b->h_dup.resize(n);
        HIPCHK(ctx, hipMemcpyAsync(b->h_dup.data(), b->d_dup.p, n * 4, hipMemcpyDeviceToHost, s));
    }
    if (!(flags & TKSMSEQ_MOL_NO_COMMENTS) && n && (rc = tsb_comments(ctx, S, m0, m1, b.get()))) return rc;
    if ((rc = b.finish(out))) return rc;
    ctx->tsb_write_ms = 0.f;
    if (ctx->timing && n) HIPCHK(ctx, hipEventElapsedTime(&ctx->tsb_write_ms, ctx->ev[0], ctx->ev[1]));
    return TKSMSEQ_OK;
}

int tksmseq_transcribe_device_ms(const tksmseq_ctx* ctx, float* plan_ms, float* write_ms) {
    if (!ctx) return TKSMSEQ_EINVAL;
    if (plan_ms) *plan_ms = ctx->tsb_plan_ms;
    if (write_ms) *write_ms = ctx->tsb_write_ms;
    return TKSMSEQ_OK;
}

int tksmseq_transcribe_text(const tksmseq_tsb_plan* plan, uint64_t first_record, uint64_t n_records, char** text, uint64_t* len) {
    if (!plan || !text || !len) return TKSMSEQ_EINVAL;
    *text = nullptr; *len = 0;
    const TsbShared& S = *plan->sh;
    const tsb::Transcripts& T = *S.tx;
    const uint64_t k0 = std::min<uint64_t>(first_record, S.emitted.size()), k1 = k0 + std::min<uint64_t>(n_records, S.emitted.size() - k0);
    std::string o;
    char num[24];
    auto put = [&](uint64_t v) { auto r = std::to_chars(num, num + sizeof num, v); o.append(num, r.ptr); };
    for (uint64_t k = k0; k < k1; k++) {
        const uint32_t r = S.emitted[k], t = S.ab.tx[r];
        o += '+'; o += S.prefix; put(k); o += '\t'; put(S.mol_first[r + 1] - S.mol_first[r]); o += '\t';
        tsb::append_comment(o, S.ab.text.data() + S.ab.cb_off[r], S.ab.cb_len[r], T.id_pool.data() + T.id_off[t], T.id_len[t]);
        o += '\n';
        for (uint32_t e = T.exon_first[t]; e < T.exon_first[t + 1]; e++) {
            o += T.contig_names[T.ex_contig[e]]; o += '\t'; put(T.ex_start[e]); o += '\t'; put(T.ex_end[e]); o += T.ex_minus[e] ? "\t-\t\n" : "\t+\t\n";
        }
    }
    char* buf = (char*)malloc(o.size() + 1);
    if (!buf) return TKSMSEQ_ENOMEM;
    memcpy(buf, o.data(), o.size()); buf[o.size()] = 0;
    *text = buf; *len = o.size();
    return TKSMSEQ_OK;
}

}  // extern "C"
