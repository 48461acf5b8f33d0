// api.cpp -- implementation of the C-ABI in include/tksmseq.h: contexts, reference, models, batches and results (the run itself: run.cpp).
// No CPU fallback exists here: every compute call launches the kernels of kernels.hip.
#include "../../include/tksmseq.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <cstdlib>
#include <memory>
#include <string>

#include "ctx.h"
#include "loop_filter.h"

static thread_local std::string g_create_error;
void set_contextless_error(const std::string& e) { g_create_error = e; }


template <class T>
static int upload(tksmseq_ctx* ctx, DevBuf& b, const std::vector<T>& v) {
    HIPCHK(ctx, b.ensure(v.size() * sizeof(T) + 16));
    if (!v.empty()) HIPCHK(ctx, hipMemcpyAsync(b.p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return TKSMSEQ_OK;
}

extern "C" {

const char* tksmseq_version(void) { return "tksm-amd seq 0.1 (gfx950)"; }

int tksmseq_create(int device, tksmseq_ctx** out) {
    if (!out) return TKSMSEQ_EINVAL;
    *out = nullptr;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) { g_create_error = "no HIP device available (this library has no CPU fallback)"; return TKSMSEQ_EDEVICE; }
    if (device < 0 || device >= n) { g_create_error = "device index out of range"; return TKSMSEQ_EINVAL; }
    e = hipSetDevice(device);
    if (e != hipSuccess) { g_create_error = hipGetErrorString(e); return TKSMSEQ_EDEVICE; }
    std::unique_ptr<tksmseq_ctx> c(new tksmseq_ctx());
    c->device = device;
    if (const char* fs = getenv("TKSMSEQ_FORCE_SLOW")) c->force_slow = fs[0] == '1';
    if (const char* tc = getenv("TKSMSEQ_TAIL_CUT")) c->tail_cut = (uint32_t)atoi(tc);
    if (const char* tc = getenv("TKSMSEQ_SMALL_ALN")) c->small_aln = (uint32_t)atoi(tc);
    if (const char* fr = getenv("TKSMSEQ_FULL_ROWS_CAP")) c->full_rows_cap = (uint32_t)std::max(0, atoi(fr));
    if (const char* tc = getenv("TKSMSEQ_WAVE_LOOP")) c->wave_loop = (uint32_t)atoi(tc);
    if (const char* tc = getenv("TKSMSEQ_TAIL_WAVE")) c->tail_wave = (uint32_t)atoi(tc);
    if (const char* tc = getenv("TKSMSEQ_TAIL_WCAP")) c->tail_wcap = atoi(tc);
    if (const char* tc = getenv("TKSMSEQ_EARLY_TAIL")) c->early_tail = (uint32_t)std::min(4096, std::max(0, atoi(tc)));
    if (const char* hl = getenv("TKSMSEQ_HBM_STATE_LEN")) c->hbm_state_len = atoi(hl);
    if (const char* dl = getenv("TKSMSEQ_DEFER_LEN")) c->defer_len = atoi(dl);
    if (const char* fp = getenv("TKSMSEQ_FULL_POOL_MB")) c->full_pool_bytes = (unsigned long long)atoll(fp) << 20;
    if (const char* nbk = getenv("TKSMSEQ_BUCKETS")) c->n_buckets = (uint32_t)std::max(1, atoi(nbk));
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess) c->n_cus = prop.multiProcessorCount;
    e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
    if (e != hipSuccess) { g_create_error = hipGetErrorString(e); return TKSMSEQ_EDEVICE; }
    c->own_stream = true;
    for (auto& ev : c->ev) (void)hipEventCreate(&ev);
    *out = c.release();
    DevCache::get().context_created();
    return TKSMSEQ_OK;
}

int tksmseq_clone(const tksmseq_ctx* src, tksmseq_ctx** out) {
    if (!src || !out) return TKSMSEQ_EINVAL;
    int rc = tksmseq_create(src->device, out);
    if (rc != TKSMSEQ_OK) return rc;
    tksmseq_ctx* c = *out;
    c->contig_names = src->contig_names; c->contig_index = src->contig_index; c->contigs = src->contigs;
    c->total_alloc = src->total_alloc; c->total_bases = src->total_bases; c->pool_blocks = src->pool_blocks;
    c->contig_declared = src->contig_declared; c->n_declared = src->n_declared;
    c->tsb = src->tsb;                                       // (the transcript table of transcribe: immutable, shared)
    c->d_packed.borrow(src->d_packed); c->d_blocktab.borrow(src->d_blocktab); c->d_pool.borrow(src->d_pool); c->d_contigs.borrow(src->d_contigs);
    c->em = src->em; c->qm = src->qm; c->idm = src->idm; c->em_uniform = src->em_uniform; c->em_alt0 = src->em_alt0;
    c->d_pself.borrow(src->d_pself); c->d_pseg.borrow(src->d_pseg); c->d_pt0.borrow(src->d_pt0); c->d_pt0b.borrow(src->d_pt0b); c->d_cdf32.borrow(src->d_cdf32); c->d_cdf.borrow(src->d_cdf); c->d_alts.borrow(src->d_alts); c->d_altenc.borrow(src->d_altenc);
    c->d_nalts.borrow(src->d_nalts); c->d_qkeys.borrow(src->d_qkeys); c->d_qoff.borrow(src->d_qoff); c->d_qcnt.borrow(src->d_qcnt);
    c->d_qcdf.borrow(src->d_qcdf); c->d_qq.borrow(src->d_qq); c->d_qtab.borrow(src->d_qtab); c->d_qent.borrow(src->d_qent);
    c->d_qpairs.borrow(src->d_qpairs); c->d_qguide.borrow(src->d_qguide);
    c->tail = src->tail; c->tail_version = src->tail_version; c->host_threads = src->host_threads;
    c->d_tail_lx.borrow(src->d_tail_lx); c->d_tail_ly.borrow(src->d_tail_ly); c->d_tail_cdf.borrow(src->d_tail_cdf); c->d_tail_chain.borrow(src->d_tail_chain);
    return TKSMSEQ_OK;
}

int tksmseq_host_alloc(uint64_t bytes, void** out) {
    if (!out) return TKSMSEQ_EINVAL;
    *out = nullptr;
    return hipHostMalloc(out, bytes ? bytes : 1, hipHostMallocDefault) == hipSuccess ? TKSMSEQ_OK : TKSMSEQ_ENOMEM;
}

void tksmseq_host_free(void* p) { if (p) (void)hipHostFree(p); }

int tksmseq_device_alloc(tksmseq_ctx* ctx, uint64_t bytes, void** out) {
    if (!ctx || !out) return TKSMSEQ_EINVAL;
    *out = nullptr;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, hipMalloc(out, bytes ? bytes : 1));
    return TKSMSEQ_OK;
}
void tksmseq_device_free(tksmseq_ctx* ctx, void* p) { if (ctx && p) { (void)hipSetDevice(ctx->device); (void)hipFree(p); } }
int tksmseq_copy_to_host(tksmseq_ctx* ctx, void* dst_host, const void* src_device, uint64_t bytes, int async) {
    if (!ctx || ((!dst_host || !src_device) && bytes)) return TKSMSEQ_EINVAL;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (bytes) HIPCHK(ctx, hipMemcpyAsync(dst_host, src_device, bytes, hipMemcpyDeviceToHost, ctx->stream));
    if (!async) HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return TKSMSEQ_OK;
}

void tksmseq_destroy(tksmseq_ctx* ctx) {
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    for (auto& ev : ctx->ev) if (ev) (void)hipEventDestroy(ev);
    for (auto& ev : ctx->evpool) (void)hipEventDestroy(ev);
    if (ctx->own_stream && ctx->stream) (void)hipStreamDestroy(ctx->stream);
    delete ctx;                                              // (helper streams, page-locked and device buffers go with it)
    DevCache::get().context_destroyed();                     // (the last context of the process frees the cached batch buffers)
}

const char* tksmseq_last_error(const tksmseq_ctx* ctx) { return ctx ? ctx->err.c_str() : g_create_error.c_str(); }

int tksmseq_set_stream(tksmseq_ctx* ctx, void* s) {
    if (!ctx) return TKSMSEQ_EINVAL;
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    if (ctx->own_stream && ctx->stream) (void)hipStreamDestroy(ctx->stream);
    if (s) { ctx->stream = (hipStream_t)s; ctx->own_stream = false; }
    else { HIPCHK(ctx, hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking)); ctx->own_stream = true; }
    return TKSMSEQ_OK;
}

int tksmseq_synchronize(tksmseq_ctx* ctx) {
    if (!ctx) return TKSMSEQ_EINVAL;
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return TKSMSEQ_OK;
}

int tksmseq_set_host_threads(tksmseq_ctx* ctx, int n) { if (!ctx || n < 1) return TKSMSEQ_EINVAL; ctx->host_threads = std::min(n, 64); return TKSMSEQ_OK; }

int tksmseq_model_available(const char* name, const char* kind) { return (name && kind && model_available(name, kind)) ? 1 : 0; }

int tksmseq_set_timing(tksmseq_ctx* ctx, int enable) { if (!ctx) return TKSMSEQ_EINVAL; ctx->timing = enable != 0; return TKSMSEQ_OK; }

// ------------------------------------------------------------------------------------------- reference
int tksmseq_reference_add_contig(tksmseq_ctx* ctx, const char* name, const uint8_t* ascii, uint64_t len, int on_device) {
    if (!ctx || !name || (!ascii && len)) return TKSMSEQ_EINVAL;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const uint64_t BLK = 1ull << tk::BLOCK_SHIFT;
    const uint64_t gstart = ctx->total_alloc;
    const uint64_t nblk = (len + BLK - 1) / BLK;
    if (gstart + nblk * BLK > (1ull << 44)) { ctx->err = "reference larger than 2^44 bases"; return TKSMSEQ_ELIMIT; }
    HIPCHK(ctx, ctx->d_packed.ensure(((gstart + nblk * BLK) >> 4) * 4 + 64, true, ctx->stream));
    HIPCHK(ctx, ctx->d_blocktab.ensure(((gstart >> tk::BLOCK_SHIFT) + nblk) * 4 + 64, true, ctx->stream));
    uint32_t* blocktab = ctx->d_blocktab.as<uint32_t>() + (gstart >> tk::BLOCK_SHIFT);
    const uint64_t CH = 64ull << 20;   // staging chunk (multiple of the block size)
    std::vector<uint32_t> flags;
    for (uint64_t off = 0; off < len; off += CH) {
        const uint64_t n = std::min(CH, len - off);
        const uint64_t cb = (n + BLK - 1) / BLK;
        const uint8_t* dsrc;
        if (on_device) dsrc = ascii + off;
        else {
            HIPCHK(ctx, ctx->d_stage.ensure(CH));
            HIPCHK(ctx, hipMemcpyAsync(ctx->d_stage.p, ascii + off, n, hipMemcpyHostToDevice, ctx->stream));
            dsrc = ctx->d_stage.as<uint8_t>();
        }
        uint32_t* bt = blocktab + (off >> tk::BLOCK_SHIFT);
        HIPCHK(ctx, hipMemsetAsync(bt, 0, cb * 4, ctx->stream));
        HIPCHK(ctx, tk::launch_pack(dsrc, n, gstart + off, ctx->d_packed.as<uint32_t>(), ctx->d_blocktab.as<uint32_t>(), ctx->stream));
        flags.resize(cb);
        HIPCHK(ctx, hipMemcpyAsync(flags.data(), bt, cb * 4, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        uint32_t newblocks = 0;
        for (auto& f : flags) { if (f) { f = ctx->pool_blocks + newblocks; newblocks++; } else f = tk::NO_BLOCK; }
        HIPCHK(ctx, hipMemcpyAsync(bt, flags.data(), cb * 4, hipMemcpyHostToDevice, ctx->stream));
        if (newblocks) {
            HIPCHK(ctx, ctx->d_pool.ensure((uint64_t)(ctx->pool_blocks + newblocks) * BLK, true, ctx->stream));
            HIPCHK(ctx, tk::launch_fill_pool(dsrc, n, gstart + off, ctx->d_blocktab.as<uint32_t>(), ctx->d_pool.as<uint8_t>(), ctx->stream));
            ctx->pool_blocks += newblocks;
        }
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    }
    // later contigs with the same name replace earlier ones (dict.update, py/sequence.py:193)
    std::string nm(name);
    auto it = ctx->contig_index.find(nm);
    if (it == ctx->contig_index.end()) {
        ctx->contig_index[nm] = (int)ctx->contig_names.size();
        ctx->contig_names.push_back(nm);
        ctx->contigs.push_back(gstart); ctx->contigs.push_back(len);
        ctx->contig_declared.push_back(0);
    } else {
        ctx->total_bases -= ctx->contigs[2 * it->second + 1];
        ctx->contigs[2 * it->second] = gstart; ctx->contigs[2 * it->second + 1] = len;
        if (ctx->contig_declared[(size_t)it->second]) { ctx->contig_declared[(size_t)it->second] = 0; ctx->n_declared--; }   // (declared before: now it has bases)
    }
    ctx->total_alloc = gstart + nblk * BLK;
    ctx->total_bases += len;
    ctx->ref_version++;
    HIPCHK(ctx, ctx->d_contigs.ensure(ctx->contigs.size() * 8 + 16));
    HIPCHK(ctx, hipMemcpyAsync(ctx->d_contigs.p, ctx->contigs.data(), ctx->contigs.size() * 8, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return TKSMSEQ_OK;
}

int tksmseq_reference_declare_contig(tksmseq_ctx* ctx, const char* name, uint64_t len) {
    if (!ctx || !name) return TKSMSEQ_EINVAL;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (len > (1ull << 44)) { ctx->err = "reference larger than 2^44 bases"; return TKSMSEQ_ELIMIT; }
    // name and length only: no packed bases behind it (gstart is never dereferenced: tksmseq_run refuses while n_declared > 0)
    std::string nm(name);
    auto it = ctx->contig_index.find(nm);
    if (it == ctx->contig_index.end()) {
        ctx->contig_index[nm] = (int)ctx->contig_names.size();
        ctx->contig_names.push_back(nm);
        ctx->contigs.push_back(ctx->total_alloc); ctx->contigs.push_back(len);
        ctx->contig_declared.push_back(1);
        ctx->n_declared++;
    } else {
        ctx->total_bases -= ctx->contigs[2 * it->second + 1];
        ctx->contigs[2 * it->second + 1] = len;
        if (!ctx->contig_declared[(size_t)it->second]) { ctx->contig_declared[(size_t)it->second] = 1; ctx->n_declared++; }
    }
    ctx->total_bases += len;
    ctx->ref_version++;
    HIPCHK(ctx, ctx->d_contigs.ensure(ctx->contigs.size() * 8 + 16));
    HIPCHK(ctx, hipMemcpyAsync(ctx->d_contigs.p, ctx->contigs.data(), ctx->contigs.size() * 8, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return TKSMSEQ_OK;
}

int tksmseq_reference_add_fasta(tksmseq_ctx* ctx, const char* path) {
    if (!ctx || !path) return TKSMSEQ_EINVAL;
    std::vector<FastaRecord> recs;
    if (!read_fasta(path, recs, ctx->err)) return TKSMSEQ_EIO;
    for (auto& r : recs) {
        int rc = tksmseq_reference_add_contig(ctx, r.name.c_str(), (const uint8_t*)r.seq.data(), r.seq.size(), 0);
        if (rc) return rc;
    }
    return TKSMSEQ_OK;
}

int tksmseq_reference_contig_id(const tksmseq_ctx* ctx, const char* name) { return (!ctx || !name) ? -1 : ctx->find(name); }

int tksmseq_reference_info(const tksmseq_ctx* ctx, uint64_t* n_contigs, uint64_t* total_bases, uint64_t* device_bytes) {
    if (!ctx) return TKSMSEQ_EINVAL;
    if (n_contigs) *n_contigs = ctx->contig_names.size();
    if (total_bases) *total_bases = ctx->total_bases;
    if (device_bytes) *device_bytes = (ctx->total_alloc >> 2) + (ctx->total_alloc >> tk::BLOCK_SHIFT) * 4 + ((uint64_t)ctx->pool_blocks << tk::BLOCK_SHIFT);
    return TKSMSEQ_OK;
}

// ------------------------------------------------------------------------------------------- models
int tksmseq_load_error_model(tksmseq_ctx* ctx, const char* name_or_path) {
    if (!ctx || !name_or_path) return TKSMSEQ_EINVAL;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    ErrorModelHost m;
    if (!load_error_model(name_or_path, m, ctx->err)) return TKSMSEQ_EIO;
    ctx->em = std::move(m);
    ctx->em_alt0 = ctx->em.type == 1;
    for (size_t i = 0; i < ctx->em.nalts.size() && ctx->em_alt0; i++)
        if (ctx->em.nalts[i] && !(ctx->em.alts[i * (size_t)ctx->em.max_alts] >> 63)) ctx->em_alt0 = false;
    ctx->em_uniform = ctx->em.type == 1;
    for (uint8_t v : ctx->em.nalts) if ((int)v != ctx->em.max_alts) { ctx->em_uniform = false; break; }
    int rc;
    if ((rc = upload(ctx, ctx->d_cdf, ctx->em.cdf))) return rc;
    {
        if (ctx->em.max_alts > 32) { ctx->err = "error models with more than 32 alternatives per k-mer are not supported"; return TKSMSEQ_ELIMIT; }
        const size_t nk = ctx->em.nalts.size(), A = (size_t)ctx->em.max_alts;
        std::vector<uint32_t> c32(nk * 32, 0xFFFFFFFFu);
        for (size_t i = 0; i < nk; i++) for (size_t a = 0; a < A; a++) c32[i * 32 + a] = ctx->em.cdf[i * A + a];
        if (ctx->em.type == 0) std::fill(c32.begin(), c32.end(), 0u);
        if ((rc = upload(ctx, ctx->d_cdf32, c32))) return rc;
        std::vector<uint32_t> ps(nk * 2);
        for (size_t i = 0; i < nk; i++) { ps[2 * i] = c32[i * 32]; ps[2 * i + 1] = ctx->em.nalts[i] ? c32[i * 32 + ctx->em.nalts[i] - 1] : 0u; }
        if ((rc = upload(ctx, ctx->d_pself, ps))) return rc;
        std::vector<uint32_t> sg(nk * 4);                     // thresholds 0, 8, 16, 24 of every row (kernels.h ErrModelView::pseg)
        for (size_t i = 0; i < nk; i++) for (int q = 0; q < 4; q++) sg[4 * i + q] = c32[i * 32 + 8 * q];
        if ((rc = upload(ctx, ctx->d_pseg, sg))) return rc;
        std::vector<uint32_t> t0(nk);
        for (size_t i = 0; i < nk; i++) t0[i] = c32[i * 32];
        if ((rc = upload(ctx, ctx->d_pt0, t0))) return rc;
        std::vector<uint16_t> t0b(tklf::LOOP_FILTER_KEYS);    // per coarse key the byte bounds of t0: k_loop's copy in LDS (loop_filter.h)
        tklf::loop_filter_build(t0.data(), nk, t0b.data());
        if ((rc = upload(ctx, ctx->d_pt0b, t0b))) return rc;
    }
    if ((rc = upload(ctx, ctx->d_alts, ctx->em.alts))) return rc;
    {
        // the alternatives once more, as the fast pipeline applies them (kernels.h ErrModelView::alts_enc): per slot the
        // 16-bit encoding it would write, bit 15 telling whether the slot differs from the k-mer's own base
        const size_t nk = ctx->em.nalts.size(), A = (size_t)ctx->em.max_alts;
        const int k = ctx->em.k;
        std::vector<uint32_t> enc(nk * A * 4, 0u);
        for (size_t i = 0; i < nk && ctx->em.type == 1; i++)
            for (size_t a = 0; a < A; a++) {
                const uint64_t alt = ctx->em.alts[i * A + a];
                uint32_t e[8] = {0, 0, 0, 0, 0, 0, 0, 0};
                int boff = 0;
                for (int j = 0; j < k; j++) {
                    const uint32_t kc = (uint32_t)(i >> (2 * (k - 1 - j))) & 3u;
                    if (alt >> 63) { e[j] = (1u << 12) | (kc & 1u) | ((kc >> 1) << 5); continue; }          // the k-mer itself
                    const uint32_t len = (uint32_t)(alt >> (3 * j)) & 7u;
                    const uint32_t codes = (uint32_t)(alt >> (24 + 2 * boff)) & ((1u << (2 * len)) - 1u);
                    boff += (int)len;
                    // symbols planar: low bits of the (up to 5) symbols in bits 0..4, high bits in bits 5..9 (what k_job queues)
                    uint32_t planar = 0;
                    for (uint32_t x = 0; x < len && x < 5; x++) planar |= (((codes >> (2 * x)) & 1u) << x) | (((codes >> (2 * x + 1)) & 1u) << (5 + x));
                    e[j] = ((len == 1 && codes == kc) ? 0u : 0x8000u) | (len << 12) | planar;
                }
                for (int q = 0; q < 4; q++) enc[(i * A + a) * 4 + q] = e[2 * q] | (e[2 * q + 1] << 16);
            }
        if ((rc = upload(ctx, ctx->d_altenc, enc))) return rc;
    }
    return upload(ctx, ctx->d_nalts, ctx->em.nalts);
}

int tksmseq_load_qscore_model(tksmseq_ctx* ctx, const char* name_or_path) {
    if (!ctx || !name_or_path) return TKSMSEQ_EINVAL;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    QScoreModelHost m;
    if (!load_qscore_model(name_or_path, m, ctx->err)) return TKSMSEQ_EIO;
    ctx->qm = std::move(m);
    int rc;
    if ((rc = upload(ctx, ctx->d_qkeys, ctx->qm.keys))) return rc;
    if ((rc = upload(ctx, ctx->d_qoff, ctx->qm.row_off))) return rc;
    if ((rc = upload(ctx, ctx->d_qcnt, ctx->qm.row_cnt))) return rc;
    if ((rc = upload(ctx, ctx->d_qcdf, ctx->qm.cdf_pool))) return rc;
    if ((rc = upload(ctx, ctx->d_qq, ctx->qm.q_pool))) return rc;
    {
        const QScoreModelHost& m2 = ctx->qm;
        const size_t ns = (size_t)m2.n_slots;
        std::vector<uint32_t> ent(ns * 4, 0), pairs(m2.q_pool.size() * 2, 0);
        std::vector<uint8_t> guide(ns * 64, 0);
        // (the flag bit needs candidate indices and q values below 128: every model we know of; otherwise the plain guide)
        bool direct = true;
        for (size_t s2 = 0; s2 < ns; s2++) if (m2.keys[s2] && m2.row_cnt[s2] > 128) direct = false;
        for (uint8_t qv : m2.q_pool) if (qv > 127) direct = false;
        for (size_t i = 0; i < m2.q_pool.size(); i++) { pairs[2 * i] = m2.cdf_pool[i]; pairs[2 * i + 1] = m2.q_pool[i]; }
        for (size_t s2 = 0; s2 < ns; s2++) {
            ent[4 * s2] = (uint32_t)m2.keys[s2]; ent[4 * s2 + 1] = (uint32_t)(m2.keys[s2] >> 32);
            ent[4 * s2 + 2] = m2.row_off[s2]; ent[4 * s2 + 3] = m2.row_cnt[s2];
            if (!m2.keys[s2]) continue;
            const uint32_t off = m2.row_off[s2], cnt = m2.row_cnt[s2];
            if (cnt > 255) { ctx->err = "q-score rows with more than 255 entries are not supported"; return TKSMSEQ_ELIMIT; }
            uint32_t a = 0;
            for (uint32_t bkt = 0; bkt < 64; bkt++) {
                // entries whose threshold is <= the smallest draw of the bucket can never be chosen in it
                const uint32_t wmin = bkt << 26, wmax = wmin | 0x3ffffffu;
                while (a + 1 < cnt && m2.cdf_pool[off + a] <= wmin) a++;
                // ... and if the largest draw of the bucket stops at the same entry, the bucket IS that entry's q: no row read
                uint32_t ah = a;
                while (ah + 1 < cnt && m2.cdf_pool[off + ah] <= wmax) ah++;
                guide[s2 * 64 + bkt] = (direct && ah == a) ? (uint8_t)(0x80u | m2.q_pool[off + a]) : (uint8_t)a;
            }
        }
        ctx->qm.guide_direct = direct;
        if ((rc = upload(ctx, ctx->d_qent, ent))) return rc;
        if ((rc = upload(ctx, ctx->d_qpairs, pairs))) return rc;
        return upload(ctx, ctx->d_qguide, guide);
    }
}

static int install_tail_model(tksmseq_ctx* ctx, TailModelHost&& m) {
    ctx->tail = std::move(m);
    ctx->tail_version++;
    if (!ctx->tail.enabled) return TKSMSEQ_OK;
    int rc;
    if ((rc = upload(ctx, ctx->d_tail_lx, ctx->tail.lx))) return rc;
    if ((rc = upload(ctx, ctx->d_tail_ly, ctx->tail.ly))) return rc;
    if ((rc = upload(ctx, ctx->d_tail_cdf, ctx->tail.cdf))) return rc;
    std::vector<tk::TailChain> ch(1);
    memcpy(ch[0].cum, ctx->tail.cum, sizeof(ch[0].cum));
    ch[0].bases = (uint32_t)ctx->tail.bases[0] | ((uint32_t)ctx->tail.bases[1] << 8) | ((uint32_t)ctx->tail.bases[2] << 16) | ((uint32_t)ctx->tail.bases[3] << 24);
    ch[0].pad = 0;
    return upload(ctx, ctx->d_tail_chain, ch);
}

int tksmseq_load_tail_model(tksmseq_ctx* ctx, const char* name_or_path) {
    if (!ctx || !name_or_path) return TKSMSEQ_EINVAL;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    TailModelHost m;
    if (!load_tail_model(name_or_path, m, ctx->err)) return TKSMSEQ_EINVAL;
    return install_tail_model(ctx, std::move(m));
}

int tksmseq_set_tail_model(tksmseq_ctx* ctx, const tksmseq_tail_model* t) {
    if (!ctx) return TKSMSEQ_EINVAL;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    TailModelHost m;
    if (t) {
        if (!t->lx || !t->ly || !t->grid) { ctx->err = "tail model: null table"; return TKSMSEQ_EINVAL; }
        if (!make_tail_model(t->lx, t->n_lx, t->ly, t->n_ly, t->grid, t->trans, t->ratio, t->bases, m, ctx->err)) return TKSMSEQ_EINVAL;
    }
    return install_tail_model(ctx, std::move(m));
}

int tksmseq_set_identity(tksmseq_ctx* ctx, double mean, double max, double stdev) {
    if (!ctx) return TKSMSEQ_EINVAL;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    IdentityHost id;
    if (!make_identity(mean, max, stdev, id, ctx->err)) return TKSMSEQ_EINVAL;
    id.set = true;
    ctx->idm = std::move(id);
    if (!ctx->idm.constant) return upload(ctx, ctx->d_qtab, ctx->idm.qtab);
    return TKSMSEQ_OK;
}

int tksmseq_prefetch_model(const char* name_or_path, const char* kind) {
    if (!name_or_path || !kind) return TKSMSEQ_EINVAL;
    std::string err;
    // (the loader's message: tksmseq_last_error(NULL) on the calling thread)
    if (!strcmp(kind, "error")) { ErrorModelHost m; if (load_error_model(name_or_path, m, err)) return TKSMSEQ_OK; g_create_error = err; return TKSMSEQ_EIO; }
    if (!strcmp(kind, "qscore")) { QScoreModelHost m; if (load_qscore_model(name_or_path, m, err)) return TKSMSEQ_OK; g_create_error = err; return TKSMSEQ_EIO; }
    g_create_error = std::string("unknown model kind: ") + kind;
    return TKSMSEQ_EINVAL;
}

int tksmseq_prefetch_identity(double mean, double max, double stdev) {
    IdentityHost id; std::string err;
    return make_identity(mean, max, stdev, id, err) ? TKSMSEQ_OK : TKSMSEQ_EINVAL;
}

int tksmseq_get_error_model(const tksmseq_ctx* ctx, int32_t* type, int32_t* k, int32_t* max_alts, uint32_t* cdf, uint64_t* alts, uint8_t* nalts) {
    if (!ctx || ctx->em.type < 0) return TKSMSEQ_ESTATE;
    if (type) *type = ctx->em.type;
    if (k) *k = ctx->em.k;
    if (max_alts) *max_alts = ctx->em.max_alts;
    if (cdf) memcpy(cdf, ctx->em.cdf.data(), ctx->em.cdf.size() * 4);
    if (alts) memcpy(alts, ctx->em.alts.data(), ctx->em.alts.size() * 8);
    if (nalts) memcpy(nalts, ctx->em.nalts.data(), ctx->em.nalts.size());
    return TKSMSEQ_OK;
}

int tksmseq_get_qscore_model(const tksmseq_ctx* ctx, int32_t* n_slots, int32_t* kmer_size, uint64_t* pool_len, uint64_t* keys,
                             uint32_t* row_off, uint32_t* row_cnt, uint32_t* cdf_pool, uint8_t* q_pool) {
    if (!ctx || ctx->qm.n_slots == 0) return TKSMSEQ_ESTATE;
    if (n_slots) *n_slots = ctx->qm.n_slots;
    if (kmer_size) *kmer_size = ctx->qm.kmer_size;
    if (pool_len) *pool_len = ctx->qm.q_pool.size();
    if (keys) memcpy(keys, ctx->qm.keys.data(), ctx->qm.keys.size() * 8);
    if (row_off) memcpy(row_off, ctx->qm.row_off.data(), ctx->qm.row_off.size() * 4);
    if (row_cnt) memcpy(row_cnt, ctx->qm.row_cnt.data(), ctx->qm.row_cnt.size() * 4);
    if (cdf_pool) memcpy(cdf_pool, ctx->qm.cdf_pool.data(), ctx->qm.cdf_pool.size() * 4);
    if (q_pool) memcpy(q_pool, ctx->qm.q_pool.data(), ctx->qm.q_pool.size());
    return TKSMSEQ_OK;
}

int tksmseq_get_identity(const tksmseq_ctx* ctx, int32_t* constant, double* value, double* beta_a, double* beta_b, double* qtab) {
    if (!ctx || !ctx->idm.set) return TKSMSEQ_ESTATE;
    if (constant) *constant = ctx->idm.constant ? 1 : 0;
    if (value) *value = ctx->idm.value;
    if (beta_a) *beta_a = ctx->idm.beta_a;
    if (beta_b) *beta_b = ctx->idm.beta_b;
    if (qtab && !ctx->idm.constant) memcpy(qtab, ctx->idm.qtab.data(), 65537 * sizeof(double));
    return TKSMSEQ_OK;
}

// ------------------------------------------------------------------------------------------- batches
static int batch_from_host(tksmseq_ctx* ctx, const tksmseq_batch_desc* d, tksmseq_batch** out, bool check_mods = true) {
    *out = nullptr;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (d->n_intervals >= 0x7fffffffull || d->n_mods >= 0x7fffffffull || d->n_reads >= 0xffffffffull) {
        ctx->err = "batch too large (split it: < 2^31 intervals/mods per batch)"; return TKSMSEQ_ELIMIT;
    }
    std::unique_ptr<tksmseq_batch> b(new tksmseq_batch());
    b->n_reads = d->n_reads; b->n_intervals = d->n_intervals; b->n_mods = d->n_mods; b->n_literals = d->n_literals;
    // validate + host-side raw lengths (python slice clamp, py/sequence.py:307)
    std::vector<uint32_t> ilen(d->n_intervals);
    const uint64_t nc = ctx->contig_names.size();
    uint32_t prev_mod = 0;
    for (uint64_t i = 0; i < d->n_intervals; i++) {
        const uint32_t* iv = d->intervals + 4 * i;
        uint64_t clen;
        if (iv[0] >> 31) {
            uint32_t li = iv[0] & 0x7fffffffu;
            if (li >= d->n_literals) { ctx->err = "interval refers to a literal that does not exist"; return TKSMSEQ_EINVAL; }
            clen = d->literals[2 * li + 1];
            if (d->literals[2 * li] + clen > d->literal_bytes) { ctx->err = "literal outside the literal pool"; return TKSMSEQ_EINVAL; }
        } else {
            if (iv[0] >= nc) { ctx->err = "interval refers to a contig that does not exist"; return TKSMSEQ_EINVAL; }
            clen = ctx->contigs[2 * (uint64_t)iv[0] + 1];
        }
        const uint64_t s = std::min<uint64_t>(iv[1], clen), e = std::min<uint64_t>(iv[2], clen);
        ilen[i] = e > s ? (uint32_t)(e - s) : 0;
        const uint32_t mb = iv[3] & 0x7fffffffu;
        if (mb < prev_mod || mb > d->n_mods) { ctx->err = "interval modification offsets are not monotone"; return TKSMSEQ_EINVAL; }
        prev_mod = mb;
    }
    // the reference raises IndexError for a modification outside its slice (py/sequence.py:238)
    for (uint64_t i = 0; i < d->n_intervals && check_mods; i++) {
        const uint32_t mb = d->intervals[4 * i + 3] & 0x7fffffffu;
        const uint32_t me = i + 1 < d->n_intervals ? (d->intervals[4 * (i + 1) + 3] & 0x7fffffffu) : (uint32_t)d->n_mods;
        for (uint32_t m = mb; m < me; m++)
            if (d->mods[2 * (uint64_t)m] >= ilen[i]) { ctx->err = "modification position outside its interval (the reference raises IndexError)"; return TKSMSEQ_EINVAL; }
    }
    b->raw_len.resize(d->n_reads);
    for (uint64_t r = 0; r < d->n_reads; r++) {
        const uint32_t ib = d->reads[2 * r], ic = d->reads[2 * r + 1];
        if ((uint64_t)ib + ic > d->n_intervals) { ctx->err = "read refers to intervals that do not exist"; return TKSMSEQ_EINVAL; }
        uint64_t t = 0;
        for (uint32_t i = 0; i < ic; i++) t += ilen[ib + i];
        if (t > 0x7fffff00ull) { ctx->err = "molecule longer than 2^31 bases"; return TKSMSEQ_ELIMIT; }
        b->raw_len[r] = (uint32_t)t;
        b->max_raw = std::max(b->max_raw, (uint32_t)t);
        b->total_raw += t;
        if ((uint64_t)d->ids[2 * r] + d->ids[2 * r + 1] > d->id_bytes) { ctx->err = "molecule id outside the id pool"; return TKSMSEQ_EINVAL; }
    }
    order_by_length(b->raw_len, b->order);
    auto up = [&](DevBuf& buf, const void* src, size_t bytes) -> int {
        HIPCHK(ctx, buf.ensure(bytes + 64));
        if (bytes) HIPCHK(ctx, hipMemcpyAsync(buf.p, src, bytes, hipMemcpyHostToDevice, ctx->stream));
        return TKSMSEQ_OK;
    };
    int rc;
    if ((rc = up(b->reads, d->reads, d->n_reads * 8))) return rc;
    // intervals + sentinel carrying n_mods
    std::vector<uint32_t> iv(d->intervals, d->intervals + 4 * d->n_intervals);
    iv.push_back(0); iv.push_back(0); iv.push_back(0); iv.push_back((uint32_t)d->n_mods);
    if ((rc = up(b->intervals, iv.data(), iv.size() * 4))) return rc;
    if ((rc = up(b->mods, d->mods, d->n_mods * 8))) return rc;
    if ((rc = up(b->literals, d->literals, d->n_literals * 16))) return rc;
    if ((rc = up(b->litpool, d->literal_pool, d->literal_bytes))) return rc;
    if ((rc = up(b->ids, d->ids, d->n_reads * 8))) return rc;
    if ((rc = up(b->idpool, d->id_pool, d->id_bytes))) return rc;
    if ((rc = up(b->d_order, b->order.data(), b->order.size() * 4))) return rc;
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    *out = b.release();
    return TKSMSEQ_OK;
}

int tksmseq_batch_create(tksmseq_ctx* ctx, const tksmseq_batch_desc* d, tksmseq_batch** out) {
    if (!ctx || !d || !out) return TKSMSEQ_EINVAL;
    return batch_from_host(ctx, d, out);
}

static int batch_from_text(tksmseq_ctx* ctx, const char* text, uint64_t len, tksmseq_batch** out, bool check_mods);

int tksmseq_batch_from_mdf_text(tksmseq_ctx* ctx, const char* text, uint64_t len, tksmseq_batch** out) { return batch_from_text(ctx, text, len, out, true); }

// For the MDF -> MDF modules (PCR, truncation), which run without a reference: contig names the context does not know are
// kept as literal names, and substitution positions are not checked against slices that cannot be taken here.
int tksmseq_molecules_from_mdf_text(tksmseq_ctx* ctx, const char* text, uint64_t len, tksmseq_batch** out) { return batch_from_text(ctx, text, len, out, false); }

static int batch_from_text(tksmseq_ctx* ctx, const char* text, uint64_t len, tksmseq_batch** out, bool check_mods) {
    if (!ctx || (!text && len) || !out) return TKSMSEQ_EINVAL;
    BatchHost h;
    const auto t_text = std::chrono::steady_clock::now();
    if (!parse_mdf_mt(text, len, *ctx, h, ctx->err, ctx->host_threads)) return TKSMSEQ_EINVAL;
    const double s_text = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_text).count();
    const double a0 = alloc_seconds();
    tksmseq_batch_desc d{};
    d.n_reads = h.reads.size() / 2; d.n_intervals = h.intervals.size() / 4; d.n_mods = h.mods.size() / 2;
    d.n_literals = h.literals.size() / 2; d.literal_bytes = h.literal_pool.size(); d.id_bytes = h.id_pool.size();
    d.reads = h.reads.data(); d.intervals = h.intervals.data(); d.mods = h.mods.data(); d.literals = h.literals.data();
    d.literal_pool = h.literal_pool.data(); d.ids = h.ids.data(); d.id_pool = h.id_pool.data();
    const int rc = batch_from_host(ctx, &d, out, check_mods);
    if (rc != TKSMSEQ_OK) return rc;
    if (verbose_level() >= 2)
        fprintf(stderr, "[tksmseq] batch from %.0f MB of MDF text: parse %.3f s, tables + upload %.3f s (of which device allocation %.3f s)\n", len / 1e6, s_text,
                std::chrono::duration<double>(std::chrono::steady_clock::now() - t_text).count() - s_text, alloc_seconds() - a0);
    // kept for PCR / truncation / the MDF writer: which reads are copies of a depth > 1 molecule, and the header comments
    tksmseq_batch* b = *out;
    bool any_dup = false;
    for (uint32_t v : h.dup) any_dup |= (v >> 31) != 0;
    if (any_dup) {
        b->h_dup = std::move(h.dup);
        HIPCHK(ctx, b->d_dup.ensure(b->h_dup.size() * 4 + 16));
        HIPCHK(ctx, hipMemcpyAsync(b->d_dup.p, b->h_dup.data(), b->h_dup.size() * 4, hipMemcpyHostToDevice, ctx->stream));
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    }
    b->h_comments = std::move(h.comments); b->h_comment_pool = std::move(h.comment_pool);
    return TKSMSEQ_OK;
}

int tksmseq_batch_info(const tksmseq_batch* b, uint64_t* n_reads, uint64_t* n_intervals, uint64_t* n_mods) {
    if (!b) return TKSMSEQ_EINVAL;
    if (n_reads) *n_reads = b->n_reads;
    if (n_intervals) *n_intervals = b->n_intervals;
    if (n_mods) *n_mods = b->n_mods;
    return TKSMSEQ_OK;
}

void tksmseq_batch_free(tksmseq_ctx* ctx, tksmseq_batch* b) {
    if (ctx) { (void)hipSetDevice(ctx->device); (void)hipStreamSynchronize(ctx->stream); }
    const auto t_free = std::chrono::steady_clock::now();
    delete b;
    if (b && verbose_level() >= 2) fprintf(stderr, "[tksmseq] batch freed in %.3f s\n", std::chrono::duration<double>(std::chrono::steady_clock::now() - t_free).count());
}

// ------------------------------------------------------------------------------------------- run
int tksmseq_set_output_buffer(tksmseq_ctx* ctx, void* p, uint64_t cap) {
    if (!ctx) return TKSMSEQ_EINVAL;
    ctx->user_out = p; ctx->user_out_cap = p ? cap : 0;
    return TKSMSEQ_OK;
}

// (tksmseq_run and tksmseq_run_diagnostics: run.cpp)

int tksmseq_result_download(tksmseq_ctx* ctx, uint8_t* records, uint64_t* offsets) {
    if (!ctx || !ctx->have_last) return TKSMSEQ_ESTATE;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (records && ctx->last.records_bytes) HIPCHK(ctx, hipMemcpyAsync(records, ctx->last.records, ctx->last.records_bytes, hipMemcpyDeviceToHost, ctx->stream));
    if (offsets) HIPCHK(ctx, hipMemcpyAsync(offsets, ctx->last.record_offsets, (ctx->last.n_reads + 1) * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return TKSMSEQ_OK;
}

int tksmseq_result_download_range(tksmseq_ctx* ctx, uint8_t* dst, uint64_t offset, uint64_t bytes, int async) {
    if (!ctx || !ctx->have_last || (!dst && bytes)) return TKSMSEQ_ESTATE;
    if (offset > ctx->last.records_bytes || bytes > ctx->last.records_bytes - offset) { ctx->err = "record range outside the last result"; return TKSMSEQ_EINVAL; }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (bytes) HIPCHK(ctx, hipMemcpyAsync(dst, (const uint8_t*)ctx->last.records + offset, bytes, hipMemcpyDeviceToHost, ctx->stream));
    if (!async) HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return TKSMSEQ_OK;
}

int tksmseq_result_copy_device(tksmseq_ctx* ctx, void* records_dst, void* offsets_dst) {
    if (!ctx || !ctx->have_last) return TKSMSEQ_ESTATE;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (records_dst && ctx->last.records_bytes && records_dst != ctx->last.records)
        HIPCHK(ctx, hipMemcpyAsync(records_dst, ctx->last.records, ctx->last.records_bytes, hipMemcpyDeviceToDevice, ctx->stream));
    if (offsets_dst) HIPCHK(ctx, hipMemcpyAsync(offsets_dst, ctx->last.record_offsets, (ctx->last.n_reads + 1) * 8, hipMemcpyDeviceToDevice, ctx->stream));
    return TKSMSEQ_OK;
}

int tksmseq_stats_download(tksmseq_ctx* ctx, int32_t* istats, double* dstats) {
    if (!ctx || !ctx->have_last || !ctx->have_stats) return TKSMSEQ_ESTATE;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (istats) HIPCHK(ctx, hipMemcpyAsync(istats, ctx->w_istats.p, ctx->last.n_reads * 64, hipMemcpyDeviceToHost, ctx->stream));
    if (dstats) HIPCHK(ctx, hipMemcpyAsync(dstats, ctx->w_dstats.p, ctx->last.n_reads * 16, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return TKSMSEQ_OK;
}

// ------------------------------------------------------------------------------------------- interleave
int tksmseq_interleave_records(tksmseq_ctx* ctx, int n_ranks, const void* const* streams, const void* const* offsets,
                               const uint64_t* n_per_rank, void* dst, uint64_t dst_capacity, uint64_t* dst_bytes) {
    if (!ctx || n_ranks < 1 || n_ranks > 16 || !streams || !offsets || !n_per_rank || !dst) return TKSMSEQ_EINVAL;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    uint64_t n_total = 0;
    for (int i = 0; i < n_ranks; i++) {
        // round-robin sharding: rank p holds ceil((N - p) / P) reads
        n_total += n_per_rank[i];
        if (i && n_per_rank[i] > n_per_rank[i - 1]) { ctx->err = "per-rank read counts are not a round-robin split"; return TKSMSEQ_EINVAL; }
    }
    if (n_per_rank[0] - n_per_rank[n_ranks - 1] > 1) { ctx->err = "per-rank read counts are not a round-robin split"; return TKSMSEQ_EINVAL; }
    HIPCHK(ctx, ctx->w_reclen.ensure(n_total * 8 + 16));
    HIPCHK(ctx, ctx->w_slotoff.ensure((n_total + 1) * 8 + 16));
    HIPCHK(ctx, ctx->w_scan.ensure(tk::scan_temp_bytes(n_total) + 64));
    HIPCHK(ctx, tk::launch_interleave_lens(n_ranks, (const uint64_t* const*)offsets, n_per_rank, n_total, ctx->w_reclen.as<uint64_t>(), ctx->stream));
    HIPCHK(ctx, tk::launch_scan(ctx->w_reclen.as<uint64_t>(), ctx->w_slotoff.as<uint64_t>(), n_total, ctx->w_scan.p, ctx->w_scan.cap, ctx->stream));
    uint64_t total = 0;
    HIPCHK(ctx, hipMemcpyAsync(&total, ctx->w_slotoff.as<uint64_t>() + n_total, 8, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    if (total > dst_capacity) { ctx->err = "interleave destination too small"; return TKSMSEQ_ENOMEM; }
    HIPCHK(ctx, tk::launch_interleave_copy(n_ranks, (const uint8_t* const*)streams, (const uint64_t* const*)offsets, n_total,
                                           ctx->w_slotoff.as<uint64_t>(), (uint8_t*)dst, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    if (dst_bytes) *dst_bytes = total;
    return TKSMSEQ_OK;
}

}  // extern "C"
