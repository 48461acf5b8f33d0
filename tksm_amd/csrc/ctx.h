// ctx.h -- internal: the context and batch objects behind the opaque handles of include/tksmseq.h (shared by api.cpp, run.cpp
// and, through mdf_batch.h, the molecule transforms mdf_ops.cpp, mdf_move.cpp, mdf_make.cpp and mdf_text.cpp).
#pragma once
#include <hip/hip_runtime.h>
#include <chrono>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/tksmseq.h"
#include "abund_kernels.h"
#include "host.h"
#include "kernels.h"
#include "tsb_host.h"

using namespace tkh;

#define HIPCHK(ctx, call)                                                                         \
    do {                                                                                          \
        hipError_t e_ = (call);                                                                   \
        if (e_ != hipSuccess) {                                                                   \
            (ctx)->err = std::string(#call) + ": " + hipGetErrorString(e_);                       \
            return TKSMSEQ_EDEVICE;                                                               \
        }                                                                                         \
    } while (0)

// (diagnostics, TKSMSEQ_VERBOSE: time this thread has spent in hipMalloc)
inline double& alloc_seconds() { static thread_local double v = 0.0; return v; }
inline unsigned& alloc_calls() { static thread_local unsigned v = 0; return v; }

// ---- Cache of device allocations, per process and device, for the buffers that live for ONE batch: the tables of a molecule batch and
// the temporaries of PCR / truncation.  hipFree waits until the whole device is idle -- every stream of every context: ~100 ms while
// three batches are in flight -- and a streaming run frees (and allocates) such buffers once per batch: the workers of `tksm sequence`
// spent a third of their cycle in tksmseq_batch_free (profiles/r04_e2e_stream.log).  A pooled buffer goes back to the cache instead
// (after the stream that used it has drained -- see DevBuf::pool_stream for who drains) and the next request of about its size takes
// it.  Bounded: beyond CACHE_LIMIT bytes per device a block is really freed; everything is freed when the last context goes.
struct DevCache {
    static constexpr int MAX_DEV = 16;
    static constexpr size_t CACHE_LIMIT = 12ull << 30;
    std::mutex m;
    std::multimap<size_t, void*> blocks[MAX_DEV];
    size_t cached[MAX_DEV] = {};
    int live_contexts = 0;
    static DevCache& get() { static DevCache c; return c; }
    // sizes in classes of 1/8 of a power of two, so that consecutive batches (a few percent apart) reuse each other's blocks
    static size_t size_class(size_t bytes) {
        if (bytes < 4096) return 4096;
        int top = 63 - __builtin_clzll((unsigned long long)bytes);
        const size_t step = (size_t)1 << (top > 3 ? top - 3 : 0);
        return (bytes + step - 1) & ~(step - 1);
    }
    void* take(int dev, size_t cap) {                        // a cached block of exactly this class, or nullptr
        if (dev < 0 || dev >= MAX_DEV) return nullptr;
        std::lock_guard<std::mutex> l(m);
        auto it = blocks[dev].find(cap);
        if (it == blocks[dev].end()) return nullptr;
        void* p = it->second;
        blocks[dev].erase(it);
        cached[dev] -= cap;
        return p;
    }
    void give(int dev, void* p, size_t cap) {
        if (dev >= 0 && dev < MAX_DEV) {
            std::lock_guard<std::mutex> l(m);
            if (live_contexts > 0 && cached[dev] + cap <= CACHE_LIMIT) { blocks[dev].emplace(cap, p); cached[dev] += cap; return; }
        }
        (void)hipFree(p);
    }
    void context_created() { std::lock_guard<std::mutex> l(m); live_contexts++; }
    void context_destroyed() {                               // the last one out frees the cache
        std::vector<void*> drop;
        {
            std::lock_guard<std::mutex> l(m);
            if (--live_contexts > 0) return;
            for (int d = 0; d < MAX_DEV; d++) { for (auto& kv : blocks[d]) drop.push_back(kv.second); blocks[d].clear(); cached[d] = 0; }
        }
        for (void* p : drop) (void)hipFree(p);
    }
};

// ---- TKSMSEQ_POISON=<32-bit word, hex> (diagnostic; read once per process): every block that DevBuf::ensure or PinnedBuf::ensure hands out
// is filled with that word first, so that a result which depends on what a recycled block held changes with the word
// (tests/test_history_gpu.py runs the same calls unset, with 00000000 and with 00000001 and compares the bytes).  The counters are per
// process; every context prints what was filled since the line before as it goes (report(), from ~tksmseq_ctx).  Hidden: the library
// exports what it exported before.
struct __attribute__((visibility("hidden"))) Poison {
    bool on = false;
    uint32_t word = 0;
    std::mutex m;
    uint64_t blocks = 0, bytes = 0, shown_blocks = 0, shown_bytes = 0;
    // 1 to 8 hex digits (a leading 0x is allowed), nothing else
    static bool parse(const char* s, uint32_t* word) {
        if (!s) return false;
        if (s[0] == '0' && (s[1] == 'x' || s[1] == 'X')) s += 2;
        uint32_t v = 0;
        int n = 0;
        for (; *s; s++, n++) {
            const int d = *s >= '0' && *s <= '9' ? *s - '0' : *s >= 'a' && *s <= 'f' ? *s - 'a' + 10 : *s >= 'A' && *s <= 'F' ? *s - 'A' + 10 : -1;
            if (d < 0 || n == 8) return false;
            v = v << 4 | (uint32_t)d;
        }
        if (!n) return false;
        *word = v;
        return true;
    }
    // the bytes [lo, hi) of a new block of ncap bytes to fill: all of it, or with `keep` what lies behind the min(old cap, ncap) bytes
    // copied from the old block; whole words (every capacity here is a multiple of 256)
    static void range(size_t old_cap, size_t ncap, bool kept, size_t* lo, size_t* hi) {
        *hi = ncap & ~(size_t)3;
        *lo = std::min(kept ? (std::min(old_cap, ncap) + 3) & ~(size_t)3 : 0, *hi);
    }
    Poison() {
        const char* e = getenv("TKSMSEQ_POISON");
        on = parse(e, &word);
        if (e && !on) fprintf(stderr, "TKSMSEQ_POISON=%s is not a 32-bit hex word: ignored\n", e);
    }
    static Poison& get() { static Poison p; return p; }
    void filled(size_t n) { std::lock_guard<std::mutex> l(m); blocks++; bytes += n; }
    // on the null stream, and waited for: the contexts' streams are non-blocking, so nothing else orders the fill against them; a
    // block that ensure() hands out has no other user (DevCache receives drained blocks only)
    hipError_t fill_device(void* p, size_t lo, size_t hi) {
        if (hi > lo) {
            hipError_t e = hipMemsetD32Async((hipDeviceptr_t)((char*)p + lo), (int)word, (hi - lo) / 4, nullptr);
            if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
            if (e != hipSuccess) return e;
        }
        filled(hi - lo);
        return hipSuccess;
    }
    void fill_host(void* p, size_t bytes) { std::fill_n((uint32_t*)p, bytes / 4, word); filled(bytes & ~(size_t)3); }
    void report() {
        std::lock_guard<std::mutex> l(m);
        fprintf(stderr, "poison %08x: %llu blocks, %llu bytes\n", word, (unsigned long long)(blocks - shown_blocks), (unsigned long long)(bytes - shown_bytes));
        shown_blocks = blocks; shown_bytes = bytes;
    }
};

struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;
    bool owned = true;                     // false: a view of another context's buffer (tksmseq_clone), read-only
    // pooled: allocations come from / go back to DevCache, and no queued work may still use a block that goes back.  With pool_stream set
    // the buffer sees to that itself: release() drains that stream first (TmpBuf, the temporaries of a call).  The tables of a batch carry
    // no stream; whoever deletes a batch drains the stream of the context that ran it first: tksmseq_batch_free for a finished batch,
    // OutBatch (mdf_batch.h) for one still under construction when a transform returns an error.
    bool pooled = false;
    hipStream_t pool_stream = nullptr;
    int dev = -1;
    // one owner per block: a buffer moves (the source is left empty), it is never copied
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    DevBuf(DevBuf&& o) noexcept : p(o.p), cap(o.cap), owned(o.owned), pooled(o.pooled), pool_stream(o.pool_stream), dev(o.dev) { o.p = nullptr; o.cap = 0; }
    void release() {
        if (p && owned) {
            if (pooled) { if (pool_stream) (void)hipStreamSynchronize(pool_stream); DevCache::get().give(dev, p, cap); }
            else (void)hipFree(p);
        }
        p = nullptr; cap = 0;
    }
    ~DevBuf() { release(); }
    void borrow(const DevBuf& o) { release(); p = o.p; cap = o.cap; owned = false; }
    hipError_t ensure(size_t bytes, bool keep = false, hipStream_t s = nullptr) {
        if (bytes <= cap && owned) return hipSuccess;
        // a borrowed buffer is never written: the first write access replaces it by a private copy
        // large work buffers get 1/8 of headroom: consecutive batches of a stream differ by a few percent, and
        // re-allocating tens of GB costs more than a batch
        size_t ncap = std::max(bytes > (64u << 20) ? bytes + bytes / 8 : bytes, owned ? cap + cap / 2 : cap);
        ncap = (ncap + 255) & ~(size_t)255;
        void* np = nullptr;
        int ndev = dev;
        if (pooled) {
            ncap = DevCache::size_class(std::max<size_t>(bytes, 1));
            if (hipGetDevice(&ndev) != hipSuccess) ndev = -1;
            np = DevCache::get().take(ndev, ncap);
        }
        if (!np) {
            const auto t_alloc = std::chrono::steady_clock::now();
            hipError_t e = hipMalloc(&np, ncap);
            alloc_seconds() += std::chrono::duration<double>(std::chrono::steady_clock::now() - t_alloc).count();
            alloc_calls()++;
            if (e != hipSuccess) return e;
        }
        hipError_t e = hipSuccess;
        const bool kept = keep && p && cap;
        if (kept) {
            e = hipMemcpyAsync(np, p, std::min(cap, ncap), hipMemcpyDeviceToDevice, s);
            if (e == hipSuccess) e = hipStreamSynchronize(s);
        }
        if (e == hipSuccess && Poison::get().on) {           // (TKSMSEQ_POISON: what the caller has not been given to keep)
            size_t lo, hi;
            Poison::range(cap, ncap, kept, &lo, &hi);
            e = Poison::get().fill_device(np, lo, hi);
        }
        if (e != hipSuccess) { if (pooled) DevCache::get().give(ndev, np, ncap); else (void)hipFree(np); return e; }
        const bool was_owned = owned;
        if (was_owned) release(); else { p = nullptr; cap = 0; }
        p = np; cap = ncap; owned = true; dev = ndev;
        return hipSuccess;
    }
    template <class T> T* as() const { return (T*)p; }
};

// a temporary of one call: from DevCache, and back to it once the stream the call works on has drained
struct TmpBuf : DevBuf {
    explicit TmpBuf(hipStream_t s) { pooled = true; pool_stream = s; }
};

// page-locked host memory that grows (with as much again as headroom) and goes with its owner
struct PinnedBuf {
    void* p = nullptr;
    size_t cap = 0;
    hipError_t ensure(size_t bytes) {
        if (bytes <= cap) return hipSuccess;
        release();
        const hipError_t e = hipHostMalloc(&p, bytes * 2, hipHostMallocDefault);
        if (e != hipSuccess) { p = nullptr; return e; }
        cap = bytes * 2;
        if (Poison::get().on) Poison::get().fill_host(p, cap);
        return hipSuccess;
    }
    void release() { if (p) (void)hipHostFree(p); p = nullptr; cap = 0; }
    ~PinnedBuf() { release(); }
    template <class T> T* as() const { return (T*)p; }
};

// A stream for work that runs underneath a context's main stream, with the two events that order it against the main stream; created
// on first use.  fork_from(main): what is launched on `stream` next starts after everything queued on main so far; launched(): marks
// the end of that work; join_into(main): main waits for it.  `used`: set by launched(), cleared by whoever starts a new run.
struct HelperStream {
    hipStream_t stream = nullptr;
    hipEvent_t start = nullptr, done = nullptr;
    bool used = false;
    hipError_t fork_from(hipStream_t main) {
        hipError_t e = stream ? hipSuccess : hipStreamCreateWithFlags(&stream, hipStreamNonBlocking);
        for (hipEvent_t* ev : {&start, &done}) if (e == hipSuccess && !*ev) e = hipEventCreateWithFlags(ev, hipEventDisableTiming);
        if (e == hipSuccess) e = hipEventRecord(start, main);
        if (e == hipSuccess) e = hipStreamWaitEvent(stream, start, 0);
        return e;
    }
    hipError_t launched() { const hipError_t e = hipEventRecord(done, stream); used = used || e == hipSuccess; return e; }
    hipError_t wait_done() { return hipEventSynchronize(done); }              // the host waits for the work marked by launched()
    hipError_t join_into(hipStream_t main) { return hipStreamWaitEvent(main, done, 0); }
    bool idle() const { return !used || hipEventQuery(done) == hipSuccess; }
    hipError_t synchronize() { return stream ? hipStreamSynchronize(stream) : hipSuccess; }
    ~HelperStream() {
        if (stream) { (void)hipStreamSynchronize(stream); (void)hipStreamDestroy(stream); }
        for (hipEvent_t ev : {start, done}) if (ev) (void)hipEventDestroy(ev);
    }
};

// positions in tksmseq_ctx::last_diag (tksmseq_run_diagnostics): the order in which Sequencer.run_diagnostics (sequence.py) names them
enum RunDiag {
    DIAG_ROUNDS, DIAG_EXACT_KERNEL_READS, DIAG_PREDICTED_STRAGGLERS, DIAG_JOBS_14_ROW_ROUNDS, DIAG_JOBS_REDONE_FULL_WIDTH, DIAG_FALLBACKS,
    DIAG_FALLBACK_REASONS, DIAG_FALLBACKS_QSCORE_JOBS, DIAG_FALLBACKS_LIST_PASS, DIAG_JOBS_ALL_ROUNDS, DIAG_BAND_EXITS,
    DIAG_WORDS = 16
};

struct tksmseq_batch {
    uint64_t n_reads = 0, n_intervals = 0, n_mods = 0, n_literals = 0;
    DevBuf reads, intervals, mods, literals, litpool, ids, idpool;
    tksmseq_batch() { for (DevBuf* b : {&reads, &intervals, &mods, &literals, &litpool, &ids, &idpool, &d_dup, &d_order, &d_tail}) b->pooled = true; }
    // what PCR / truncation / the MDF writer need beyond Seq (batches parsed from MDF text only)
    std::vector<uint32_t> h_dup;         // [n_reads] bit 31: copy of a depth > 1 molecule, low bits: its index (unroll naming)
    DevBuf d_dup;
    std::vector<uint32_t> h_comments;    // [n_reads][2] header comment of every read's molecule
    std::vector<char> h_comment_pool;
    std::vector<uint32_t> raw_len;       // host copy, for sizing
    std::vector<uint32_t> order;         // reads sorted by raw length (bucketed k_err launches)
    DevBuf d_order;
    uint32_t max_raw = 0;
    uint64_t total_raw = 0;
    // tail noise: raw_len / max_raw / order describe splice + tail while a tail model applies to the run
    std::vector<uint32_t> splice_len;    // the spliced lengths (filled the first time a tail is added)
    DevBuf d_tail;                       // [n_reads] tail lengths of the run keyed below
    bool tail_on = false;
    uint64_t tail_key[4] = {};           // seed, first read index, stride, model version
    // cached scratch sizing, keyed by (k, cap_num, cap_den, cap_add)
    int cache_k = -1, cache_num = 0, cache_den = 0, cache_add = 0;
    uint64_t cache_scratch = 0;
};

struct tksmseq_ctx : ContigLookup {
    int device = 0;
    int n_cus = 256;
    hipStream_t stream = nullptr;
    // wave-wide kernel for the reads that cannot take the fast pipeline, underneath the rounds: a few streams, each with
    // its own slice of the per-wave trace buffer, so that launches for reads found in different rounds overlap
    static constexpr int N_SIDE = 4, SIDE_WAVES = 512;
    HelperStream side[N_SIDE];
    // predicted stragglers: their straggler-kernel launch runs on a stream of its own from round 0 on (run.cpp)
    HelperStream early;
    uint32_t early_tail = 1024;           // at most this many reads (and only from a batch with a long tail of predicted visits); 0: never
    DevBuf f_early;
    bool own_stream = false;
    std::string err;

    // reference
    std::vector<std::string> contig_names;
    std::unordered_map<std::string, int> contig_index;
    std::vector<uint64_t> contigs;        // {gstart, len}
    uint64_t total_alloc = 0;             // bases allocated in the global coordinate (block aligned)
    uint64_t total_bases = 0;
    uint32_t pool_blocks = 0;
    // contigs declared by name and length only (tksmseq_reference_declare_contig): tksmseq_run refuses while there are any
    std::vector<uint8_t> contig_declared; uint32_t n_declared = 0;
    // random-wgs: the contig table as its kernels read it (running sums, names), rebuilt when the reference has changed
    uint64_t ref_version = 0, wgs_version = ~0ull;
    DevBuf d_wgs_sofar, d_wgs_nameoff, d_wgs_namelen, d_wgs_names;
    DevBuf d_packed, d_blocktab, d_pool, d_contigs, d_stage;
    // transcribe: the transcript table (host; shared with clones and plans, replaced -- never changed -- by tksmseq_transcripts_add_gtf) and
    // its device form: exon tuples in the interval layout of a batch, contigs resolved against THIS context's reference (a name it does not
    // know is a literal of every output batch), rebuilt when the table or the reference has changed
    std::shared_ptr<const tsb::Transcripts> tsb;
    uint64_t tsb_dev_serial = 0, tsb_ref_version = ~0ull;      // (serial 0: no device form yet)
    DevBuf d_tsb_first, d_tsb_exons, d_tsb_lits, d_tsb_litpool;
    uint64_t tsb_n_lits = 0, tsb_lit_bytes = 0;
    float tsb_plan_ms = 0.f, tsb_write_ms = 0.f;          // device time of the last plan / tksmseq_transcribe by HIP events (tksmseq_set_timing)
    // mutate: the device form of the variant table used last (tk::MutView), the context's contigs resolved against the table's names;
    // rebuilt when another table comes or the reference has changed
    uint64_t mut_serial = 0, mut_ref_version = ~0ull;         // (serial 0: no device form yet)
    DevBuf d_mut_refctg, d_mut_nameoff, d_mut_names, d_mut_delfirst, d_mut_ptfirst, d_mut_delfrom, d_mut_delto, d_mut_ptpos, d_mut_ptinfo, d_mut_insent, d_mut_inspool;

    // models
    ErrorModelHost em; QScoreModelHost qm; IdentityHost idm;
    bool em_uniform = false, em_alt0 = false;
    TailModelHost tail; uint64_t tail_version = 0;
    DevBuf d_tail_lx, d_tail_ly, d_tail_cdf, d_tail_chain;
    DevBuf d_pself, d_pseg, d_pt0, d_pt0b, d_cdf32, d_cdf, d_alts, d_altenc, d_nalts, d_qkeys, d_qoff, d_qcnt, d_qcdf, d_qq, d_qtab, d_qent, d_qpairs, d_qguide;

    // per-run work buffers
    DevBuf w_rawlen, w_slotcap, w_slotoff, w_outlen, w_ident, w_reclen, w_recoff, w_status, w_scan, w_trace, w_counter,
        w_scratch, w_records, w_istats, w_dstats, w_sums, w_fullpool, w_biglist, w_bigscratch, w_bigtrace;
    unsigned long long full_pool_bytes = 1ull << 30;
    // fast Badread pipeline state (see kernels.h FastBuffers)
    DevBuf f_state, f_nb, f_fplanes, f_jmeta[2], f_redo, f_jpopd, f_trace, f_tracefull, f_slow, f_defer, f_defercnt, f_frag2, f_row64;
    std::vector<uint32_t> h_row64;        // host copy of the state-row offsets of the current run
    // what the host and the device exchange in every round, in one copy each way: f_round = {job counts of the even rounds,
    // counters, job counts of the odd rounds} -> h_round; h_geo = {prefix, bases, range geometry} -> f_geoall (page-locked)
    DevBuf f_round, f_geoall;
    PinnedBuf h_round, h_geo;
    bool force_slow = false;
    uint32_t tail_cut = 0;   // > 0: hand the last reads of a batch to the wave-wide kernel (diagnostic)
    int tail_wcap = 2048;                 // columns of a re-estimation window the straggler kernel aligns itself (its LDS holds 2048; smaller: tests)
    uint32_t tail_wave = 4096;            // rounds with at most this many reads left: one launch that runs every remaining visit of a read on a wave of its own (k_loopw<true>); 0: never
    uint32_t wave_loop = 16384;           // rounds with at most this many reads left run the error loop one wave per read (k_loopw)
    uint32_t full_rows_cap = 0;           // diagnostic: the full-width pass sees at most this many pool rows (0: all of them); what does not fit is handed to the exact kernel
    uint32_t small_aln = 131072;          // rounds with at most this many alignment jobs are latency-bound: every job with all 64 rows in one launch
    uint32_t n_buckets = 16;
    int defer_len = 0;          // reads longer than this align for their q-scores after the regular rounds, all together
    int hbm_state_len = 2304;   // fragments longer than this are edited in HBM instead of being staged in LDS every round
    std::vector<hipEvent_t> evpool;
    uint32_t last_diag[DIAG_WORDS] = {};  // tksmseq_run_diagnostics, indexed by RunDiag
    void* user_out = nullptr; uint64_t user_out_cap = 0;
    bool timing = false;
    int host_threads = 1;       // host threads for MDF parsing (tksmseq_set_host_threads)
    hipEvent_t ev[6] = {};
    tksmseq_result last{};
    bool have_last = false, have_stats = false;
    // device-side BGZF (gzip_api.cpp): per-chunk tables, and the compressed stream of the last gzip call (from DevCache: its size changes
    // with every batch)
    DevBuf g_counts, g_nlscan, g_sizes, g_offs, g_plans, g_out;
    tksmseq_gzip_result last_gzip{};
    bool have_gzip = false, last_fastq = false;   // last_fastq: the record format of `last`

    int find(const std::string& name) const override {
        auto it = contig_index.find(name);
        return it == contig_index.end() ? -1 : it->second;
    }
    ~tksmseq_ctx() { if (Poison::get().on) Poison::get().report(); }
};

// the permutation that orders n keys (stable; sort: abund_sort_u32 / abund_sort_u64 over bits [0, end_bit)), and the sorted keys; queued on
// the context's stream (abundance; shuffle)
template <class K, class Sort>
int sort_pairs(tksmseq_ctx* ctx, Sort sort, const K* keys, K* keys_sorted, uint32_t* perm, uint32_t n, int end_bit) {
    hipStream_t s = ctx->stream;
    TmpBuf d_iota(s), d_temp(s);
    HIPCHK(ctx, d_iota.ensure((size_t)n * 4));
    HIPCHK(ctx, tk::launch_abund_iota(d_iota.as<uint32_t>(), n, s));
    size_t bytes = 0;
    HIPCHK(ctx, sort(nullptr, &bytes, keys, keys_sorted, d_iota.as<uint32_t>(), perm, n, end_bit, s));
    HIPCHK(ctx, d_temp.ensure(bytes + 256));
    HIPCHK(ctx, sort(d_temp.p, &bytes, keys, keys_sorted, d_iota.as<uint32_t>(), perm, n, end_bit, s));
    return TKSMSEQ_OK;
}

// a batch whose tables were written on the device (PCR, truncation): lengths, sorted order and sizing on the host
int finalize_device_batch(tksmseq_ctx* ctx, tksmseq_batch* b);

// the message tksmseq_last_error(NULL) gives on the calling thread (api.cpp): for calls that fail without a context
void set_contextless_error(const std::string& e);

// TKSMSEQ_VERBOSE: 0 when unset, otherwise at least 1
inline int verbose_level() { const char* v = getenv("TKSMSEQ_VERBOSE"); return v ? std::max(1, atoi(v)) : 0; }
