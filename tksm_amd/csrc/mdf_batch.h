// mdf_batch.h -- internal: what the host sides of the molecule transforms share (mdf_ops.cpp: molecules edited; mdf_move.cpp: whole
// molecules moved; mdf_make.cpp: molecules made; mdf_text.cpp: the comment grammar and the MDF writer): views of a batch for the kernels,
// the scan, host copies of a batch's tables, header comments, and the builder of an output batch (MolPlacement, OutBatch).
#pragma once
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "ctx.h"
#include "mdf_kernels.h"

// the device's Philox on the host: the keys of PCR's subsample, the draw of tksmseq_glue_joins
struct Ph4h { uint32_t x, y, z, w; };
inline Ph4h philox_host(uint64_t seed, uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3) {
    uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
    for (int r = 0; r < 10; r++) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c0 = n0; c1 = (uint32_t)p1; c2 = n2; c3 = (uint32_t)p0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    return Ph4h{c0, c1, c2, c3};
}

inline tk::BatchView view_of(const tksmseq_batch* b) {
    return tk::BatchView{b->reads.as<uint32_t>(), b->intervals.as<uint32_t>(), b->mods.as<uint32_t>(), b->literals.as<uint64_t>(),
                         b->litpool.as<uint8_t>(), b->ids.as<uint32_t>(), b->idpool.as<uint8_t>(), b->n_reads, (uint32_t)b->n_literals};
}

// every (unrolled) molecule of a batch, or the n_kept of them that `keep` lists (a device array)
inline tk::MolView mol_view(const tksmseq_batch* in, const uint32_t* keep, uint64_t n_kept) {
    return tk::MolView{view_of(in), in->d_dup.p ? in->d_dup.as<uint32_t>() : nullptr, in->n_intervals, in->n_mods, keep, n_kept};
}
inline tk::MolView mol_view(const tksmseq_batch* in) { return mol_view(in, nullptr, in->n_reads); }

// exclusive scan of in[0, n) into out[0, n], queued; the total is out[n], *total once the stream has drained
inline int scan_async(tksmseq_ctx* ctx, DevBuf& in, DevBuf& out, uint64_t n, uint64_t* total) {
    HIPCHK(ctx, out.ensure((n + 1) * 8 + 16));
    HIPCHK(ctx, ctx->w_scan.ensure(tk::scan_temp_bytes(n) + 64));
    HIPCHK(ctx, tk::launch_scan(in.as<uint64_t>(), out.as<uint64_t>(), n, ctx->w_scan.p, ctx->w_scan.cap, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(total, out.as<uint64_t>() + n, 8, hipMemcpyDeviceToHost, ctx->stream));
    return TKSMSEQ_OK;
}
inline int scan_to(tksmseq_ctx* ctx, DevBuf& in, DevBuf& out, uint64_t n, uint64_t* total) {
    const int rc = scan_async(ctx, in, out, n, total);
    if (rc) return rc;
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return TKSMSEQ_OK;
}

// `bytes` of host memory into d (sized for them, with some slack), queued; src must live until the stream has drained
inline int upload(tksmseq_ctx* ctx, DevBuf& d, const void* src, size_t bytes) {
    HIPCHK(ctx, d.ensure(bytes + 64));
    if (bytes) HIPCHK(ctx, hipMemcpyAsync(d.p, src, bytes, hipMemcpyHostToDevice, ctx->stream));
    return TKSMSEQ_OK;
}

// ---- header comments (mdf_text.cpp) --------------------------------------------------------------------------------------------------
using Meta = std::map<std::string, std::vector<std::string>>;
Meta parse_meta(const char* c, size_t n);                   // "k=v1,v2;flag;" -> key -> values ("." for a bare key)
std::string dump_meta(const Meta& meta);
std::string normalize_comment(const char* c, size_t n, const std::vector<std::pair<std::string, std::string>>& extra);      // parse, append, dump
std::string fmt_double(double v);                           // fmt's "{}" of a double

// [c, c + len) goes behind b's comment pool, *off says where (CommentCopier::put below has the same check and append written out).  who / hint: for the message of the 4 GB limit
inline int comment_bytes(tksmseq_ctx* ctx, tksmseq_batch* b, const char* c, size_t len, const char* who, const char* hint, uint32_t* off) {
    if (b->h_comment_pool.size() + len >= 0xffffffffull) {
        ctx->err = std::string(who) + ": more than 4 GB of header comments in one batch (" + hint + ")";
        return TKSMSEQ_ELIMIT;
    }
    *off = (uint32_t)b->h_comment_pool.size();
    b->h_comment_pool.insert(b->h_comment_pool.end(), c, c + len);
    return TKSMSEQ_OK;
}
// one more header comment behind b's: its (offset, length) entry and its bytes
inline int append_comment(tksmseq_ctx* ctx, tksmseq_batch* b, const std::string& c, const char* who, const char* hint = "split the input") {
    uint32_t off = 0;
    const int rc = comment_bytes(ctx, b, c.data(), c.size(), who, hint, &off);
    if (rc) return rc;
    b->h_comments.push_back(off); b->h_comments.push_back((uint32_t)c.size());
    return TKSMSEQ_OK;
}

// Host copies of a batch's device tables.  fetch() copies the chosen groups and returns when the context's stream has drained (so it
// covers copies the caller has queued before it, too).
struct HostTables {
    enum { SEGMENTS = 1, MODS = 2, IDS = 4 };      // reads, intervals and literals | substitutions | ids and their pool
    std::vector<uint32_t> reads, ivs, mods, ids;
    std::vector<uint64_t> lits;
    std::vector<char> lpool, idpool;
    int fetch(tksmseq_ctx* ctx, const tksmseq_batch* b, int what) {
        hipError_t e = hipSuccess;
        auto get = [&](auto& v, const DevBuf& d, size_t count) {
            v.resize(count);
            if (count && e == hipSuccess) e = hipMemcpyAsync(v.data(), d.p, count * sizeof v[0], hipMemcpyDeviceToHost, ctx->stream);
        };
        if (what & SEGMENTS) { get(reads, b->reads, 2 * b->n_reads); get(ivs, b->intervals, 4 * (b->n_intervals + 1)); get(lits, b->literals, 2 * b->n_literals); get(lpool, b->litpool, b->litpool.cap); }
        if (what & MODS) get(mods, b->mods, 2 * b->n_mods);
        if (what & IDS) { get(ids, b->ids, 2 * b->n_reads); get(idpool, b->idpool, b->idpool.cap); }
        const hipError_t drained = hipStreamSynchronize(ctx->stream);      // (after a failed copy as well: the ones before it write into the vectors)
        if (e == hipSuccess) e = drained;
        if (e != hipSuccess) { ctx->err = std::string("copying a batch's tables to the host: ") + hipGetErrorString(e); return TKSMSEQ_EDEVICE; }
        return TKSMSEQ_OK;
    }
    // an interval's contig as the MDF text names it: the literal itself, or the reference's name
    void append_contig(const tksmseq_ctx* ctx, uint32_t c, std::string& out) const {
        if (c >> 31) { const size_t li = c & 0x7fffffffu; out.append(lpool.data() + lits[2 * li], (size_t)lits[2 * li + 1]); }
        else out += ctx->contig_names[c];
    }
};

inline void append_u32(std::string& o, uint32_t v) {      // (decimal, without an allocation: the text writer's inner loop)
    char tmp[10]; int k = 10;
    do { tmp[--k] = (char)('0' + v % 10u); v /= 10u; } while (v);
    o.append(tmp + k, (size_t)(10 - k));
}
// the id of molecule r of b as the writer prints it: a copy of a depth > 1 molecule carries its index (id_0, id_1, ...: src/mdf.h:97-105).
// H: b's tables with IDS fetched
inline void append_written_id(const HostTables& H, const tksmseq_batch* b, uint64_t r, std::string& out) {
    out.append(H.idpool.data() + H.ids[2 * r], H.ids[2 * r + 1]);
    if (!b->h_dup.empty() && (b->h_dup[r] >> 31)) { out += '_'; append_u32(out, b->h_dup[r] & 0x7fffffffu); }
}
inline std::string written_id(const HostTables& H, const tksmseq_batch* b, uint64_t r) { std::string id; append_written_id(H, b, r, id); return id; }

// ---- the output batch of a transform ---------------------------------------------------------------------------------------------
// What the transforms share: scan the per-molecule counts, check the size limits, allocate the five tables, and -- after the caller's
// write kernels -- write the sentinel interval, finalize and hand the batch over.
// The rule for device memory: nothing goes back to DevCache while work queued on the context's stream may still touch it.  A TmpBuf
// drains the stream itself when it lets go; the tables of the batch under construction carry no stream, so the destructor here drains
// before they go, on every exit that has not handed the batch over.  Neither depends on the order in which a caller declares them.

// Where the molecules of one output (of one input, for concat) go: per molecule its three counts, which a count kernel writes; their
// exclusive scans, which a write kernel reads; and the three totals.  All six arrays are TmpBufs of the context's stream.
struct MolPlacement {
    tksmseq_ctx* ctx;
    TmpBuf n_ivl, n_mod, n_id, o_ivl, o_mod, o_id;
    uint64_t t_ivl = 0, t_mod = 0, t_id = 0;       // (there once the stream has drained after scan())
    explicit MolPlacement(tksmseq_ctx* c)
        : ctx(c), n_ivl(c->stream), n_mod(c->stream), n_id(c->stream), o_ivl(c->stream), o_mod(c->stream), o_id(c->stream) {}
    // room for the counts of n molecules
    int counts(uint64_t n, tk::MolCounts& c) {
        for (DevBuf* x : {(DevBuf*)&n_ivl, (DevBuf*)&n_mod, (DevBuf*)&n_id}) HIPCHK(ctx, x->ensure(n * 8 + 16));
        c = tk::MolCounts{n_ivl.as<uint64_t>(), n_mod.as<uint64_t>(), n_id.as<uint64_t>()};
        return TKSMSEQ_OK;
    }
    // counts -> offsets and totals, queued: whoever calls drains the stream before reading a total
    int scan(uint64_t n) {
        int rc;
        if ((rc = scan_async(ctx, n_ivl, o_ivl, n, &t_ivl)) || (rc = scan_async(ctx, n_mod, o_mod, n, &t_mod))) return rc;
        return scan_async(ctx, n_id, o_id, n, &t_id);
    }
    tk::MolOffsets offsets() const { return tk::MolOffsets{o_ivl.as<uint64_t>(), o_mod.as<uint64_t>(), o_id.as<uint64_t>()}; }
};

struct OutBatch {
    tksmseq_ctx* ctx;
    std::unique_ptr<tksmseq_batch> b{new tksmseq_batch()};
    MolPlacement at;                                // where every molecule's intervals, substitutions and id bytes start, and how many there are
    uint32_t sentinel[4] = {0u, 0u, 0u, 0u};        // (lives as long as its queued copy may)
    explicit OutBatch(tksmseq_ctx* c) : ctx(c), at(c) {}
    ~OutBatch() { if (b) (void)hipStreamSynchronize(ctx->stream); }
    tksmseq_batch* get() const { return b.get(); }
    tksmseq_batch* operator->() const { return b.get(); }
    tk::MolOut tables() const { return tk::MolOut{b->reads.as<uint32_t>(), b->intervals.as<uint32_t>(), b->mods.as<uint32_t>(), b->ids.as<uint32_t>(), b->idpool.as<uint8_t>()}; }

    // Literals (contigs whose name is their sequence) are shared by reference, so the batch gets its own table: the entries and the pool of
    // `in` (the pool copied whole, its capacity; in null: none), then room for n_new entries and new_bytes pool bytes behind them, which
    // start at lit_base / pool_base.
    uint32_t lit_base = 0; uint64_t pool_base = 0;
    int literals(const tksmseq_batch* in, uint64_t n_new = 0, uint64_t new_bytes = 0) {
        lit_base = in ? (uint32_t)in->n_literals : 0u; pool_base = in ? in->litpool.cap : 0;
        if (lit_base + n_new >= 0x80000000ull) { ctx->err = "more than 2^31 literals in one batch (split the input)"; return TKSMSEQ_ELIMIT; }
        b->n_literals = lit_base + n_new;
        HIPCHK(ctx, b->literals.ensure(b->n_literals * 16 + 64));
        HIPCHK(ctx, b->litpool.ensure(pool_base + new_bytes + 64));
        if (lit_base) HIPCHK(ctx, hipMemcpyAsync(b->literals.p, in->literals.p, lit_base * 16ull, hipMemcpyDeviceToDevice, ctx->stream));
        if (pool_base) HIPCHK(ctx, hipMemcpyAsync(b->litpool.p, in->litpool.p, pool_base, hipMemcpyDeviceToDevice, ctx->stream));
        return TKSMSEQ_OK;
    }
    // The usual sequence: counts(n_in) for the count kernel, place(n_in, n_out, ...) -- scans, ONE synchronisation, limits, tables -- and
    // offsets() for the write kernel.  A caller whose n_out itself comes out of a scan (filter, glue) queues scan(n_in) with its own, drains
    // the stream once for all of them and calls alloc(n_out, ...).
    int counts(uint64_t n_in, tk::MolCounts& c) { return at.counts(n_in, c); }
    int scan(uint64_t n_in) { return at.scan(n_in); }
    tk::MolOffsets offsets() const { return at.offsets(); }
    int place(uint64_t n_in, uint64_t n_out, const char* who, const char* hint = "split the input") {
        const int rc = at.scan(n_in);
        if (rc) return rc;
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        return alloc(n_out, who, hint);
    }
    // ... and for a caller that knows the totals already (random-wgs, transcribe, concat): no scan, no synchronisation
    int place_known(uint64_t n_out, uint64_t t_ivl, uint64_t t_mod, uint64_t t_id, const char* who, const char* hint) {
        at.t_ivl = t_ivl; at.t_mod = t_mod; at.t_id = t_id;
        return alloc(n_out, who, hint);
    }
    // The size limits of a batch: read, interval and id offsets are 32-bit, and an interval keeps its strand in bit 31 of its substitution
    // index.  who: the caller's prefix of the message.
    int limits(uint64_t n, const char* who, const char* hint) {
        if (n >= 0xffffffffull) { ctx->err = std::string(who) + "more than 2^32 output molecules in one call"; return TKSMSEQ_ELIMIT; }
        if (at.t_ivl >= 0x7fffffffull || at.t_mod >= 0x7fffffffull || at.t_id >= 0xffffffffull) { ctx->err = std::string(who) + "output batch too large (" + hint + ")"; return TKSMSEQ_ELIMIT; }
        return TKSMSEQ_OK;
    }
    // the tables of n molecules with the placement's totals: its intervals (and the sentinel behind them), substitutions and id bytes
    int alloc(uint64_t n, const char* who, const char* hint = "split the input") {
        const int rc = limits(n, who, hint);
        if (rc) return rc;
        b->n_reads = n; b->n_intervals = at.t_ivl; b->n_mods = at.t_mod;
        HIPCHK(ctx, b->reads.ensure(n * 8 + 64));
        HIPCHK(ctx, b->intervals.ensure((at.t_ivl + 1) * 16 + 64));
        HIPCHK(ctx, b->mods.ensure(at.t_mod * 8 + 64));
        HIPCHK(ctx, b->ids.ensure(n * 8 + 64));
        HIPCHK(ctx, b->idpool.ensure(at.t_id + 64));
        return TKSMSEQ_OK;
    }
    // after the write kernels: the interval behind the last carries n_mods; lengths, order and sizing; *out owns the batch from here
    int finish(tksmseq_batch** out) {
        sentinel[3] = (uint32_t)at.t_mod;
        HIPCHK(ctx, hipMemcpyAsync(b->intervals.as<uint32_t>() + 4 * at.t_ivl, sentinel, 16, hipMemcpyHostToDevice, ctx->stream));
        const int rc = finalize_device_batch(ctx, b.get());
        if (rc) return rc;
        *out = b.release();
        return TKSMSEQ_OK;
    }
};

// the header comments of one side of a partition, or of one input of a concatenation: entry (off, len) of `in`'s pool goes behind b's;
// the copies of a record, which follow one another and share an entry, share the new one too
struct CommentCopier {
    uint32_t last_off = 0, last_len = 0, last_new = 0; bool any = false;
    int put(tksmseq_ctx* ctx, tksmseq_batch* b, const tksmseq_batch* in, uint64_t r, const char* who) {
        const uint32_t off = in->h_comments[2 * r], len = in->h_comments[2 * r + 1];
        if (any && off == last_off && len == last_len) { b->h_comments.push_back(last_new); b->h_comments.push_back(len); return TKSMSEQ_OK; }
        // (the check and the append of comment_bytes, written out: going through it made merge, glue and shuffle of a million molecules
        // with a comment each 4 - 9 % slower, profiles/mdf_split_times.log)
        if (b->h_comment_pool.size() + len >= 0xffffffffull) { ctx->err = std::string(who) + ": more than 4 GB of header comments in one batch (split the input)"; return TKSMSEQ_ELIMIT; }
        any = true; last_off = off; last_len = len; last_new = (uint32_t)b->h_comment_pool.size();
        b->h_comments.push_back(last_new); b->h_comments.push_back(len);
        b->h_comment_pool.insert(b->h_comment_pool.end(), in->h_comment_pool.begin() + off, in->h_comment_pool.begin() + off + len);
        return TKSMSEQ_OK;
    }
};
// the comments of n_out more molecules of b: output molecule j gets the entry of molecule source_index(j) of `in`
template <class F>
int gather_comments(OutBatch& b, const tksmseq_batch* in, const char* who, uint64_t n_out, F source_index) {
    b->h_comments.reserve(b->h_comments.size() + 2 * n_out);
    CommentCopier cc;
    for (uint64_t j = 0; j < n_out; j++) {
        const int rc = cc.put(b.ctx, b.get(), in, source_index(j), who);
        if (rc) return rc;
    }
    return TKSMSEQ_OK;
}
