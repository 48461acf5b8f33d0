// mdf_ops.cpp -- host side of the molecule-description transforms upstream of Seq (BASELINE config 5) and of the MDF writer:
//   tksmseq_pcr            src/pcr.cpp:22-89, :138 (presets), :215-229 (whole input in memory, at most 2 x target templates)
//   tksmseq_truncate       src/truncate.cpp:23-65, :77-227, :322-351, :362-404
//   tksmseq_polya / _tag / _scb / _flip   src/polyA.cpp:133-148, src/tag.cpp:70-113, src/scb.cpp:57-80, src/interval.h:908-920
//   tksmseq_filter / _concat   src/filter.cpp:21-117, :196-212 (a two-way partition); Mrg = `cat` of MDF files (batches joined)
//   tksmseq_glue / _shuffle    src/unsegment.cpp:88-105 (chains of glued molecules), src/shuffle.cpp:23-44 (the buffer as two sorts and a gather)
//   tksmseq_wgs            src/random_wgs.cpp:181-207 (no input: the molecules are made on the device)
//   tksmseq_append_noise   src/append_noise.cpp:83-128 (tail-noise: a random literal or a hairpin behind every molecule)
//   tksmseq_transcribe     src/transcribe.cpp:170-197 (no input batch: abundance rows x the context's transcript table)
//   tksmseq_mutate         a variant table applied to every segment (the table format of src/mutate.cpp:157-181; the transform is this build's own)
//   tksmseq_batch_to_mdf_text   molecule_descriptor::operator<<, src/interval.h:898-905 (+ dump_comment :880-890)
// The molecule tables stay on the device from one transform to the next and into tksmseq_run; only sizes, per-read lengths
// (which the host needs to size and order a Seq batch) and, for the text writer, the tables themselves come back.
#include <atomic>
#include <charconv>
#include <cmath>
#include <cstring>
#include <map>
#include <memory>
#include <unordered_map>

#include "ctx.h"
#include <thread>
#include "filter_host.h"
#include "mdf_kernels.h"
#include "mut_host.h"

namespace {

struct Ph4h { uint32_t x, y, z, w; };
Ph4h philox_host(uint64_t seed, uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3) {
    uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
    for (int r = 0; r < 10; r++) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c0 = n0; c1 = (uint32_t)p1; c2 = n2; c3 = (uint32_t)p0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    return Ph4h{c0, c1, c2, c3};
}

tk::BatchView view_of(const tksmseq_batch* b) {
    return tk::BatchView{b->reads.as<uint32_t>(), b->intervals.as<uint32_t>(), b->mods.as<uint32_t>(), b->literals.as<uint64_t>(),
                         b->litpool.as<uint8_t>(), b->ids.as<uint32_t>(), b->idpool.as<uint8_t>(), b->n_reads, (uint32_t)b->n_literals};
}

// every (unrolled) molecule of a batch, or the n_kept of them that `keep` lists (a device array)
tk::MolView mol_view(const tksmseq_batch* in, const uint32_t* keep, uint64_t n_kept) {
    return tk::MolView{view_of(in), in->d_dup.p ? in->d_dup.as<uint32_t>() : nullptr, in->n_intervals, in->n_mods, keep, n_kept};
}
tk::MolView mol_view(const tksmseq_batch* in) { return mol_view(in, nullptr, in->n_reads); }

// exclusive scan of in[0, n) into out[0, n], queued; the total is out[n], *total once the stream has drained
int scan_async(tksmseq_ctx* ctx, DevBuf& in, DevBuf& out, uint64_t n, uint64_t* total) {
    HIPCHK(ctx, out.ensure((n + 1) * 8 + 16));
    HIPCHK(ctx, ctx->w_scan.ensure(tk::scan_temp_bytes(n) + 64));
    HIPCHK(ctx, tk::launch_scan(in.as<uint64_t>(), out.as<uint64_t>(), n, ctx->w_scan.p, ctx->w_scan.cap, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(total, out.as<uint64_t>() + n, 8, hipMemcpyDeviceToHost, ctx->stream));
    return TKSMSEQ_OK;
}
int scan_to(tksmseq_ctx* ctx, DevBuf& in, DevBuf& out, uint64_t n, uint64_t* total) {
    const int rc = scan_async(ctx, in, out, n, total);
    if (rc) return rc;
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return TKSMSEQ_OK;
}

using Meta = std::map<std::string, std::vector<std::string>>;

// molecule_descriptor::comment (src/interval.h:809-830): "k=v1,v2;flag;" -> key -> values ("." for a bare key)
Meta parse_meta(const char* c, size_t n) {
    Meta meta;
    size_t a = 0;
    while (a < n) {
        size_t b = a;
        while (b < n && c[b] != ';') b++;
        if (b > a) {
            const std::string f(c + a, b - a);
            const size_t eq = f.find('=');
            if (eq == std::string::npos) meta[f].push_back(".");
            else {
                size_t k1 = f.find_first_not_of('='), k2 = f.find('=', k1 == std::string::npos ? 0 : k1);
                const std::string key = k1 == std::string::npos ? std::string() : f.substr(k1, k2 - k1);
                size_t v = k2 == std::string::npos ? f.size() : k2;
                while (v < f.size() && f[v] == '=') v++;
                size_t ve = f.find('=', v);
                const std::string vals = f.substr(v, ve == std::string::npos ? std::string::npos : ve - v);
                size_t p = 0;
                while (p < vals.size()) {
                    size_t q = vals.find(',', p);
                    if (q == std::string::npos) q = vals.size();
                    if (q > p) meta[key].push_back(vals.substr(p, q - p));
                    p = q + 1;
                }
            }
        }
        a = b + 1;
    }
    return meta;
}

// dump_comment (src/interval.h:880-890)
std::string dump_meta(const Meta& meta) {
    std::string out;
    for (auto& kv : meta) {
        if (kv.second.empty()) continue;
        out += kv.first;
        if (kv.second[0] != ".") {
            out += '=';
            for (size_t i = 0; i < kv.second.size(); i++) { if (i) out += ','; out += kv.second[i]; }
        }
        out += ';';
    }
    return out;
}

// std::map<string, vector<string>> round trip of a header comment (molecule_descriptor::comment / dump_comment,
// src/interval.h:809-830, :880-890), with extra values appended
std::string normalize_comment(const char* c, size_t n, const std::vector<std::pair<std::string, std::string>>& extra) {
    Meta meta = parse_meta(c, n);
    for (auto& kv : extra) meta[kv.first].push_back(kv.second);
    return dump_meta(meta);
}

// fmt's "{}" of a double: the shortest digits that round-trip, in FIXED notation while the decimal exponent is in [-4, 16) and in
// exponent notation outside (like Python's repr; std::to_chars alone would switch to "1e+05" as soon as that is shorter)
std::string fmt_double(double v) {
    char buf[64];
    auto r = std::to_chars(buf, buf + sizeof buf, v, std::chars_format::scientific);
    std::string sci(buf, r.ptr);                          // d[.ddd]e[+-]XX: read the exponent off it
    const size_t e = sci.find('e');
    const int ex = e == std::string::npos ? 0 : atoi(sci.c_str() + e + 1);
    if (!std::isfinite(v) || ex < -4 || ex >= 16) {
        r = std::to_chars(buf, buf + sizeof buf, v);
        return std::string(buf, r.ptr);
    }
    r = std::to_chars(buf, buf + sizeof buf, v, std::chars_format::fixed);
    return std::string(buf, r.ptr);
}

// one more header comment behind b's: its (offset, length) entry and its bytes.  who / hint: for the message of the 4 GB limit
int append_comment(tksmseq_ctx* ctx, tksmseq_batch* b, const std::string& c, const char* who, const char* hint = "split the input") {
    if (b->h_comment_pool.size() + c.size() >= 0xffffffffull) {
        ctx->err = std::string(who) + ": more than 4 GB of header comments in one batch (" + hint + ")";
        return TKSMSEQ_ELIMIT;
    }
    b->h_comments.push_back((uint32_t)b->h_comment_pool.size()); b->h_comments.push_back((uint32_t)c.size());
    b->h_comment_pool.insert(b->h_comment_pool.end(), c.begin(), c.end());
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

// ---- the output batch of a transform ---------------------------------------------------------------------------------------------
// What pcr, truncate, the segment edits and random-wgs share: scan the per-molecule counts, check the size limits, allocate the five
// tables, and -- after the caller's write kernels -- write the sentinel interval, finalize and hand the batch over.
// The rule for device memory: nothing goes back to DevCache while work queued on the context's stream may still touch it.  A TmpBuf
// drains the stream itself when it lets go; the tables of the batch under construction carry no stream, so the destructor here drains
// before they go, on every exit that has not handed the batch over.  Neither depends on the order in which a caller declares them.
struct OutBatch {
    tksmseq_ctx* ctx;
    std::unique_ptr<tksmseq_batch> b{new tksmseq_batch()};
    TmpBuf o_ivl, o_mod, o_id;                      // where every molecule's intervals, substitutions and id bytes start (scan())
    uint64_t t_ivl = 0, t_mod = 0, t_id = 0;        // ... and how many there are in all
    uint32_t sentinel[4] = {0u, 0u, 0u, 0u};        // (lives as long as its queued copy may)
    explicit OutBatch(tksmseq_ctx* c) : ctx(c), o_ivl(c->stream), o_mod(c->stream), o_id(c->stream) {}
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
    // the three counts of each of n molecules (device arrays) -> offsets and totals; one synchronisation
    int scan(DevBuf& n_ivl, DevBuf& n_mod, DevBuf& n_idl, uint64_t n) {
        int rc;
        if ((rc = scan_async(ctx, n_ivl, o_ivl, n, &t_ivl)) || (rc = scan_async(ctx, n_mod, o_mod, n, &t_mod)) || (rc = scan_async(ctx, n_idl, o_id, n, &t_id))) return rc;
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        return TKSMSEQ_OK;
    }
    // The size limits of a batch: read, interval and id offsets are 32-bit, and an interval keeps its strand in bit 31 of its substitution
    // index.  who: the caller's prefix of the message.
    int limits(uint64_t n, const char* who, const char* hint) {
        if (n >= 0xffffffffull) { ctx->err = std::string(who) + "more than 2^32 output molecules in one call"; return TKSMSEQ_ELIMIT; }
        if (t_ivl >= 0x7fffffffull || t_mod >= 0x7fffffffull || t_id >= 0xffffffffull) { ctx->err = std::string(who) + "output batch too large (" + hint + ")"; return TKSMSEQ_ELIMIT; }
        return TKSMSEQ_OK;
    }
    // the tables of n molecules with t_ivl intervals (and the sentinel behind them), t_mod substitutions and t_id id bytes
    int alloc(uint64_t n, const char* who, const char* hint = "split the input") {
        const int rc = limits(n, who, hint);
        if (rc) return rc;
        b->n_reads = n; b->n_intervals = t_ivl; b->n_mods = t_mod;
        HIPCHK(ctx, b->reads.ensure(n * 8 + 64));
        HIPCHK(ctx, b->intervals.ensure((t_ivl + 1) * 16 + 64));
        HIPCHK(ctx, b->mods.ensure(t_mod * 8 + 64));
        HIPCHK(ctx, b->ids.ensure(n * 8 + 64));
        HIPCHK(ctx, b->idpool.ensure(t_id + 64));
        return TKSMSEQ_OK;
    }
    // after the write kernels: the interval behind the last carries n_mods; lengths, order and sizing; *out owns the batch from here
    int finish(tksmseq_batch** out) {
        sentinel[3] = (uint32_t)t_mod;
        HIPCHK(ctx, hipMemcpyAsync(b->intervals.as<uint32_t>() + 4 * t_ivl, sentinel, 16, hipMemcpyHostToDevice, ctx->stream));
        const int rc = finalize_device_batch(ctx, b.get());
        if (rc) return rc;
        *out = b.release();
        return TKSMSEQ_OK;
    }
};

}  // namespace

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
    if (!keep.empty()) { HIPCHK(ctx, d_keep.ensure(n_kept * 4 + 16)); HIPCHK(ctx, hipMemcpyAsync(d_keep.p, keep.data(), n_kept * 4, hipMemcpyHostToDevice, s)); }
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
    TmpBuf d_keep(s), d_cnt(s), d_off(s), d_status(s), n_mol(s), n_mask(s), n_ivl(s), n_mod(s), n_idl(s);
    if (!keep.empty()) { HIPCHK(ctx, d_keep.ensure(n_kept * 4 + 16)); HIPCHK(ctx, hipMemcpyAsync(d_keep.p, keep.data(), n_kept * 4, hipMemcpyHostToDevice, s)); }
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
    for (DevBuf* x : {&n_mask, &n_ivl, &n_mod, &n_idl}) HIPCHK(ctx, x->ensure(n_nodes * 8 + 16));
    HIPCHK(ctx, tk::launch_pcr_list(M, P, d_off.as<uint64_t>(), n_mol.as<uint32_t>(), n_mask.as<uint64_t>(), n_ivl.as<uint64_t>(), n_mod.as<uint64_t>(),
                                    n_idl.as<uint64_t>(), s));
    if ((rc = b.scan(n_ivl, n_mod, n_idl, n_nodes)) || (rc = b.alloc(n_nodes, "PCR: ")) || (rc = b.literals(in))) return rc;
    HIPCHK(ctx, tk::launch_pcr_write(M, P, n_nodes, n_mol.as<uint32_t>(), n_mask.as<uint64_t>(), b.o_ivl.as<uint64_t>(), b.o_mod.as<uint64_t>(),
                                     b.o_id.as<uint64_t>(), b.tables(), s));
    // comments follow the template (re-serialised the way the reference's reader / writer pair does)
    if (!in->h_comments.empty() && !(p->flags & TKSMSEQ_MOL_NO_COMMENTS)) {
        std::vector<uint32_t> mol(n_nodes);
        HIPCHK(ctx, hipMemcpyAsync(mol.data(), n_mol.p, n_nodes * 4, hipMemcpyDeviceToHost, s));
        HIPCHK(ctx, hipStreamSynchronize(s));
        b->h_comments.reserve(2 * n_nodes);
        for (uint64_t j = 0; j < n_nodes; j++) {
            const uint32_t u = mol[j];
            if (j && u == mol[j - 1]) {                                   // (a further copy of the same template: its entry again)
                const size_t k = b->h_comments.size();
                const uint32_t off = b->h_comments[k - 2], len = b->h_comments[k - 1];
                b->h_comments.push_back(off); b->h_comments.push_back(len);
            } else if ((rc = append_comment(ctx, b.get(), normalize_comment(in->h_comment_pool.data() + in->h_comments[2 * (size_t)u], in->h_comments[2 * (size_t)u + 1], {}),
                                            "PCR", "use template slices"))) return rc;
        }
    }
    return b.finish(out);
}

int tksmseq_truncate(tksmseq_ctx* ctx, const tksmseq_batch* in, const tksmseq_trc_params* p, tksmseq_batch** out) {
    if (!ctx || !in || !p || !out) return TKSMSEQ_EINVAL;
    *out = nullptr;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const uint64_t n = in->n_reads;
    tk::TrcParams T{};
    T.seed = p->seed; T.mode = p->mode; T.mu = p->mu; T.sigma = p->sigma; T.min_len = 100;      // truncate()'s default min_val
    T.always_end = p->always_end ? 1 : 0; T.models_length = p->kde_models_length ? 1 : 0;
    TmpBuf d_x(s), d_y(s), d_cdf(s), d_rn(s), d_sl(s), d_sc(s);
    TrcModelHost tm;
    auto upv = [&](DevBuf& b, const void* src, size_t bytes) -> int {
        HIPCHK(ctx, b.ensure(bytes + 64));
        if (bytes) HIPCHK(ctx, hipMemcpyAsync(b.p, src, bytes, hipMemcpyHostToDevice, s));
        return TKSMSEQ_OK;
    };
    int rc;
    if (p->mode == TKSMSEQ_TRC_KDE) {
        if (!p->kde_model_path) { ctx->err = "truncate: the KDE mode needs a model file"; return TKSMSEQ_EINVAL; }
        if (!load_trc_model(p->kde_model_path, tm, ctx->err)) return TKSMSEQ_EIO;
        if (!p->always_end && !tm.have_sider) { ctx->err = "truncate: the model has no end_mtx (use --always-end)"; return TKSMSEQ_EINVAL; }
        T.nx = (int)tm.xlab.size(); T.ny = (int)tm.ylab.size(); T.have_sider = tm.have_sider ? 1 : 0; T.ns = (int)tm.slab.size();
        if ((rc = upv(d_x, tm.xlab.data(), tm.xlab.size() * 8)) || (rc = upv(d_y, tm.ylab.data(), tm.ylab.size() * 8)) ||
            (rc = upv(d_cdf, tm.cdf.data(), tm.cdf.size() * 8)) || (rc = upv(d_rn, tm.row_n.data(), tm.row_n.size() * 4)) ||
            (rc = upv(d_sl, tm.slab.data(), tm.slab.size() * 8)) || (rc = upv(d_sc, tm.scdf.data(), tm.scdf.size() * 8))) return rc;
        T.xlab = d_x.as<long long>(); T.ylab = d_y.as<long long>(); T.cdf = d_cdf.as<double>(); T.row_n = d_rn.as<int>();
        T.slab = d_sl.as<double>(); T.scdf = d_sc.as<double>();
    } else if (p->mode != TKSMSEQ_TRC_NORMAL && p->mode != TKSMSEQ_TRC_LOGNORMAL) { ctx->err = "truncate: unknown mode"; return TKSMSEQ_EINVAL; }
    else if (!std::isfinite(p->mu) || !std::isfinite(p->sigma)) { ctx->err = "truncate: mu and sigma must be finite"; return TKSMSEQ_EINVAL; }
    const tk::MolView M = mol_view(in);
    OutBatch b(ctx);
    TmpBuf kf(s), kt(s), tl(s), ts(s), n_ivl(s), n_mod(s), n_idl(s);
    HIPCHK(ctx, kf.ensure(n * 4 + 16)); HIPCHK(ctx, kt.ensure(n * 4 + 16));
    for (DevBuf* x : {&tl, &ts, &n_ivl, &n_mod, &n_idl}) HIPCHK(ctx, x->ensure(n * 8 + 16));
    HIPCHK(ctx, tk::launch_trc_plan(M, T, p->first_molecule_index, kf.as<uint32_t>(), kt.as<uint32_t>(), tl.as<double>(), ts.as<double>(),
                                    n_ivl.as<uint64_t>(), n_mod.as<uint64_t>(), n_idl.as<uint64_t>(), s));
    // (a truncated batch is no larger than its input, so the limits cannot trip here: checked all the same, like every other output)
    if ((rc = b.scan(n_ivl, n_mod, n_idl, n)) || (rc = b.alloc(n, "truncate: ")) || (rc = b.literals(in))) return rc;
    HIPCHK(ctx, tk::launch_trc_write(M, kf.as<uint32_t>(), kt.as<uint32_t>(), b.o_ivl.as<uint64_t>(), b.o_mod.as<uint64_t>(), b.o_id.as<uint64_t>(), b.tables(), s));
    // comments: the template's, plus truncated=chr:start-end,... for what was cut away and (KDE mode) TR=<length>,<3' share>
    // (src/truncate.cpp:54-60, :343).  Needs the input tables on the host.
    if (!in->h_comments.empty() && !(p->flags & TKSMSEQ_MOL_NO_COMMENTS)) {
        HostTables H;
        std::vector<uint32_t> hkf(n), hkt(n);
        std::vector<double> htl(n), hts(n);
        HIPCHK(ctx, hipMemcpyAsync(hkf.data(), kf.p, n * 4, hipMemcpyDeviceToHost, s));
        HIPCHK(ctx, hipMemcpyAsync(hkt.data(), kt.p, n * 4, hipMemcpyDeviceToHost, s));
        HIPCHK(ctx, hipMemcpyAsync(htl.data(), tl.p, n * 8, hipMemcpyDeviceToHost, s));
        HIPCHK(ctx, hipMemcpyAsync(hts.data(), ts.p, n * 8, hipMemcpyDeviceToHost, s));
        if ((rc = H.fetch(ctx, in, HostTables::SEGMENTS))) return rc;          // (drains the stream: the four copies above as well)
        const auto &reads = H.reads, &ivs = H.ivs;
        auto chr_of = [&](uint32_t c) -> std::string { std::string name; H.append_contig(ctx, c, name); return name; };
        for (uint64_t r = 0; r < n; r++) {
            std::vector<std::pair<std::string, std::string>> extra;
            const int w0 = (int)(hkf[r] & 0x7fffffffu), w1 = (int)(hkt[r] & 0x7fffffffu);
            const bool cut5 = hkf[r] >> 31, cut3 = hkt[r] >> 31;
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
                        if (minus) extra.push_back({"truncated", chr_of(iv[0]) + ":" + std::to_string(st + keepn) + "-" + std::to_string(en)});
                        else extra.push_back({"truncated", chr_of(iv[0]) + ":" + std::to_string(st) + "-" + std::to_string(en - keepn)});
                        found = true;
                    } else if (found) extra.push_back({"truncated", chr_of(iv[0]) + ":" + std::to_string(st) + "-" + std::to_string(en)});
                    c += sz;
                }
            }
            if (p->mode == TKSMSEQ_TRC_KDE) {
                char sr[32]; snprintf(sr, sizeof sr, "%.2f", hts[r]);
                extra.push_back({"TR", fmt_double(htl[r]) + "," + sr});
            }
            if ((rc = append_comment(ctx, b.get(), normalize_comment(in->h_comment_pool.data() + in->h_comments[2 * r], in->h_comments[2 * r + 1], extra), "truncate"))) return rc;
        }
    }
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
    TmpBuf n_ivl(s), n_mod(s), n_idl(s);
    for (DevBuf* x : {&n_ivl, &n_mod, &n_idl}) HIPCHK(ctx, x->ensure(n * 8 + 16));
    HIPCHK(ctx, tk::launch_edit_count(M, pre, post, n_ivl.as<uint64_t>(), n_mod.as<uint64_t>(), n_idl.as<uint64_t>(), s));
    if (pal) HIPCHK(ctx, tk::launch_pal_count(M, pal->P, pal->first, pal->plan, n_ivl.as<uint64_t>(), n_mod.as<uint64_t>(), s));
    int rc;
    if ((rc = b.scan(n_ivl, n_mod, n_idl, n)) || (rc = b.alloc(n, ""))) return rc;
    const tk::MolOut O = b.tables();
    HIPCHK(ctx, tk::launch_edit_write(M, pre, post, flip, b->literals.as<uint64_t>(), b.o_ivl.as<uint64_t>(), b.o_mod.as<uint64_t>(), b.o_id.as<uint64_t>(), O, s));
    if (pal) HIPCHK(ctx, tk::launch_pal_write(M, pal->P, pal->first, pal->plan, b.o_ivl.as<uint64_t>(), b.o_mod.as<uint64_t>(), O, s));
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
        HIPCHK(ctx, d_fmt[e].ensure(fmt[e].size() + 16));
        HIPCHK(ctx, hipMemcpyAsync(d_fmt[e].p, fmt[e].data(), fmt[e].size(), hipMemcpyHostToDevice, s));
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
    std::string id(H.idpool.data() + H.ids[2 * r], H.ids[2 * r + 1]);
    if (!in->h_dup.empty() && (in->h_dup[r] >> 31)) id += "_" + std::to_string(in->h_dup[r] & 0x7fffffffu);
    return id;
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
    HIPCHK(ctx, d_post.ensure(n * 4 + 16));
    if (n) HIPCHK(ctx, hipMemcpyAsync(d_post.p, post.data(), n * 4, hipMemcpyHostToDevice, s));
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

// ---- filter and concat -----------------------------------------------------------------------------------------------------------
// the conditions of a call, parsed and checked; false: ctx->err says "Invalid condition: <text>"
static bool filter_conditions(tksmseq_ctx* ctx, const tksmseq_filter_params* p, std::vector<tkh::FilterCond>& out) {
    static const char* ops[6] = {"<", "<=", ">", ">=", "==", "!="};
    for (uint64_t k = 0; k < p->n_conditions; k++) {
        const tksmseq_filter_cond& q = p->conditions[k];
        tkh::FilterCond c;
        std::string shown;
        bool ok = q.text || q.kind == TKSMSEQ_FLT_SIZE;
        if (q.kind == TKSMSEQ_FLT_TEXT) { shown = q.text ? q.text : ""; ok = ok && tkh::parse_filter_condition(shown, c); }
        else if (q.kind == TKSMSEQ_FLT_INFO) { c.kind = q.kind; c.key = q.text ? q.text : ""; shown = "info " + c.key; }
        else if (q.kind == TKSMSEQ_FLT_SIZE) {
            c.kind = q.kind; c.cmp = q.cmp; c.value = q.value;
            ok = q.cmp >= TKSMSEQ_FLT_LT && q.cmp <= TKSMSEQ_FLT_NE && q.value >= 0 && q.value <= 0x7fffffffll;
            shown = std::string("size ") + (q.cmp >= 0 && q.cmp < 6 ? ops[q.cmp] : "?") + std::to_string(q.value);
        } else if (q.kind == TKSMSEQ_FLT_LOCUS) {
            c.kind = q.kind; c.key = q.text ? q.text : ""; c.ranged = q.ranged != 0; c.start = q.start; c.end = q.end;
            shown = "locus " + c.key + (c.ranged ? ":" + std::to_string(q.start) + "-" + std::to_string(q.end) : std::string());
            ok = ok && (!c.ranged || (q.start >= 0 && q.end >= 0 && q.start <= 0x7fffffffll && q.end <= 0x80000000ll));
        } else { ok = false; shown = "kind " + std::to_string(q.kind); }
        if (!ok) { ctx->err = "Invalid condition: " + shown; return false; }
        out.push_back(std::move(c));
    }
    return true;
}

// the header comments of one side of a partition, or of one input of a concatenation: entry (off, len) of `in`'s pool goes behind b's;
// the copies of a record, which follow one another and share an entry, share the new one too
struct CommentCopier {
    uint32_t last_off = 0, last_len = 0, last_new = 0; bool any = false;
    int put(tksmseq_ctx* ctx, tksmseq_batch* b, const tksmseq_batch* in, uint64_t r, const char* who) {
        const uint32_t off = in->h_comments[2 * r], len = in->h_comments[2 * r + 1];
        if (any && off == last_off && len == last_len) { b->h_comments.push_back(last_new); b->h_comments.push_back(len); return TKSMSEQ_OK; }
        if (b->h_comment_pool.size() + len >= 0xffffffffull) { ctx->err = std::string(who) + ": more than 4 GB of header comments in one batch (split the input)"; return TKSMSEQ_ELIMIT; }
        any = true; last_off = off; last_len = len; last_new = (uint32_t)b->h_comment_pool.size();
        b->h_comments.push_back(last_new); b->h_comments.push_back(len);
        b->h_comment_pool.insert(b->h_comment_pool.end(), in->h_comment_pool.begin() + off, in->h_comment_pool.begin() + off + len);
        return TKSMSEQ_OK;
    }
};

int tksmseq_filter(tksmseq_ctx* ctx, const tksmseq_batch* in, const tksmseq_filter_params* p, tksmseq_batch** out_true, tksmseq_batch** out_false) {
    if (!ctx || !in || !p || !out_true || (p->n_conditions && !p->conditions)) return TKSMSEQ_EINVAL;
    *out_true = nullptr;
    if (out_false) *out_false = nullptr;
    std::vector<tkh::FilterCond> conds;
    if (!filter_conditions(ctx, p, conds)) return TKSMSEQ_EINVAL;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const uint64_t n = in->n_reads;
    const bool both = out_false != nullptr;
    // `info`: the conjunction of the info conditions, a byte per molecule; the copies of a record follow one another and share a
    // comment entry, which is read once
    std::vector<const std::string*> keys;
    for (auto& c : conds) if (c.kind == TKSMSEQ_FLT_INFO) keys.push_back(&c.key);
    std::vector<uint8_t> info;
    if (!keys.empty()) {
        info.assign(n, 0);
        if (!in->h_comments.empty()) {
            for (uint64_t r = 0; r < n; r++) {
                const uint32_t off = in->h_comments[2 * r], len = in->h_comments[2 * r + 1];
                if (r && off == in->h_comments[2 * r - 2] && len == in->h_comments[2 * r - 1]) { info[r] = info[r - 1]; continue; }
                const Meta meta = parse_meta(in->h_comment_pool.data() + off, len);
                bool ok = true;
                for (const std::string* k : keys) {                      // (src/filter.cpp:32-44)
                    auto f = meta.find(*k);
                    ok = ok && f != meta.end() && !f->second.empty() && f->second[0] != ".";
                }
                info[r] = ok ? 1 : 0;
            }
        }
    }
    // the device's conditions: size and locus, the contig resolved here, its name uploaded for the literal segments
    std::vector<tk::FltCond> dc;
    std::string names;
    for (auto& c : conds) {
        if (c.kind == TKSMSEQ_FLT_INFO) continue;
        tk::FltCond d{};
        if (c.kind == TKSMSEQ_FLT_SIZE) { d.kind = tk::FLT_SIZE; d.cmp = c.cmp; d.value = c.value; }
        else {
            d.kind = tk::FLT_LOCUS;
            const int ci = ctx->find(c.key);
            d.contig = ci >= 0 ? (uint32_t)ci : 0xffffffffu;
            d.name_len = (uint32_t)c.key.size(); d.value = (long long)names.size();      // (offset into `names` until the upload)
            names += c.key;
            d.ranged = c.ranged ? 1 : 0; d.start = c.start; d.end = c.end;
        }
        dc.push_back(d);
    }
    TmpBuf d_conds(s), d_names(s), d_info(s), d_side(s), d_flag(s), d_rank(s), cnt[6] = {TmpBuf(s), TmpBuf(s), TmpBuf(s), TmpBuf(s), TmpBuf(s), TmpBuf(s)};
    HIPCHK(ctx, d_names.ensure(names.size() + 16));
    if (!names.empty()) HIPCHK(ctx, hipMemcpyAsync(d_names.p, names.data(), names.size(), hipMemcpyHostToDevice, s));
    for (auto& d : dc) if (d.kind == tk::FLT_LOCUS) { d.name = d_names.as<uint8_t>() + d.value; d.value = 0; }
    HIPCHK(ctx, d_conds.ensure(dc.size() * sizeof(tk::FltCond) + 16));
    if (!dc.empty()) HIPCHK(ctx, hipMemcpyAsync(d_conds.p, dc.data(), dc.size() * sizeof(tk::FltCond), hipMemcpyHostToDevice, s));
    if (!keys.empty()) {
        HIPCHK(ctx, d_info.ensure(n + 16));
        if (n) HIPCHK(ctx, hipMemcpyAsync(d_info.p, info.data(), n, hipMemcpyHostToDevice, s));
    }
    HIPCHK(ctx, d_side.ensure(n + 16));
    HIPCHK(ctx, d_flag.ensure(n * 8 + 16));
    for (int k = 0; k < (both ? 6 : 3); k++) HIPCHK(ctx, cnt[k].ensure(n * 8 + 16));
    const tk::MolView M = mol_view(in);
    const tk::FltCounts CT{cnt[0].as<uint64_t>(), cnt[1].as<uint64_t>(), cnt[2].as<uint64_t>()};
    const tk::FltCounts CF = both ? tk::FltCounts{cnt[3].as<uint64_t>(), cnt[4].as<uint64_t>(), cnt[5].as<uint64_t>()} : tk::FltCounts{nullptr, nullptr, nullptr};
    HIPCHK(ctx, tk::launch_flt_pred(M, d_conds.as<tk::FltCond>(), (uint32_t)dc.size(), keys.empty() ? nullptr : d_info.as<uint8_t>(), p->negate ? 1 : 0,
                                    d_side.as<uint8_t>(), d_flag.as<uint64_t>(), CT, CF, s));
    OutBatch bt(ctx), bf(ctx);
    uint64_t n_true = 0;
    int rc;
    if ((rc = scan_async(ctx, d_flag, d_rank, n, &n_true)) || (rc = bt.scan(cnt[0], cnt[1], cnt[2], n))) return rc;      // (the second drains the stream: n_true is there)
    if (both && (rc = bf.scan(cnt[3], cnt[4], cnt[5], n))) return rc;
    if ((rc = bt.alloc(n_true, "filter: ")) || (rc = bt.literals(in))) return rc;
    if (both && ((rc = bf.alloc(n - n_true, "filter: ")) || (rc = bf.literals(in)))) return rc;
    const tk::FltOffsets OT{bt.o_ivl.as<uint64_t>(), bt.o_mod.as<uint64_t>(), bt.o_id.as<uint64_t>()};
    const tk::FltOffsets OF = both ? tk::FltOffsets{bf.o_ivl.as<uint64_t>(), bf.o_mod.as<uint64_t>(), bf.o_id.as<uint64_t>()} : tk::FltOffsets{nullptr, nullptr, nullptr};
    HIPCHK(ctx, tk::launch_flt_write(M, d_side.as<uint8_t>(), d_rank.as<uint64_t>(), OT, OF, bt.tables(), both ? bf.tables() : tk::MolOut{}, s));
    if (!in->h_comments.empty() && !(p->flags & TKSMSEQ_MOL_NO_COMMENTS)) {
        std::vector<uint8_t> side(n);
        if (n) HIPCHK(ctx, hipMemcpyAsync(side.data(), d_side.p, n, hipMemcpyDeviceToHost, s));
        HIPCHK(ctx, hipStreamSynchronize(s));
        CommentCopier ct, cf;
        for (uint64_t r = 0; r < n; r++) {
            if (side[r]) rc = ct.put(ctx, bt.get(), in, r, "filter");
            else rc = both ? cf.put(ctx, bf.get(), in, r, "filter") : TKSMSEQ_OK;
            if (rc) return rc;
        }
    }
    tksmseq_batch *t = nullptr, *f = nullptr;
    if ((rc = bt.finish(&t))) return rc;
    if (both && (rc = bf.finish(&f))) { tksmseq_batch_free(ctx, t); return rc; }
    *out_true = t;
    if (both) *out_false = f;
    return TKSMSEQ_OK;
}

int tksmseq_concat(tksmseq_ctx* ctx, const tksmseq_batch* const* in, uint64_t n_in, int32_t flags, tksmseq_batch** out) {
    if (!ctx || !in || !out) return TKSMSEQ_EINVAL;
    *out = nullptr;
    if (n_in == 0) { ctx->err = "concat: no input batches"; return TKSMSEQ_EINVAL; }
    for (uint64_t k = 0; k < n_in; k++) if (!in[k]) return TKSMSEQ_EINVAL;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    // every input's counts (ids with their unroll suffix) and their scans; one synchronisation for all
    struct Part { std::unique_ptr<TmpBuf> cnt[3], off[3]; uint64_t total[3] = {0, 0, 0}; };
    std::vector<Part> parts(n_in);
    int rc;
    for (uint64_t k = 0; k < n_in; k++) {
        const uint64_t n = in[k]->n_reads;
        for (int q = 0; q < 3; q++) { parts[k].cnt[q].reset(new TmpBuf(s)); parts[k].off[q].reset(new TmpBuf(s)); HIPCHK(ctx, parts[k].cnt[q]->ensure(n * 8 + 16)); }
        HIPCHK(ctx, tk::launch_edit_count(mol_view(in[k]), nullptr, nullptr, parts[k].cnt[0]->as<uint64_t>(), parts[k].cnt[1]->as<uint64_t>(), parts[k].cnt[2]->as<uint64_t>(), s));
        for (int q = 0; q < 3; q++) if ((rc = scan_async(ctx, *parts[k].cnt[q], *parts[k].off[q], n, &parts[k].total[q]))) return rc;
    }
    HIPCHK(ctx, hipStreamSynchronize(s));
    OutBatch b(ctx);
    uint64_t n_mol = 0, n_lit = 0, pool = 0;
    for (uint64_t k = 0; k < n_in; k++) {
        n_mol += in[k]->n_reads; b.t_ivl += parts[k].total[0]; b.t_mod += parts[k].total[1]; b.t_id += parts[k].total[2];
        n_lit += in[k]->n_literals; pool += in[k]->litpool.cap;
    }
    if ((rc = b.alloc(n_mol, "concat: ", "fewer or smaller inputs")) || (rc = b.literals(nullptr, n_lit, pool))) return rc;
    tk::CatBase base{0, 0, 0, 0, 0u, 0};
    for (uint64_t k = 0; k < n_in; k++) {
        if (in[k]->litpool.cap) HIPCHK(ctx, hipMemcpyAsync(b->litpool.as<uint8_t>() + base.pool, in[k]->litpool.p, in[k]->litpool.cap, hipMemcpyDeviceToDevice, s));
        HIPCHK(ctx, tk::launch_cat_write(mol_view(in[k]), parts[k].off[0]->as<uint64_t>(), parts[k].off[1]->as<uint64_t>(), parts[k].off[2]->as<uint64_t>(), base,
                                         b->literals.as<uint64_t>(), b.tables(), s));
        base.mol += in[k]->n_reads; base.ivl += parts[k].total[0]; base.mod += parts[k].total[1]; base.id += parts[k].total[2];
        base.lit += (uint32_t)in[k]->n_literals; base.pool += in[k]->litpool.cap;
    }
    bool any_comments = false;
    for (uint64_t k = 0; k < n_in; k++) any_comments = any_comments || !in[k]->h_comments.empty();
    if (any_comments && !(flags & TKSMSEQ_MOL_NO_COMMENTS)) {
        b->h_comments.reserve(2 * n_mol);
        for (uint64_t k = 0; k < n_in; k++) {
            CommentCopier cc;
            for (uint64_t r = 0; r < in[k]->n_reads; r++) {
                if (in[k]->h_comments.empty()) { b->h_comments.push_back((uint32_t)b->h_comment_pool.size()); b->h_comments.push_back(0u); }
                else if ((rc = cc.put(ctx, b.get(), in[k], r, "concat"))) return rc;
            }
        }
    }
    return b.finish(out);
}

// ---- unsegment and shuffle -------------------------------------------------------------------------------------------------------
// joins(g) of the glue definition on the host: the draw of k_glue_plan (ST_GLUE = 30), word for word
int tksmseq_glue_joins(uint64_t seed, double probability, uint64_t molecule_index) {
    if (molecule_index == 0) return 0;
    const Ph4h w = philox_host(seed, (uint32_t)molecule_index, (uint32_t)(molecule_index >> 32), 30u, 0u);
    return (double)w.x * (1.0 / 4294967296.0) < probability ? 1 : 0;
}

int tksmseq_glue(tksmseq_ctx* ctx, const tksmseq_batch* in, const tksmseq_glue_params* p, tksmseq_batch** out) {
    if (!ctx || !in || !p || !out) return TKSMSEQ_EINVAL;
    *out = nullptr;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const uint64_t n = in->n_reads;
    const tk::MolView M = mol_view(in);
    TmpBuf d_join(s), d_head(s), d_rank(s), n_ivl(s), n_mod(s), n_idl(s);
    HIPCHK(ctx, d_join.ensure(n + 16));
    for (DevBuf* x : {(DevBuf*)&d_head, (DevBuf*)&n_ivl, (DevBuf*)&n_mod, (DevBuf*)&n_idl}) HIPCHK(ctx, x->ensure(n * 8 + 16));
    HIPCHK(ctx, tk::launch_glue_plan(M, p->seed, p->probability, p->first_molecule_index, d_join.as<uint8_t>(), d_head.as<uint64_t>(), n_ivl.as<uint64_t>(),
                                     n_mod.as<uint64_t>(), n_idl.as<uint64_t>(), s));
    OutBatch b(ctx);
    uint64_t n_heads = 0;
    int rc;
    if ((rc = scan_async(ctx, d_head, d_rank, n, &n_heads)) || (rc = b.scan(n_ivl, n_mod, n_idl, n))) return rc;      // (the second drains the stream: n_heads is there)
    if ((rc = b.alloc(n_heads, "glue: ")) || (rc = b.literals(in))) return rc;
    HIPCHK(ctx, tk::launch_glue_write(M, d_join.as<uint8_t>(), d_rank.as<uint64_t>(), b.o_ivl.as<uint64_t>(), b.o_mod.as<uint64_t>(), b.o_id.as<uint64_t>(), b.tables(), s));
    // comments: a head without joiners keeps its entry; a glued head's is parsed, gets the written ids of its joiners under Cat
    // (add_comment("Cat", md.get_id()), src/unsegment.cpp:99) and is dumped again; a joiner's own comment is dropped
    const bool glued = n_heads < n;
    if (!(p->flags & TKSMSEQ_MOL_NO_COMMENTS) && (glued || !in->h_comments.empty())) {
        std::vector<uint8_t> join(n);
        HostTables H;
        if (n) HIPCHK(ctx, hipMemcpyAsync(join.data(), d_join.p, n, hipMemcpyDeviceToHost, s));
        if (glued) { if ((rc = H.fetch(ctx, in, HostTables::IDS))) return rc; }
        else HIPCHK(ctx, hipStreamSynchronize(s));
        const bool have = !in->h_comments.empty();
        b->h_comments.reserve(2 * n_heads);
        CommentCopier cc;
        for (uint64_t r = 0; r < n;) {
            uint64_t e = r + 1;
            while (e < n && join[e]) e++;
            if (e == r + 1) {
                if (have) rc = cc.put(ctx, b.get(), in, r, "glue");
                else { b->h_comments.push_back((uint32_t)b->h_comment_pool.size()); b->h_comments.push_back(0u); rc = TKSMSEQ_OK; }
            } else {
                Meta meta = have ? parse_meta(in->h_comment_pool.data() + in->h_comments[2 * r], in->h_comments[2 * r + 1]) : Meta();
                std::vector<std::string>& cat = meta["Cat"];
                for (uint64_t q = r + 1; q < e; q++) {
                    std::string id(H.idpool.data() + H.ids[2 * q], H.ids[2 * q + 1]);
                    if (!in->h_dup.empty() && (in->h_dup[q] >> 31)) id += "_" + std::to_string(in->h_dup[q] & 0x7fffffffu);
                    cat.push_back(std::move(id));
                }
                rc = append_comment(ctx, b.get(), dump_meta(meta), "glue");
            }
            if (rc) return rc;
            r = e;
        }
    }
    return b.finish(out);
}

int tksmseq_shuffle(tksmseq_ctx* ctx, const tksmseq_batch* in, const tksmseq_shuffle_params* p, tksmseq_batch** out) {
    if (!ctx || !in || !p || !out) return TKSMSEQ_EINVAL;
    *out = nullptr;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const uint64_t n = in->n_reads;
    if (n >= 0xffffffffull) { ctx->err = "shuffle: more than 2^32 molecules in one call"; return TKSMSEQ_ELIMIT; }
    // whole mode is the windowed rule with a slot per molecule: no arrivals
    const uint32_t B = (p->buffer_size == 0 || p->buffer_size >= n) ? (uint32_t)n : (uint32_t)p->buffer_size;
    const uint64_t m = n - B;
    int rc;
    TmpBuf d_key(s), d_key_s(s), d_order(s), d_slot(s), d_slot_s(s), d_arr_s(s), d_src(s), n_ivl(s), n_mod(s), n_idl(s);
    for (DevBuf* x : {(DevBuf*)&d_key, (DevBuf*)&d_key_s}) HIPCHK(ctx, x->ensure((size_t)B * 8 + 16));
    for (DevBuf* x : {(DevBuf*)&d_slot, (DevBuf*)&d_slot_s, (DevBuf*)&d_arr_s}) HIPCHK(ctx, x->ensure((size_t)m * 4 + 16));
    HIPCHK(ctx, d_order.ensure((size_t)B * 4 + 16));
    HIPCHK(ctx, d_src.ensure(n * 4 + 16));
    for (DevBuf* x : {(DevBuf*)&n_ivl, (DevBuf*)&n_mod, (DevBuf*)&n_idl}) HIPCHK(ctx, x->ensure(n * 8 + 16));
    // the arrivals by slot (t order kept inside a slot), then the slots by key (slot order kept among equal keys)
    int slot_bits = 1;
    while (slot_bits < 32 && (1ull << slot_bits) < (uint64_t)B) slot_bits++;
    HIPCHK(ctx, tk::launch_shf_slot(m, B, p->seed, d_slot.as<uint32_t>(), s));
    if (m && (rc = sort_pairs<uint32_t>(ctx, tk::abund_sort_u32, d_slot.as<uint32_t>(), d_slot_s.as<uint32_t>(), d_arr_s.as<uint32_t>(), (uint32_t)m, slot_bits))) return rc;
    HIPCHK(ctx, tk::launch_shf_evict(m, B, d_slot_s.as<uint32_t>(), d_arr_s.as<uint32_t>(), d_src.as<uint32_t>(), s));
    HIPCHK(ctx, tk::launch_shf_key(B, p->seed, d_key.as<uint64_t>(), s));
    if (B && (rc = sort_pairs<uint64_t>(ctx, tk::abund_sort_u64, d_key.as<uint64_t>(), d_key_s.as<uint64_t>(), d_order.as<uint32_t>(), B, 64))) return rc;
    HIPCHK(ctx, tk::launch_shf_occupant(B, m, d_order.as<uint32_t>(), d_slot_s.as<uint32_t>(), d_arr_s.as<uint32_t>(), d_src.as<uint32_t>() + m, s));
    // the gather in that order
    const tk::MolView M = mol_view(in);
    HIPCHK(ctx, tk::launch_gather_count(M, d_src.as<uint32_t>(), n, n_ivl.as<uint64_t>(), n_mod.as<uint64_t>(), n_idl.as<uint64_t>(), s));
    OutBatch b(ctx);
    if ((rc = b.scan(n_ivl, n_mod, n_idl, n)) || (rc = b.alloc(n, "shuffle: ")) || (rc = b.literals(in))) return rc;
    HIPCHK(ctx, tk::launch_gather_write(M, d_src.as<uint32_t>(), n, b.o_ivl.as<uint64_t>(), b.o_mod.as<uint64_t>(), b.o_id.as<uint64_t>(), b.tables(), s));
    // comments: the input's entries in the new order (the order comes to the host once)
    if (!in->h_comments.empty() && !(p->flags & TKSMSEQ_MOL_NO_COMMENTS)) {
        std::vector<uint32_t> src(n);
        if (n) HIPCHK(ctx, hipMemcpyAsync(src.data(), d_src.p, n * 4, hipMemcpyDeviceToHost, s));
        HIPCHK(ctx, hipStreamSynchronize(s));
        b->h_comments.reserve(2 * n);
        CommentCopier cc;
        for (uint64_t j = 0; j < n; j++) if ((rc = cc.put(ctx, b.get(), in, src[j], "shuffle"))) return rc;
    }
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
    HIPCHK(ctx, d_alpha.ensure(k + 16));
    HIPCHK(ctx, hipMemcpyAsync(d_alpha.p, p->alphabet, k, hipMemcpyHostToDevice, s));
    const tk::NoiseParams P{p->seed, p->dist == TKSMSEQ_NOISE_LOGNORMAL ? tk::NOISE_LOGNORMAL : tk::NOISE_NORMAL, p->mu, p->sigma, p->error_rate,
                            d_alpha.as<uint8_t>(), (uint32_t)k};
    const tk::MolView M = mol_view(in);
    OutBatch b(ctx);
    int rc;
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
    hipStream_t s = ctx->stream;
    HIPCHK(ctx, ctx->d_wgs_sofar.ensure(nc * 8 + 16)); HIPCHK(ctx, ctx->d_wgs_nameoff.ensure(nc * 4 + 16));
    HIPCHK(ctx, ctx->d_wgs_namelen.ensure(nc * 4 + 16)); HIPCHK(ctx, ctx->d_wgs_names.ensure(pool.size() + 16));
    HIPCHK(ctx, hipMemcpyAsync(ctx->d_wgs_sofar.p, so_far.data(), nc * 8, hipMemcpyHostToDevice, s));
    HIPCHK(ctx, hipMemcpyAsync(ctx->d_wgs_nameoff.p, noff.data(), nc * 4, hipMemcpyHostToDevice, s));
    HIPCHK(ctx, hipMemcpyAsync(ctx->d_wgs_namelen.p, nlen.data(), nc * 4, hipMemcpyHostToDevice, s));
    if (!pool.empty()) HIPCHK(ctx, hipMemcpyAsync(ctx->d_wgs_names.p, pool.data(), pool.size(), hipMemcpyHostToDevice, s));
    HIPCHK(ctx, hipStreamSynchronize(s));
    ctx->wgs_version = ctx->ref_version;
    return TKSMSEQ_OK;
}

int tksmseq_wgs(tksmseq_ctx* ctx, const tksmseq_wgs_params* p, tksmseq_batch** out, tksmseq_wgs_progress* progress) {
    if (!ctx || !p || !out || !progress) return TKSMSEQ_EINVAL;
    *out = nullptr;
    memset(progress, 0, sizeof *progress);
    // validate_arguments (src/random_wgs.cpp:118-125), plus what std:: leaves undefined
    if (p->dist < TKSMSEQ_WGS_NORMAL || p->dist > TKSMSEQ_WGS_EXPONENTIAL) { ctx->err = "Invalid fragment length distribution"; return TKSMSEQ_EINVAL; }
    if (!std::isfinite(p->a) || !std::isfinite(p->b) || !(p->a > 0.0) || p->b < 0.0 || (p->dist == TKSMSEQ_WGS_UNIFORM && p->b < p->a)) {
        ctx->err = "Invalid fragment length distribution parameters"; return TKSMSEQ_EINVAL;
    }
    const size_t nc = ctx->contig_names.size();
    if (!nc || !ctx->total_bases) { ctx->err = "random-wgs: the reference has no contigs (or none with a base)"; return TKSMSEQ_ESTATE; }
    for (size_t i = 0; i < nc; i++)
        if (ctx->contigs[2 * i + 1] >= 0x80000000ull) { ctx->err = "random-wgs: contig " + ctx->contig_names[i] + " has 2^31 bases or more"; return TKSMSEQ_ELIMIT; }
    const uint64_t n = p->n_candidates;
    if (n > (1ull << 28)) { ctx->err = "random-wgs: more than 2^28 candidates in one call (split the range)"; return TKSMSEQ_ELIMIT; }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    int rc = wgs_table(ctx);
    if (rc) return rc;
    progress->next_candidate = p->first_candidate; progress->molecules = p->molecules_before; progress->bases = p->bases_before;
    const bool owed = p->base_count > 0 && p->bases_before < (uint64_t)p->base_count;
    progress->reached = owed ? 0 : 1;
    const uint64_t nn = owed ? n : 0;                                   // (nothing owed: an empty batch, no candidate taken)
    TmpBuf d_plan(s), d_flag(s), d_bases(s), d_rank(s), d_bsum(s), d_idlen(s), d_idoff(s), d_cut(s);
    uint64_t h[8] = {0, 0, 0, 0, 0, 0, 0, 0};                           // cut[4], rank[n], bsum[n], idoff[n]
    if (nn) {
        HIPCHK(ctx, d_plan.ensure(nn * 16 + 16));
        for (DevBuf* b : {&d_flag, &d_bases, &d_idlen}) HIPCHK(ctx, b->ensure(nn * 8 + 16));
        for (DevBuf* b : {&d_rank, &d_bsum, &d_idoff}) HIPCHK(ctx, b->ensure((nn + 1) * 8 + 16));
        HIPCHK(ctx, d_cut.ensure(64));
        HIPCHK(ctx, ctx->w_scan.ensure(tk::scan_temp_bytes(nn) + 64));
        HIPCHK(ctx, hipMemsetAsync(d_cut.p, 0, 64, s));
        const tk::WgsParams W{p->seed, p->dist, p->a, p->b, ctx->total_bases, (uint32_t)nc};
        HIPCHK(ctx, tk::launch_wgs_plan(W, ctx->d_wgs_sofar.as<uint64_t>(), p->first_candidate, nn, d_plan.as<uint4>(), d_flag.as<uint64_t>(), d_bases.as<uint64_t>(), s));
        HIPCHK(ctx, tk::launch_scan(d_flag.as<uint64_t>(), d_rank.as<uint64_t>(), nn, ctx->w_scan.p, ctx->w_scan.cap, s));
        HIPCHK(ctx, tk::launch_scan(d_bases.as<uint64_t>(), d_bsum.as<uint64_t>(), nn, ctx->w_scan.p, ctx->w_scan.cap, s));
        HIPCHK(ctx, tk::launch_wgs_cut(nn, d_plan.as<uint4>(), d_rank.as<uint64_t>(), d_bsum.as<uint64_t>(), ctx->d_wgs_namelen.as<uint32_t>(), p->molecules_before,
                                       p->bases_before, (uint64_t)p->base_count, d_idlen.as<uint64_t>(), d_cut.as<uint64_t>(), s));
        HIPCHK(ctx, tk::launch_scan(d_idlen.as<uint64_t>(), d_idoff.as<uint64_t>(), nn, ctx->w_scan.p, ctx->w_scan.cap, s));
        HIPCHK(ctx, hipMemcpyAsync(h, d_cut.p, 32, hipMemcpyDeviceToHost, s));
        HIPCHK(ctx, hipMemcpyAsync(h + 4, d_rank.as<uint64_t>() + nn, 8, hipMemcpyDeviceToHost, s));
        HIPCHK(ctx, hipMemcpyAsync(h + 5, d_bsum.as<uint64_t>() + nn, 8, hipMemcpyDeviceToHost, s));
        HIPCHK(ctx, hipMemcpyAsync(h + 6, d_idoff.as<uint64_t>() + nn, 8, hipMemcpyDeviceToHost, s));
        HIPCHK(ctx, hipStreamSynchronize(s));
    }
    const bool reached = h[3] != 0;
    const uint64_t n_mol = reached ? h[0] : h[4], n_bases = reached ? h[1] : h[5];
    // one segment per molecule, no substitutions, no literals (the scans above are this module's own: rank and cut)
    OutBatch b(ctx);
    b.t_ivl = n_mol; b.t_mod = 0; b.t_id = h[6];
    if ((rc = b.alloc(n_mol, "random-wgs: ", "fewer candidates per call")) || (rc = b.literals(nullptr))) return rc;
    if (n_mol)
        HIPCHK(ctx, tk::launch_wgs_write(nn, d_plan.as<uint4>(), d_rank.as<uint64_t>(), d_idlen.as<uint64_t>(), d_idoff.as<uint64_t>(), ctx->d_wgs_nameoff.as<uint32_t>(),
                                         ctx->d_wgs_namelen.as<uint32_t>(), ctx->d_wgs_names.as<uint8_t>(), p->molecules_before, b.tables(), s));
    if ((rc = b.finish(out))) return rc;
    if (nn) {
        progress->next_candidate = p->first_candidate + (reached ? h[2] : nn);
        progress->molecules = p->molecules_before + n_mol; progress->bases = p->bases_before + n_bases;
        progress->reached = reached ? 1 : 0;
    }
    return TKSMSEQ_OK;
}

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
    HIPCHK(ctx, ctx->d_tsb_first.ensure(T.exon_first.size() * 4 + 16)); HIPCHK(ctx, ctx->d_tsb_exons.ensure(E * 16 + 16));
    HIPCHK(ctx, ctx->d_tsb_lits.ensure(lits.size() * 8 + 16)); HIPCHK(ctx, ctx->d_tsb_litpool.ensure(pool.size() + 16));
    HIPCHK(ctx, hipMemcpyAsync(ctx->d_tsb_first.p, T.exon_first.data(), T.exon_first.size() * 4, hipMemcpyHostToDevice, s));
    if (E) HIPCHK(ctx, hipMemcpyAsync(ctx->d_tsb_exons.p, ex.data(), E * 16, hipMemcpyHostToDevice, s));
    if (!lits.empty()) HIPCHK(ctx, hipMemcpyAsync(ctx->d_tsb_lits.p, lits.data(), lits.size() * 8, hipMemcpyHostToDevice, s));
    if (!pool.empty()) HIPCHK(ctx, hipMemcpyAsync(ctx->d_tsb_litpool.p, pool.data(), pool.size(), hipMemcpyHostToDevice, s));
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
    const tsb::Transcripts& T = *S.tx;
    const uint64_t R = S.ab.rows(), total = S.mol_first.back();
    const uint64_t m0 = std::min(first_molecule, total), n = std::min(n_molecules, total - m0), m1 = m0 + n;
    auto exons_of = [&](uint64_t r) { const uint32_t t = S.ab.tx[r]; return (uint64_t)(T.exon_first[t + 1] - T.exon_first[t]); };
    auto owner = [&](uint64_t m) { return (uint64_t)(std::upper_bound(S.mol_first.begin(), S.mol_first.end(), m) - S.mol_first.begin()) - 1; };
    auto id_len = [&](uint64_t r) { return S.prefix.size() + (uint64_t)ndig_host((uint64_t)(std::lower_bound(S.emitted.begin(), S.emitted.end(), (uint32_t)r) - S.emitted.begin())); };
    // where molecule m's intervals and id bytes start in the whole run's
    auto bases = [&](uint64_t m, uint64_t& ivl, uint64_t& idb) {
        if (m >= total) { ivl = S.ivl_first[R]; idb = S.id_first[R]; return; }
        const uint64_t r = owner(m), copy = m - S.mol_first[r];
        ivl = S.ivl_first[r] + copy * exons_of(r); idb = S.id_first[r] + copy * id_len(r);
    };
    uint64_t ivl0 = 0, id0 = 0, ivl1 = 0, id1 = 0;
    if (n) { bases(m0, ivl0, id0); bases(m1, ivl1, id1); }
    OutBatch b(ctx);
    b.t_ivl = ivl1 - ivl0; b.t_mod = 0; b.t_id = id1 - id0;
    if ((rc = b.alloc(n, "transcribe: ", "fewer molecules per call")) || (rc = b.literals(nullptr, ctx->tsb_n_lits, ctx->tsb_lit_bytes))) return rc;
    if (ctx->tsb_n_lits) HIPCHK(ctx, hipMemcpyAsync(b->literals.p, ctx->d_tsb_lits.p, ctx->tsb_n_lits * 16, hipMemcpyDeviceToDevice, s));
    if (ctx->tsb_lit_bytes) HIPCHK(ctx, hipMemcpyAsync(b->litpool.p, ctx->d_tsb_litpool.p, ctx->tsb_lit_bytes, hipMemcpyDeviceToDevice, s));
    HIPCHK(ctx, b->d_dup.ensure(n * 4 + 16));
    if (n) {
        const tk::TsbPlanView V{R, plan->d_tx.as<uint32_t>(), plan->d_mol_first.as<uint64_t>(), plan->d_rank.as<uint64_t>(), plan->d_ivl_first.as<uint64_t>(),
                                plan->d_id_first.as<uint64_t>(), ctx->d_tsb_first.as<uint32_t>(), ctx->d_tsb_exons.as<uint4>(), plan->d_prefix.as<uint8_t>(), (uint32_t)S.prefix.size()};
        if (ctx->timing) HIPCHK(ctx, hipEventRecord(ctx->ev[0], s));
        HIPCHK(ctx, tk::launch_tsb_write(V, m0, n, ivl0, b.t_ivl, id0, b.tables(), b->d_dup.as<uint32_t>(), s));
        if (ctx->timing) HIPCHK(ctx, hipEventRecord(ctx->ev[1], s));
        b->h_dup.resize(n);
        HIPCHK(ctx, hipMemcpyAsync(b->h_dup.data(), b->d_dup.p, n * 4, hipMemcpyDeviceToHost, s));
    }
    if (!(flags & TKSMSEQ_MOL_NO_COMMENTS) && n) {
        // the copies of a row share one comment: work per row touched, and one (offset, length) pair per molecule
        b->h_comments.reserve(2 * n);
        std::string c;
        for (uint64_t r = owner(m0), m = m0; m < m1; r++) {
            const uint64_t end = std::min(S.mol_first[r + 1], m1);
            if (end <= m) continue;
            const uint32_t t = S.ab.tx[r];
            c.clear();
            tsb::append_comment(c, S.ab.text.data() + S.ab.cb_off[r], S.ab.cb_len[r], T.id_pool.data() + T.id_off[t], T.id_len[t]);
            if (b->h_comment_pool.size() + c.size() >= 0xffffffffull) { ctx->err = "transcribe: more than 4 GB of header comments in one batch (fewer molecules per call)"; return TKSMSEQ_ELIMIT; }
            const uint32_t off = (uint32_t)b->h_comment_pool.size(), cl = (uint32_t)c.size();
            b->h_comment_pool.insert(b->h_comment_pool.end(), c.begin(), c.end());
            for (; m < end; m++) { b->h_comments.push_back(off); b->h_comments.push_back(cl); }
        }
    }
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
        auto up = [&](DevBuf& d, const void* p, size_t bytes) {
            hipError_t e = d.ensure(bytes + 16);
            if (e == hipSuccess && bytes) e = hipMemcpyAsync(d.p, p, bytes, hipMemcpyHostToDevice, s);
            return e;
        };
        HIPCHK(ctx, up(ctx->d_mut_refctg, ref_ctg.data(), ref_ctg.size() * 4));
        HIPCHK(ctx, up(ctx->d_mut_nameoff, name_off.data(), name_off.size() * 4));
        HIPCHK(ctx, up(ctx->d_mut_names, names.data(), names.size()));
        HIPCHK(ctx, up(ctx->d_mut_delfirst, T.del_first.data(), T.del_first.size() * 4));
        HIPCHK(ctx, up(ctx->d_mut_ptfirst, T.pt_first.data(), T.pt_first.size() * 4));
        HIPCHK(ctx, up(ctx->d_mut_delfrom, T.del_from.data(), T.del_from.size() * 4));
        HIPCHK(ctx, up(ctx->d_mut_delto, T.del_to.data(), T.del_to.size() * 4));
        HIPCHK(ctx, up(ctx->d_mut_ptpos, T.pt_pos.data(), T.pt_pos.size() * 4));
        HIPCHK(ctx, up(ctx->d_mut_ptinfo, T.pt_info.data(), T.pt_info.size() * 8));
        HIPCHK(ctx, up(ctx->d_mut_insent, T.ins_ent.data(), T.ins_ent.size() * 8));
        HIPCHK(ctx, up(ctx->d_mut_inspool, T.ins_pool.data(), T.ins_pool.size()));
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
    TmpBuf lit_ctg(s), n_ivl(s), n_mod(s), n_idl(s);
    HIPCHK(ctx, lit_ctg.ensure(in->n_literals * 4 + 16));
    const tk::MolView M = mol_view(in);
    HIPCHK(ctx, tk::launch_mut_resolve(M.B, V, lit_ctg.as<uint32_t>(), b->literals.as<uint64_t>(), b.lit_base, b.pool_base, s));
    for (DevBuf* x : {&n_ivl, &n_mod, &n_idl}) HIPCHK(ctx, x->ensure(n * 8 + 16));
    HIPCHK(ctx, tk::launch_mut_count(M, V, lit_ctg.as<uint32_t>(), n_ivl.as<uint64_t>(), n_mod.as<uint64_t>(), n_idl.as<uint64_t>(), s));
    if ((rc = b.scan(n_ivl, n_mod, n_idl, n)) || (rc = b.alloc(n, "mutate: "))) return rc;
    HIPCHK(ctx, tk::launch_mut_write(M, V, lit_ctg.as<uint32_t>(), b.lit_base, b.o_ivl.as<uint64_t>(), b.o_mod.as<uint64_t>(), b.o_id.as<uint64_t>(), b.tables(), s));
    edit_comments(in, b, p->flags);
    return b.finish(out);
}

int tksmseq_batch_to_mdf_text(tksmseq_ctx* ctx, const tksmseq_batch* b, char** text, uint64_t* len) {
    if (!ctx || !b || !text || !len) return TKSMSEQ_EINVAL;
    *text = nullptr; *len = 0;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const uint64_t n = b->n_reads;
    HostTables H;
    const int rc = H.fetch(ctx, b, HostTables::SEGMENTS | HostTables::MODS | HostTables::IDS);
    if (rc) return rc;
    const auto &reads = H.reads, &ivs = H.ivs, &mods = H.mods, &ids = H.ids;
    const auto& idpool = H.idpool;
    // One molecule per read, depth 1: what every C++ module of the reference writes after reading with unroll = true
    // (copies of a depth > 1 molecule are named id_0, id_1, ...: src/mdf.h:97-105).  print_tsv: "+id<TAB>depth<TAB>comment".
    // The reads are formatted in contiguous shares, one per host thread (tksmseq_set_host_threads), and the shares copied into
    // the result side by side.
    auto put_u32 = [](std::string& o, uint32_t v) {
        char tmp[10]; int k = 10;
        do { tmp[--k] = (char)('0' + v % 10u); v /= 10u; } while (v);
        o.append(tmp + k, (size_t)(10 - k));
    };
    auto format = [&](uint64_t r0, uint64_t r1, std::string& out) {
        out.reserve((r1 - r0) * 112);
        for (uint64_t r = r0; r < r1; r++) {
            out += '+';
            out.append(idpool.data() + ids[2 * r], ids[2 * r + 1]);
            if (!b->h_dup.empty() && (b->h_dup[r] >> 31)) { out += '_'; put_u32(out, b->h_dup[r] & 0x7fffffffu); }
            out += "\t1\t";
            if (!b->h_comments.empty()) out += normalize_comment(b->h_comment_pool.data() + b->h_comments[2 * r], b->h_comments[2 * r + 1], {});
            out += '\n';
            const uint32_t ib = reads[2 * r], ic = reads[2 * r + 1];
            for (uint32_t i = 0; i < ic; i++) {
                const uint32_t* iv = ivs.data() + 4 * (size_t)(ib + i);
                H.append_contig(ctx, iv[0], out);
                out += '\t'; put_u32(out, iv[1]); out += '\t'; put_u32(out, iv[2]); out += '\t';
                out += (iv[3] >> 31) ? '-' : '+';
                out += '\t';
                const uint32_t mb = iv[3] & 0x7fffffffu, me = iv[7] & 0x7fffffffu;
                for (uint32_t q = mb; q < me; q++) { if (q > mb) out += ','; put_u32(out, mods[2 * (size_t)q]); out += (char)mods[2 * (size_t)q + 1]; }
                out += '\n';
            }
        }
    };
    const uint64_t nt = std::max<uint64_t>(1, std::min<uint64_t>((uint64_t)std::max(1, ctx->host_threads), n / 1024 + 1));
    std::vector<std::string> parts(nt);
    {
        std::vector<std::thread> th;
        for (uint64_t t = 1; t < nt; t++) th.emplace_back([&, t]() { format(n * t / nt, n * (t + 1) / nt, parts[t]); });
        format(0, n / nt, parts[0]);
        for (auto& x : th) x.join();
    }
    uint64_t total = 0;
    std::vector<uint64_t> at(nt);
    for (uint64_t t = 0; t < nt; t++) { at[t] = total; total += parts[t].size(); }
    char* buf = (char*)malloc(total + 1);
    if (!buf) return TKSMSEQ_ENOMEM;
    {
        std::vector<std::thread> th;
        for (uint64_t t = 1; t < nt; t++) th.emplace_back([&, t]() { memcpy(buf + at[t], parts[t].data(), parts[t].size()); });
        memcpy(buf, parts[0].data(), parts[0].size());
        for (auto& x : th) x.join();
    }
    buf[total] = 0;
    *text = buf; *len = total;
    return TKSMSEQ_OK;
}

void tksmseq_text_free(char* text) { free(text); }

}  // extern "C"
