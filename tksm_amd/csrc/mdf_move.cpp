// mdf_move.cpp -- host side of the transforms that move whole molecules: every output molecule is an input molecule (or a chain of them)
//   tksmseq_filter / _concat   src/filter.cpp:21-117, :196-212 (a two-way partition); Mrg = `cat` of MDF files (batches joined)
//   tksmseq_glue / _shuffle    src/unsegment.cpp:88-105 (chains of glued molecules), src/shuffle.cpp:23-44 (the buffer as two sorts and a gather)
// All of them place with OutBatch (mdf_batch.h) and copy with copy_molecule (mdf_kernels.hip); the tables stay on the device.
#include "filter_host.h"
#include "mdf_batch.h"

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

// `info`: the conjunction of the info conditions, a byte per molecule (false: there is no such condition); the copies of a record follow
// one another and share a comment entry, which is read once
static bool filter_info(const tksmseq_batch* in, const std::vector<tkh::FilterCond>& conds, std::vector<uint8_t>& info) {
    std::vector<const std::string*> keys;
    for (auto& c : conds) if (c.kind == TKSMSEQ_FLT_INFO) keys.push_back(&c.key);
    if (keys.empty()) return false;
    const uint64_t n = in->n_reads;
    info.assign(n, 0);
    if (in->h_comments.empty()) return true;
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
    return true;
}

// the device's conditions: size and locus, the contig resolved here, its name uploaded for the literal segments.  dc and names live until
// the stream has drained
static int filter_device_conds(tksmseq_ctx* ctx, const std::vector<tkh::FilterCond>& conds, std::vector<tk::FltCond>& dc, std::string& names,
                               DevBuf& d_conds, DevBuf& d_names) {
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
    int rc = upload(ctx, d_names, names.data(), names.size());
    if (rc) return rc;
    for (auto& d : dc) if (d.kind == tk::FLT_LOCUS) { d.name = d_names.as<uint8_t>() + d.value; d.value = 0; }
    return upload(ctx, d_conds, dc.data(), dc.size() * sizeof(tk::FltCond));
}

// the comments of both sides (bf null: of the true side), each in input order
static int filter_comments(tksmseq_ctx* ctx, const tksmseq_batch* in, const DevBuf& d_side, OutBatch& bt, OutBatch* bf) {
    const uint64_t n = in->n_reads;
    std::vector<uint8_t> side(n);
    if (n) HIPCHK(ctx, hipMemcpyAsync(side.data(), d_side.p, n, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    CommentCopier ct, cf;                                             // (one pass over `side` serves both: no index lists for gather_comments)
    for (uint64_t r = 0; r < n; r++) {
        int rc = TKSMSEQ_OK;
        if (side[r]) rc = ct.put(ctx, bt.get(), in, r, "filter");
        else if (bf) rc = cf.put(ctx, bf->get(), in, r, "filter");
        if (rc) return rc;
    }
    return TKSMSEQ_OK;
}

// comments of a glued batch: a head without joiners keeps its entry; a glued head's is parsed, gets the written ids of its joiners under Cat
// (add_comment("Cat", md.get_id()), src/unsegment.cpp:99) and is dumped again; a joiner's own comment is dropped
static int glue_comments(tksmseq_ctx* ctx, const tksmseq_batch* in, const DevBuf& d_join, uint64_t n_heads, OutBatch& b) {
    const uint64_t n = in->n_reads;
    const bool glued = n_heads < n, have = !in->h_comments.empty();
    std::vector<uint8_t> join(n);
    HostTables H;
    int rc;
    if (n) HIPCHK(ctx, hipMemcpyAsync(join.data(), d_join.p, n, hipMemcpyDeviceToHost, ctx->stream));
    if (glued) { if ((rc = H.fetch(ctx, in, HostTables::IDS))) return rc; }
    else HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
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
            for (uint64_t q = r + 1; q < e; q++) cat.push_back(written_id(H, in, q));
            rc = append_comment(ctx, b.get(), dump_meta(meta), "glue");
        }
        if (rc) return rc;
        r = e;
    }
    return TKSMSEQ_OK;
}

extern "C" {

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
    std::vector<uint8_t> info;
    const bool have_info = filter_info(in, conds, info);
    std::vector<tk::FltCond> dc;
    std::string names;
    TmpBuf d_conds(s), d_names(s), d_info(s), d_side(s), d_flag(s), d_rank(s);
    int rc;
    if ((rc = filter_device_conds(ctx, conds, dc, names, d_conds, d_names))) return rc;
    if (have_info && (rc = upload(ctx, d_info, info.data(), n))) return rc;
    HIPCHK(ctx, d_side.ensure(n + 16));
    HIPCHK(ctx, d_flag.ensure(n * 8 + 16));
    OutBatch bt(ctx), bf(ctx);
    tk::MolCounts CT{}, CF{nullptr, nullptr, nullptr};              // (CF.ivl null: no false side)
    if ((rc = bt.counts(n, CT)) || (both && (rc = bf.counts(n, CF)))) return rc;
    const tk::MolView M = mol_view(in);
    HIPCHK(ctx, tk::launch_flt_pred(M, d_conds.as<tk::FltCond>(), (uint32_t)dc.size(), have_info ? d_info.as<uint8_t>() : nullptr, p->negate ? 1 : 0,
                                    d_side.as<uint8_t>(), d_flag.as<uint64_t>(), CT, CF, s));
    uint64_t n_true = 0;
    if ((rc = scan_async(ctx, d_flag, d_rank, n, &n_true)) || (rc = bt.scan(n)) || (both && (rc = bf.scan(n)))) return rc;
    HIPCHK(ctx, hipStreamSynchronize(s));                               // (one drain: n_true and both sides' totals are there)
    if ((rc = bt.alloc(n_true, "filter: ")) || (rc = bt.literals(in))) return rc;
    if (both && ((rc = bf.alloc(n - n_true, "filter: ")) || (rc = bf.literals(in)))) return rc;
    HIPCHK(ctx, tk::launch_flt_write(M, d_side.as<uint8_t>(), d_rank.as<uint64_t>(), bt.offsets(), both ? bf.offsets() : tk::MolOffsets{nullptr, nullptr, nullptr},
                                     bt.tables(), both ? bf.tables() : tk::MolOut{}, s));
    if (!in->h_comments.empty() && !(p->flags & TKSMSEQ_MOL_NO_COMMENTS) && (rc = filter_comments(ctx, in, d_side, bt, both ? &bf : nullptr))) return rc;
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
    std::vector<MolPlacement> parts;
    parts.reserve(n_in);
    int rc;
    for (uint64_t k = 0; k < n_in; k++) {
        parts.emplace_back(ctx);
        tk::MolCounts C{};
        if ((rc = parts[k].counts(in[k]->n_reads, C))) return rc;
        HIPCHK(ctx, tk::launch_edit_count(mol_view(in[k]), nullptr, nullptr, C, s));
        if ((rc = parts[k].scan(in[k]->n_reads))) return rc;
    }
    HIPCHK(ctx, hipStreamSynchronize(s));
    OutBatch b(ctx);
    uint64_t n_mol = 0, n_lit = 0, pool = 0, t_ivl = 0, t_mod = 0, t_id = 0;
    for (uint64_t k = 0; k < n_in; k++) {
        n_mol += in[k]->n_reads; t_ivl += parts[k].t_ivl; t_mod += parts[k].t_mod; t_id += parts[k].t_id;
        n_lit += in[k]->n_literals; pool += in[k]->litpool.cap;
    }
    if ((rc = b.place_known(n_mol, t_ivl, t_mod, t_id, "concat: ", "fewer or smaller inputs")) || (rc = b.literals(nullptr, n_lit, pool))) return rc;
    tk::CatBase base{0, 0, 0, 0, 0u, 0};
    for (uint64_t k = 0; k < n_in; k++) {
        if (in[k]->litpool.cap) HIPCHK(ctx, hipMemcpyAsync(b->litpool.as<uint8_t>() + base.pool, in[k]->litpool.p, in[k]->litpool.cap, hipMemcpyDeviceToDevice, s));
        HIPCHK(ctx, tk::launch_cat_write(mol_view(in[k]), parts[k].offsets(), base, b->literals.as<uint64_t>(), b.tables(), s));
        base.mol += in[k]->n_reads; base.ivl += parts[k].t_ivl; base.mod += parts[k].t_mod; base.id += parts[k].t_id;
        base.lit += (uint32_t)in[k]->n_literals; base.pool += in[k]->litpool.cap;
    }
    bool any_comments = false;
    for (uint64_t k = 0; k < n_in; k++) any_comments = any_comments || !in[k]->h_comments.empty();
    if (any_comments && !(flags & TKSMSEQ_MOL_NO_COMMENTS)) {
        b->h_comments.reserve(2 * n_mol);
        for (uint64_t k = 0; k < n_in; k++) {
            if (!in[k]->h_comments.empty()) { if ((rc = gather_comments(b, in[k], "concat", in[k]->n_reads, [](uint64_t r) { return r; }))) return rc; }
            else for (uint64_t r = 0; r < in[k]->n_reads; r++) { b->h_comments.push_back((uint32_t)b->h_comment_pool.size()); b->h_comments.push_back(0u); }
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
    TmpBuf d_join(s), d_head(s), d_rank(s);
    HIPCHK(ctx, d_join.ensure(n + 16));
    HIPCHK(ctx, d_head.ensure(n * 8 + 16));
    OutBatch b(ctx);
    tk::MolCounts C{};
    int rc;
    if ((rc = b.counts(n, C))) return rc;
    HIPCHK(ctx, tk::launch_glue_plan(M, p->seed, p->probability, p->first_molecule_index, d_join.as<uint8_t>(), d_head.as<uint64_t>(), C, s));
    uint64_t n_heads = 0;
    if ((rc = scan_async(ctx, d_head, d_rank, n, &n_heads)) || (rc = b.scan(n))) return rc;
    HIPCHK(ctx, hipStreamSynchronize(s));                               // (one drain: n_heads and the totals are there)
    if ((rc = b.alloc(n_heads, "glue: ")) || (rc = b.literals(in))) return rc;
    HIPCHK(ctx, tk::launch_glue_write(M, d_join.as<uint8_t>(), d_rank.as<uint64_t>(), b.offsets(), b.tables(), s));
    if (!(p->flags & TKSMSEQ_MOL_NO_COMMENTS) && (n_heads < n || !in->h_comments.empty()) && (rc = glue_comments(ctx, in, d_join, n_heads, b))) return rc;
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
    TmpBuf d_key(s), d_key_s(s), d_order(s), d_slot(s), d_slot_s(s), d_arr_s(s), d_src(s);
    for (DevBuf* x : {(DevBuf*)&d_key, (DevBuf*)&d_key_s}) HIPCHK(ctx, x->ensure((size_t)B * 8 + 16));
    for (DevBuf* x : {(DevBuf*)&d_slot, (DevBuf*)&d_slot_s, (DevBuf*)&d_arr_s}) HIPCHK(ctx, x->ensure((size_t)m * 4 + 16));
    HIPCHK(ctx, d_order.ensure((size_t)B * 4 + 16));
    HIPCHK(ctx, d_src.ensure(n * 4 + 16));
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
    OutBatch b(ctx);
    tk::MolCounts C{};
    if ((rc = b.counts(n, C))) return rc;
    HIPCHK(ctx, tk::launch_gather_count(M, d_src.as<uint32_t>(), n, C, s));
    if ((rc = b.place(n, n, "shuffle: ")) || (rc = b.literals(in))) return rc;
    HIPCHK(ctx, tk::launch_gather_write(M, d_src.as<uint32_t>(), n, b.offsets(), b.tables(), s));
    // comments: the input's entries in the new order (the order comes to the host once)
    if (!in->h_comments.empty() && !(p->flags & TKSMSEQ_MOL_NO_COMMENTS)) {
        std::vector<uint32_t> src(n);
        if (n) HIPCHK(ctx, hipMemcpyAsync(src.data(), d_src.p, n * 4, hipMemcpyDeviceToHost, s));
        HIPCHK(ctx, hipStreamSynchronize(s));
        if ((rc = gather_comments(b, in, "shuffle", n, [&](uint64_t j) { return src[j]; }))) return rc;
    }
    return b.finish(out);
}

}  // extern "C"
