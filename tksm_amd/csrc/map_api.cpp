// map_api.cpp -- C-ABI of map: tksmseq_map, tksmseq_map_align, tksmseq_map_extend, tksmseq_map_split and tksmseq_map_targets (include/tksmseq.h).  The host reads and checks (ms_host.cpp's FASTQ reader, map_host.cpp), packs
// the reads of a chunk and formats the PAF; the sketch of targets and reads, the index, the seeds, the chains and the choice of the lines run
// on the device (map_kernels.hip, with the radix sort of abundance and the run kernels of model-sequence), and with alignment the anchors of
// the written chains, their banded alignment and the run-length code of its columns (map_align_kernels.hip), and with extension the X-drop
// extension of both ends of every written chain (map_extend_kernels.hip), and with split the rounds of every group and the supplementary lines
// of every read (map_split_kernels.hip) in place of the chain launch and the selection.
#include <cstring>
#include <string>
#include <vector>

#include "abund_host.h"
#include "ctx.h"
#include "map_align_kernels.h"
#include "map_extend_kernels.h"
#include "map_host.h"
#include "map_kernels.h"
#include "map_split_kernels.h"
#include "map_targets.h"
#include "ms_kernels.h"
#include "tool_run.h"

namespace {

constexpr uint64_t MAP_LIMIT = 1ull << 31;
constexpr uint64_t MAP_ANCHORS_MIN = 1ull << 20, MAP_ANCHORS_MAX = 1ull << 24;      // the anchor budget of a chunk lies between these
constexpr uint64_t MAP_ANCHOR_BYTES = 128;                                           // device bytes an anchor takes through sort and chain
enum { ST_SKETCH, ST_INDEX, ST_SEED, ST_CHAIN, ST_SELECT };
constexpr int RC_SPLIT = -1000;                                                      // (internal) the chunk has more anchors than the budget

int bit_length(uint64_t n) { int b = 1; while (b < 64 && (n >> b)) b++; return b; }    // the bits of n itself (at least 1).  Not abund_api.cpp's bits_for, which holds n VALUES

// what align reads of a chunk, and what it hands back: outs[l], and runs[run_off[l] .. run_off[l + 1]) of line l
struct MapChunkBufs { const TmpBuf &d_codes, &d_valid, &d_seqs, &d_chain, &d_list, &d_gstart, &d_k1f, &d_pred; };
struct MapAligned { std::vector<tkh::MapAlnOut> outs; std::vector<uint64_t> run_off, runs; };
// what extend hands back: ends[2 l + end] of line l; with alignment traced[2 l + end] = the index of that end in outs and run_off, or -1
// when it did not move
struct MapExtended { std::vector<tkh::MapExtEnd> ends; std::vector<int64_t> traced; std::vector<tkh::MapAlnOut> outs; std::vector<uint64_t> run_off, runs; };

// what the call maps to: the context's reference, or a target set ("map, annotated targets").  The image and the { voff, len } table on the
// device; names, lengths and first validity words on the host
struct MapTargetView {
    const uint32_t *codes = nullptr, *valid = nullptr;
    const tk::MapSeq* seqs = nullptr;
    const std::vector<std::string>* names = nullptr;
    std::vector<uint64_t> lens, voff;
    size_t n() const { return lens.size(); }
};

// the state of one call
struct MapRun {
    tksmseq_ctx* ctx;
    hipStream_t s;
    tksmseq_map_params p;
    uint32_t permille;
    tksmseq_map_info info{};
    bool aligned = false;
    tksmseq_align_params ap{63, 0};
    tksmseq_align_info ainfo{};
    uint64_t align_budget = tkh::MAP_ALN_BYTES_MAX;
    bool extended = false;
    tksmseq_extend_params xp{31, 40, 2000, 0};
    tksmseq_extend_info xinfo{};
    bool split = false;
    tksmseq_split_params sp{4, 30, 8, 0};
    tksmseq_split_info sinfo{};
    Events<2> ev;
    MapTargetView tv;
    const tksmseq_targets* targets = nullptr;                  // with it tv is its image; without, build_index fills tv from the reference
    bool genome_coords = false;
    tksmseq_project_info pinfo{};
    std::string first_unprojected;
    // the index: distinct hashes with their runs in the sorted entries
    TmpBuf d_tvalid, d_tseq, d_dkey, d_dcount, d_dstart, d_iseq, d_ips;
    uint32_t n_distinct = 0;
    uint64_t anchor_budget = MAP_ANCHORS_MAX;
    const tkh::MsReads* reads = nullptr;
    std::vector<std::string> names;
    std::string paf;

    MapRun(tksmseq_ctx* c, const tksmseq_map_params& q)
        : ctx(c), s(c->stream), p(q), permille(tkh::map_permille(q.secondary_ratio)), d_tvalid(s), d_tseq(s), d_dkey(s), d_dcount(s), d_dstart(s), d_iseq(s), d_ips(s) {}

    // a stage's device time: one synchronization per stage
    int begin() { return ev.mark(ctx, 0); }
    int end(int stage) { return end(info.stage_ms[stage]); }
    int end(float& sum) {
        if (int rc = ev.mark(ctx, 1)) return rc;
        HIPCHK(ctx, hipStreamSynchronize(s));
        return ev.add(ctx, 0, sum);
    }
    // the minimizers of the tiled sequences: count, scan, write.  n_out minimizers in d_hash / d_seq / d_ps
    int sketch(const uint32_t* codes, const uint32_t* valid, const tk::MapSeq* seqs, const std::vector<tkh::MapTile>& tiles, TmpBuf& d_tiles, TmpBuf& d_hash, TmpBuf& d_seq,
               TmpBuf& d_ps, uint64_t& n_out) {
        n_out = 0;
        HIPCHK(ctx, d_hash.ensure(8)); HIPCHK(ctx, d_seq.ensure(4)); HIPCHK(ctx, d_ps.ensure(4));
        if (tiles.empty()) return TKSMSEQ_OK;
        const uint32_t n_tiles = (uint32_t)tiles.size();
        TmpBuf d_cnt(s), d_off(s);
        HIPCHK(ctx, upload(d_tiles, tiles.data(), tiles.size(), s));
        HIPCHK(ctx, d_cnt.ensure(((size_t)n_tiles + 1) * 8));
        HIPCHK(ctx, d_off.ensure(((size_t)n_tiles + 1) * 8));
        const tk::MapSketch S{codes, valid, seqs, d_tiles.as<tk::MapTile>(), n_tiles, (uint32_t)p.k, (uint32_t)p.w};
        HIPCHK(ctx, tk::launch_map_sketch_count(S, d_cnt.as<uint64_t>(), s));
        if (int rc = scan_u64(ctx, d_cnt.as<uint64_t>(), d_off.as<uint64_t>(), n_tiles)) return rc;
        if (int rc = fetch_u64(ctx, d_off.as<uint64_t>() + n_tiles, n_out)) return rc;
        if (n_out >= (1ull << 32)) { ctx->err = "map: 2^32 minimizers or more in one pass"; return TKSMSEQ_ELIMIT; }
        HIPCHK(ctx, d_hash.ensure(std::max<size_t>(n_out, 1) * 8));
        HIPCHK(ctx, d_seq.ensure(std::max<size_t>(n_out, 1) * 4));
        HIPCHK(ctx, d_ps.ensure(std::max<size_t>(n_out, 1) * 4));
        HIPCHK(ctx, tk::launch_map_sketch_write(S, d_off.as<uint64_t>(), d_hash.as<uint64_t>(), d_seq.as<uint32_t>(), d_ps.as<uint32_t>(), s));
        HIPCHK(ctx, hipStreamSynchronize(s));                   // (d_cnt and d_off go with this scope)
        return TKSMSEQ_OK;
    }

    int build_index();
    int chunk(uint32_t r0, uint32_t r1);
    int align(const std::vector<tkh::MapAlnLine>& lines, uint64_t segments, uint64_t col_words, bool alone, const std::string& first_name, const MapChunkBufs& c, MapAligned& a);
    int extend(const std::vector<uint32_t>& line_chain, bool alone, const std::string& first_name, const MapChunkBufs& c, MapExtended& x);
};

int MapRun::build_index() {
    const size_t n_t = tv.n();
    std::vector<tkh::MapSeq> tseq(n_t);
    std::vector<tkh::MapTile> tiles;
    for (size_t t = 0; t < n_t; t++) {
        tseq[t] = {tv.voff[t], (uint32_t)tv.lens[t], 0u};
        tkh::map_add_tiles((uint32_t)t, tv.lens[t], (uint32_t)p.k, (uint32_t)p.w, tiles);
    }
    const tk::RefView R{ctx->d_packed.as<uint32_t>(), ctx->d_blocktab.as<uint32_t>(), ctx->d_pool.as<uint8_t>(), ctx->d_contigs.as<uint64_t>(), (uint32_t)n_t};
    const uint64_t n_vwords = ctx->total_alloc / 32;
    TmpBuf d_tiles(s), d_hash(s), d_seq(s), d_ps(s);
    auto t0 = std::chrono::steady_clock::now();
    if (!targets) {
        HIPCHK(ctx, upload(d_tseq, tseq.data(), tseq.size(), s));
        HIPCHK(ctx, d_tvalid.ensure(std::max<size_t>(n_vwords, 1) * 4));
        HIPCHK(ctx, hipStreamSynchronize(s));
        tv.codes = R.packed; tv.valid = d_tvalid.as<uint32_t>(); tv.seqs = d_tseq.as<tk::MapSeq>();
    }
    info.upload_ms += ms_since(t0);

    if (int rc = begin()) return rc;
    if (!targets) HIPCHK(ctx, tk::launch_map_ref_valid(R, n_vwords, d_tvalid.as<uint32_t>(), s));
    uint64_t n_tm = 0;
    if (int rc = sketch(tv.codes, tv.valid, tv.seqs, tiles, d_tiles, d_hash, d_seq, d_ps, n_tm)) return rc;
    if (int rc = end(ST_SKETCH)) return rc;
    info.target_minimizers = n_tm;

    HIPCHK(ctx, d_dkey.ensure(8)); HIPCHK(ctx, d_dcount.ensure(8)); HIPCHK(ctx, d_dstart.ensure(8)); HIPCHK(ctx, d_iseq.ensure(4)); HIPCHK(ctx, d_ips.ensure(4));
    if (!n_tm) return TKSMSEQ_OK;
    const uint32_t n = (uint32_t)n_tm;
    if (int rc = begin()) return rc;
    TmpBuf d_sorted(s), d_perm(s), d_dropped(s);
    HIPCHK(ctx, d_sorted.ensure((size_t)n * 8));
    HIPCHK(ctx, d_perm.ensure((size_t)n * 4));
    HIPCHK(ctx, d_iseq.ensure((size_t)n * 4));
    HIPCHK(ctx, d_ips.ensure((size_t)n * 4));
    HIPCHK(ctx, d_dropped.ensure(8));
    // stable: entries of one hash stay in (target, p) order
    if (int rc = sort_pairs<uint64_t>(ctx, tk::abund_sort_u64, d_hash.as<uint64_t>(), d_sorted.as<uint64_t>(), d_perm.as<uint32_t>(), n, 64)) return rc;
    HIPCHK(ctx, tk::launch_ms_gather_u32(d_seq.as<uint32_t>(), d_perm.as<uint32_t>(), n, d_iseq.as<uint32_t>(), s));
    HIPCHK(ctx, tk::launch_ms_gather_u32(d_ps.as<uint32_t>(), d_perm.as<uint32_t>(), n, d_ips.as<uint32_t>(), s));
    uint64_t run_info[2] = {};                                  // (word 0: the runs)
    if (int rc = run_starts(ctx, d_sorted.as<uint64_t>(), nullptr, n, d_dstart, run_info)) return rc;
    const uint64_t n_runs = run_info[0];
    if (n_runs > n) { ctx->err = "map: more distinct hashes than minimizers"; return TKSMSEQ_EDEVICE; }
    n_distinct = (uint32_t)n_runs;
    HIPCHK(ctx, d_dkey.ensure((size_t)n_distinct * 8));
    HIPCHK(ctx, d_dcount.ensure((size_t)n_distinct * 8));
    HIPCHK(ctx, tk::launch_ms_run_write(d_sorted.as<uint64_t>(), nullptr, d_dstart.as<uint32_t>(), n_distinct, nullptr, nullptr, d_dkey.as<uint64_t>(), nullptr,
                                        d_dcount.as<uint64_t>(), s));
    HIPCHK(ctx, tk::launch_map_dropped(d_dcount.as<uint64_t>(), n_distinct, (uint64_t)p.max_occ, (unsigned long long*)d_dropped.p, s));
    uint64_t dropped = 0;
    if (int rc = fetch_u64(ctx, d_dropped.as<uint64_t>(), dropped)) return rc;
    if (int rc = end(ST_INDEX)) return rc;
    info.distinct_hashes = n_distinct;
    info.dropped_hashes = dropped;
    return TKSMSEQ_OK;
}

// reads [r0, r1): their lines appended to paf, or RC_SPLIT (nothing appended, no counter touched) when they have more anchors than the budget
int MapRun::chunk(uint32_t r0, uint32_t r1) {
    const uint32_t n = r1 - r0, slots = (uint32_t)p.max_secondary + (split ? (uint32_t)sp.segments : 1u);
    const uint32_t rounds = split ? (uint32_t)sp.chains : 1u;                    // chains a group has room for
    std::vector<uint32_t> h_codes, h_valid;
    std::vector<tkh::MapSeq> h_seqs;
    std::vector<tkh::MapTile> tiles;
    TmpBuf d_codes(s), d_valid(s), d_seqs(s), d_tiles(s), d_rh(s), d_rread(s), d_rps(s);
    auto t0 = std::chrono::steady_clock::now();
    tkh::map_pack_reads(*reads, r0, r1, h_codes, h_valid, h_seqs);
    for (uint32_t r = 0; r < n; r++) tkh::map_add_tiles(r, h_seqs[r].len, (uint32_t)p.k, (uint32_t)p.w, tiles);
    HIPCHK(ctx, upload(d_codes, h_codes.data(), h_codes.size(), s));
    HIPCHK(ctx, upload(d_valid, h_valid.data(), h_valid.size(), s));
    HIPCHK(ctx, upload(d_seqs, h_seqs.data(), h_seqs.size(), s));
    HIPCHK(ctx, hipStreamSynchronize(s));
    const double upload_ms = ms_since(t0);

    // ---- sketch
    uint64_t n_rm64 = 0;
    if (int rc = begin()) return rc;
    if (int rc = sketch(d_codes.as<uint32_t>(), d_valid.as<uint32_t>(), d_seqs.as<tk::MapSeq>(), tiles, d_tiles, d_rh, d_rread, d_rps, n_rm64)) return rc;
    if (int rc = end(ST_SKETCH)) return rc;
    const uint32_t n_rm = (uint32_t)n_rm64;

    // ---- seed: count, scan, write, and the two stable sorts that order the anchors by (read, target, rel, p, qa)
    TmpBuf d_run(s), d_cnt(s), d_off(s), d_k1(s), d_k2(s), d_k1f(s), d_k2s(s), d_gstart(s), d_list(s);
    uint64_t n_anchors = 0, n_groups = 0, n_chained = 0;
    if (int rc = begin()) return rc;
    HIPCHK(ctx, d_run.ensure(std::max<size_t>(n_rm, 1) * 4));
    HIPCHK(ctx, d_cnt.ensure(((size_t)n_rm + 1) * 8));
    HIPCHK(ctx, d_off.ensure(((size_t)n_rm + 1) * 8));
    if (n_rm) {
        HIPCHK(ctx, tk::launch_map_seed_count(d_rh.as<uint64_t>(), n_rm, d_dkey.as<uint64_t>(), d_dcount.as<uint64_t>(), n_distinct, (uint64_t)p.max_occ, d_run.as<uint32_t>(),
                                              d_cnt.as<uint64_t>(), s));
        if (int rc = scan_u64(ctx, d_cnt.as<uint64_t>(), d_off.as<uint64_t>(), n_rm)) return rc;
        if (int rc = fetch_u64(ctx, d_off.as<uint64_t>() + n_rm, n_anchors)) return rc;
    }
    if (n_anchors > anchor_budget) {
        if (int rc = end(ST_SEED)) return rc;
        if (n > 1) return RC_SPLIT;                              // (the device time of the attempt stays in stage_ms: it was spent)
        ctx->err = "map: read " + names[r0] + " has " + std::to_string(n_anchors) + " anchors, more than a chunk may hold";
        return TKSMSEQ_ELIMIT;
    }
    const uint32_t na = (uint32_t)n_anchors;
    HIPCHK(ctx, d_gstart.ensure(((size_t)na + 2) * 4));
    HIPCHK(ctx, d_list.ensure(std::max<size_t>(na, 1) * 4));
    HIPCHK(ctx, d_k1f.ensure(std::max<size_t>(na, 1) * 8));
    HIPCHK(ctx, d_k2s.ensure(std::max<size_t>(na, 1) * 8));
    if (na) {
        TmpBuf d_k1s(s), d_perm1(s), d_k2g(s), d_perm2(s), d_flag(s), d_scanned(s);
        HIPCHK(ctx, d_k1.ensure((size_t)na * 8));
        HIPCHK(ctx, d_k2.ensure((size_t)na * 8));
        HIPCHK(ctx, d_k1s.ensure((size_t)na * 8));
        HIPCHK(ctx, d_k2g.ensure((size_t)na * 8));
        HIPCHK(ctx, d_perm1.ensure((size_t)na * 4));
        HIPCHK(ctx, d_perm2.ensure((size_t)na * 4));
        HIPCHK(ctx, tk::launch_map_seed_write(d_rread.as<uint32_t>(), d_rps.as<uint32_t>(), d_run.as<uint32_t>(), d_cnt.as<uint64_t>(), d_off.as<uint64_t>(), n_rm,
                                              d_dstart.as<uint32_t>(), d_iseq.as<uint32_t>(), d_ips.as<uint32_t>(), d_seqs.as<tk::MapSeq>(), (uint32_t)p.k, d_k1.as<uint64_t>(),
                                              d_k2.as<uint64_t>(), s));
        if (int rc = sort_pairs<uint64_t>(ctx, tk::abund_sort_u64, d_k1.as<uint64_t>(), d_k1s.as<uint64_t>(), d_perm1.as<uint32_t>(), na, 62)) return rc;
        HIPCHK(ctx, tk::launch_ms_gather_u64(d_k2.as<uint64_t>(), d_perm1.as<uint32_t>(), na, d_k2g.as<uint64_t>(), s));
        if (int rc = sort_pairs<uint64_t>(ctx, tk::abund_sort_u64, d_k2g.as<uint64_t>(), d_k2s.as<uint64_t>(), d_perm2.as<uint32_t>(), na, 32 + bit_length(n))) return rc;
        HIPCHK(ctx, tk::launch_ms_gather_u64(d_k1s.as<uint64_t>(), d_perm2.as<uint32_t>(), na, d_k1f.as<uint64_t>(), s));
        uint64_t run_info[2] = {};
        if (int rc = run_starts(ctx, d_k2s.as<uint64_t>(), nullptr, na, d_gstart, run_info)) return rc;
        n_groups = run_info[0];
        if (n_groups > na) { ctx->err = "map: more groups than anchors"; return TKSMSEQ_EDEVICE; }
        // groups that cannot reach min_count anchors leave before any chaining
        HIPCHK(ctx, d_flag.ensure(((size_t)n_groups + 1) * 8));
        HIPCHK(ctx, d_scanned.ensure(((size_t)n_groups + 1) * 8));
        HIPCHK(ctx, tk::launch_map_group_flags(d_gstart.as<uint32_t>(), (uint32_t)n_groups, (uint32_t)p.min_count, d_flag.as<uint64_t>(), s));
        if (int rc = scan_u64(ctx, d_flag.as<uint64_t>(), d_scanned.as<uint64_t>(), n_groups)) return rc;
        if (int rc = fetch_u64(ctx, d_scanned.as<uint64_t>() + n_groups, n_chained)) return rc;
        if (n_chained > n_groups) { ctx->err = "map: more surviving groups than groups"; return TKSMSEQ_EDEVICE; }
        HIPCHK(ctx, tk::launch_map_group_list(d_flag.as<uint64_t>(), d_scanned.as<uint64_t>(), (uint32_t)n_groups, d_list.as<uint32_t>(), s));
        HIPCHK(ctx, hipStreamSynchronize(s));                   // (the temporaries of this scope go)
    }
    if (int rc = end(ST_SEED)) return rc;

    // ---- chain: one wave per surviving group; with split all rounds of the group, chain c * rounds + r its round r
    const uint32_t n_listed = (uint32_t)n_chained, nc = n_listed * rounds;       // (n_listed <= 2^24 anchors, rounds <= 16)
    TmpBuf d_pred(s), d_chain(s), d_rem(s), d_listx(s);
    std::vector<tkh::MapChain> chains(nc);
    float chain_ms = 0.f, select_ms = 0.f;
    if (int rc = begin()) return rc;
    HIPCHK(ctx, d_pred.ensure(std::max<size_t>(na, 1) * 4));
    HIPCHK(ctx, d_chain.ensure(std::max<size_t>(nc, 1) * sizeof(tk::MapChain)));
    const tk::MapChainParams CP{(uint32_t)p.k, (uint32_t)p.max_gap, (uint32_t)p.bandwidth, (uint32_t)p.min_count, (uint32_t)p.min_score};
    if (split) {
        HIPCHK(ctx, d_rem.ensure(std::max<size_t>(na, 1) * 4));
        HIPCHK(ctx, d_listx.ensure(std::max<size_t>(nc, 1) * 4));
        HIPCHK(ctx, tk::launch_map_chain_split(d_k1f.as<uint64_t>(), d_k2s.as<uint64_t>(), d_gstart.as<uint32_t>(), d_list.as<uint32_t>(), n_listed, CP, rounds,
                                               d_rem.as<uint32_t>(), d_pred.as<uint32_t>(), d_chain.as<tk::MapChain>(), s));
        HIPCHK(ctx, tk::launch_map_split_list(d_list.as<uint32_t>(), n_listed, rounds, d_listx.as<uint32_t>(), s));
    } else {
        HIPCHK(ctx, tk::launch_map_chain(d_k1f.as<uint64_t>(), d_k2s.as<uint64_t>(), d_gstart.as<uint32_t>(), d_list.as<uint32_t>(), nc, CP, d_pred.as<uint32_t>(),
                                         d_chain.as<tk::MapChain>(), s));
    }
    if (int rc = end(chain_ms)) return rc;
    info.stage_ms[ST_CHAIN] += chain_ms;

    // ---- select: the kept chains by (read, score descending), target and rel ascending by the sort's stability
    // (with split every line has a mapq of its own, and a read says how many of its lines step A wrote and how many candidates step B refused)
    TmpBuf d_key(s), d_keys(s), d_perm(s), d_nl(s), d_mq(s), d_lines(s), d_nf(s), d_rej(s);
    std::vector<uint32_t> n_lines(n), mapq(split ? (size_t)n * slots : n), lines((size_t)n * slots), n_first(split ? n : 0), rejected(split ? n : 0);
    if (int rc = begin()) return rc;
    HIPCHK(ctx, d_key.ensure(std::max<size_t>(nc, 1) * 8));
    HIPCHK(ctx, d_keys.ensure(std::max<size_t>(nc, 1) * 8));
    HIPCHK(ctx, d_perm.ensure(std::max<size_t>(nc, 1) * 4));
    HIPCHK(ctx, d_nl.ensure((size_t)n * 4));
    HIPCHK(ctx, d_mq.ensure(mapq.size() * 4));
    HIPCHK(ctx, d_lines.ensure((size_t)n * slots * 4));
    if (nc) {
        HIPCHK(ctx, tk::launch_map_chain_keys(d_chain.as<tk::MapChain>(), nc, d_key.as<uint64_t>(), s));
        if (int rc = sort_pairs<uint64_t>(ctx, tk::abund_sort_u64, d_key.as<uint64_t>(), d_keys.as<uint64_t>(), d_perm.as<uint32_t>(), nc, 64)) return rc;
    }
    if (split) {
        HIPCHK(ctx, d_nf.ensure((size_t)n * 4));
        HIPCHK(ctx, d_rej.ensure((size_t)n * 4));
        const tk::MapSplitSelect SS{permille, (uint32_t)p.max_secondary, rounds, (uint32_t)sp.overlap, (uint32_t)sp.segments};
        HIPCHK(ctx, tk::launch_map_select_split(d_keys.as<uint64_t>(), d_perm.as<uint32_t>(), d_chain.as<tk::MapChain>(), d_seqs.as<tk::MapSeq>(), nc, n, SS, d_nl.as<uint32_t>(),
                                                d_nf.as<uint32_t>(), d_mq.as<uint32_t>(), d_lines.as<uint32_t>(), d_rej.as<uint32_t>(), s));
        HIPCHK(ctx, hipMemcpyAsync(n_first.data(), d_nf.p, (size_t)n * 4, hipMemcpyDeviceToHost, s));
        HIPCHK(ctx, hipMemcpyAsync(rejected.data(), d_rej.p, (size_t)n * 4, hipMemcpyDeviceToHost, s));
    } else {
        HIPCHK(ctx, tk::launch_map_select(d_keys.as<uint64_t>(), d_perm.as<uint32_t>(), nc, n, permille, (uint32_t)p.max_secondary, d_nl.as<uint32_t>(), d_mq.as<uint32_t>(),
                                          d_lines.as<uint32_t>(), s));
    }
    HIPCHK(ctx, hipMemcpyAsync(n_lines.data(), d_nl.p, (size_t)n * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(ctx, hipMemcpyAsync(mapq.data(), d_mq.p, mapq.size() * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(ctx, hipMemcpyAsync(lines.data(), d_lines.p, (size_t)n * slots * 4, hipMemcpyDeviceToHost, s));
    if (nc) HIPCHK(ctx, hipMemcpyAsync(chains.data(), d_chain.p, (size_t)nc * sizeof(tk::MapChain), hipMemcpyDeviceToHost, s));
    if (int rc = end(select_ms)) return rc;
    info.stage_ms[ST_SELECT] += select_ms;

    // ---- the lines of the chunk: checked, with alignment aligned, then written
    std::vector<tkh::MapAlnLine> alines;
    std::vector<uint32_t> line_chain;
    MapAligned al;
    MapExtended ex;
    uint64_t segments = 0, col_words = 0;
    for (uint32_t r = 0; r < n; r++) {
        if (n_lines[r] > slots || (split && (n_first[r] > n_lines[r] || n_first[r] > (uint32_t)p.max_secondary + 1u || (n_lines[r] && !n_first[r])))) {
            ctx->err = "map: more lines for a read than it may have"; return TKSMSEQ_EDEVICE;
        }
        for (uint32_t i = 0; i < n_lines[r]; i++) {
            const uint32_t c = lines[(size_t)r * slots + i];
            if (c >= nc || chains[c].read != r || (chains[c].tr >> 1) >= tv.n()) { ctx->err = "map: a line of a chain that does not exist"; return TKSMSEQ_EDEVICE; }
            if (aligned) tkh::map_align_add_line(c, chains[c], segments, col_words, alines);
            line_chain.push_back(c);
        }
    }
    const MapChunkBufs bufs{d_codes, d_valid, d_seqs, d_chain, split ? d_listx : d_list, d_gstart, d_k1f, d_pred};
    if (aligned && !alines.empty())
        if (int rc = align(alines, segments, col_words, n == 1, names[r0], bufs, al)) return rc;
    if (extended && !line_chain.empty())
        if (int rc = extend(line_chain, n == 1, names[r0], bufs, ex)) return rc;
    t0 = std::chrono::steady_clock::now();
    size_t at = 0;
    std::vector<uint64_t> joined_runs;
    std::vector<std::pair<uint32_t, uint32_t>> p_iv;                // the read intervals of a read's tp:A:P lines, the primary first
    std::vector<uint32_t> p_rank;
    for (uint32_t r = 0; r < n; r++) {
        if (!n_lines[r]) { info.unmapped++; continue; }
        info.mapped++;
        const uint32_t first = split ? n_first[r] : n_lines[r], sn = 1u + n_lines[r] - first;
        if (sn > 1u) {
            p_iv.clear();
            for (uint32_t i = 0; i < n_lines[r]; i = std::max(i + 1u, first)) {
                const tkh::MapChain& x = chains[lines[(size_t)r * slots + i]];
                p_iv.push_back((x.tr & 1u) ? std::make_pair(h_seqs[r].len - x.qe, h_seqs[r].len - x.qs) : std::make_pair(x.qs, x.qe));
            }
            tkh::map_split_ranks(p_iv, p_rank);
            sinfo.split_reads++;
            sinfo.supplementary += sn - 1u;
        }
        if (split) sinfo.rejected_overlap += rejected[r];
        for (uint32_t i = 0; i < n_lines[r]; i++, at++) {
            const uint32_t c = lines[(size_t)r * slots + i], t = chains[c].tr >> 1;
            const bool is_p = i == 0 || i >= first;                 // the primary or a supplementary line
            const uint32_t mq = split ? mapq[(size_t)r * slots + i] : (i ? 0u : mapq[r]);
            const uint32_t si = sn > 1u && is_p ? p_rank[i ? 1u + i - first : 0u] : 0u, tag_n = is_p ? sn : 0u;
            tkh::MapChain ch = chains[c];
            const tkh::MapAlnOut* ao = aligned ? &al.outs[at] : nullptr;
            const uint64_t* runs = aligned ? al.runs.data() + al.run_off[at] : nullptr;
            tkh::MapAlnOut joined;
            if (extended) {
                const tkh::MapExtEnd &le = ex.ends[2 * at], &re = ex.ends[2 * at + 1];
                if (le.ei > ch.tstart || le.ej > ch.qs || re.ei > tv.lens[t] - ch.tend || re.ej > h_seqs[r].len - ch.qe) {
                    ctx->err = "map: an extension left its sequence"; return TKSMSEQ_EDEVICE;
                }
                ch = tkh::map_extended_chain(ch, le, re);
                ch.nmatch += le.m + re.m;
                if (aligned) {
                    const int64_t li = ex.traced[2 * at], ri = ex.traced[2 * at + 1];
                    joined = tkh::map_join_columns(li < 0 ? nullptr : &ex.outs[li], li < 0 ? nullptr : ex.runs.data() + ex.run_off[li], *ao, runs,
                                                   ri < 0 ? nullptr : &ex.outs[ri], ri < 0 ? nullptr : ex.runs.data() + ex.run_off[ri], joined_runs);
                    ao = &joined; runs = joined_runs.data();
                }
                xinfo.lines++;
                xinfo.ends_moved += (le.ei + le.ej > 0) + (re.ei + re.ej > 0);
                xinfo.target_gained += le.ei + re.ei; xinfo.read_gained += le.ej + re.ej; xinfo.matches += le.m + re.m;
                xinfo.antidiagonals += le.steps + re.steps; xinfo.cells += le.cells + re.cells;
                xinfo.longest = std::max<uint64_t>(xinfo.longest, std::max(le.ei + le.ej, re.ei + re.ej));
            }
            const size_t line_at = paf.size();
            if (aligned)
                tkh::map_paf_line_aligned(names[r0 + r], h_seqs[r].len, (*tv.names)[t], tv.lens[t], ch, mq, is_p, *ao, runs, ap.eqx != 0, paf, tag_n, si);
            else
                tkh::map_paf_line(names[r0 + r], h_seqs[r].len, (*tv.names)[t], tv.lens[t], ch, mq, is_p, paf, tag_n, si);
            if (genome_coords) {
                pinfo.lines++;
                if (targets->h.projectable[t] && ch.tend > ch.tstart) {
                    std::string line = paf.substr(line_at, paf.size() - 1 - line_at);
                    const uint32_t ci = targets->h.contig[t];
                    pinfo.junctions += tkh::map_project_line(line, targets->h, t, targets->names[t], targets->contig_names[ci], targets->contig_lens[ci]);
                    paf.resize(line_at);
                    paf += line; paf += '\n';
                    pinfo.projected++;
                } else {
                    if (!pinfo.unprojected) first_unprojected = targets->names[t];
                    pinfo.unprojected++;
                }
            }
            info.lines++;
            if (!is_p) info.secondary++;
        }
    }
    for (size_t l = 0; l < al.outs.size(); l++) {
        ainfo.lines++;
        ainfo.segments += chains[alines[l].chain].cnt;
        ainfo.cells += al.outs[l].cells;
        ainfo.columns += al.outs[l].ncols; ainfo.matches += al.outs[l].eq; ainfo.mismatches += al.outs[l].x; ainfo.inserted += al.outs[l].ins; ainfo.deleted += al.outs[l].del;
    }
    info.write_ms += ms_since(t0);
    info.upload_ms += upload_ms;
    info.read_minimizers += n_rm;
    info.anchors += n_anchors;
    info.groups += n_groups;
    info.chained_groups += n_chained;
    info.chunks++;
    if (split) {
        for (uint32_t c = 0; c < nc; c++) {
            sinfo.rounds += chains[c].cnt > 0;                      // (a round that ran has a chain of at least one anchor)
            sinfo.later_chains += chains[c].kept && c % rounds;
        }
        sinfo.split_ms += chain_ms + select_ms;
    }
    return TKSMSEQ_OK;
}

// the alignment of the chunk's lines: outs[l], and runs[run_off[l] .. run_off[l + 1]) of line l.  RC_SPLIT (no counter touched) when it does not
// fit the budget and the chunk has more than one read
int MapRun::align(const std::vector<tkh::MapAlnLine>& lines, uint64_t segments, uint64_t col_words, bool alone, const std::string& first_name, const MapChunkBufs& c, MapAligned& a) {
    const uint32_t nl = (uint32_t)lines.size();
    auto over = [&](const char* what) {
        if (!alone) return (int)RC_SPLIT;
        ctx->err = "map: the alignment of read " + first_name + " (" + what + ") does not fit the device bytes a chunk may take";
        return (int)TKSMSEQ_ELIMIT;
    };
    if (tkh::map_align_fixed_bytes(nl, segments, col_words, 0) >= align_budget) return over("its anchors and columns");
    TmpBuf d_lines(s), d_path(s), d_cols(s), d_out(s), d_words(s), d_tb(s), d_roff(s), d_runs(s);
    if (int rc = begin()) return rc;
    HIPCHK(ctx, upload(d_lines, lines.data(), lines.size(), s));
    HIPCHK(ctx, d_path.ensure(segments * 8));
    HIPCHK(ctx, d_cols.ensure(std::max<uint64_t>(col_words, 1) * 4));
    HIPCHK(ctx, d_out.ensure((size_t)nl * sizeof(tk::MapAlnOut)));
    HIPCHK(ctx, d_words.ensure(16));                               // longest, flags
    HIPCHK(ctx, hipMemsetAsync(d_words.p, 0, 16, s));
    uint32_t* words = d_words.as<uint32_t>();
    HIPCHK(ctx, tk::launch_map_align_path(d_lines.as<tk::MapAlnLine>(), nl, c.d_chain.as<tk::MapChain>(), c.d_list.as<uint32_t>(), c.d_gstart.as<uint32_t>(), c.d_k1f.as<uint64_t>(),
                                          c.d_pred.as<uint32_t>(), (uint32_t)p.k, d_path.as<uint64_t>(), words, words + 1, s));
    uint32_t h_words[4] = {};
    HIPCHK(ctx, hipMemcpyAsync(h_words, words, 16, hipMemcpyDeviceToHost, s));
    HIPCHK(ctx, hipStreamSynchronize(s));
    if (h_words[1]) { ctx->err = "map: the anchors of a written chain were not found again (flags " + std::to_string(h_words[1]) + ")"; return TKSMSEQ_EDEVICE; }
    const uint32_t longest = h_words[0];
    const uint32_t waves = tkh::map_align_waves(align_budget, tkh::map_align_fixed_bytes(nl, segments, col_words, 0), nl, longest);
    if (!waves) { if (int rc = end(ainfo.align_ms)) return rc; return over("its traceback store"); }
    const uint32_t tb_stride = longest + 1u;
    HIPCHK(ctx, d_tb.ensure((size_t)waves * tb_stride * tkh::MAP_ALN_TB_BYTES));
    const tk::MapAlnSeqs Q{tv.codes, tv.valid, tv.seqs, c.d_codes.as<uint32_t>(), c.d_valid.as<uint32_t>(), c.d_seqs.as<tk::MapSeq>()};
    HIPCHK(ctx, tk::launch_map_align(d_lines.as<tk::MapAlnLine>(), nl, c.d_chain.as<tk::MapChain>(), d_path.as<uint64_t>(), Q, (uint32_t)p.k, (uint32_t)ap.band, ap.eqx ? 1u : 0u,
                                     waves, tb_stride, d_tb.as<uint64_t>(), d_cols.as<uint32_t>(), d_out.as<tk::MapAlnOut>(), words + 1, s));
    a.outs.resize(nl);
    HIPCHK(ctx, hipMemcpyAsync(a.outs.data(), d_out.p, (size_t)nl * sizeof(tk::MapAlnOut), hipMemcpyDeviceToHost, s));
    HIPCHK(ctx, hipMemcpyAsync(h_words, words, 16, hipMemcpyDeviceToHost, s));
    HIPCHK(ctx, hipStreamSynchronize(s));
    if (h_words[1]) { ctx->err = "map: an alignment left its segment (flags " + std::to_string(h_words[1]) + ")"; return TKSMSEQ_EDEVICE; }
    a.run_off.assign((size_t)nl + 1, 0);
    for (uint32_t l = 0; l < nl; l++) {
        if (a.outs[l].ncols > lines[l].cap || a.outs[l].runs > a.outs[l].ncols) { ctx->err = "map: more columns than a line may have"; return TKSMSEQ_EDEVICE; }
        a.run_off[l + 1] = a.run_off[l] + a.outs[l].runs;
    }
    const uint64_t n_runs = a.run_off[nl];
    // (the traceback stores have gone by now: the runs take their place in the budget)
    if (tkh::map_align_fixed_bytes(nl, segments, col_words, n_runs) >= align_budget) { if (int rc = end(ainfo.align_ms)) return rc; return over("its CIGAR"); }
    d_tb.release();
    HIPCHK(ctx, upload(d_roff, a.run_off.data(), a.run_off.size(), s));
    HIPCHK(ctx, d_runs.ensure(std::max<uint64_t>(n_runs, 1) * 8));
    HIPCHK(ctx, tk::launch_map_align_encode(d_lines.as<tk::MapAlnLine>(), nl, d_out.as<tk::MapAlnOut>(), d_cols.as<uint32_t>(), d_roff.as<uint64_t>(), ap.eqx ? 1u : 0u,
                                            d_runs.as<uint64_t>(), s));
    a.runs.resize((size_t)n_runs + 1);
    if (n_runs) HIPCHK(ctx, hipMemcpyAsync(a.runs.data(), d_runs.p, (size_t)n_runs * 8, hipMemcpyDeviceToHost, s));
    if (int rc = end(ainfo.align_ms)) return rc;
    ainfo.longest_segment = std::max<uint64_t>(ainfo.longest_segment, longest);
    return TKSMSEQ_OK;
}

// the extension of both ends of the chunk's lines: x.ends[2 l + end], and with alignment the columns and runs of the ends that moved.
// RC_SPLIT (no counter touched) when it does not fit the budget and the chunk has more than one read
int MapRun::extend(const std::vector<uint32_t>& line_chain, bool alone, const std::string& first_name, const MapChunkBufs& c, MapExtended& x) {
    const uint64_t nt64 = 2ull * line_chain.size();
    auto over = [&](const char* what) {
        if (!alone) return (int)RC_SPLIT;
        ctx->err = "map: the extension of read " + first_name + " (" + what + ") does not fit the device bytes a chunk may take";
        return (int)TKSMSEQ_ELIMIT;
    };
    if (nt64 >= (1ull << 31) || tkh::map_extend_fixed_bytes(nt64, 0, 0, 0) >= align_budget) return over("its ends");
    const uint32_t nt = (uint32_t)nt64;
    std::vector<tkh::MapExtTask> tasks(nt);
    for (uint32_t e = 0; e < nt; e++) tasks[e] = {line_chain[e / 2], e & 1u, 0u, 0u, 0u, 0u};
    TmpBuf d_tasks(s), d_ends(s), d_words(s);
    if (int rc = begin()) return rc;
    HIPCHK(ctx, upload(d_tasks, tasks.data(), tasks.size(), s));
    HIPCHK(ctx, d_ends.ensure((size_t)nt * sizeof(tk::MapExtEnd)));
    HIPCHK(ctx, d_words.ensure(16));                               // flags
    HIPCHK(ctx, hipMemsetAsync(d_words.p, 0, 16, s));
    uint32_t* flags = d_words.as<uint32_t>();
    const tk::MapAlnSeqs Q{tv.codes, tv.valid, tv.seqs, c.d_codes.as<uint32_t>(), c.d_valid.as<uint32_t>(), c.d_seqs.as<tk::MapSeq>()};
    const tk::MapExtParams P{(uint32_t)xp.band, (uint32_t)xp.drop, (uint32_t)xp.max_ext, aligned && ap.eqx ? 1u : 0u};
    HIPCHK(ctx, tk::launch_map_extend(d_tasks.as<tk::MapExtTask>(), nt, c.d_chain.as<tk::MapChain>(), Q, P, std::min<uint32_t>((nt + 3u) / 4u * 4u, tkh::MAP_ALN_WAVES), d_ends.as<tk::MapExtEnd>(),
                                      flags, s));
    x.ends.resize(nt);
    uint32_t h_flags = 0;
    HIPCHK(ctx, hipMemcpyAsync(x.ends.data(), d_ends.p, (size_t)nt * sizeof(tk::MapExtEnd), hipMemcpyDeviceToHost, s));
    HIPCHK(ctx, hipMemcpyAsync(&h_flags, flags, 4, hipMemcpyDeviceToHost, s));
    HIPCHK(ctx, hipStreamSynchronize(s));
    if (h_flags) { ctx->err = "map: a written chain does not lie in its sequences (flags " + std::to_string(h_flags) + ")"; return TKSMSEQ_EDEVICE; }
    x.traced.assign(nt, -1);
    if (!aligned) return end(xinfo.extend_ms);

    // ---- the second pass: the ends that moved, their columns sized by the cell the first pass found
    std::vector<tkh::MapExtTask> moved;
    uint64_t col_words = 0;
    uint32_t longest = 0;
    for (uint32_t e = 0; e < nt; e++) {
        const tkh::MapExtEnd& b = x.ends[e];
        if (b.ei > (uint32_t)xp.max_ext || b.ej > (uint32_t)xp.max_ext) { ctx->err = "map: an extension beyond max_ext"; return TKSMSEQ_EDEVICE; }
        const uint32_t cap = b.ei + b.ej;
        if (!cap) continue;
        x.traced[e] = (int64_t)moved.size();
        moved.push_back({tasks[e].chain, tasks[e].end, (uint32_t)col_words, cap, b.ei, b.ej});
        col_words += ((uint64_t)cap + 15) / 16;
        longest = std::max(longest, cap);
    }
    const uint32_t nm = (uint32_t)moved.size();
    if (!nm) return end(xinfo.extend_ms);
    // (at most a run a column is what this sizing assumes; the exact count is known before the runs are written)
    const uint64_t fixed = tkh::map_extend_fixed_bytes(nt, nm, col_words, 0);
    const uint32_t waves = tkh::map_align_waves(align_budget, fixed, nm, longest);   // (0 when the columns alone are over the budget: no col_off was cut short then)
    if (!waves) { if (int rc = end(xinfo.extend_ms)) return rc; return over("its traceback store"); }
    const uint32_t tb_stride = longest + 1u;
    TmpBuf d_moved(s), d_cols(s), d_out(s), d_tb(s), d_lines(s), d_roff(s), d_runs(s);
    HIPCHK(ctx, upload(d_moved, moved.data(), moved.size(), s));
    HIPCHK(ctx, d_cols.ensure(col_words * 4));
    HIPCHK(ctx, d_out.ensure((size_t)nm * sizeof(tk::MapAlnOut)));
    HIPCHK(ctx, d_tb.ensure((size_t)waves * tb_stride * tkh::MAP_ALN_TB_BYTES));
    HIPCHK(ctx, tk::launch_map_extend_trace(d_moved.as<tk::MapExtTask>(), nm, c.d_chain.as<tk::MapChain>(), Q, P, waves, tb_stride, d_tb.as<uint64_t>(), d_cols.as<uint32_t>(),
                                            d_out.as<tk::MapAlnOut>(), flags, s));
    x.outs.resize(nm);
    HIPCHK(ctx, hipMemcpyAsync(x.outs.data(), d_out.p, (size_t)nm * sizeof(tk::MapAlnOut), hipMemcpyDeviceToHost, s));
    HIPCHK(ctx, hipMemcpyAsync(&h_flags, flags, 4, hipMemcpyDeviceToHost, s));
    HIPCHK(ctx, hipStreamSynchronize(s));
    if (h_flags) { ctx->err = "map: an extension's way back left its cells (flags " + std::to_string(h_flags) + ")"; return TKSMSEQ_EDEVICE; }
    // the encoder of the alignment takes the ends as lines of their own: a left end's columns start its words, a right end's end them
    std::vector<tkh::MapAlnLine> lines(nm);
    x.run_off.assign((size_t)nm + 1, 0);
    for (uint32_t l = 0; l < nm; l++) {
        const tkh::MapAlnOut& o = x.outs[l];
        if (o.ncols > moved[l].cap || o.runs > o.ncols || !o.ncols || o.eq + o.x + o.del != moved[l].ei || o.eq + o.x + o.ins != moved[l].ej) {
            ctx->err = "map: an extension's columns do not lead to its cell"; return TKSMSEQ_EDEVICE;
        }
        lines[l] = {moved[l].chain, 0u, moved[l].col_off, moved[l].end ? moved[l].cap : o.ncols};
        x.run_off[l + 1] = x.run_off[l] + o.runs;
    }
    for (uint32_t e = 0; e < nt; e++)
        if (x.traced[e] >= 0 && x.outs[(size_t)x.traced[e]].eq != x.ends[e].m) { ctx->err = "map: the two passes of an extension count other matches"; return TKSMSEQ_EDEVICE; }
    const uint64_t n_runs = x.run_off[nm];
    if (tkh::map_extend_fixed_bytes(nt, nm, col_words, n_runs) >= align_budget) { if (int rc = end(xinfo.extend_ms)) return rc; return over("its CIGAR"); }
    d_tb.release();
    HIPCHK(ctx, upload(d_lines, lines.data(), lines.size(), s));
    HIPCHK(ctx, upload(d_roff, x.run_off.data(), x.run_off.size(), s));
    HIPCHK(ctx, d_runs.ensure(std::max<uint64_t>(n_runs, 1) * 8));
    HIPCHK(ctx, tk::launch_map_align_encode(d_lines.as<tk::MapAlnLine>(), nm, d_out.as<tk::MapAlnOut>(), d_cols.as<uint32_t>(), d_roff.as<uint64_t>(), ap.eqx ? 1u : 0u,
                                            d_runs.as<uint64_t>(), s));
    x.runs.resize((size_t)n_runs + 1);
    if (n_runs) HIPCHK(ctx, hipMemcpyAsync(x.runs.data(), d_runs.p, (size_t)n_runs * 8, hipMemcpyDeviceToHost, s));
    return end(xinfo.extend_ms);
}

}  // namespace

extern "C" int tksmseq_map_targets(tksmseq_ctx* ctx, const tksmseq_targets* targets, const tksmseq_map_targets_params* tp, const tksmseq_map_params* params,
                                   const tksmseq_align_params* align, const tksmseq_extend_params* extend, const tksmseq_split_params* split, const char* reads_paths,
                                   const char* paf_out, tksmseq_map_info* info_out, tksmseq_align_info* align_info, tksmseq_extend_info* extend_info,
                                   tksmseq_split_info* split_info, tksmseq_project_info* project_info) {
    if (!ctx) return TKSMSEQ_EINVAL;
    if (!reads_paths || !paf_out || !*paf_out) { ctx->err = "map: null argument"; return TKSMSEQ_EINVAL; }
    const bool genome_coords = tp && tp->genome_coords;
    if (genome_coords && !targets) { ctx->err = "map: genome_coords needs a target set"; return TKSMSEQ_EINVAL; }
    if (targets)
        if (int rc = map_targets_check(ctx, targets)) return rc;
    tksmseq_map_params p{};
    p.k = 15; p.w = 10; p.max_occ = 500; p.max_gap = 5000; p.bandwidth = 500; p.min_count = 3; p.min_score = 40; p.secondary_ratio = 0.8; p.max_secondary = 5;
    if (params) p = *params;
    if (!tkh::map_check_params(p, ctx->err)) return TKSMSEQ_EINVAL;
    if (align && !tkh::map_check_align(p, *align, ctx->err)) return TKSMSEQ_EINVAL;
    if (extend && !tkh::map_check_extend(*extend, ctx->err)) return TKSMSEQ_EINVAL;
    if (split && !tkh::map_check_split(*split, ctx->err)) return TKSMSEQ_EINVAL;
    if (!targets) {
        if (ctx->contigs.empty()) { ctx->err = "map: the context has no reference"; return TKSMSEQ_EINVAL; }
        if (ctx->n_declared) { ctx->err = "map: the reference has contigs that are declared only"; return TKSMSEQ_EINVAL; }
        if (ctx->contigs.size() / 2 >= MAP_LIMIT) { ctx->err = "map: 2^31 targets or more"; return TKSMSEQ_ELIMIT; }
        for (size_t t = 0; t < ctx->contigs.size() / 2; t++)
            if (ctx->contigs[2 * t + 1] >= MAP_LIMIT) { ctx->err = "map: target " + ctx->contig_names[t] + " has 2^31 bases or more"; return TKSMSEQ_ELIMIT; }
    }

    // ---- the host reads
    auto t0 = std::chrono::steady_clock::now();
    tkh::MsReads reads;
    const std::string list = reads_paths;
    if (int rc = tkh::load_fastq_list(list, reads, ctx->err, MAP_LIMIT)) {
        if (rc == TKSMSEQ_ELIMIT) ctx->err = "map: 2^31 reads or more";
        return rc;
    }
    if (!reads.size()) { ctx->err = "map: no reads in " + list; return TKSMSEQ_EINVAL; }
    const uint32_t n_reads = (uint32_t)reads.size();
    for (uint32_t r = 0; r < n_reads; r++)
        if (reads.off[r + 1] - reads.off[r] >= MAP_LIMIT) { ctx->err = "map: a read of 2^31 bases or more"; return TKSMSEQ_ELIMIT; }

    MapRun run(ctx, p);
    run.reads = &reads;
    if (align) { run.aligned = true; run.ap = *align; }
    if (extend) { run.extended = true; run.xp = *extend; }
    if (split) { run.split = true; run.sp = *split; }
    run.names = reads.names();
    MapTargetView& tv = run.tv;
    if (targets) {                                               // (the limits of a target set were checked when it was made)
        run.targets = targets; run.genome_coords = genome_coords;
        tv.codes = targets->d_codes.as<uint32_t>(); tv.valid = targets->d_valid.as<uint32_t>(); tv.seqs = targets->d_seqs.as<tk::MapSeq>();
        tv.names = &targets->names;
        tv.lens.assign(targets->h.len.begin(), targets->h.len.end());
        tv.voff.assign(targets->h.voff.begin(), targets->h.voff.end() - 1);
    } else {
        tv.names = &ctx->contig_names;
        for (size_t t = 0; t < ctx->contigs.size() / 2; t++) { tv.voff.push_back(ctx->contigs[2 * t] / 32); tv.lens.push_back(ctx->contigs[2 * t + 1]); }
    }
    run.info.reads = n_reads;
    run.info.read_ms = ms_since(t0);

    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (int rc = run.ev.create(ctx)) return rc;
    if (int rc = run.build_index()) return rc;

    uint64_t chunk_reads = p.chunk_reads;
    {
        size_t free_b = 0, total_b = 0;
        HIPCHK(ctx, hipMemGetInfo(&free_b, &total_b));
        const uint64_t anchor_bytes = MAP_ANCHOR_BYTES + (split ? tkh::map_split_anchor_bytes(*split, p.min_count) : 0);
        run.anchor_budget = std::max(MAP_ANCHORS_MIN, std::min<uint64_t>(MAP_ANCHORS_MAX, free_b / 4 / anchor_bytes));
        run.align_budget = std::min<uint64_t>(tkh::MAP_ALN_BYTES_MAX, std::max<uint64_t>(free_b / 4, 1ull << 20));
        if (!chunk_reads) {
            // per read: its packed letters, and about two minimizers in w + 1 positions through sketch and seed
            const uint64_t mean = reads.off[n_reads] / n_reads + 1;
            chunk_reads = std::max<uint64_t>(1ull << 10, std::min<uint64_t>(free_b / 8 / (mean * 16 + 64), 1ull << 20));
            // with alignment about four bytes a base: a line's anchors (8 bytes every w + 1 bases or so), its columns and its runs
            if (run.aligned) chunk_reads = std::max<uint64_t>(1ull << 10, std::min<uint64_t>(chunk_reads, run.align_budget / (mean * 4 + 64)));
        }
    }
    // chunks in input order; one with more anchors than the budget is halved and tried again
    std::vector<std::pair<uint32_t, uint32_t>> todo;
    for (uint64_t r0 = ((uint64_t)n_reads - 1) / chunk_reads * chunk_reads;; r0 -= chunk_reads) {
        todo.emplace_back((uint32_t)r0, (uint32_t)std::min<uint64_t>(n_reads, r0 + chunk_reads));
        if (!r0) break;
    }
    while (!todo.empty()) {
        const auto c = todo.back();
        todo.pop_back();
        const int rc = run.chunk(c.first, c.second);
        if (rc == RC_SPLIT) {
            const uint32_t mid = c.first + (c.second - c.first) / 2;
            todo.emplace_back(mid, c.second);
            todo.emplace_back(c.first, mid);
        } else if (rc) return rc;
    }
    tksmseq_map_info& info = run.info;
    for (float ms : info.stage_ms) info.device_ms += ms;

    t0 = std::chrono::steady_clock::now();
    std::string e;
    if (!tkh::write_abundance_file(paf_out, run.paf, e)) { ctx->err = "map: cannot write " + std::string(paf_out); return TKSMSEQ_EIO; }
    info.write_ms += ms_since(t0);
    if (info_out) *info_out = info;
    if (align_info) *align_info = run.ainfo;
    if (extend_info) *extend_info = run.xinfo;
    if (split_info) *split_info = run.sinfo;
    if (project_info) *project_info = run.pinfo;
    // (not an error: the note the module logs, tksmseq_last_error after TKSMSEQ_OK)
    if (run.pinfo.unprojected) ctx->err = "map: " + std::to_string(run.pinfo.unprojected) + " lines stay in transcript coordinates, the first on " + run.first_unprojected;
    return TKSMSEQ_OK;
}

extern "C" int tksmseq_map_split(tksmseq_ctx* ctx, const tksmseq_map_params* params, const tksmseq_align_params* align, const tksmseq_extend_params* extend,
                                 const tksmseq_split_params* split, const char* reads_paths, const char* paf_out, tksmseq_map_info* info_out, tksmseq_align_info* align_info,
                                 tksmseq_extend_info* extend_info, tksmseq_split_info* split_info) {
    return tksmseq_map_targets(ctx, nullptr, nullptr, params, align, extend, split, reads_paths, paf_out, info_out, align_info, extend_info, split_info, nullptr);
}

extern "C" int tksmseq_map_extend(tksmseq_ctx* ctx, const tksmseq_map_params* params, const tksmseq_align_params* align, const tksmseq_extend_params* extend,
                                  const char* reads_paths, const char* paf_out, tksmseq_map_info* info_out, tksmseq_align_info* align_info, tksmseq_extend_info* extend_info) {
    return tksmseq_map_split(ctx, params, align, extend, nullptr, reads_paths, paf_out, info_out, align_info, extend_info, nullptr);
}

extern "C" int tksmseq_map_align(tksmseq_ctx* ctx, const tksmseq_map_params* params, const tksmseq_align_params* align, const char* reads_paths, const char* paf_out,
                                 tksmseq_map_info* info_out, tksmseq_align_info* align_info) {
    return tksmseq_map_extend(ctx, params, align, nullptr, reads_paths, paf_out, info_out, align_info, nullptr);
}

extern "C" int tksmseq_map(tksmseq_ctx* ctx, const tksmseq_map_params* params, const char* reads_paths, const char* paf_out, tksmseq_map_info* info_out) {
    return tksmseq_map_align(ctx, params, nullptr, reads_paths, paf_out, info_out, nullptr);
}
