// map_host.cpp -- host side of map (see map_host.h; the rules are stated in include/tksmseq.h).
#include "map_host.h"

#include <algorithm>
#include <cmath>

namespace tkh {

bool map_check_params(const tksmseq_map_params& p, std::string& err) {
    auto bad = [&](const char* what) { err = std::string("map: ") + what; return false; };
    if (p.k < 4 || p.k > 28) return bad("k must be in [4, 28]");
    if (p.w < 1 || p.w > 64) return bad("w must be in [1, 64]");
    if (p.max_occ < 1) return bad("max_occ must be at least 1");
    if (p.max_gap < 0) return bad("max_gap must not be negative");
    if (p.bandwidth < 0) return bad("bandwidth must not be negative");
    if (p.min_count < 1) return bad("min_count must be at least 1");
    if (p.min_score < 0) return bad("min_score must not be negative");
    if (!(p.secondary_ratio >= 0.0 && p.secondary_ratio <= 1.0)) return bad("secondary_ratio must be in [0, 1]");
    if (p.max_secondary < 0 || p.max_secondary > 1000) return bad("max_secondary must be in [0, 1000]");
    if (p.chunk_reads > 0x7FFFFFFFull) return bad("chunk_reads must be below 2^31");
    return true;
}

uint32_t map_permille(double secondary_ratio) { return (uint32_t)std::floor(secondary_ratio * 1000.0 + 0.5); }

void map_add_tiles(uint32_t seq, uint64_t len, uint32_t k, uint32_t w, std::vector<MapTile>& tiles) {
    const uint64_t windows = map_windows(len, k, w);
    for (uint64_t j0 = 0; j0 < windows; j0 += MAP_TILE_WINDOWS) tiles.push_back({seq, (uint32_t)j0});
}

void map_pack_reads(const MsReads& reads, uint32_t r0, uint32_t r1, std::vector<uint32_t>& codes, std::vector<uint32_t>& valid, std::vector<MapSeq>& seqs) {
    seqs.clear();
    uint64_t words = 0;
    for (uint32_t r = r0; r < r1; r++) {
        const uint64_t len = reads.off[r + 1] - reads.off[r];
        seqs.push_back({words, (uint32_t)len, 0u});
        words += (len + 31) / 32;
    }
    valid.assign((size_t)words, 0u);
    codes.assign((size_t)words * 2, 0u);
    uint8_t code[256];
    for (int b = 0; b < 256; b++) code[b] = b == 'A' ? 0 : b == 'C' ? 1 : b == 'G' ? 2 : b == 'T' ? 3 : 4;
    for (uint32_t r = r0; r < r1; r++) {
        const MapSeq& q = seqs[r - r0];
        const uint8_t* base = reads.bases.data() + reads.off[r];
        uint32_t *c = codes.data() + 2 * q.voff, *v = valid.data() + q.voff;
        for (uint32_t j = 0; j < q.len; j++) {
            const uint32_t x = code[base[j]];
            if (x > 3u) continue;
            c[j >> 4] |= x << (2u * (j & 15u));
            v[j >> 5] |= 1u << (j & 31u);
        }
    }
}

namespace {
// the fifteen fields both forms of a line share, without the line's end
void paf_fields(const std::string& qname, uint32_t qlen, const std::string& tname, uint64_t tlen, const MapChain& c, uint32_t mapq, bool primary, uint32_t nmatch, uint32_t blen,
                std::string& out) {
    const bool rel = (c.tr & 1u) != 0;
    // a reverse chain lies in the reverse-complemented read: the interval is given in the read as it was sequenced
    const uint32_t qstart = rel ? qlen - c.qe : c.qs, qend = rel ? qlen - c.qs : c.qe;
    out += qname; out += '\t';
    out += std::to_string(qlen); out += '\t';
    out += std::to_string(qstart); out += '\t';
    out += std::to_string(qend); out += '\t';
    out += rel ? '-' : '+'; out += '\t';
    out += tname; out += '\t';
    out += std::to_string(tlen); out += '\t';
    out += std::to_string(c.tstart); out += '\t';
    out += std::to_string(c.tend); out += '\t';
    out += std::to_string(nmatch); out += '\t';
    out += std::to_string(blen); out += '\t';
    out += std::to_string(mapq); out += '\t';
    out += primary ? "tp:A:P" : "tp:A:S";
    out += "\tcm:i:"; out += std::to_string(c.cnt);
    out += "\ts1:i:"; out += std::to_string(c.score);
}

// the two tags of a read with several tp:A:P lines
void split_tags(uint32_t sn, uint32_t si, std::string& out) {
    if (sn < 2) return;
    out += "\tsn:i:"; out += std::to_string(sn);
    out += "\tsi:i:"; out += std::to_string(si);
}
}  // namespace

void map_paf_line(const std::string& qname, uint32_t qlen, const std::string& tname, uint64_t tlen, const MapChain& c, uint32_t mapq, bool primary, std::string& out,
                  uint32_t sn, uint32_t si) {
    paf_fields(qname, qlen, tname, tlen, c, mapq, primary, c.nmatch, std::max(c.tend - c.tstart, c.qe - c.qs), out);
    split_tags(sn, si, out);
    out += '\n';
}

bool map_check_align(const tksmseq_map_params& p, const tksmseq_align_params& a, std::string& err) {
    if (a.band < 1 || a.band > 63) { err = "map: align band must be in [1, 63]"; return false; }
    if (p.max_gap > MAP_ALN_MAX_GAP) { err = "map: max_gap must be at most 65536 with alignment"; return false; }
    return true;
}

uint64_t map_align_fixed_bytes(uint64_t lines, uint64_t segments, uint64_t col_words, uint64_t runs) {
    return lines * (sizeof(MapAlnLine) + sizeof(MapAlnOut) + 8) + 8 + segments * 8 + col_words * 4 + runs * 8;
}

uint32_t map_align_waves(uint64_t budget, uint64_t fixed, uint64_t lines, uint32_t longest) {
    if (fixed >= budget) return 0;
    const uint64_t per_wave = ((uint64_t)longest + 1) * MAP_ALN_TB_BYTES;
    uint64_t waves = std::min<uint64_t>((budget - fixed) / per_wave, MAP_ALN_WAVES) / 4 * 4;
    waves = std::min(waves, (lines + 3) / 4 * 4);
    return (uint32_t)waves;
}

void map_paf_line_aligned(const std::string& qname, uint32_t qlen, const std::string& tname, uint64_t tlen, const MapChain& c, uint32_t mapq, bool primary,
                          const MapAlnOut& a, const uint64_t* runs, bool eqx, std::string& out, uint32_t sn, uint32_t si) {
    paf_fields(qname, qlen, tname, tlen, c, mapq, primary, a.eq, a.ncols, out);
    split_tags(sn, si, out);
    out += "\tNM:i:"; out += std::to_string((uint64_t)a.x + a.ins + a.del);
    out += "\tcg:Z:";
    const char* ops = eqx ? "=XID" : "MMID";
    for (uint32_t r = 0; r < a.runs; r++) {
        const uint64_t first = runs[r] >> 2, next = r + 1 < a.runs ? runs[r + 1] >> 2 : a.ncols;
        out += std::to_string(next - first);
        out += ops[runs[r] & 3u];
    }
    out += '\n';
}

bool map_check_extend(const tksmseq_extend_params& e, std::string& err) {
    if (e.band < 1 || e.band > 63) { err = "map: extend band must be in [1, 63]"; return false; }
    if (e.drop < 1 || e.drop > 1000) { err = "map: extend drop must be in [1, 1000]"; return false; }
    if (e.max_ext < 1 || e.max_ext > 32768) { err = "map: extend max_ext must be in [1, 32768]"; return false; }
    return true;
}

uint64_t map_extend_fixed_bytes(uint64_t tasks, uint64_t traced, uint64_t col_words, uint64_t runs) {
    return tasks * (sizeof(MapExtTask) + sizeof(MapExtEnd)) + 8 + traced * (sizeof(MapExtTask) + sizeof(MapAlnOut) + sizeof(MapAlnLine) + 8) + 8 + col_words * 4 + runs * 8;
}

MapAlnOut map_join_columns(const MapAlnOut* left, const uint64_t* left_runs, const MapAlnOut& mid, const uint64_t* mid_runs, const MapAlnOut* right,
                           const uint64_t* right_runs, std::vector<uint64_t>& runs) {
    MapAlnOut o{};
    runs.clear();
    auto add = [&](const MapAlnOut& a, const uint64_t* r) {
        for (uint32_t i = 0; i < a.runs; i++) {
            const uint64_t op = r[i] & 3u;
            if (runs.empty() || (runs.back() & 3u) != op) runs.push_back(((r[i] >> 2) + o.ncols) << 2 | op);
        }
        o.ncols += a.ncols; o.eq += a.eq; o.x += a.x; o.ins += a.ins; o.del += a.del; o.cells += a.cells;
    };
    if (left) add(*left, left_runs);
    add(mid, mid_runs);
    if (right) add(*right, right_runs);
    o.runs = (uint32_t)runs.size();
    return o;
}

bool map_check_split(const tksmseq_split_params& s, std::string& err) {
    if (s.chains < 1 || s.chains > 16) { err = "map: split chains must be in [1, 16]"; return false; }
    if (s.overlap < 0) { err = "map: split overlap must not be negative"; return false; }
    if (s.segments < 2 || s.segments > 64) { err = "map: split segments must be in [2, 64]"; return false; }
    return true;
}

uint64_t map_split_anchor_bytes(const tksmseq_split_params& s, int32_t min_count) {
    // a chain, its key before and after the sort, its place in the permutation and its group's entry in the expanded list
    const uint64_t per_chain = sizeof(MapChain) + 8 + 8 + 4 + 4, groups_share = (uint64_t)std::max(min_count, 1);
    return 4 + ((uint64_t)s.chains * per_chain + groups_share - 1) / groups_share;
}

void map_split_ranks(const std::vector<std::pair<uint32_t, uint32_t>>& iv, std::vector<uint32_t>& rank) {
    std::vector<uint32_t> order(iv.size());
    for (uint32_t i = 0; i < order.size(); i++) order[i] = i;
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return iv[a] < iv[b]; });
    rank.assign(iv.size(), 0u);
    for (uint32_t i = 0; i < order.size(); i++) rank[order[i]] = i;
}

int map_targets_select(const tsb::Transcripts& T, const std::vector<int32_t>& contig_of, const std::vector<uint64_t>& contigs, MapTargets& out, std::string& err) {
    out = MapTargets();
    tksmseq_targets_info& info = out.info;
    info.transcripts = T.n();
    for (uint64_t t = 0; t < T.n(); t++) {
        const uint32_t e0 = T.exon_first[t], e1 = T.exon_first[t + 1];
        bool all_empty = true, unknown = false, bad = false;
        uint64_t sum = 0;
        for (uint32_t e = e0; e < e1; e++) {
            all_empty = all_empty && T.ex_start[e] == T.ex_end[e];
            const int32_t ci = contig_of[T.ex_contig[e]];
            if (ci < 0) { unknown = true; continue; }
            if (T.ex_end[e] < T.ex_start[e] || T.ex_end[e] > contigs[2 * (size_t)ci + 1]) bad = true;
            else sum += T.ex_end[e] - T.ex_start[e];
        }
        if (all_empty) { info.skipped_empty++; continue; }
        if (unknown) { info.skipped_unknown_contig++; continue; }
        if (bad) { info.skipped_bad_exon++; continue; }
        const std::string id(T.id_pool.data() + T.id_off[t], T.id_len[t]);
        if (out.n() + 1 >= (1ull << 31)) { err = "map: 2^31 targets or more"; return TKSMSEQ_ELIMIT; }
        if (sum >= (1ull << 31)) { err = "map: target " + id + " has 2^31 letters or more"; return TKSMSEQ_ELIMIT; }
        if (info.letters + sum >= (1ull << 36)) { err = "map: 2^36 target letters or more"; return TKSMSEQ_ELIMIT; }
        // the non-empty exons in file order, and whether they walk one strand of one contig without turning back
        bool proj = true;
        uint32_t cum = 0;
        const size_t first = out.exons.size();
        for (uint32_t e = e0; e < e1; e++) {
            const uint32_t s = T.ex_start[e], en = T.ex_end[e], minus = T.ex_minus[e] ? 1u : 0u;
            if (s == en) continue;
            const uint32_t ci = (uint32_t)contig_of[T.ex_contig[e]];
            if (out.exons.size() > first) {
                const size_t prev = out.exons.size() - 1;
                proj = proj && ci == out.contig.back() && minus == out.minus.back() && (minus ? en <= out.ex_start[prev] : s >= out.ex_end[prev]);
            } else {
                out.contig.push_back(ci);
                out.minus.push_back((uint8_t)minus);
            }
            out.exons.push_back({contigs[2 * (size_t)ci] + s, cum, (en - s) | minus << 31});
            out.ex_start.push_back(s);
            out.ex_end.push_back(en);
            cum += en - s;
        }
        out.tx.push_back((uint32_t)t);
        out.len.push_back((uint32_t)sum);
        out.projectable.push_back(proj ? 1 : 0);
        out.voff.push_back(out.voff.back() + (sum + 31) / 32);
        out.efirst.push_back(out.exons.size());
        info.letters += sum;
        info.projectable += proj;
    }
    info.targets = out.n();
    info.exons = out.exons.size();
    info.image_vwords = out.voff.back();
    if (!out.n()) { err = "map: no transcript of the table can be a target"; return TKSMSEQ_EINVAL; }
    return TKSMSEQ_OK;
}

void map_targets_fasta(const MapTargets& T, const std::vector<std::string>& names, const uint32_t* codes, const uint32_t* valid, int32_t line_width, std::string& out) {
    for (size_t t = 0; t < T.n(); t++) {
        out += '>'; out += names[t]; out += '\n';
        const uint32_t *c = codes + 2 * T.voff[t], *v = valid + T.voff[t];
        const uint32_t len = T.len[t], width = line_width > 0 ? (uint32_t)line_width : len;
        for (uint32_t j = 0; j < len; j++) {
            out += (v[j >> 5] >> (j & 31u)) & 1u ? "ACGT"[(c[j >> 4] >> (2u * (j & 15u))) & 3u] : 'N';
            if ((j + 1) % width == 0 && j + 1 < len) out += '\n';
        }
        out += '\n';
    }
}

uint64_t map_project_line(std::string& line, const MapTargets& T, uint32_t t, const std::string& tx_name, const std::string& contig_name, uint64_t contig_len) {
    std::vector<std::string> f;
    for (size_t at = 0;;) {
        const size_t tab = line.find('\t', at);
        f.push_back(line.substr(at, tab == std::string::npos ? std::string::npos : tab - at));
        if (tab == std::string::npos) break;
        at = tab + 1;
    }
    const uint64_t a = std::stoull(f[7]), b = std::stoull(f[8]);
    const bool minus = T.minus[t] != 0, rel = f[4] == "-";
    const size_t e0 = (size_t)T.efirst[t], e1 = (size_t)T.efirst[t + 1];
    auto exon_len = [&](size_t e) { return (uint64_t)(T.exons[e].len_minus & 0x7FFFFFFFu); };
    auto exon_of = [&](uint64_t x) { size_t e = e0; while (e + 1 < e1 && T.exons[e + 1].cum <= x) e++; return e; };
    auto G = [&](uint64_t x) { const size_t e = exon_of(x); const uint64_t o = x - T.exons[e].cum; return minus ? T.ex_end[e] - 1 - o : T.ex_start[e] + o; };
    const size_t ea = exon_of(a), eb = exon_of(b - 1);
    uint64_t junctions = eb - ea;
    f[4] = rel != minus ? "-" : "+";
    f[5] = contig_name;
    f[6] = std::to_string(contig_len);
    f[7] = std::to_string(minus ? G(b - 1) : G(a));
    f[8] = std::to_string((minus ? G(a) : G(b - 1)) + 1);
    for (size_t i = 12; i < f.size(); i++) {
        if (f[i].compare(0, 5, "cg:Z:") != 0) continue;
        std::vector<std::pair<uint64_t, char>> runs;
        auto add = [&](uint64_t n, char op) { if (!runs.empty() && runs.back().second == op) runs.back().first += n; else runs.emplace_back(n, op); };
        uint64_t x = a;
        size_t e = ea;
        junctions = 0;
        for (size_t at = 5; at < f[i].size();) {
            uint64_t n = 0;
            while (at < f[i].size() && f[i][at] >= '0' && f[i][at] <= '9') n = n * 10 + (uint64_t)(f[i][at++] - '0');
            const char op = f[i][at++];
            if (op == 'I') { add(n, op); continue; }
            while (n) {
                if (x == T.exons[e].cum + exon_len(e) && e + 1 < e1) {      // the next exon's first target-consuming column
                    const uint64_t gap = minus ? T.ex_start[e] - T.ex_end[e + 1] : T.ex_start[e + 1] - T.ex_end[e];
                    if (gap) { add(gap, 'N'); junctions++; }
                    e++;
                }
                uint64_t take = std::min<uint64_t>(n, T.exons[e].cum + exon_len(e) - x);
                if (!take) take = n;                                       // (columns behind the target's end: none in a line of this build)
                add(take, op);
                x += take; n -= take;
            }
        }
        if (minus) std::reverse(runs.begin(), runs.end());
        f[i] = "cg:Z:";
        for (const auto& r : runs) { f[i] += std::to_string(r.first); f[i] += r.second; }
    }
    f.push_back("tx:Z:" + tx_name);
    line.clear();
    for (size_t i = 0; i < f.size(); i++) { if (i) line += '\t'; line += f[i]; }
    return junctions;
}

}  // namespace tkh
