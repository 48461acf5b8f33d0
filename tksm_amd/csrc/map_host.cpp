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

void map_paf_line(const std::string& qname, uint32_t qlen, const std::string& tname, uint64_t tlen, const MapChain& c, uint32_t mapq, bool primary, std::string& out) {
    const bool rel = (c.tr & 1u) != 0;
    // a reverse chain lies in the reverse-complemented read: the interval is given in the read as it was sequenced
    const uint32_t qstart = rel ? qlen - c.qe : c.qs, qend = rel ? qlen - c.qs : c.qe;
    const uint32_t blen = std::max(c.tend - c.tstart, c.qe - c.qs);
    out += qname; out += '\t';
    out += std::to_string(qlen); out += '\t';
    out += std::to_string(qstart); out += '\t';
    out += std::to_string(qend); out += '\t';
    out += rel ? '-' : '+'; out += '\t';
    out += tname; out += '\t';
    out += std::to_string(tlen); out += '\t';
    out += std::to_string(c.tstart); out += '\t';
    out += std::to_string(c.tend); out += '\t';
    out += std::to_string(c.nmatch); out += '\t';
    out += std::to_string(blen); out += '\t';
    out += std::to_string(mapq); out += '\t';
    out += primary ? "tp:A:P" : "tp:A:S";
    out += "\tcm:i:"; out += std::to_string(c.cnt);
    out += "\ts1:i:"; out += std::to_string(c.score);
    out += '\n';
}

}  // namespace tkh
