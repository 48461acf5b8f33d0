// bm_host.cpp -- host side of barcode-match (see bm_host.h; the rules are stated in include/tksmseq.h).
#include "bm_host.h"

#include <algorithm>
#include <cstring>
#include <unordered_map>

namespace tkh {

bool bm_is_acgt(const std::string& s, size_t lo, size_t hi) {
    if (s.size() < lo || s.size() > hi) return false;
    for (char c : s) if (bm_code((uint8_t)c) > 3u) return false;
    return true;
}

bool parse_bm_whitelist(const char* text, size_t len, bool revcomp, BmWhitelist& out, std::string& err, bool* limit) {
    std::unordered_map<uint64_t, uint64_t> seen;       // key -> line
    uint64_t line_no = 0;
    for (size_t pos = 0; pos < len;) {
        const char* nl = (const char*)memchr(text + pos, '\n', len - pos);
        size_t b = pos, e = nl ? (size_t)(nl - text) : len;
        pos = e + 1;
        line_no++;
        if (e > b && text[e - 1] == '\r') e--;
        if (e == b) continue;
        auto fail = [&](const std::string& what) { err = "whitelist line " + std::to_string(line_no) + ": " + what; return false; };
        if (out.text.size() >= (1u << 27) - 1u) { err = "barcode-match: 2^27 whitelist lines or more"; if (limit) *limit = true; return false; }
        const size_t L = e - b;
        if (L < 4 || L > 32) return fail("a barcode of " + std::to_string(L) + " letters (4 to 32 are possible)");
        if (out.L && L != out.L) return fail("a barcode of " + std::to_string(L) + " letters after barcodes of " + std::to_string(out.L));
        out.L = (uint32_t)L;
        uint64_t key = 0;
        for (size_t i = 0; i < L; i++) {
            const uint32_t c = bm_code((uint8_t)text[b + i]);
            if (c > 3u) return fail("a letter outside ACGT");
            // letter i of the matched spelling: with revcomp the complement of the file's letter L - 1 - i
            if (revcomp) key |= (uint64_t)(3u - c) << (2 * (L - 1 - i)); else key |= (uint64_t)c << (2 * i);
        }
        const auto ins = seen.emplace(key, line_no);
        if (!ins.second) return fail("the barcode of line " + std::to_string(ins.first->second) + " again");
        out.text.emplace_back(text + b, L);
        out.keys.push_back(key);
    }
    if (out.text.empty()) { err = "the whitelist is empty"; return false; }
    return true;
}

void bm_pack_ends(const MsReads& reads, uint32_t r0, uint32_t r1, uint32_t letters, std::vector<uint32_t>& codes, std::vector<uint32_t>& valid,
                  std::vector<uint32_t>& len) {
    const size_t n = r1 - r0, n2 = 2 * n, wc = (letters + 15u) / 16u, wv = (letters + 31u) / 32u;
    codes.assign(wc * n2, 0u);
    valid.assign(wv * n2, 0u);
    len.assign(n, 0u);
    // byte -> code of the byte (forward) and of its complement (reverse); 4: outside ACGT
    uint8_t fwd[256], rev[256];
    for (int b = 0; b < 256; b++) { fwd[b] = (uint8_t)bm_code((uint8_t)b); rev[b] = (uint8_t)bm_code(bm_complement((uint8_t)b)); }
    // 32 lanes (16 reads) are packed side by side first, so that a word row of the transposed arrays is written 128 bytes at a time
    constexpr size_t GROUP = 32;
    std::vector<uint32_t> gc(GROUP * wc), gv(GROUP * wv);
    for (size_t lane0 = 0; lane0 < n2; lane0 += GROUP) {
        const size_t lanes = std::min(GROUP, n2 - lane0);
        std::fill(gc.begin(), gc.end(), 0u);
        std::fill(gv.begin(), gv.end(), 0u);
        for (size_t g = 0; g < lanes; g++) {
            const size_t k = (lane0 + g) / 2;
            const bool o = ((lane0 + g) & 1u) != 0;
            const uint64_t off = reads.off[r0 + k], length = reads.off[r0 + k + 1] - off;
            const uint32_t m = (uint32_t)std::min<uint64_t>(length, letters);
            len[k] = m;
            uint32_t *c_row = gc.data() + g * wc, *v_row = gv.data() + g * wv;
            const uint8_t* base = reads.bases.data() + off;
            for (uint32_t j0 = 0; j0 < m; j0 += 32u) {       // 32 letters: two code words and one validity word
                uint64_t cw = 0;
                uint32_t vw = 0;
                const uint32_t t_end = std::min(32u, m - j0);
                for (uint32_t t = 0; t < t_end; t++) {
                    const uint32_t j = j0 + t, c = o ? rev[base[length - 1 - j]] : fwd[base[j]], ok = c <= 3u ? 1u : 0u;
                    cw |= (uint64_t)(c & 3u & (0u - ok)) << (2u * t);
                    vw |= ok << t;
                }
                c_row[j0 >> 4] = (uint32_t)cw;
                if (t_end > 16u) c_row[(j0 >> 4) + 1u] = (uint32_t)(cw >> 32);
                v_row[j0 >> 5] = vw;
            }
        }
        for (size_t w = 0; w < wc; w++) for (size_t g = 0; g < lanes; g++) codes[w * n2 + lane0 + g] = gc[g * wc + w];
        for (size_t w = 0; w < wv; w++) for (size_t g = 0; g < lanes; g++) valid[w * n2 + lane0 + g] = gv[g * wv + w];
    }
}

void bm_oriented_slice(const MsReads& reads, uint32_t r, bool reverse, uint32_t start, uint32_t n, std::string& out) {
    const uint64_t off = reads.off[r], length = reads.off[r + 1] - off;
    out.clear();
    for (uint32_t j = start; j < start + n && j < length; j++) out.push_back((char)(reverse ? bm_complement(reads.bases[off + length - 1 - j]) : reads.bases[off + j]));
}

}  // namespace tkh
