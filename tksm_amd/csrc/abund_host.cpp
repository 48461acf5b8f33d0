// abund_host.cpp -- host side of abundance: PAF reader and interner, lr-br / whitelist readers, --cb-count draws, TSV writer (abund_host.h).
#include "abund_host.h"

#include <zlib.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string_view>

namespace tkh {

namespace {
// what this reader takes of Python's int(): optional blanks (space, CR) and sign, decimal digits, nothing else -- no underscores, no other
// whitespace: it refuses more than the reference does, never less
bool py_int(const char* a, const char* e, long long& v) {
    while (a < e && (*a == ' ' || *a == '\r')) a++;
    while (e > a && (e[-1] == ' ' || e[-1] == '\r')) e--;
    bool neg = false;
    if (a < e && (*a == '+' || *a == '-')) neg = *a++ == '-';
    if (a == e) return false;
    unsigned long long u = 0;
    for (; a < e; a++) {
        if (*a < '0' || *a > '9') return false;
        if (u > (1ull << 52) / 10) return false;
        u = u * 10 + (unsigned long long)(*a - '0');
    }
    v = neg ? -(long long)u : (long long)u;
    return true;
}
constexpr uint64_t LIMIT = 1ull << 31;
}  // namespace

bool parse_paf_abund(const char* text, size_t len, AbundInput& out, std::string& err, bool* limit) {
    out = AbundInput();
    if (limit) *limit = false;
    std::unordered_map<std::string_view, uint32_t> reads, targets;
    std::vector<std::string_view> rviews, tviews;
    // file order first: the read of every line and its four values
    std::vector<uint32_t> line_read, l_tid, l_tstart, l_nmatch, l_blen, l_qlen;
    const char* p = text;
    const char* const end = text + len;
    uint64_t line_no = 0;
    auto fail = [&](const char* what) { err = "PAF line " + std::to_string(line_no) + ": " + what; return false; };
    while (p < end) {
        const char* nl = (const char*)memchr(p, '\n', (size_t)(end - p));
        const char* le = nl ? nl : end;
        line_no++;
        const char* col[12];
        int nc = 0;
        col[nc++] = p;
        for (const char* q = p; q < le && nc < 12; q++) if (*q == '\t') col[nc++] = q + 1;
        if (nc < 11) return fail("fewer than 11 columns");
        if (nc < 12) col[nc] = le + 1;                       // (col[k + 1] - 1 ends column k)
        long long v[4], q = 0;
        static const int used[4] = {7, 9, 10, 1};
        for (int k = 0; k < 4; k++) {
            if (!py_int(col[used[k]], col[used[k] + 1] - 1, k < 3 ? v[k] : q)) return fail("query length, target start, matches and block length (columns 2, 8, 10, 11) must be integers");
            const long long x = k < 3 ? v[k] : q;
            if (x < 0 || (uint64_t)x >= LIMIT) return fail("a value outside [0, 2^31) in columns 2, 8, 10 or 11");
        }
        if (line_read.size() + 1 >= LIMIT) { err = "abundance: 2^31 alignment records or more"; if (limit) *limit = true; return false; }
        const std::string_view rname(col[0], (size_t)(col[1] - 1 - col[0])), tname(col[5], (size_t)(col[6] - 1 - col[5]));
        auto ri = reads.emplace(rname, (uint32_t)rviews.size());
        if (ri.second) { rviews.push_back(rname); l_qlen.push_back((uint32_t)q); }
        auto ti = targets.emplace(tname, (uint32_t)tviews.size());
        if (ti.second) tviews.push_back(tname);
        line_read.push_back(ri.first->second);
        l_tid.push_back(ti.first->second); l_tstart.push_back((uint32_t)v[0]); l_nmatch.push_back((uint32_t)v[1]); l_blen.push_back((uint32_t)v[2]);
        p = nl ? nl + 1 : end;
    }
    out.n_lines = line_no;
    const size_t n_reads = rviews.size(), n_rec = line_read.size();
    out.rnames.assign(rviews.begin(), rviews.end());
    out.tnames.assign(tviews.begin(), tviews.end());
    out.qlen.swap(l_qlen);
    // group by read, file order kept within a read (a counting sort)
    out.rec_off.assign(n_reads + 1, 0);
    for (uint32_t r : line_read) out.rec_off[(size_t)r + 1]++;
    for (size_t r = 0; r < n_reads; r++) out.rec_off[r + 1] += out.rec_off[r];
    std::vector<uint32_t> at(out.rec_off.begin(), out.rec_off.end() - 1);
    out.tid.resize(n_rec); out.tstart.resize(n_rec); out.nmatch.resize(n_rec); out.blen.resize(n_rec);
    for (size_t i = 0; i < n_rec; i++) {
        const uint32_t d = at[line_read[i]]++;
        out.tid[d] = l_tid[i]; out.tstart[d] = l_tstart[i]; out.nmatch[d] = l_nmatch[i]; out.blen[d] = l_blen[i];
    }
    return true;
}

bool abund_read_file(const std::string& path, std::string& out, std::string& err) {
    out.clear();
    gzFile f = gzopen(path.c_str(), "rb");
    if (!f) { err = "Could not open file " + path; return false; }
    gzbuffer(f, 1 << 18);
    char buf[1 << 16];
    int n;
    while ((n = gzread(f, buf, sizeof buf)) > 0) out.append(buf, (size_t)n);
    const bool bad = n < 0;
    gzclose(f);
    if (bad) { err = "Could not read file " + path; return false; }
    return true;
}

bool parse_lr_br(const char* text, size_t len, std::unordered_map<std::string, std::string>& out, std::string& err) {
    out.clear();
    const char* p = text;
    const char* const end = text + len;
    uint64_t line_no = 0;
    while (p < end) {
        const char* nl = (const char*)memchr(p, '\n', (size_t)(end - p));
        const char* le = nl ? nl : end;
        line_no++;
        const char* col[6];
        int nc = 0;
        col[nc++] = p;
        for (const char* q = p; q < le; q++) if (*q == '\t') { if (nc == 5) { nc = 6; break; } col[nc++] = q + 1; }
        if (nc != 5) { err = "lr-br line " + std::to_string(line_no) + ": expected exactly five tab-separated columns"; return false; }
        col[5] = le + 1;
        if (col[3] - 1 - col[2] == 1 && *col[2] == '1') out[std::string(col[0], (size_t)(col[1] - 1 - col[0]))] = std::string(col[4], (size_t)(le - col[4]));
        p = nl ? nl + 1 : end;
    }
    return true;
}

void parse_whitelist(const char* text, size_t len, std::vector<std::string>& out) {
    out.clear();
    const char* p = text;
    const char* const end = text + len;
    while (p < end) {
        const char* nl = (const char*)memchr(p, '\n', (size_t)(end - p));
        const char* le = nl ? nl : end;
        out.emplace_back(p, (size_t)(le - p));
        p = nl ? nl + 1 : end;
    }
}

bool abund_check_args(long long cb_count, const char* lr_br, const char* pattern_, const char* txt_, double dropout, double mu, double sigma, std::string& err) {
    if (cb_count <= 0) return true;
    const std::string pattern = pattern_ ? pattern_ : "", txt = txt_ ? txt_ : "";
    if (lr_br && *lr_br) { err = "--lr-br must not be set with --cb-count"; return false; }
    if (pattern.empty() && txt.empty()) { err = "--cb-pattern or --cb-txt must be set with --cb-count"; return false; }
    for (char c : pattern)
        if (!iupac_letters(c)) { err = std::string("--cb-pattern must contain only valid IUPAC nucleotide letters: <") + c + "> not in A,C,G,T,R,Y,K,M,S,W,B,D,H,V,N"; return false; }
    if (!(dropout >= 0.0 && dropout <= 1.0)) { err = "--cb-dropout must be between 0 and 1"; return false; }
    if (!(sigma > 0.0) || !std::isfinite(sigma) || !std::isfinite(mu)) { err = "--cb-lognorm-params takes MEAN,SD with SD above 0"; return false; }
    return true;
}

void abund_philox(uint64_t seed, uint64_t g, uint32_t stream, uint32_t n, uint32_t w[4]) {
    uint32_t c0 = (uint32_t)g, c1 = (uint32_t)(g >> 32), c2 = stream, c3 = n, k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
    for (int r = 0; r < 10; r++) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c0 = n0; c1 = (uint32_t)p1; c2 = n2; c3 = (uint32_t)p0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    w[0] = c0; w[1] = c1; w[2] = c2; w[3] = c3;
}

const char* iupac_letters(char c) {
    switch (c) {
        case 'A': return "A"; case 'C': return "C"; case 'G': return "G"; case 'T': return "T";
        case 'R': return "AG"; case 'Y': return "CT"; case 'K': return "GT"; case 'M': return "AC"; case 'S': return "CG"; case 'W': return "AT";
        case 'B': return "CGT"; case 'D': return "AGT"; case 'H': return "ACT"; case 'V': return "ACG"; case 'N': return "ACGT";
        default: return nullptr;
    }
}

bool barcodes_from_pattern(const std::string& pattern, uint32_t count, uint64_t seed, std::vector<std::string>& out) {
    out.clear();
    for (char c : pattern) if (!iupac_letters(c)) return false;
    for (uint32_t b = 0; b < count; b++) {
        std::string s(pattern.size(), 'N');
        for (size_t p = 0; p < pattern.size(); p++) {
            const char* set = iupac_letters(pattern[p]);
            uint32_t w[4];
            abund_philox(seed, b, ST_ABUND_BC, (uint32_t)p, w);
            s[p] = set[(size_t)(((uint64_t)w[0] * strlen(set)) >> 32)];
        }
        out.push_back(std::move(s));
    }
    return true;
}

void barcodes_from_whitelist(const std::vector<std::string>& list, uint32_t count, uint64_t seed, std::vector<std::string>& out) {
    out.clear();
    for (uint32_t b = 0; b < count && !list.empty(); b++) {
        uint32_t w[4];
        abund_philox(seed, b, ST_ABUND_BC_TXT, 0, w);
        out.push_back(list[(size_t)(((uint64_t)w[0] * (uint64_t)list.size()) >> 32)]);
    }
}

void cell_cdf(uint32_t count, uint64_t seed, double mu, double sigma, double dropout, std::vector<double>& cdf) {
    cdf.assign((size_t)count + 1, 0.0);
    double acc = 0.0;
    for (uint32_t b = 0; b < count; b++) {
        uint32_t w[4];
        abund_philox(seed, b, ST_ABUND_WEIGHT, 0, w);
        const double u1 = ((double)w[0] + 1.0) * (1.0 / 4294967296.0), u2 = (double)w[1] * (1.0 / 4294967296.0);
        const double z = std::sqrt(-2.0 * std::log(u1)) * std::cos(6.283185307179586 * u2);
        const double wt = dropout >= 1.0 ? 0.0 : std::exp(mu + sigma * z);
        acc += wt;
        cdf[b] = acc;
    }
    cdf[count] = dropout >= 1.0 ? 1.0 : acc + acc * dropout / (1.0 - dropout);
}

bool abundance_tsv(const std::vector<AbundRow>& rows, const std::vector<std::string>& tnames, const std::vector<std::string>& cells, std::string& out) {
    out = "target_id\ttpm\tcell\n";
    char num[400];
    for (const AbundRow& r : rows) {
        if (r.tid >= tnames.size() || r.cell >= cells.size()) return false;
        const double tpm = r.a * 1000000.0;
        if (tpm < 0.001) continue;
        snprintf(num, sizeof num, "%.3f", tpm);
        if (!strcmp(num, "0.000")) continue;
        out += tnames[r.tid]; out += '\t'; out += num; out += '\t'; out += cells[r.cell]; out += '\n';
    }
    return true;
}

bool write_abundance_file(const std::string& path, const std::string& text, std::string& err) {
    const std::string tmp = path + ".tmp";
    bool ok;
    if (path.size() >= 3 && path.compare(path.size() - 3, 3, ".gz") == 0) {
        gzFile f = gzopen(tmp.c_str(), "wb");
        if (!f) { err = "cannot write " + path; return false; }
        ok = true;
        for (size_t at = 0; at < text.size() && ok; at += 1u << 30) {
            const unsigned n = (unsigned)std::min<size_t>(1u << 30, text.size() - at);
            ok = gzwrite(f, text.data() + at, n) == (int)n;
        }
        ok = (gzclose(f) == Z_OK) && ok;
    } else {
        FILE* f = fopen(tmp.c_str(), "wb");
        if (!f) { err = "cannot write " + path; return false; }
        ok = fwrite(text.data(), 1, text.size(), f) == text.size();
        ok = (fclose(f) == 0) && ok;
    }
    if (!ok || rename(tmp.c_str(), path.c_str()) != 0) { remove(tmp.c_str()); err = "cannot write " + path; return false; }
    return true;
}

}  // namespace tkh
