// ms_host.cpp -- host side of model-sequence (see ms_host.h; the rules are stated in include/tksmseq.h).
#include "ms_host.h"

#include "../../include/tksmseq.h"
#include "abund_host.h"

#include <algorithm>
#include <cstddef>
#include <cstdio>
#include <cstring>

namespace tkh {

namespace {

// the next line of text[pos, len): [b, e) without its '\n' and a '\r' before it; false at the end of the text
bool next_line(const char* text, size_t len, size_t& pos, size_t& b, size_t& e) {
    if (pos >= len) return false;
    b = pos;
    const char* nl = (const char*)memchr(text + pos, '\n', len - pos);
    e = nl ? (size_t)(nl - text) : len;
    pos = e + 1;
    if (e > b && text[e - 1] == '\r') e--;
    return true;
}

uint8_t upper(uint8_t c) { return c >= 'a' && c <= 'z' ? (uint8_t)(c - 32) : c; }

// an integer in [0, 2^31): digits only
bool small_int(const char* b, const char* e, uint32_t& out) {
    if (b == e || e - b > 10) return false;
    uint64_t v = 0;
    for (const char* p = b; p < e; p++) {
        if (*p < '0' || *p > '9') return false;
        v = v * 10 + (uint64_t)(*p - '0');
    }
    if (v >= (1ull << 31)) return false;
    out = (uint32_t)v;
    return true;
}

}  // namespace

bool parse_fastq(const char* text, size_t len, MsReads& out, std::string& err) {
    size_t pos = 0, b[4], e[4];
    uint64_t rec = 0;
    auto fail = [&](const char* what) { err = "FASTQ record " + std::to_string(rec) + ": " + what; return false; };
    while (pos < len) {
        rec++;
        // (empty lines between records and at the end of the file are passed over)
        do { if (!next_line(text, len, pos, b[0], e[0])) return true; } while (e[0] == b[0]);
        for (int i = 1; i < 4; i++)
            if (!next_line(text, len, pos, b[i], e[i])) return fail("the file ends inside the record");
        if (text[b[0]] != '@') return fail("the header does not start with '@'");
        if (e[2] == b[2] || text[b[2]] != '+') return fail("the third line does not start with '+'");
        if (e[1] - b[1] != e[3] - b[3]) return fail("sequence and quality differ in length");
        size_t ne = b[0] + 1;
        while (ne < e[0] && text[ne] != ' ' && text[ne] != '\t') ne++;
        if (out.size() >= 0xFFFFFFFFull) { err = "model-sequence: 2^32 reads or more"; return false; }
        if (!out.index.emplace(std::string(text + b[0] + 1, ne - b[0] - 1), (uint32_t)out.size()).second) return fail("a read of this name came before");
        for (size_t i = b[3]; i < e[3]; i++) {
            const int q = (int)(unsigned char)text[i] - 33;
            if (q < 0 || q > 93) return fail("a quality outside '!' .. '~'");
        }
        for (size_t i = b[1]; i < e[1]; i++) out.bases.push_back(upper((uint8_t)text[i]));
        for (size_t i = b[3]; i < e[3]; i++) out.quals.push_back((uint8_t)((unsigned char)text[i] - 33));
        out.off.push_back(out.bases.size());
    }
    return true;
}

int load_fastq_list(const std::string& list, MsReads& out, std::string& err, uint64_t read_limit) {
    std::string text, e;
    for (size_t a = 0; a <= list.size();) {
        size_t b = list.find(',', a);
        if (b == std::string::npos) b = list.size();
        if (b > a) {
            const std::string path = list.substr(a, b - a);
            text.clear();
            if (!abund_read_file(path, text, err)) return TKSMSEQ_EIO;
            if (!parse_fastq(text.data(), text.size(), out, e)) { err = path + ": " + e; return e.compare(0, 5, "FASTQ") ? TKSMSEQ_ELIMIT : TKSMSEQ_EINVAL; }
            if (read_limit && out.size() >= read_limit) { err.clear(); return TKSMSEQ_ELIMIT; }
        }
        a = b + 1;
    }
    return TKSMSEQ_OK;
}

bool parse_paf_ms(const char* text, size_t len, const MsReads& reads, const std::unordered_map<std::string, uint32_t>& targets,
                  const std::vector<uint64_t>& target_len, uint64_t max_alignments, MsAlignments& out, std::string& err) {
    size_t pos = 0, lb, le;
    uint64_t line_no = 0;
    std::vector<std::pair<size_t, size_t>> col;
    std::vector<uint32_t> ops;
    while (next_line(text, len, pos, lb, le)) {
        line_no++;
        if (max_alignments && out.aln.size() >= max_alignments) break;
        if (le == lb) continue;
        out.lines++;
        auto fail = [&](const std::string& what) { err = "PAF line " + std::to_string(line_no) + ": " + what; return false; };
        col.clear();
        for (size_t a = lb;;) {
            const char* t = (const char*)memchr(text + a, '\t', le - a);
            const size_t z = t ? (size_t)(t - text) : le;
            col.emplace_back(a, z);
            if (!t) break;
            a = z + 1;
        }
        if (col.size() < 12) return fail("fewer than 12 columns");
        const char *cg = nullptr, *cg_end = nullptr;
        bool supplementary = false;
        for (size_t c = 12; c < col.size(); c++) {
            const char* p = text + col[c].first;
            const size_t n = col[c].second - col[c].first;
            if (n >= 5 && !memcmp(p, "cg:Z:", 5)) { cg = p + 5; cg_end = p + n; }
            else if (n == 6 && !memcmp(p, "tp:A:S", 6)) supplementary = true;
        }
        if (!cg) { out.no_cigar++; continue; }
        if (supplementary) { out.supplementary++; continue; }
        const auto rd = reads.index.find(std::string(text + col[0].first, col[0].second - col[0].first));
        if (rd == reads.index.end()) { out.unknown_read++; continue; }
        const auto tg = targets.find(std::string(text + col[5].first, col[5].second - col[5].first));
        if (tg == targets.end()) { out.unknown_target++; continue; }
        // the ops: digits then a letter; a letter outside M = X I D skips the line, anything else is malformed
        ops.clear();
        uint64_t used_q = 0, used_t = 0;
        bool other_op = false, malformed = cg == cg_end;
        for (const char* p = cg; p < cg_end && !malformed;) {
            const char* d = p;
            while (p < cg_end && *p >= '0' && *p <= '9') p++;
            uint32_t n = 0;
            if (p == cg_end || !small_int(d, p, n) || n >= (1u << 30)) { malformed = true; break; }
            const char op = *p++;
            int code;
            if (op == 'M' || op == '=' || op == 'X') code = MS_OP_M;
            else if (op == 'I') code = MS_OP_I;
            else if (op == 'D') code = MS_OP_D;
            else if ((op >= 'A' && op <= 'Z') || (op >= 'a' && op <= 'z')) { other_op = true; continue; }
            else { malformed = true; break; }
            if (!n) continue;
            if (code != MS_OP_D) used_q += n;
            if (code != MS_OP_I) used_t += n;
            if (!ops.empty() && (int)(ops.back() & 3u) == code && (ops.back() >> 2) + n < (1u << 30)) ops.back() += n << 2;
            else ops.push_back(n << 2 | (uint32_t)code);
        }
        if (malformed) return fail("the cg:Z: tag is no CIGAR");
        if (other_op) { out.cigar_op++; continue; }
        MsAln a{};
        a.read = rd->second; a.tid = tg->second;
        uint32_t* const dst[6] = {&a.qlen, &a.qstart, &a.qend, nullptr, &a.tstart, &a.tend};
        const int cols[6] = {1, 2, 3, 0, 7, 8};
        for (int i = 0; i < 6; i++)
            if (dst[i] && !small_int(text + col[cols[i]].first, text + col[cols[i]].second, *dst[i]))
                return fail("column " + std::to_string(cols[i] + 1) + " is no integer in [0, 2^31)");
        const size_t sl = col[4].second - col[4].first;
        if (sl != 1 || (text[col[4].first] != '+' && text[col[4].first] != '-')) return fail("column 5 is neither + nor -");
        a.strand = text[col[4].first] == '-';
        if (a.qstart > a.qend || a.qend > a.qlen) return fail("the query range is not inside the query");
        if (a.tstart > a.tend || a.tend > target_len[a.tid]) return fail("the target range is not inside the reference contig");
        if (a.qlen != reads.off[a.read + 1] - reads.off[a.read]) return fail("column 2 differs from the length of the FASTQ read");
        if (used_q != a.qend - a.qstart || used_t != a.tend - a.tstart) return fail("the CIGAR does not consume the aligned ranges");
        if (out.ops.size() + ops.size() >= 0xFFFFFFFFull) { err = "model-sequence: 2^32 ops or more"; return false; }
        a.op_off = (uint32_t)out.ops.size(); a.n_ops = (uint32_t)ops.size();
        out.ops.insert(out.ops.end(), ops.begin(), ops.end());
        out.aln.push_back(a);
    }
    return true;
}

void error_model_text(int k, const std::vector<MsErrRow>& rows, std::string& out) {
    out.clear();
    out.reserve(rows.size() * 64);
    char kmer[16], alt[MS_MAX_ALT_LEN + 4], num[64];
    for (size_t idx = 0; idx < rows.size(); idx++) {
        const MsErrRow& r = rows[idx];
        for (int j = 0; j < k; j++) kmer[j] = "ACGT"[(idx >> (2 * (k - 1 - j))) & 3];
        kmer[k] = 0;
        out += kmer;
        if (!r.total) { out += ",1.000000;\n"; continue; }
        snprintf(num, sizeof num, ",%.6f;", (double)r.self / (double)r.total);
        out += num;
        for (uint32_t a = 0; a < r.n_alt && a < (uint32_t)MS_MAX_ALT; a++) {
            const int n = std::min<int>((int)(r.alt[a] >> 24), MS_MAX_ALT_LEN);
            for (int j = 0; j < n; j++) alt[j] = "ACGT"[(r.alt[a] >> (22 - 2 * j)) & 3];
            alt[n] = 0;
            out += alt;
            snprintf(num, sizeof num, ",%.6f;", (double)r.count[a] / (double)r.total);
            out += num;
        }
        out += '\n';
    }
}

std::string ms_key_text(uint64_t key) {
    const int n = std::min<int>((int)(key >> 58), MS_KEY_MAX);
    std::string s((size_t)n, '=');
    for (int j = 0; j < n; j++) s[(size_t)j] = "=DIX"[(key >> (56 - 2 * j)) & 3];
    return s;
}

bool qscore_select(const std::vector<MsQRow>& best, const MsQRow forced[3], uint64_t max_output, std::vector<MsQRow>& out, std::string& err) {
    for (int f = 0; f < 3; f++)
        if (!forced[f].n) { err = "model-sequence: no '" + ms_key_text(forced[f].key) + "' column in any used alignment (the q-score model needs the keys =, X and I)"; return false; }
    out.assign(best.begin(), best.begin() + (std::ptrdiff_t)std::min<uint64_t>(best.size(), max_output));
    auto is_forced = [&](uint64_t key) { return key == forced[0].key || key == forced[1].key || key == forced[2].key; };
    for (int f = 0; f < 3; f++) {
        bool there = false;
        for (const auto& r : out) there = there || r.key == forced[f].key;
        if (there) continue;
        if (out.size() >= max_output)
            for (size_t i = out.size(); i-- > 0;)
                if (!is_forced(out[i].key)) { out.erase(out.begin() + (std::ptrdiff_t)i); break; }
        out.push_back(forced[f]);
    }
    std::stable_sort(out.begin(), out.end(), [](const MsQRow& a, const MsQRow& b) { return a.n != b.n ? a.n > b.n : a.key < b.key; });
    return true;
}

namespace {
void qscore_line(const std::string& name, const MsQRow& r, std::string& out) {
    char num[64];
    out += name;
    snprintf(num, sizeof num, ";%llu;", (unsigned long long)r.n);
    out += num;
    for (int q = 0; q < MS_Q; q++) {
        if (!r.count[q]) continue;
        int n = snprintf(num, sizeof num, "%d:%.6f", q, (double)r.count[q] / (double)r.n);
        while (n > 0 && num[n - 1] == '0') n--;
        out.append(num, (size_t)n);
        out += ',';
    }
    out += '\n';
}
}  // namespace

void qscore_model_text(const MsQRow& overall, const std::vector<MsQRow>& rows, std::string& out) {
    out.clear();
    qscore_line("overall", overall, out);
    for (const auto& r : rows) qscore_line(ms_key_text(r.key), r, out);
}

}  // namespace tkh
