// mut_host.cpp -- the variant table of mutate: reader and normal form (see mut_host.h).  Host only.
#include "mut_host.h"

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <map>

namespace mut {

namespace {

inline bool is_space(char c) { return c == ' ' || c == '\t' || c == '\v' || c == '\f' || c == '\r'; }
inline bool is_digit(char c) { return c >= '0' && c <= '9'; }

// an integer in [0, 2^31 - 1], digits only
bool parse_pos(const char* p, size_t n, uint32_t& out) {
    if (!n) return false;
    uint64_t v = 0;
    for (size_t i = 0; i < n; i++) {
        if (!is_digit(p[i])) return false;
        v = v * 10 + (uint64_t)(p[i] - '0');
        if (v > MAX_POS) return false;
    }
    out = (uint32_t)v;
    return true;
}

struct Point { uint32_t pos; uint64_t line; uint64_t info; const char* seq; uint32_t seq_len; };
struct Contig { std::vector<std::pair<uint32_t, uint32_t>> dels; std::vector<Point> pts; };

// names in the order the device searches them: shorter first, then bytes
struct NameLess {
    bool operator()(const std::string& a, const std::string& b) const { return a.size() != b.size() ? a.size() < b.size() : memcmp(a.data(), b.data(), a.size()) < 0; }
};

}  // namespace

int Variants::find(const char* name, size_t len) const {
    size_t lo = 0, hi = names.size();
    while (lo < hi) {
        const size_t mid = (lo + hi) / 2;
        const std::string& m = names[mid];
        const int c = m.size() != len ? (m.size() < len ? -1 : 1) : memcmp(m.data(), name, len);
        if (c == 0) return (int)mid;
        if (c < 0) lo = mid + 1; else hi = mid;
    }
    return -1;
}

bool parse_variants(const char* text, size_t len, const std::string& name, Variants& out, std::string& err, bool& limit) {
    limit = false;
    std::map<std::string, Contig, NameLess> contigs;
    Variants v;
    uint64_t line = 0;
    auto fail = [&](const char* why, bool is_limit = false) {
        err = name + ":" + std::to_string(line) + ": " + why;
        limit = is_limit;
        return false;
    };
    size_t a = 0;
    while (a < len) {
        size_t b = a;
        while (b < len && text[b] != '\n') b++;
        line++;
        // the first three fields of [a, b)
        const char* f[3] = {nullptr, nullptr, nullptr}; size_t fl[3] = {0, 0, 0};
        size_t i = a;
        int nf = 0;
        while (nf < 3) {
            while (i < b && is_space(text[i])) i++;
            if (i == b) break;
            const size_t j = i;
            while (i < b && !is_space(text[i])) i++;
            f[nf] = text + j; fl[nf] = i - j; nf++;
        }
        a = b + 1;
        if (nf == 0) continue;
        if (nf < 3) return fail("a variant line has three fields: CONTIG POS MOD");
        if (v.rows + 1 >= 0x80000000ull) return fail("a variant table of 2^31 rows or more is not supported", true);
        v.rows++;
        uint32_t pos = 0;
        if (!parse_pos(f[1], fl[1], pos)) return fail("POS is not an integer in [0, 2147483647]");
        const char* m = f[2]; const size_t ml = fl[2];
        bool digits = true;
        for (size_t k = 0; k < ml; k++) digits = digits && is_digit(m[k]);
        Contig& c = contigs[std::string(f[0], fl[0])];
        if (digits) {
            uint32_t end = 0;
            if (!parse_pos(m, ml, end)) return fail("the end of a deletion is not an integer in [0, 2147483647]");
            v.deletions++;
            if (end != pos) c.dels.emplace_back(std::min(pos, end), std::max(pos, end));
        } else if (ml == 1) {
            if (m[0] == '.') return fail("an SNV needs a letter: a lone '.' changes nothing");
            v.snvs++;
            c.pts.push_back(Point{pos, line, PT_LETTER | ((uint64_t)(uint8_t)m[0] << 32), nullptr, 0});
        } else {
            if (ml - 1 > MAX_INSERTION) return fail("an insertion of more than 1048576 letters is not supported", true);
            v.insertions++;
            c.pts.push_back(Point{pos, line, PT_INSERTION | (m[0] == '.' ? 0ull : PT_LETTER | ((uint64_t)(uint8_t)m[0] << 32)), m + 1, (uint32_t)(ml - 1)});
        }
    }
    // the normal form, contig by contig in the search order
    for (auto& kv : contigs) {
        Contig& c = kv.second;
        v.names.push_back(kv.first);
        std::sort(c.dels.begin(), c.dels.end());
        const size_t d0 = v.del_from.size();
        for (auto& d : c.dels) {
            if (v.del_from.size() > d0 && d.first <= v.del_to.back()) v.del_to.back() = std::max(v.del_to.back(), d.second);
            else { v.del_from.push_back(d.first); v.del_to.push_back(d.second); }
        }
        std::stable_sort(c.pts.begin(), c.pts.end(), [](const Point& x, const Point& y) { return x.pos < y.pos; });      // (pushed in line order)
        size_t d = d0;
        for (const Point& p : c.pts) {
            while (d < v.del_to.size() && v.del_to[d] <= p.pos) d++;
            if (d < v.del_from.size() && v.del_from[d] <= p.pos) { v.dropped_points++; continue; }
            uint64_t info = p.info;
            if (info & PT_INSERTION) {
                info |= (uint64_t)v.n_insertions_kept();
                v.ins_ent.push_back(v.ins_pool.size()); v.ins_ent.push_back(p.seq_len);
                v.ins_pool.append(p.seq, p.seq_len);
            }
            v.pt_pos.push_back(p.pos); v.pt_info.push_back(info);
        }
        v.del_first.push_back((uint32_t)v.del_from.size());
        v.pt_first.push_back((uint32_t)v.pt_pos.size());
    }
    v.deleted_ranges = v.del_from.size();
    out = std::move(v);
    return true;
}

bool read_variants(const std::string& path, Variants& out, std::string& err, bool& limit, bool& io) {
    io = false; limit = false;
    FILE* f = fopen(path.c_str(), "rb");
    if (!f) { err = "Could not open variant table " + path + "!"; io = true; return false; }
    std::string text;
    char buf[1 << 16];
    size_t n;
    while ((n = fread(buf, 1, sizeof buf, f)) > 0) text.append(buf, n);
    fclose(f);
    return parse_variants(text.data(), text.size(), path, out, err, limit);
}

}  // namespace mut
