// filter_host.h -- the condition parser of `filter` (FilterCondition's constructor, src/filter.cpp:24-115), shared by tksmseq_filter
// (mdf_move.cpp) and `tksm filter` (mdf_modules.cpp), which checks its conditions before it opens a file or a device.
#pragma once
#include <cerrno>
#include <climits>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../include/tksmseq.h"

namespace tkh {

struct FilterCond {
    int kind = TKSMSEQ_FLT_TEXT, cmp = 0;   // TKSMSEQ_FLT_INFO / _SIZE / _LOCUS once parsed; size: TKSMSEQ_FLT_LT .. _NE
    std::string key;                        // info: the key; locus: the contig name
    long long value = 0;                    // size: N
    bool ranged = false;                    // locus: CHR:S-E or CHR:S given
    long long start = 0, end = 0;           // ... [S, E), or [S, S + 1)
};

// rsplit (src/util.h:175-185): every piece between delimiters, empty ones included
inline std::vector<std::string> filter_split(const std::string& s, char delim) {
    std::vector<std::string> out;
    size_t a = 0, b;
    while ((b = s.find(delim, a)) != std::string::npos) { out.push_back(s.substr(a, b - a)); a = b + 1; }
    out.push_back(s.substr(a));
    return out;
}

// std::stoi: leading white space, a sign, digits; what follows the digits is ignored; no digits or a value outside int: no number
inline bool filter_stoi(const std::string& s, long long& out) {
    errno = 0;
    char* e = nullptr;
    const long v = strtol(s.c_str(), &e, 10);
    if (e == s.c_str() || errno == ERANGE || v < INT_MIN || v > INT_MAX) return false;
    out = v;
    return true;
}

// false: "Invalid condition: <text>".  Refused beyond what the reference throws on: an unknown kind (it leaves an empty
// std::function, called later), a negative size value (it wraps to unsigned) and a negative coordinate.
inline bool parse_filter_condition(const std::string& text, FilterCond& c) {
    const std::vector<std::string> f = filter_split(text, ' ');
    if (f.size() != 2) return false;
    c = FilterCond();
    if (f[0] == "info") { c.kind = TKSMSEQ_FLT_INFO; c.key = f[1]; return true; }
    if (f[0] == "size") {
        if (f[1].size() < 2) return false;
        const std::string op = f[1][1] == '=' ? f[1].substr(0, 2) : f[1].substr(0, 1);
        static const char* ops[6] = {"<", "<=", ">", ">=", "==", "!="};
        c.kind = TKSMSEQ_FLT_SIZE; c.cmp = -1;
        for (int k = 0; k < 6; k++) if (op == ops[k]) c.cmp = k;
        return filter_stoi(f[1].substr(op.size()), c.value) && c.cmp >= 0 && c.value >= 0;      // (the number first, as the reference: either way refused)
    }
    if (f[0] == "locus") {
        const std::vector<std::string> r = filter_split(f[1], ':');
        c.kind = TKSMSEQ_FLT_LOCUS; c.key = r[0];
        if (r.size() == 1) return true;
        const std::vector<std::string> se = filter_split(r[1], '-');
        c.ranged = true;
        if (!filter_stoi(se[0], c.start)) return false;
        if (se.size() == 1) c.end = c.start + 1;
        else if (!filter_stoi(se[1], c.end)) return false;
        return c.start >= 0 && c.end >= 0;
    }
    return false;
}

}  // namespace tkh
