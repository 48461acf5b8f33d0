// kde_host.cpp -- host side of model-truncation: PAF reader, end-ratio histogram, model writer (see kde_host.h).
#include "kde_host.h"

#include <cerrno>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>


namespace tkh {

namespace {
// Python's int(): optional blanks and sign, decimal digits, nothing else
bool py_int(const char* a, const char* e, long long& v) {
    while (a < e && (*a == ' ' || *a == '\r')) a++;
    while (e > a && (e[-1] == ' ' || e[-1] == '\r')) e--;
    bool neg = false;
    if (a < e && (*a == '+' || *a == '-')) neg = *a++ == '-';
    if (a == e) return false;
    unsigned long long u = 0;
    for (; a < e; a++) {
        if (*a < '0' || *a > '9') return false;
        if (u > (1ull << 52) / 10) return false;             // beyond what a double holds exactly: no alignment has such a coordinate
        u = u * 10 + (unsigned long long)(*a - '0');
    }
    v = neg ? -(long long)u : (long long)u;
    return true;
}
}  // namespace

bool parse_paf_sample(const char* text, size_t len, bool model_lengths, PafSample& out, std::string& err) {
    out.xy.clear(); out.ratios.clear();
    static const char tag[] = "tp:A:P";
    const char* p = text;
    const char* const end = text + len;
    uint64_t line_no = 0;
    while (p < end) {
        const char* nl = (const char*)memchr(p, '\n', (size_t)(end - p));
        const char* le = nl ? nl : end;
        line_no++;
        bool primary = false;
        for (const char* q = p; q + 6 <= le && !primary; q++) primary = !memcmp(q, tag, 6);
        if (primary) {
            const char* col[10];
            int nc = 0;
            col[nc++] = p;
            for (const char* q = p; q < le && nc < 10; q++) if (*q == '\t') col[nc++] = q + 1;
            if (nc < 10) col[nc] = le + 1;                   // (col[k + 1] - 1 ends column k)
            long long tlen = 0, tstart = 0, tend = 0;
            if (nc < 9 || !py_int(col[6], col[7] - 1, tlen) || !py_int(col[7], col[8] - 1, tstart) || !py_int(col[8], col[9] - 1, tend)) {
                err = "PAF line " + std::to_string(line_no) + ": target length, start and end (columns 7 - 9) must be integers";
                return false;
            }
            const bool plus = col[5] - 1 - col[4] == 1 && *col[4] == '+';
            long long trunc;
            if (model_lengths) {
                const long long alen = tend - tstart;
                trunc = tlen - alen;
                out.xy.push_back((double)tlen); out.xy.push_back((double)alen);
                if (trunc != 0) out.ratios.push_back((double)(plus ? tlen - tend : tstart) / (double)trunc);
            } else {
                trunc = tstart + (tlen - tend);
                out.xy.push_back((double)trunc); out.xy.push_back((double)tlen);
                if (trunc > 0) out.ratios.push_back((double)(plus ? tlen - tend : tstart) / (double)trunc);
            }
        }
        p = nl ? nl + 1 : end;
    }
    return true;
}

bool read_paf_sample(const std::string& path, bool model_lengths, PafSample& out, std::string& err) {
    FILE* f = fopen(path.c_str(), "rb");
    if (!f) { err = "Could not open file " + path; return false; }
    std::string text;
    char buf[1 << 16];
    size_t n;
    while ((n = fread(buf, 1, sizeof buf, f)) > 0) text.append(buf, n);
    const bool bad = ferror(f) != 0;
    fclose(f);
    if (bad) { err = "Could not read file " + path; return false; }
    return parse_paf_sample(text.data(), text.size(), model_lengths, out, err);
}

void end_histogram(const std::vector<double>& ratios, std::vector<long long>& counts, std::vector<double>& labels) {
    double edge[101];
    for (int k = 0; k <= 100; k++) edge[k] = 0.0 + (double)k * 0.01;      // np.arange: start + k * delta
    counts.assign(100, 0);
    labels.assign(edge + 1, edge + 101);
    for (double v : ratios) {
        if (!(v >= edge[0]) || !(v <= edge[100])) continue;
        int k = (int)(v * 100.0);
        if (k > 99) k = 99;
        while (k > 0 && v < edge[k]) k--;
        while (k < 99 && v >= edge[k + 1]) k++;
        counts[(size_t)k]++;
    }
}

bool kde_grid_axes(long long start, long long end, long long step, std::vector<long long>& idx, std::vector<double>& centres) {
    idx.clear(); centres.clear();
    if (step <= 0 || end < start) return false;
    if (((unsigned long long)end - (unsigned long long)start) / (unsigned long long)step > (1ull << 20)) return false;      // (callers bound the axis far below this)
    for (long long v = start; v < end + 1; v += step) idx.push_back(v);
    if (idx.size() < 2) return false;
    for (size_t k = 0; k + 1 < idx.size(); k++) {
        const long long s = idx[k] + idx[k + 1];
        centres.push_back((double)(s >= 0 ? s / 2 : -((-s + 1) / 2)));   // floor division
    }
    return true;
}

bool write_trc_model_json(const std::string& path, const std::vector<double>& P, const std::vector<long long>& idx,
                          const std::vector<long long>& counts, const std::vector<double>& labels, std::string& err) {
    const size_t g = idx.size() - 1;
    if (idx.size() < 2 || P.size() != g * g || counts.size() != labels.size()) { err = "model writer: shapes disagree"; return false; }
    for (double v : P) if (!std::isfinite(v)) { err = "model writer: a density is not finite"; return false; }
    const std::string tmp = path + ".tmp";
    FILE* f = fopen(tmp.c_str(), "wb");
    if (!f) { err = "cannot write " + path; return false; }
    // json.dump(..., indent=4)'s layout
    fprintf(f, "[\n    {\n        \"name\": \"KDE_mtx\",\n        \"shape\": [\n            %zu,\n            %zu\n        ],\n        \"data\": [\n", g, g);
    for (size_t j = 0; j < g; j++)
        for (size_t i = 0; i < g; i++) fprintf(f, "            %.17g%s\n", P[i * g + j], j + 1 == g && i + 1 == g ? "" : ",");
    fprintf(f, "        ],\n        \"labels\": [\n");
    for (int rep = 0; rep < 2; rep++)
        for (size_t k = 1; k <= g; k++) fprintf(f, "            %lld%s\n", idx[k], rep == 1 && k == g ? "" : ",");
    fprintf(f, "        ]\n    },\n    {\n        \"name\": \"end_mtx\",\n        \"shape\": [\n            %zu\n        ],\n        \"data\": [\n", counts.size());
    for (size_t k = 0; k < counts.size(); k++) fprintf(f, "            %lld%s\n", counts[k], k + 1 == counts.size() ? "" : ",");
    fprintf(f, "        ],\n        \"labels\": [\n");
    for (size_t k = 0; k < labels.size(); k++) fprintf(f, "            %.17g%s\n", labels[k], k + 1 == labels.size() ? "" : ",");
    fprintf(f, "        ]\n    }\n]");
    const bool bad = ferror(f) != 0;
    const bool closed = fclose(f) == 0;
    if (bad || !closed || rename(tmp.c_str(), path.c_str()) != 0) { remove(tmp.c_str()); err = "cannot write " + path; return false; }
    return true;
}

}  // namespace tkh
