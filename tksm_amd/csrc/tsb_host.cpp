// tsb_host.cpp -- the GTF reader and the abundance join of transcribe (see tsb_host.h).  One pass over the bytes of a file: no string is
// built per line, an id is looked up with one probe sequence of an open-addressing table over the id pool.
#include "tsb_host.h"

#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <unordered_map>

namespace tsb {

uint64_t IdIndex::hash(const char* s, size_t n) {      // FNV-1a
    uint64_t h = 1469598103934665603ull;
    for (size_t i = 0; i < n; i++) { h ^= (unsigned char)s[i]; h *= 1099511628211ull; }
    return h ^ (h >> 29);
}

namespace {

bool same(const Transcripts& t, uint32_t i, const char* id, size_t len) {
    return t.id_len[i] == len && (len == 0 || memcmp(t.id_pool.data() + t.id_off[i], id, len) == 0);
}

void index_put(Transcripts& t, uint32_t i) {
    IdIndex& x = t.index;
    const size_t mask = x.slot.size() - 1;
    size_t p = IdIndex::hash(t.id_pool.data() + t.id_off[i], t.id_len[i]) & mask;
    while (x.slot[p]) p = (p + 1) & mask;
    x.slot[p] = i + 1;
    x.used++;
}

void index_grow(Transcripts& t) {
    IdIndex& x = t.index;
    if (!x.slot.empty() && (uint64_t)(x.used + 1) * 2 <= x.slot.size()) return;
    const size_t cap = x.slot.empty() ? 1024 : x.slot.size() * 2;
    x.slot.assign(cap, 0u);
    x.used = 0;
    for (uint32_t i = 0; i < (uint32_t)t.n(); i++) index_put(t, i);
}

// a transcript without exons yet; the caller has checked that the id is new
uint32_t add_transcript(Transcripts& t, const char* id, size_t len) {
    index_grow(t);
    const uint32_t i = (uint32_t)t.n();
    t.id_off.push_back((uint32_t)t.id_pool.size()); t.id_len.push_back((uint32_t)len);
    t.id_pool.append(id, len);
    index_put(t, i);
    return i;
}

// std::stoi of a coordinate field: leading white space, an optional sign, digits; what follows the digits is ignored.  false: no digit,
// or a value outside [lo, 2^31 - 1]
bool coordinate(const char* p, const char* e, long long lo, long long& out) {
    while (p < e && (*p == ' ' || (*p >= '\t' && *p <= '\r'))) p++;
    bool neg = false;
    if (p < e && (*p == '+' || *p == '-')) { neg = *p == '-'; p++; }
    if (p >= e || *p < '0' || *p > '9') return false;
    long long v = 0;
    while (p < e && *p >= '0' && *p <= '9') { v = v * 10 + (*p - '0'); if (v > 0x7fffffffll) return false; p++; }
    if (neg) v = -v;
    out = v;
    return v >= lo;
}

// info[key] of field 8 (src/interval.h:261-274): the LAST ';' piece whose first token (quotes stripped) is key; its second token with
// quotes stripped.  false: no such attribute
bool attribute(const char* p, const char* e, const char* key, const char*& vb, const char*& ve) {
    const size_t klen = strlen(key);
    bool found = false;
    while (p <= e) {
        const char* q = (const char*)memchr(p, ';', (size_t)(e - p));
        const char* pe = q ? q : e;
        const char *a = p, *b = pe;                                   // strip_str(piece, " ")
        while (a < b && *a == ' ') a++;
        while (b > a && b[-1] == ' ') b--;
        if (b - a > 1) {
            const char* t1 = (const char*)memchr(a, ' ', (size_t)(b - a));      // rsplit(piece, " "): tokens 0 and 1
            const char *k0 = a, *k1 = t1 ? t1 : b;
            while (k0 < k1 && *k0 == '"') k0++;
            while (k1 > k0 && k1[-1] == '"') k1--;
            if ((size_t)(k1 - k0) == klen && memcmp(k0, key, klen) == 0) {
                const char *v0 = b, *v1 = b;                          // (no second token: "")
                if (t1) { v0 = t1 + 1; const char* t2 = (const char*)memchr(v0, ' ', (size_t)(b - v0)); v1 = t2 ? t2 : b; }
                while (v0 < v1 && *v0 == '"') v0++;
                while (v1 > v0 && v1[-1] == '"') v1--;
                vb = v0; ve = v1; found = true;
            }
        }
        if (!q) break;
        p = q + 1;
    }
    return found;
}

std::string where(const std::string& name, uint64_t line) { return name + ":" + std::to_string(line) + ": "; }

}  // namespace

int Transcripts::find(const char* id, size_t len) const {
    if (index.slot.empty()) return -1;
    const size_t mask = index.slot.size() - 1;
    size_t p = IdIndex::hash(id, len) & mask;
    while (index.slot[p]) {
        if (same(*this, index.slot[p] - 1, id, len)) return (int)(index.slot[p] - 1);
        p = (p + 1) & mask;
    }
    return -1;
}

bool parse_gtf(const char* text, size_t len, const std::string& name, bool skip_non_coding, Transcripts& into, std::string& err) {
    // the file's own table first: a duplicate id inside the file appends, one from an earlier file wins
    Transcripts local;
    struct Exon { uint32_t tx, contig, start, end; uint8_t minus; };
    std::vector<Exon> exons;
    std::vector<uint32_t> n_ex;
    std::unordered_map<std::string, uint32_t> contig_of;
    const char* last_c = nullptr; size_t last_cl = 0; uint32_t last_ci = 0;
    int current = -1;
    uint64_t line_no = 0;
    const char *p = text, *end = text + len;
    while (p < end) {
        const char* nl = (const char*)memchr(p, '\n', (size_t)(end - p));
        const char* le = nl ? nl : end;
        line_no++;
        const char* ls = p;
        p = nl ? nl + 1 : end;
        if (ls == le || *ls == '#') continue;
        const char *f0[9], *f1[9];                                   // field k is [f0[k], f1[k]); a field 8 ends at its tab when more follow
        int nf = 0;
        for (const char* q = ls; nf < 9;) {
            const char* t = (const char*)memchr(q, '\t', (size_t)(le - q));
            f0[nf] = q; f1[nf] = t ? t : le;
            nf++;
            if (!t) break;
            q = t + 1;
        }
        if (nf < 9) { err = where(name, line_no) + "a GTF line has 9 tab-separated fields, this one has " + std::to_string(nf); return false; }
        auto fb = [&](int k) { return f0[k]; };
        auto fe = [&](int k) { return f1[k]; };
        long long start = 0, stop = 0;
        if (!coordinate(fb(3), fe(3), 1, start) || !coordinate(fb(4), fe(4), 0, stop)) {
            err = where(name, line_no) + "start and end must be numbers between 1 (end: 0) and 2147483647"; return false;
        }
        const char *vb = nullptr, *ve = nullptr;
        if (skip_non_coding) {
            const bool has = attribute(fb(8), fe(8), "gene_biotype", vb, ve);
            if (!has || (size_t)(ve - vb) != 14 || memcmp(vb, "protein_coding", 14) != 0) continue;
        }
        const size_t tl = (size_t)(fe(2) - fb(2));
        if (tl == 10 && memcmp(fb(2), "transcript", 10) == 0) {
            if (!attribute(fb(8), fe(8), "transcript_id", vb, ve)) vb = ve = fb(8);      // (info["transcript_id"] of a line without one: "")
            const int have = local.find(vb, (size_t)(ve - vb));
            if (have >= 0) current = have;
            else {
                if (local.n() >= 0x7fffffffull || local.id_pool.size() + (size_t)(ve - vb) >= 0xffffffffull) { err = name + ": more than 2^31 transcripts or 4 GB of ids"; return false; }
                current = (int)add_transcript(local, vb, (size_t)(ve - vb));
                n_ex.push_back(0);
            }
        } else if (tl == 4 && memcmp(fb(2), "exon", 4) == 0) {
            if (current < 0) { err = where(name, line_no) + "an exon line before any transcript line"; return false; }
            const size_t cl = (size_t)(fe(0) - fb(0));
            uint32_t ci;
            if (last_c && cl == last_cl && memcmp(last_c, fb(0), cl) == 0) ci = last_ci;
            else {
                auto it = contig_of.emplace(std::string(fb(0), cl), (uint32_t)local.contig_names.size());
                if (it.second) local.contig_names.push_back(it.first->first);
                ci = it.first->second; last_c = fb(0); last_cl = cl; last_ci = ci;
            }
            if (exons.size() >= 0x7fffffffull) { err = name + ": more than 2^31 exons"; return false; }
            exons.push_back(Exon{(uint32_t)current, ci, (uint32_t)(start - 1), (uint32_t)stop, (uint8_t)((fe(6) - fb(6)) == 1 && *fb(6) == '+' ? 0 : 1)});
            n_ex[(size_t)current]++;
        }
    }
    // merge: the file's transcripts that `into` does not know, in file order, each with its exons in file order
    std::vector<uint32_t> first(local.n() + 1, 0u), fill;
    for (size_t t = 0; t < local.n(); t++) first[t + 1] = first[t] + n_ex[t];
    fill.assign(first.begin(), first.end() - 1);
    std::vector<uint32_t> order(exons.size());
    for (uint32_t e = 0; e < (uint32_t)exons.size(); e++) order[fill[exons[e].tx]++] = e;
    std::vector<uint32_t> contig_map(local.contig_names.size(), 0xffffffffu);
    std::unordered_map<std::string, uint32_t> into_contigs;
    for (uint32_t i = 0; i < (uint32_t)into.contig_names.size(); i++) into_contigs.emplace(into.contig_names[i], i);
    for (uint32_t t = 0; t < (uint32_t)local.n(); t++) {
        const char* id = local.id_pool.data() + local.id_off[t];
        if (into.find(id, local.id_len[t]) >= 0) continue;
        if (into.n() >= 0x7fffffffull || into.n_exons() + n_ex[t] >= 0x7fffffffull || into.id_pool.size() + local.id_len[t] >= 0xffffffffull) {
            err = name + ": more than 2^31 transcripts or exons, or 4 GB of ids, in the transcript table"; return false;
        }
        add_transcript(into, id, local.id_len[t]);
        for (uint32_t k = first[t]; k < first[t + 1]; k++) {
            const Exon& x = exons[order[k]];
            if (contig_map[x.contig] == 0xffffffffu) {
                auto it = into_contigs.emplace(local.contig_names[x.contig], (uint32_t)into.contig_names.size());
                if (it.second) into.contig_names.push_back(local.contig_names[x.contig]);
                contig_map[x.contig] = it.first->second;
            }
            into.ex_contig.push_back(contig_map[x.contig]); into.ex_start.push_back(x.start); into.ex_end.push_back(x.end); into.ex_minus.push_back(x.minus);
        }
        into.exon_first.push_back((uint32_t)into.n_exons());
    }
    return true;
}

bool read_gtf(const std::string& path, bool skip_non_coding, Transcripts& into, std::string& err, bool& io) {
    io = false;
    FILE* f = fopen(path.c_str(), "rb");
    if (!f) { io = true; err = "Could not open GTF file " + path + "!"; return false; }
    std::string text;
    char buf[1 << 16];
    size_t n;
    while ((n = fread(buf, 1, sizeof buf, f)) > 0) text.append(buf, n);
    const bool bad = ferror(f) != 0;
    fclose(f);
    if (bad) { io = true; err = "Could not read GTF file " + path + "!"; return false; }
    // (a failed parse leaves `into` as it was: it is only appended to once the whole file has been read)
    return parse_gtf(text.data(), text.size(), path, skip_non_coding, into, err);
}

double parse_tpm(const char* p, size_t n, size_t* taken, bool* ok) {
    size_t i = 0;
    if (i < n && (p[i] == '+' || p[i] == '-')) i++;
    bool digits = false, point = false;
    for (; i < n; i++) {
        if (p[i] >= '0' && p[i] <= '9') digits = true;
        else if (p[i] == '.' && !point) point = true;
        else break;
    }
    bool good = digits;
    if (digits && i < n && (p[i] == 'e' || p[i] == 'E')) {
        i++;
        if (i < n && (p[i] == '+' || p[i] == '-')) i++;
        bool ed = false;
        for (; i < n && p[i] >= '0' && p[i] <= '9'; i++) ed = true;
        good = ed;
    }
    *taken = i;
    *ok = false;
    if (!good) return 0.0;
    char tmp[64];
    std::string big;
    const char* z;
    if (i < sizeof tmp) { memcpy(tmp, p, i); tmp[i] = 0; z = tmp; } else { big.assign(p, i); z = big.c_str(); }
    const double v = strtod(z, nullptr);
    if (std::isinf(v)) return v > 0 ? DBL_MAX : -DBL_MAX;
    *ok = true;
    return v;
}

bool parse_abundance(const char* text, size_t len, bool use_whole_id, const Transcripts& t, Abundance& out, std::string& err) {
    if (len >= 0xfffffffeull) { err = "an abundance table of 4 GB or more (split it into several files)"; return false; }
    out = Abundance();
    out.text.assign(text, len);
    const char *base = out.text.data(), *p = base, *end = base + len;
    auto is_ws = [](char c) { return c == ' ' || (c >= '\t' && c <= '\r'); };
    {   // std::getline(...): the header, whatever it holds
        const char* nl = (const char*)memchr(p, '\n', (size_t)(end - p));
        p = nl ? nl + 1 : end;
    }
    double sum = 0.0;
    while (p < end) {
        const char* nl = (const char*)memchr(p, '\n', (size_t)(end - p));
        const char* le = nl ? nl : end;
        const char* q = p;
        p = nl ? nl + 1 : end;
        const char *id = "BEG"; size_t idl = 3;
        double tpm = 0.0;
        const char* cb = base; size_t cbl = 0;
        while (q < le && is_ws(*q)) q++;
        if (q < le) {
            id = q;
            while (q < le && !is_ws(*q)) q++;
            idl = (size_t)(q - id);
            while (q < le && is_ws(*q)) q++;
            if (q < le) {
                size_t taken = 0; bool ok = false;
                const char* tok = q;
                while (q < le && !is_ws(*q)) q++;
                tpm = parse_tpm(tok, (size_t)(q - tok), &taken, &ok);
                if (ok) {                                            // the third token starts where the number ended
                    q = tok + taken;
                    while (q < le && is_ws(*q)) q++;
                    cb = q;
                    while (q < le && !is_ws(*q)) q++;
                    cbl = (size_t)(q - cb);
                    if (!cbl) cb = base;
                }
            }
        }
        if (!use_whole_id) { const char* dot = (const char*)memchr(id, '.', idl); if (dot) idl = (size_t)(dot - id); }
        const int ti = t.find(id, idl);
        out.tx.push_back(ti < 0 ? Abundance::NONE : (uint32_t)ti);
        out.tpm.push_back(tpm);
        out.cb_off.push_back((uint32_t)(cb - base)); out.cb_len.push_back((uint32_t)cbl);
        if (ti < 0) {
            // ("BEG" is not in the text: such a row's id is marked by the length 3 at offset 2^32 - 1)
            out.missing_off.push_back(id >= base && id < end ? (uint32_t)(id - base) : 0xffffffffu); out.missing_len.push_back((uint32_t)idl);
        }
        sum += tpm;
        if (out.tx.size() >= 0xfffffffeull) { err = "more than 2^32 - 2 rows in one abundance table"; return false; }
    }
    out.sum_tpm = sum;
    return true;
}

void append_comment(std::string& out, const char* cb, size_t cb_len, const char* tid, size_t tid_len) {
    out += "CB";
    if (!(cb_len == 1 && cb[0] == '.')) { out += '='; out.append(cb, cb_len); }
    out += ";tid";
    if (!(tid_len == 1 && tid[0] == '.')) { out += '='; out.append(tid, tid_len); }
    out += ';';
}

}  // namespace tsb
