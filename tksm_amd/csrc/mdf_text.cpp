// mdf_text.cpp -- molecule batches as MDF text, and the header-comment grammar the transforms share (mdf_batch.h):
//   parse_meta / dump_meta / normalize_comment   molecule_descriptor::comment / dump_comment, src/interval.h:809-830, :880-890
//   tksmseq_batch_to_mdf_text   molecule_descriptor::operator<<, src/interval.h:898-905 (+ dump_comment :880-890)
// The molecule tables stay on the device from one transform to the next; for the text they come back to the host (HostTables).
#include <charconv>
#include <cmath>
#include <cstring>
#include <thread>

#include "mdf_batch.h"

// molecule_descriptor::comment (src/interval.h:809-830): "k=v1,v2;flag;" -> key -> values ("." for a bare key)
Meta parse_meta(const char* c, size_t n) {
    Meta meta;
    size_t a = 0;
    while (a < n) {
        size_t b = a;
        while (b < n && c[b] != ';') b++;
        if (b > a) {
            const std::string f(c + a, b - a);
            const size_t eq = f.find('=');
            if (eq == std::string::npos) meta[f].push_back(".");
            else {
                size_t k1 = f.find_first_not_of('='), k2 = f.find('=', k1 == std::string::npos ? 0 : k1);
                const std::string key = k1 == std::string::npos ? std::string() : f.substr(k1, k2 - k1);
                size_t v = k2 == std::string::npos ? f.size() : k2;
                while (v < f.size() && f[v] == '=') v++;
                size_t ve = f.find('=', v);
                const std::string vals = f.substr(v, ve == std::string::npos ? std::string::npos : ve - v);
                size_t p = 0;
                while (p < vals.size()) {
                    size_t q = vals.find(',', p);
                    if (q == std::string::npos) q = vals.size();
                    if (q > p) meta[key].push_back(vals.substr(p, q - p));
                    p = q + 1;
                }
            }
        }
        a = b + 1;
    }
    return meta;
}

// dump_comment (src/interval.h:880-890)
std::string dump_meta(const Meta& meta) {
    std::string out;
    for (auto& kv : meta) {
        if (kv.second.empty()) continue;
        out += kv.first;
        if (kv.second[0] != ".") {
            out += '=';
            for (size_t i = 0; i < kv.second.size(); i++) { if (i) out += ','; out += kv.second[i]; }
        }
        out += ';';
    }
    return out;
}

// std::map<string, vector<string>> round trip of a header comment (molecule_descriptor::comment / dump_comment,
// src/interval.h:809-830, :880-890), with extra values appended
std::string normalize_comment(const char* c, size_t n, const std::vector<std::pair<std::string, std::string>>& extra) {
    Meta meta = parse_meta(c, n);
    for (auto& kv : extra) meta[kv.first].push_back(kv.second);
    return dump_meta(meta);
}

// fmt's "{}" of a double: the shortest digits that round-trip, in FIXED notation while the decimal exponent is in [-4, 16) and in
// exponent notation outside (like Python's repr; std::to_chars alone would switch to "1e+05" as soon as that is shorter)
std::string fmt_double(double v) {
    char buf[64];
    auto r = std::to_chars(buf, buf + sizeof buf, v, std::chars_format::scientific);
    std::string sci(buf, r.ptr);                          // d[.ddd]e[+-]XX: read the exponent off it
    const size_t e = sci.find('e');
    const int ex = e == std::string::npos ? 0 : atoi(sci.c_str() + e + 1);
    if (!std::isfinite(v) || ex < -4 || ex >= 16) {
        r = std::to_chars(buf, buf + sizeof buf, v);
        return std::string(buf, r.ptr);
    }
    r = std::to_chars(buf, buf + sizeof buf, v, std::chars_format::fixed);
    return std::string(buf, r.ptr);
}


// One molecule per read, depth 1: what every C++ module of the reference writes after reading with unroll = true
// (copies of a depth > 1 molecule are named id_0, id_1, ...: src/mdf.h:97-105).  print_tsv: "+id<TAB>depth<TAB>comment".
static void format_molecules(const tksmseq_ctx* ctx, const tksmseq_batch* b, const HostTables& H, uint64_t r0, uint64_t r1, std::string& out) {
    const auto &reads = H.reads, &ivs = H.ivs, &mods = H.mods;
    out.reserve((r1 - r0) * 112);
    for (uint64_t r = r0; r < r1; r++) {
        out += '+';
        append_written_id(H, b, r, out);
        out += "\t1\t";
        if (!b->h_comments.empty()) out += normalize_comment(b->h_comment_pool.data() + b->h_comments[2 * r], b->h_comments[2 * r + 1], {});
        out += '\n';
        const uint32_t ib = reads[2 * r], ic = reads[2 * r + 1];
        for (uint32_t i = 0; i < ic; i++) {
            const uint32_t* iv = ivs.data() + 4 * (size_t)(ib + i);
            H.append_contig(ctx, iv[0], out);
            out += '\t'; append_u32(out, iv[1]); out += '\t'; append_u32(out, iv[2]); out += '\t';
            out += (iv[3] >> 31) ? '-' : '+';
            out += '\t';
            const uint32_t mb = iv[3] & 0x7fffffffu, me = iv[7] & 0x7fffffffu;
            for (uint32_t q = mb; q < me; q++) { if (q > mb) out += ','; append_u32(out, mods[2 * (size_t)q]); out += (char)mods[2 * (size_t)q + 1]; }
            out += '\n';
        }
    }
}

// work(t) for t = 0 .. nt - 1, each on a thread of its own (0 on the caller's)
template <class F>
static void on_threads(uint64_t nt, F work) {
    std::vector<std::thread> th;
    for (uint64_t t = 1; t < nt; t++) th.emplace_back([&work, t]() { work(t); });
    work(0);
    for (auto& x : th) x.join();
}

extern "C" {

// The reads are formatted in contiguous shares, one per host thread (tksmseq_set_host_threads), and the shares copied into the result
// side by side.
int tksmseq_batch_to_mdf_text(tksmseq_ctx* ctx, const tksmseq_batch* b, char** text, uint64_t* len) {
    if (!ctx || !b || !text || !len) return TKSMSEQ_EINVAL;
    *text = nullptr; *len = 0;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const uint64_t n = b->n_reads;
    HostTables H;
    const int rc = H.fetch(ctx, b, HostTables::SEGMENTS | HostTables::MODS | HostTables::IDS);
    if (rc) return rc;
    const uint64_t nt = std::max<uint64_t>(1, std::min<uint64_t>((uint64_t)std::max(1, ctx->host_threads), n / 1024 + 1));
    std::vector<std::string> parts(nt);
    on_threads(nt, [&](uint64_t t) { format_molecules(ctx, b, H, n * t / nt, n * (t + 1) / nt, parts[t]); });
    uint64_t total = 0;
    std::vector<uint64_t> at(nt);
    for (uint64_t t = 0; t < nt; t++) { at[t] = total; total += parts[t].size(); }
    char* buf = (char*)malloc(total + 1);
    if (!buf) return TKSMSEQ_ENOMEM;
    on_threads(nt, [&](uint64_t t) { memcpy(buf + at[t], parts[t].data(), parts[t].size()); });
    buf[total] = 0;
    *text = buf; *len = total;
    return TKSMSEQ_OK;
}

void tksmseq_text_free(char* text) { free(text); }

}  // extern "C"
