// gzip_core_check.cpp -- the serial pieces of the device-side BGZF encoder (tksm_amd/csrc/gzip_core.h) run on the host: reads a file,
// encodes it chunk by chunk the way gzip_kernels.hip does (strips taken one after the other instead of by 256 lanes), writes the
// members to stdout without the EOF member.  tests/test_gzip_device.py feeds it the edge cases and inflates the result with zlib, so
// that tokeniser, length limiting and block headers are checked without a GPU.
//     g++ -O2 -std=c++17 -I tksm_amd/csrc tools/gzip_core_check.cpp -o gzip_core_check && ./gzip_core_check raw|fasta|fastq FILE > out.gz
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "gzip_core.h"

using namespace tkgz;

static uint32_t crc32_of(const uint8_t* d, size_t n) {
    uint32_t r = 0xFFFFFFFFu;
    for (size_t i = 0; i < n; i++) { r ^= d[i]; for (int k = 0; k < 8; k++) r = (r & 1u) ? 0xEDB88320u ^ (r >> 1) : r >> 1; }
    return ~r;
}

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: gzip_core_check raw|fasta|fastq FILE\n"); return 2; }
    const std::string f = argv[1];
    const int fmt = f == "fastq" ? FMT_FASTQ : f == "fasta" ? FMT_FASTA : FMT_RAW;
    std::vector<uint8_t> in;
    { FILE* fp = fopen(argv[2], "rb"); if (!fp) return 2; uint8_t buf[65536]; size_t g; while ((g = fread(buf, 1, sizeof buf, fp)) > 0) in.insert(in.end(), buf, buf + g); fclose(fp); }
    uint32_t nl_before = 0;
    for (size_t base = 0; base < in.size(); base += CHUNK) {
        const uint8_t* d = in.data() + base;
        const uint32_t n = (uint32_t)std::min<size_t>(CHUNK, in.size() - base);
        std::vector<uint32_t> strip_nl(STRIPS + 1, nl_before & 3u);
        auto sb = [&](uint32_t t) { return std::min(t * STRIP, n); };
        for (uint32_t t = 0; t < STRIPS; t++) strip_nl[t + 1] = strip_nl[t] + (uint32_t)std::count(d + sb(t), d + sb(t + 1), '\n');
        static uint32_t hist[NCLS][NSYM], sw[NCLS][NSYM], hdr[NCLS][HDR_WORDS], code[NCLS][NSYM], hbits[NCLS];
        static uint16_t ss[NCLS][NSYM], rle[NCLS][320];
        static uint8_t ll[NCLS][NSYM];
        memset(hist, 0, sizeof hist); memset(hdr, 0, sizeof hdr); memset(ll, 0, sizeof ll);
        uint32_t extra = 0;
        for (uint32_t t = 0; t < STRIPS; t++)
            walk_strip(d, sb(t), sb(t + 1), fmt, fmt == FMT_RAW ? 0u : strip_nl[t], [&](uint32_t, uint32_t cls, uint32_t pcls, uint8_t c, uint32_t run) {
                if (cls != pcls) hist[cls][256]++;
                if (run) { uint32_t sym, eb, ev; length_symbol(run, sym, eb, ev); hist[cls][sym]++; extra += eb + 1; } else hist[cls][c]++;
            });
        bool fits = true;
        uint32_t bits = extra + FINAL_BITS;
        for (int c = 0; c < NCLS; c++) {
            std::vector<std::pair<uint32_t, uint16_t>> used;
            for (int s = 0; s < 286; s++) if (hist[c][s]) used.push_back({hist[c][s], (uint16_t)s});
            std::sort(used.begin(), used.end());
            for (size_t i = 0; i < used.size(); i++) { sw[c][i] = used[i].first; ss[c][i] = used[i].second; }
            hbits[c] = 0;
            if (!used.empty()) {
                limited_lengths(sw[c], ss[c], (int)used.size(), 15, ll[c]);
                hbits[c] = block_header(ll[c], hdr[c], rle[c]);
                if (!hbits[c]) fits = false;
            }
            canonical_codes(ll[c], NSYM, code[c]);
            for (int s = 0; s < NSYM; s++) bits += hist[c][s] * ll[c][s];
            bits += hist[c][256] * hbits[c];
        }
        uint32_t payload = (bits + 7) / 8;
        const bool dynamic = fits && payload < n + STORED_OVERHEAD;
        if (!dynamic) payload = n + STORED_OVERHEAD;
        std::vector<uint32_t> out((payload + 3) / 4 + 1, 0);
        if (dynamic) {
            BitSink sink(out.data(), (uint32_t)out.size());
            uint32_t last = 0;
            auto put_code = [&](uint32_t cv) { sink.put(cv & 0xffffu, cv >> 16); };
            for (uint32_t t = 0; t < STRIPS; t++)
                walk_strip(d, sb(t), sb(t + 1), fmt, fmt == FMT_RAW ? 0u : strip_nl[t], [&](uint32_t, uint32_t cls, uint32_t pcls, uint8_t c, uint32_t run) {
                    if (cls != pcls) {
                        if (pcls != ~0u) put_code(code[pcls][256]);
                        for (uint32_t i = 0; i < hbits[cls] / 32; i++) sink.put(hdr[cls][i], 32);
                        if (hbits[cls] & 31u) sink.put(hdr[cls][hbits[cls] / 32] & ((1u << (hbits[cls] & 31u)) - 1u), hbits[cls] & 31u);
                    }
                    if (run) { uint32_t sym, eb, ev; length_symbol(run, sym, eb, ev); put_code(code[cls][sym]); if (eb) sink.put(ev, eb); sink.put(0, 1); }
                    else put_code(code[cls][c]);
                    last = cls;
                });
            put_code(code[last][256]);
            sink.put(FINAL_VALUE, FINAL_BITS);
            if (!sink.ok || sink.bits != bits) { fprintf(stderr, "planned %u bits, wrote %u\n", bits, sink.bits); return 1; }
        }
        const uint32_t bsize = MEMBER_OVERHEAD + payload - 1;
        const uint8_t h[18] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0, (uint8_t)(bsize & 0xff), (uint8_t)(bsize >> 8)};
        fwrite(h, 1, 18, stdout);
        if (dynamic) fwrite(out.data(), 1, payload, stdout);
        else { const uint8_t s5[5] = {1, (uint8_t)(n & 0xff), (uint8_t)(n >> 8), (uint8_t)(~n & 0xff), (uint8_t)((~n >> 8) & 0xff)}; fwrite(s5, 1, 5, stdout); fwrite(d, 1, n, stdout); }
        const uint32_t tr[2] = {crc32_of(d, n), n};
        fwrite(tr, 1, 8, stdout);
        nl_before = strip_nl[STRIPS];
    }
    return 0;
}
