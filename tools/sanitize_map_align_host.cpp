// sanitize_map_align_host.cpp -- the host-only code of map -c (map_host.cpp: the parameter checks, the aligned PAF line with its run-length
// printing, the line table and the budget arithmetic) as a stand-alone program for ASan / UBSan.  Build and run (tests/test_map_align.py does):
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -I tksm_amd/csrc tools/sanitize_map_align_host.cpp tksm_amd/csrc/map_host.cpp \
//       tksm_amd/csrc/ms_host.cpp tksm_amd/csrc/abund_host.cpp -lz -o sanitize_map_align_host && ./sanitize_map_align_host
// Prints "key values" lines the test compares with tests/map_align_spec.py.
#include <cstdio>
#include <string>
#include <vector>

#include "map_host.h"

int main() {
    // ---- parameter checks: "check <label> <ok> <message>"
    tksmseq_map_params p{};
    p.k = 15; p.w = 10; p.max_occ = 500; p.max_gap = 5000; p.bandwidth = 500; p.min_count = 3; p.min_score = 40; p.secondary_ratio = 0.8; p.max_secondary = 5;
    struct Case { const char* label; int32_t band, max_gap; };
    for (const Case& c : {Case{"defaults", 63, 5000}, Case{"band1", 1, 5000}, Case{"band0", 0, 5000}, Case{"band64", 64, 5000}, Case{"band-1", -1, 5000},
                          Case{"gap65536", 63, 65536}, Case{"gap65537", 63, 65537}, Case{"gapmax", 63, 0x7FFFFFFF}}) {
        tksmseq_map_params q = p;
        q.max_gap = c.max_gap;
        const tksmseq_align_params a{c.band, 0};
        std::string err;
        const bool ok = tkh::map_check_align(q, a, err);
        printf("check %s %d %s\n", c.label, ok ? 1 : 0, err.c_str());
    }

    // ---- the aligned line: "paf <line>".  Columns as letters, run-length coded here the way the device hands the runs over.
    auto line = [](const std::string& columns, bool eqx, uint32_t rel, bool primary) {
        tkh::MapAlnOut a{};
        std::vector<uint64_t> runs;
        char last = 0;
        for (size_t x = 0; x < columns.size(); x++) {
            const char c = columns[x];
            const uint32_t code = c == '=' ? 0u : c == 'X' ? 1u : c == 'I' ? 2u : 3u, op = eqx || code >= 2u ? code : 0u;
            a.eq += code == 0u; a.x += code == 1u; a.ins += code == 2u; a.del += code == 3u;
            if (!x || (char)op != last) runs.push_back((uint64_t)x << 2 | op);
            last = (char)op;
        }
        a.ncols = (uint32_t)columns.size();
        a.runs = (uint32_t)runs.size();
        tkh::MapChain c{};
        c.read = 0; c.tr = 2u | rel; c.score = 120; c.cnt = 9; c.nmatch = 101;
        c.tstart = 10; c.tend = 10 + a.eq + a.x + a.del; c.qs = 4; c.qe = 4 + a.eq + a.x + a.ins; c.kept = 1;
        std::string out;
        tkh::map_paf_line_aligned("read/1", 200000, "tx", 300000, c, primary ? 60u : 0u, primary, a, runs.data(), eqx, out);
        printf("paf %s", out.c_str());
    };
    const std::string mixed = std::string(5, '=') + "X" + std::string(3, '=') + "II" + "D" + "XX" + std::string(4, '=');
    line(mixed, false, 0, true);
    line(mixed, true, 0, true);
    line(mixed, true, 1, false);
    line("=", false, 0, true);
    line("", false, 0, true);                                                      // (no run at all: an empty CIGAR, never written by map)
    line(std::string(70000, '=') + "D" + std::string(66000, 'I'), true, 0, true);    // runs longer than 2^16
    line(std::string(40000, '=') + std::string(40000, 'X'), false, 1, true);          // ... and one M run made of both

    // ---- the line table and the budget: "table <chain> <seg_off> <col_off> <cap>", "bytes ...", "waves ..."
    std::vector<tkh::MapAlnLine> lines;
    uint64_t segments = 0, col_words = 0;
    const uint32_t spans[][3] = {{100, 90, 7}, {1, 1, 1}, {16, 0, 1}, {17, 0, 2}, {65536, 65536, 3}};       // target span, read span, anchors
    for (uint32_t i = 0; i < 5; i++) {
        tkh::MapChain c{};
        c.tstart = 5; c.tend = 5 + spans[i][0]; c.qs = 9; c.qe = 9 + spans[i][1]; c.cnt = spans[i][2];
        tkh::map_align_add_line(10 + i, c, segments, col_words, lines);
    }
    for (const auto& l : lines) printf("table %u %u %u %u\n", l.chain, l.seg_off, l.col_off, l.cap);
    printf("table_end %llu %llu\n", (unsigned long long)segments, (unsigned long long)col_words);
    printf("bytes %llu %llu\n", (unsigned long long)tkh::map_align_fixed_bytes(lines.size(), segments, col_words, 0),
           (unsigned long long)tkh::map_align_fixed_bytes(1ull << 31, 1ull << 33, 1ull << 32, 1ull << 34));
    const uint64_t budget = tkh::MAP_ALN_BYTES_MAX;
    for (const uint64_t fixed : {(uint64_t)0, budget - 1984, budget - 1983, budget, budget + 1})
        for (const uint32_t longest : {30u, 131072u})
            for (const uint64_t n : {(uint64_t)1, (uint64_t)5, (uint64_t)1 << 20})
                printf("waves %llu %u %llu %u\n", (unsigned long long)fixed, longest, (unsigned long long)n, tkh::map_align_waves(budget, fixed, n, longest));
    return 0;
}
