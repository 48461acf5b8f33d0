// sanitize_map_split_host.cpp -- the host-only code of map --split (map_host.cpp: the parameter checks, the two tags of a line, the ranks of
// a read's tp:A:P lines, the budget arithmetic) as a stand-alone program for ASan / UBSan.  Build and run (tests/test_map_split.py does):
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -I tksm_amd/csrc tools/sanitize_map_split_host.cpp tksm_amd/csrc/map_host.cpp \
//       tksm_amd/csrc/ms_host.cpp tksm_amd/csrc/abund_host.cpp -lz -o sanitize_map_split_host && ./sanitize_map_split_host
// Prints "key values" lines the test compares with what include/tksmseq.h ("map, split reads") says.
#include <cstdio>
#include <string>
#include <utility>
#include <vector>

#include "map_host.h"

int main() {
    // ---- parameter checks: "check <label> <ok> <message>"
    struct Case { const char* label; int32_t chains, overlap, segments; };
    for (const Case& c : {Case{"defaults", 4, 30, 8}, Case{"lowest", 1, 0, 2}, Case{"highest", 16, 0x7FFFFFFF, 64}, Case{"chains0", 0, 30, 8}, Case{"chains17", 17, 30, 8},
                          Case{"overlap-1", 4, -1, 8}, Case{"segments1", 4, 30, 1}, Case{"segments65", 4, 30, 65}, Case{"chains-1", -1, 30, 8}}) {
        const tksmseq_split_params s{c.chains, c.overlap, c.segments, 0};
        std::string err;
        const bool ok = tkh::map_check_split(s, err);
        printf("check %s %d %s\n", c.label, ok ? 1 : 0, err.c_str());
    }

    // ---- a line without and with the tags, plain and aligned: "paf <line>"
    tkh::MapChain c{};
    c.read = 0; c.tr = 2u; c.score = 120; c.cnt = 9; c.nmatch = 190; c.tstart = 40; c.tend = 240; c.qs = 100; c.qe = 300; c.kept = 1;
    const tkh::MapAlnOut a{205, 180, 20, 5, 0, 3, 0};
    const uint64_t runs[3] = {0ull << 2 | 0u, 100ull << 2 | 2u, 105ull << 2 | 0u};
    std::string out;
    tkh::map_paf_line("read/1", 1000, "tx", 5000, c, 60u, true, out);
    tkh::map_paf_line("read/1", 1000, "tx", 5000, c, 60u, true, out, 3u, 2u);
    tkh::map_paf_line_aligned("read/1", 1000, "tx", 5000, c, 60u, true, a, runs, false, out, 3u, 2u);
    tkh::map_paf_line_aligned("read/1", 1000, "tx", 5000, c, 60u, true, a, runs, false, out, 1u, 0u);
    for (size_t at = 0; at < out.size();) {
        const size_t end = out.find('\n', at);
        printf("paf %s\n", out.substr(at, end - at).c_str());
        at = end + 1;
    }

    // ---- the ranks of a read's tp:A:P lines by (qstart, qend, order): "ranks ..."
    for (const std::vector<std::pair<uint32_t, uint32_t>>& iv :
         {std::vector<std::pair<uint32_t, uint32_t>>{{50, 60}, {0, 10}, {70, 80}, {0, 10}}, std::vector<std::pair<uint32_t, uint32_t>>{{5, 9}}, std::vector<std::pair<uint32_t, uint32_t>>{}}) {
        std::vector<uint32_t> rank;
        tkh::map_split_ranks(iv, rank);
        std::string text;
        for (uint32_t r : rank) text += (text.empty() ? "" : " ") + std::to_string(r);
        printf("ranks %s\n", text.c_str());
    }

    // ---- the budget: "bytes ..."
    printf("bytes %llu %llu %llu\n", (unsigned long long)tkh::map_split_anchor_bytes(tksmseq_split_params{4, 30, 8, 0}, 3),
           (unsigned long long)tkh::map_split_anchor_bytes(tksmseq_split_params{16, 30, 8, 0}, 1), (unsigned long long)tkh::map_split_anchor_bytes(tksmseq_split_params{1, 30, 8, 0}, 0));
    return 0;
}
