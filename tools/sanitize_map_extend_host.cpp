// sanitize_map_extend_host.cpp -- the host-only code of map --extend (map_host.cpp: the parameter checks, the moved corners, the join of
// an end's columns and runs with the chain's, the budget arithmetic) as a stand-alone program for ASan / UBSan.  Build and run
// (tests/test_map_extend.py does):
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -I tksm_amd/csrc tools/sanitize_map_extend_host.cpp tksm_amd/csrc/map_host.cpp \
//       tksm_amd/csrc/ms_host.cpp tksm_amd/csrc/abund_host.cpp -lz -o sanitize_map_extend_host && ./sanitize_map_extend_host
// Prints "key values" lines the test compares with tests/map_extend_spec.py.
#include <cstdio>
#include <string>
#include <vector>

#include "map_host.h"

namespace {
// columns as letters -> what the device hands over for them: the counts and the runs (first column << 2 | op)
tkh::MapAlnOut coded(const std::string& columns, bool eqx, std::vector<uint64_t>& runs) {
    tkh::MapAlnOut a{};
    runs.clear();
    uint32_t last = 4;
    for (size_t x = 0; x < columns.size(); x++) {
        const char c = columns[x];
        const uint32_t code = c == '=' ? 0u : c == 'X' ? 1u : c == 'I' ? 2u : 3u, op = eqx || code >= 2u ? code : 0u;
        a.eq += code == 0u; a.x += code == 1u; a.ins += code == 2u; a.del += code == 3u;
        if (op != last) runs.push_back((uint64_t)x << 2 | op);
        last = op;
    }
    a.ncols = (uint32_t)columns.size();
    a.runs = (uint32_t)runs.size();
    return a;
}
}  // namespace

int main() {
    // ---- parameter checks: "check <label> <ok> <message>"
    struct Case { const char* label; int32_t band, drop, max_ext; };
    for (const Case& c : {Case{"defaults", 31, 40, 2000}, Case{"lowest", 1, 1, 1}, Case{"highest", 63, 1000, 32768}, Case{"band0", 0, 40, 2000}, Case{"band64", 64, 40, 2000},
                          Case{"drop0", 31, 0, 2000}, Case{"drop1001", 31, 1001, 2000}, Case{"max0", 31, 40, 0}, Case{"max32769", 31, 40, 32769}, Case{"band-1", -1, 40, 2000}}) {
        const tksmseq_extend_params e{c.band, c.drop, c.max_ext, 0};
        std::string err;
        const bool ok = tkh::map_check_extend(e, err);
        printf("check %s %d %s\n", c.label, ok ? 1 : 0, err.c_str());
    }

    // ---- a line with both ends, one end, no end: "paf <line>"
    auto line = [](const std::string& left, const std::string& mid, const std::string& right, bool eqx, uint32_t rel) {
        std::vector<uint64_t> lr, mr, rr, runs;
        const tkh::MapAlnOut l = coded(left, eqx, lr), m = coded(mid, eqx, mr), r = coded(right, eqx, rr);
        tkh::MapChain c{};
        c.read = 0; c.tr = 2u | rel; c.score = 120; c.cnt = 9; c.nmatch = 101;
        c.tstart = 100000; c.tend = 100000 + m.eq + m.x + m.del; c.qs = 90000; c.qe = 90000 + m.eq + m.x + m.ins; c.kept = 1;
        const tkh::MapExtEnd le{l.eq + l.x + l.del, l.eq + l.x + l.ins, l.eq, 0, 0}, re{r.eq + r.x + r.del, r.eq + r.x + r.ins, r.eq, 0, 0};
        const tkh::MapChain moved = tkh::map_extended_chain(c, le, re);
        const tkh::MapAlnOut all = tkh::map_join_columns(left.empty() ? nullptr : &l, lr.data(), m, mr.data(), right.empty() ? nullptr : &r, rr.data(), runs);
        std::string out;
        tkh::map_paf_line_aligned("read/1", 200000, "tx", 300000, moved, 60u, true, all, runs.data(), eqx, out);
        printf("paf %s", out.c_str());
        tkh::MapChain plain = moved;
        plain.nmatch += le.m + re.m;
        out.clear();
        tkh::map_paf_line("read/1", 200000, "tx", 300000, plain, 60u, true, out);
        printf("plain %s", out.c_str());
    };
    const std::string mid = std::string(20, '=') + "X" + std::string(5, '=') + "I" + std::string(9, '=');
    for (const bool eqx : {false, true})
        for (const uint32_t rel : {0u, 1u}) {
            line("==X==", mid, "=D===", eqx, rel);                                  // the same op on both sides of both seams
            line("==XX", "X" + mid + "I", "I==", eqx, rel);                          // X meets X, I meets I: one run each
            line("", mid, "===", eqx, rel);
            line("=I=", mid, "", eqx, rel);
            line("", mid, "", eqx, rel);
            line(std::string(70000, '=') + "D", mid, "X" + std::string(66000, '='), eqx, rel);
        }

    // ---- the budget: "bytes ..."
    printf("bytes %llu %llu %llu\n", (unsigned long long)tkh::map_extend_fixed_bytes(10, 0, 0, 0), (unsigned long long)tkh::map_extend_fixed_bytes(10, 7, 100, 50),
           (unsigned long long)tkh::map_extend_fixed_bytes(1ull << 32, 1ull << 32, 1ull << 33, 1ull << 34));
    return 0;
}
