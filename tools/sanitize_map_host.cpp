// AddressSanitizer + UBSan over the host-only code of map (csrc/map_host.cpp): the parameter checks, the ratio's rounding, the tiles of the
// sketch, the packer of the reads (incl. empty reads, lengths around the word sizes and bytes outside ACGT) and the PAF line.  CPU only,
// never loaded into Python:
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-omit-frame-pointer -I tksm_amd/csrc -o /tmp/sanitize_map_host \
//       tools/sanitize_map_host.cpp tksm_amd/csrc/map_host.cpp tksm_amd/csrc/ms_host.cpp tksm_amd/csrc/abund_host.cpp -lz
//   /tmp/sanitize_map_host reads.fq
// Prints one "key value..." line per result (tests/test_map.py compares them with the specification).
#include <cstdio>
#include <cstring>

#include "abund_host.h"
#include "map_host.h"
using namespace tkh;

static tksmseq_map_params defaults() {
    tksmseq_map_params p{};
    p.k = 15; p.w = 10; p.max_occ = 500; p.max_gap = 5000; p.bandwidth = 500; p.min_count = 3; p.min_score = 40; p.secondary_ratio = 0.8; p.max_secondary = 5;
    return p;
}

static void params_case(const char* label, const tksmseq_map_params& p) {
    std::string err;
    const bool ok = map_check_params(p, err);
    printf("params %s %d %s\n", label, (int)ok, err.c_str());
}

int main(int argc, char** argv) {
    if (argc < 2) { fprintf(stderr, "usage: %s reads.fq\n", argv[0]); return 2; }
    { tksmseq_map_params p = defaults(); params_case("defaults", p); }
    { tksmseq_map_params p = defaults(); p.k = 3; params_case("k3", p); }
    { tksmseq_map_params p = defaults(); p.k = 29; params_case("k29", p); }
    { tksmseq_map_params p = defaults(); p.k = 4; p.w = 64; params_case("k4w64", p); }
    { tksmseq_map_params p = defaults(); p.w = 0; params_case("w0", p); }
    { tksmseq_map_params p = defaults(); p.w = 65; params_case("w65", p); }
    { tksmseq_map_params p = defaults(); p.max_occ = 0; params_case("occ0", p); }
    { tksmseq_map_params p = defaults(); p.max_gap = -1; params_case("gap-1", p); }
    { tksmseq_map_params p = defaults(); p.bandwidth = -1; params_case("bw-1", p); }
    { tksmseq_map_params p = defaults(); p.min_count = 0; params_case("count0", p); }
    { tksmseq_map_params p = defaults(); p.min_score = -1; params_case("score-1", p); }
    { tksmseq_map_params p = defaults(); p.secondary_ratio = 1.5; params_case("ratio1.5", p); }
    { tksmseq_map_params p = defaults(); p.secondary_ratio = -0.1; params_case("ratio-0.1", p); }
    { tksmseq_map_params p = defaults(); p.secondary_ratio = __builtin_nan(""); params_case("ratio_nan", p); }
    { tksmseq_map_params p = defaults(); p.max_secondary = 1001; params_case("n1001", p); }
    { tksmseq_map_params p = defaults(); p.chunk_reads = 1ull << 31; params_case("chunk2^31", p); }
    for (double r : {0.0, 0.0004, 0.0005, 0.8, 0.7995, 0.79949, 0.5, 1.0}) printf("permille %.5f %u\n", r, map_permille(r));

    for (uint32_t k : {4u, 15u, 28u})
        for (uint32_t w : {1u, 10u, 64u})
            for (uint64_t len : {(uint64_t)0, (uint64_t)k - 1, (uint64_t)k, (uint64_t)k + w - 2, (uint64_t)k + w - 1, (uint64_t)k + w, (uint64_t)k + w + 190, (uint64_t)k + w + 191,
                                 (uint64_t)k + w + 192, (uint64_t)5000}) {
                std::vector<MapTile> tiles;
                map_add_tiles(7, len, k, w, tiles);
                printf("tiles %u %u %llu %llu %zu %u\n", k, w, (unsigned long long)len, (unsigned long long)map_windows(len, k, w), tiles.size(), tiles.empty() ? 0u : tiles.back().j0);
            }

    std::string text, e;
    if (!abund_read_file(argv[1], text, e)) { printf("error %s\n", e.c_str()); return 1; }
    MsReads reads;
    if (!parse_fastq(text.data(), text.size(), reads, e)) { printf("error %s\n", e.c_str()); return 1; }
    const uint32_t n = (uint32_t)reads.size();
    // all reads at once, and every read alone: the letters come back, 'N' where the validity bit is clear
    auto pack_case = [&](uint32_t alone, uint32_t r0, uint32_t r1) {
        std::vector<uint32_t> codes, valid;
        std::vector<MapSeq> seqs;
        map_pack_reads(reads, r0, r1, codes, valid, seqs);
        for (uint32_t r = r0; r < r1; r++) {
            const MapSeq& q = seqs[r - r0];
            std::string back;
            for (uint32_t j = 0; j < q.len; j++) {
                const bool ok = (valid[q.voff + (j >> 5)] >> (j & 31)) & 1u;
                back.push_back(ok ? "ACGT"[(codes[2 * q.voff + (j >> 4)] >> (2 * (j & 15))) & 3u] : 'N');
            }
            printf("packed %u %u %u %llu %s\n", alone, r, q.len, (unsigned long long)q.voff, back.c_str());
        }
        printf("pack_words %u %u %zu %zu\n", alone, r0, codes.size(), valid.size());
    };
    pack_case(0, 0, n);
    for (uint32_t r = 0; r < n; r++) pack_case(1, r, r + 1);

    std::string out;
    MapChain c{3, 5 << 1 | 0, 120, 9, 101, 10, 140, 4, 131, 1};
    map_paf_line("read/1", 200, "tx", 1000, c, 60, true, out);
    c.tr = 5 << 1 | 1;
    map_paf_line("read/1", 200, "tx", 1000, c, 0, false, out);
    MapChain z{0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    map_paf_line("", 0, "", 0, z, 0, true, out);
    printf("paf %s", out.c_str());
    return 0;
}
