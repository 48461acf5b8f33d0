// sanitize_map_targets_host.cpp -- the host-only code of map -g (map_host.cpp: which transcripts become targets and their counters, the layout
// of the image, the FASTA formatter and the projection of a line to genome coordinates) as a stand-alone program for ASan / UBSan.  Build
// and run (tests/test_map_targets.py does):
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -I tksm_amd/csrc tools/sanitize_map_targets_host.cpp tksm_amd/csrc/map_host.cpp \
//       tksm_amd/csrc/ms_host.cpp tksm_amd/csrc/abund_host.cpp -lz -o sanitize_map_targets_host && ./sanitize_map_targets_host
// Prints "key values" lines the test compares with tests/map_targets_spec.py on the same table.
#include <cstdio>
#include <string>
#include <vector>

#include "map_host.h"

namespace {

struct Exon { const char* contig; uint32_t start, end; bool minus; };
struct Tx { const char* id; std::vector<Exon> exons; };

const std::vector<Tx> TABLE = {
    {"A", {{"c1", 10, 30, false}, {"c1", 40, 45, false}}},
    {"B", {{"c1", 60, 80, true}, {"c1", 50, 55, true}}},
    {"C", {}},
    {"D", {{"c1", 5, 5, false}}},
    {"E", {{"cX", 0, 10, false}}},
    {"F", {{"c1", 90, 101, false}}},
    {"G", {{"c1", 0, 10, false}, {"c2", 40, 50, true}}},
    {"H", {{"c1", 20, 30, false}, {"c1", 30, 33, false}, {"c1", 33, 33, false}, {"c1", 35, 40, false}}},
    {"I", {{"c1", 50, 60, false}, {"c1", 40, 45, false}}},
    {"J", {{"c1", 30, 20, false}}},
    {"K", {{"cX", 0, 10, false}, {"c1", 90, 101, false}}},
    {"L", {{"cd", 3, 3, false}, {"c1", 0, 33, false}}},
    {"M", {{"c2", 0, 1, true}}},
    {"N", {{"c2", 0, 32, false}, {"c2", 32, 50, true}}},
};

std::string genome_letters(uint32_t n, uint32_t seed) {
    std::string s;
    uint32_t x = seed;
    for (uint32_t i = 0; i < n; i++) {
        x = x * 1664525u + 1013904223u;
        s += (i % 23 == 7) ? 'N' : "ACGT"[x >> 30];
    }
    return s;
}

}  // namespace

int main() {
    // ---- the reference: c1 (100 letters), c2 (50), cd declared only
    const std::vector<std::string> ref_names = {"c1", "c2", "cd"};
    const std::vector<std::string> ref_letters = {genome_letters(100, 1), genome_letters(50, 2), ""};
    const std::vector<uint64_t> contigs = {0, 100, 4096, 50, 8192, 70};
    const std::vector<bool> declared = {false, false, true};
    for (size_t c = 0; c < 2; c++) printf("genome %s %s\n", ref_names[c].c_str(), ref_letters[c].c_str());

    // ---- the table
    tsb::Transcripts T;
    for (const Tx& tx : TABLE) {
        T.id_off.push_back((uint32_t)T.id_pool.size());
        T.id_len.push_back((uint32_t)std::string(tx.id).size());
        T.id_pool += tx.id;
        for (const Exon& e : tx.exons) {
            size_t ci = 0;
            while (ci < T.contig_names.size() && T.contig_names[ci] != e.contig) ci++;
            if (ci == T.contig_names.size()) T.contig_names.push_back(e.contig);
            T.ex_contig.push_back((uint32_t)ci); T.ex_start.push_back(e.start); T.ex_end.push_back(e.end); T.ex_minus.push_back(e.minus ? 1 : 0);
        }
        T.exon_first.push_back((uint32_t)T.ex_start.size());
    }
    std::vector<int32_t> contig_of;
    for (const std::string& name : T.contig_names) {
        int32_t ci = -1;
        for (size_t c = 0; c < ref_names.size(); c++) if (ref_names[c] == name && !declared[c]) ci = (int32_t)c;
        contig_of.push_back(ci);
    }

    // ---- the selection, the counters and the layout: "info ...", "target ...", "exon ..."
    tkh::MapTargets M;
    std::string err;
    const int rc = tkh::map_targets_select(T, contig_of, contigs, M, err);
    const tksmseq_targets_info& I = M.info;
    printf("info %d %llu %llu %llu %llu %llu %llu %llu %llu %llu\n", rc, (unsigned long long)I.transcripts, (unsigned long long)I.targets, (unsigned long long)I.letters,
           (unsigned long long)I.exons, (unsigned long long)I.skipped_empty, (unsigned long long)I.skipped_unknown_contig, (unsigned long long)I.skipped_bad_exon,
           (unsigned long long)I.projectable, (unsigned long long)I.image_vwords);
    std::vector<std::string> names;
    for (size_t t = 0; t < M.n(); t++) {
        names.emplace_back(T.id_pool.data() + T.id_off[M.tx[t]], T.id_len[M.tx[t]]);
        printf("target %s %u %llu %d\n", names[t].c_str(), M.len[t], (unsigned long long)M.voff[t], (int)M.projectable[t]);
        for (uint64_t e = M.efirst[t]; e < M.efirst[t + 1]; e++)
            printf("exon %s %llu %u %u %u %u %u\n", names[t].c_str(), (unsigned long long)M.exons[e].g, M.exons[e].cum, M.exons[e].len_minus & 0x7FFFFFFFu, M.exons[e].len_minus >> 31,
                   M.ex_start[e], M.ex_end[e]);
    }
    // a table without a target, and none at all
    {
        tsb::Transcripts none;
        tkh::MapTargets m2;
        std::string e2;
        const int rc2 = tkh::map_targets_select(none, {}, contigs, m2, e2);
        printf("empty %d %s\n", rc2, e2.c_str());
    }

    // ---- the FASTA of an image packed letter by letter here: "fasta <width> <text with | for a line end>"
    std::vector<uint32_t> codes(2 * M.voff.back()), valid(M.voff.back());
    for (size_t t = 0; t < M.n(); t++) {
        uint32_t j = 0;
        for (uint64_t e = M.efirst[t]; e < M.efirst[t + 1]; e++) {
            const uint32_t len = M.exons[e].len_minus & 0x7FFFFFFFu;
            const bool minus = M.exons[e].len_minus >> 31;
            const std::string& g = ref_letters[M.exons[e].g / 4096];
            for (uint32_t i = 0; i < len; i++, j++) {
                const char ch = g[minus ? M.ex_end[e] - 1 - i : M.ex_start[e] + i];
                const std::string acgt = "ACGT";
                const size_t code = acgt.find(ch);
                if (code == std::string::npos) continue;
                codes[2 * M.voff[t] + (j >> 4)] |= (uint32_t)(minus ? 3 - code : code) << (2 * (j & 15));
                valid[M.voff[t] + (j >> 5)] |= 1u << (j & 31);
            }
        }
    }
    for (int32_t width : {60, 0, 1, 7, 33}) {
        std::string text;
        tkh::map_targets_fasta(M, names, codes.data(), valid.data(), width, text);
        for (char& ch : text) if (ch == '\n') ch = '|';
        printf("fasta %d %s\n", width, text.c_str());
    }

    // ---- the projection: "line <target> <line>" as it goes in, "project <junctions> <line>" as it comes out
    struct Line { const char* target; const char* text; };
    const std::vector<Line> lines = {
        {"A", "r1\t40\t0\t25\t+\tA\t25\t0\t25\t25\t25\t60\ttp:A:P\tcm:i:3\ts1:i:25"},
        {"A", "r1\t40\t0\t25\t+\tA\t25\t0\t25\t25\t25\t60\ttp:A:P\tcm:i:3\ts1:i:25\tNM:i:0\tcg:Z:25M"},
        {"A", "r2\t40\t2\t30\t-\tA\t25\t1\t24\t20\t29\t60\ttp:A:P\tcm:i:3\ts1:i:25\tNM:i:9\tcg:Z:10=2X7=3I1D2=2I1="},
        {"A", "r3\t40\t0\t20\t+\tA\t25\t0\t20\t20\t20\t60\ttp:A:P\tcm:i:3\ts1:i:25\tsn:i:2\tsi:i:1\tNM:i:0\tcg:Z:20="},
        {"A", "r4\t40\t0\t18\t+\tA\t25\t18\t25\t13\t18\t60\ttp:A:S\tcm:i:3\ts1:i:25\tNM:i:5\tcg:Z:1=4D5I2="},
        {"B", "r5\t40\t0\t25\t+\tB\t25\t0\t25\t25\t25\t60\ttp:A:P\tcm:i:3\ts1:i:25"},
        {"B", "r5\t40\t0\t25\t-\tB\t25\t0\t25\t25\t25\t60\ttp:A:P\tcm:i:3\ts1:i:25\tNM:i:0\tcg:Z:25M"},
        {"B", "r6\t40\t5\t31\t+\tB\t25\t3\t23\t15\t28\t7\ttp:A:P\tcm:i:3\ts1:i:25\tNM:i:13\tcg:Z:5=6I12=3D2I"},
        {"H", "r7\t40\t0\t18\t+\tH\t18\t0\t18\t18\t18\t60\ttp:A:P\tcm:i:3\ts1:i:25\tNM:i:0\tcg:Z:18="},
        {"H", "r8\t40\t0\t9\t+\tH\t18\t9\t14\t3\t9\t60\ttp:A:P\tcm:i:3\ts1:i:25\tNM:i:6\tcg:Z:1=4I2D2="},
        {"H", "r9\t40\t0\t4\t+\tH\t18\t9\t13\t4\t4\t60\ttp:A:P\tcm:i:3\ts1:i:25"},
        {"M", "r10\t40\t0\t1\t-\tM\t1\t0\t1\t1\t1\t0\ttp:A:P\tcm:i:1\ts1:i:1\tNM:i:0\tcg:Z:1="},
    };
    for (const Line& l : lines) {
        uint32_t t = 0;
        while (names[t] != l.target) t++;
        std::string line = l.text;
        printf("line %s %s\n", l.target, line.c_str());
        const uint32_t ci = M.contig[t];
        const uint64_t j = tkh::map_project_line(line, M, t, names[t], ref_names[ci], contigs[2 * ci + 1]);
        printf("project %llu %s\n", (unsigned long long)j, line.c_str());
    }
    return 0;
}
