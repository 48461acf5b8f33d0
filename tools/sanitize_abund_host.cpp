// AddressSanitizer + UBSan over the host-only code of abundance (csrc/abund_host.cpp): the PAF reader and interner incl. truncated and
// garbage lines, the lr-br and whitelist readers, the barcode / weight draws and the TSV writer.  CPU only, never loaded into Python:
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-omit-frame-pointer -I tksm_amd/csrc -o /tmp/sanitize_abund_host \
//       tools/sanitize_abund_host.cpp tksm_amd/csrc/abund_host.cpp -lz
//   /tmp/sanitize_abund_host tests/golden/abundance/reads.paf tests/golden/abundance/lr_matches.tsv /tmp/abund_host_out
// Prints one "key value..." line per result (tests/test_abundance.py compares them with the specification).
#include "abund_host.h"
#include <cstdio>
#include <cstring>
using namespace tkh;
int main(int argc, char** argv) {
    if (argc < 4) { fprintf(stderr, "usage: %s reads.paf lr_matches.tsv out_dir\n", argv[0]); return 2; }
    const std::string dir = argv[3];
    std::string text, e;
    AbundInput in;
    if (!abund_read_file(argv[1], text, e) || !parse_paf_abund(text.data(), text.size(), in, e)) { printf("error %s\n", e.c_str()); return 1; }
    unsigned long long sum = 0;
    for (size_t i = 0; i < in.tid.size(); i++) sum += (unsigned long long)(i + 1) * (in.tid[i] + 3ull * in.tstart[i] + 5ull * in.nmatch[i] + 7ull * in.blen[i]);
    unsigned long long qsum = 0;
    for (size_t r = 0; r < in.qlen.size(); r++) qsum += (unsigned long long)(r + 1) * in.qlen[r];
    printf("paf %zu %zu %zu %llu %llu %llu\n", in.rnames.size(), in.tnames.size(), in.tid.size(), (unsigned long long)in.n_lines, sum, qsum);
    printf("first %s %s %s %s\n", in.rnames.front().c_str(), in.rnames.back().c_str(), in.tnames.front().c_str(), in.tnames.back().c_str());
    // the same file truncated at every 997th byte: parses or names a line, never reads past the end
    int ok = 0, bad = 0;
    for (size_t cut = 0; cut < text.size(); cut += 997) {
        std::string part(text.data(), cut);              // (a copy: the sanitizer sees its exact end)
        AbundInput t; std::string err;
        if (parse_paf_abund(part.data(), part.size(), t, err)) ok++; else { bad++; if (err.compare(0, 9, "PAF line ") != 0) { printf("error %s\n", err.c_str()); return 1; } }
    }
    printf("truncated %d %d\n", ok, bad);
    const char* texts[] = {"", "\n", "a", "a\t1\t0\t1\t+\tt\t9\t0\t1\t1", "a\t1\t0\t1\t+\tt\t9\t0\t1\t1\t1", "a\t1\t0\t1\t+\tt\t9\t0\t1\t1\t1\n", "a\t1\t0\t1\t+\tt\t9\t0\t1\t1\t1\textra\tmore\n",
                           "a\tx\t0\t1\t+\tt\t9\t0\t1\t1\t1\n", "a\t1\t0\t1\t+\tt\t9\t0\t1\t1\t\n", "a\t1\t0\t1\t+\tt\t9\t-1\t1\t1\t1\n", "a\t1\t0\t1\t+\tt\t9\t0\t1\t2147483648\t1\n",
                           "a\t 7 \t0\t1\t+\tt\t9\t+3\t1\t1\t1\r\n", "a\t1\t0\t1\t+\tt\t9\t0\t1\t1\t1\n\nb\t1\t0\t1\t+\tt\t9\t0\t1\t1\t1\n", "\t1\t\t\t\t\t\t0\t\t1\t1\n",
                           "a\t1\t0\t1\t+\tt\t9\t0\t1\t1\t1\nb\t2\t0\t1\t+\tu\t9\t0\t1\t1\t1\na\t3\t0\t1\t+\tu\t9\t5\t1\t6\t7\n", "\xff\xfe\t\x01\n", "a\t1\t0\t1\t+\tt\t9\t0\t1\t99999999999999999999\t1\n"};
    for (const char* t : texts) {
        AbundInput a; std::string err;
        std::string copy(t);
        const bool good = parse_paf_abund(copy.data(), copy.size(), a, err);
        printf("parse %d %zu %zu %zu %s\n", (int)good, a.rnames.size(), a.tnames.size(), a.tid.size(), err.c_str());
    }
    {   // grouping: the third text above, read a's records are lines 1 and 3
        AbundInput a; std::string err; std::string copy(texts[14]);
        parse_paf_abund(copy.data(), copy.size(), a, err);
        printf("group");
        for (uint32_t v : a.rec_off) printf(" %u", v);
        printf(" |"); for (size_t i = 0; i < a.tid.size(); i++) printf(" %u:%u:%u:%u", a.tid[i], a.tstart[i], a.nmatch[i], a.blen[i]);
        printf(" |"); for (uint32_t v : a.qlen) printf(" %u", v);
        printf("\n");
    }
    std::unordered_map<std::string, std::string> lr;
    if (!abund_read_file(argv[2], text, e) || !parse_lr_br(text.data(), text.size(), lr, e)) { printf("error %s\n", e.c_str()); return 1; }
    unsigned long long h = 0;
    for (auto& kv : lr) for (char c : kv.first + "=" + kv.second) h += (unsigned char)c;
    printf("lrbr %zu %llu\n", lr.size(), h);
    const char* lrs[] = {"", "a\tb\t1\td\tBC", "a\tb\t1\td\tBC\n", "a\tb\t1\td\n", "a\tb\t1\td\tBC\textra\n", "a\tb\t11\td\tBC\n", "a\tb\t1\td\tX\na\tb\t1\td\tY\na\tb\t0\td\tZ\n", "\t\t\t\t\n", "\n"};
    for (const char* t : lrs) {
        std::unordered_map<std::string, std::string> m; std::string err; std::string copy(t);
        const bool good = parse_lr_br(copy.data(), copy.size(), m, err);
        printf("lrparse %d %zu %s %s\n", (int)good, m.size(), m.count("a") ? m["a"].c_str() : "-", err.c_str());
    }
    std::vector<std::string> wl;
    const std::string wtext = "AAA\nCCC\n\nGGG";
    parse_whitelist(wtext.data(), wtext.size(), wl);
    printf("whitelist %zu %s|%s|%s|%s\n", wl.size(), wl[0].c_str(), wl[1].c_str(), wl[2].c_str(), wl[3].c_str());
    std::vector<std::string> bc;
    printf("pattern_ok %d %d\n", (int)barcodes_from_pattern("NRYKMSWBDHVACGT", 5, 42, bc), (int)barcodes_from_pattern("NNX", 5, 42, bc));
    barcodes_from_pattern("NRYKMSWBDHVACGT", 5, 42, bc);
    printf("barcodes"); for (auto& b : bc) printf(" %s", b.c_str()); printf("\n");
    barcodes_from_whitelist(wl, 6, 7, bc);
    printf("drawn"); for (auto& b : bc) printf(" [%s]", b.c_str()); printf("\n");
    std::vector<double> cdf;
    cell_cdf(4, 42, 10.0, 1.0, 0.2, cdf);
    printf("cdf"); for (double v : cdf) printf(" %.17g", v); printf("\n");
    cell_cdf(3, 42, 10.0, 1.0, 1.0, cdf);
    printf("cdf_all_dropout"); for (double v : cdf) printf(" %.17g", v); printf("\n");
    cell_cdf(0, 42, 10.0, 1.0, 0.5, cdf);
    printf("cdf_none %zu\n", cdf.size());
    std::string why;
    printf("args %d %d %d %d %d %d\n", (int)abund_check_args(0, "x", "Q", "", 7.0, 0.0, -1.0, why), (int)abund_check_args(2, "x", "N", "", 0.2, 10, 1, why),
           (int)abund_check_args(2, "", "", "", 0.2, 10, 1, why), (int)abund_check_args(2, nullptr, "NX", nullptr, 0.2, 10, 1, why),
           (int)abund_check_args(2, "", "N", "", 1.5, 10, 1, why), (int)abund_check_args(2, "", "N", "", 0.2, 10, 0.0, why));
    std::vector<AbundRow> rows{{0, 0, 0.5}, {1, 1, 0.25}, {0, 1, 9.99e-10}, {1, 0, 1.0004e-9}, {0, 0, 0.0}, {1, 1, 1.2345675e-4}};
    std::vector<std::string> tn{"t0", "t1"}, cn{".", "ACGT"};
    std::string tsv;
    printf("tsv_ok %d\n", (int)abundance_tsv(rows, tn, cn, tsv));
    rows.push_back({2, 0, 0.1});
    std::string none;
    printf("tsv_bad %d\n", (int)abundance_tsv(rows, tn, cn, none));
    printf("write %d %d %d\n", (int)write_abundance_file(dir + "/a.tsv", tsv, e), (int)write_abundance_file(dir + "/a.tsv.gz", tsv, e),
           (int)write_abundance_file(dir + "/no/such/dir/a.tsv", tsv, e));
    std::string back;
    printf("gz_round_trip %d\n", (int)(abund_read_file(dir + "/a.tsv.gz", back, e) && back == tsv));
    printf("missing %d\n", (int)abund_read_file(dir + "/nothing.here", back, e));
    return 0;
}
