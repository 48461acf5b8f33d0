// AddressSanitizer + UBSan over the host-only code of mutate (csrc/mut_host.cpp): the reader of a variant table, which reads user files,
// and its normal form, over the golden table and malformed ones.  CPU only, never loaded into Python:
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer -I tksm_amd/csrc \
//       -o /tmp/sanitize_mut_host tools/sanitize_mut_host.cpp tksm_amd/csrc/mut_host.cpp
//   /tmp/sanitize_mut_host tests/golden/mutate/variants.tsv
// Prints one line per case; texts are copied into heap blocks of their exact size first, so that a read past the end is seen.
#include "mut_host.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
using namespace mut;

static std::string slurp(const char* path) {
    std::string s; FILE* f = fopen(path, "rb");
    if (!f) { fprintf(stderr, "cannot read %s\n", path); exit(2); }
    char buf[4096]; size_t n;
    while ((n = fread(buf, 1, sizeof buf, f)) > 0) s.append(buf, n);
    fclose(f);
    return s;
}
// an exact-size copy without a terminating byte
struct Exact { std::unique_ptr<char[]> p; size_t n; explicit Exact(const std::string& s) : p(new char[s.size() ? s.size() : 1]), n(s.size()) { memcpy(p.get(), s.data(), n); } };

static bool table_case(const char* what, const std::string& text) {
    Exact e(text);
    Variants v; std::string err; bool limit = false;
    const bool ok = parse_variants(e.p.get(), e.n, what, v, err, limit);
    // walk everything the device form is made of
    uint64_t sum = 0;
    for (size_t k = 0; k < v.names.size(); k++) {
        for (uint32_t d = v.del_first[k]; d < v.del_first[k + 1]; d++) sum += v.del_to[d] - v.del_from[d];
        for (uint32_t q = v.pt_first[k]; q < v.pt_first[k + 1]; q++)
            if (v.pt_info[q] & PT_INSERTION) { const uint64_t li = (uint32_t)v.pt_info[q]; sum += (uint8_t)v.ins_pool[v.ins_ent[2 * li] + v.ins_ent[2 * li + 1] - 1]; }
        if (v.find(v.names[k].data(), v.names[k].size()) != (int)k) { printf("find() does not find contig %zu\n", k); exit(1); }
    }
    printf("%-28s ok=%d limit=%d contigs=%zu rows=%llu snvs=%llu ins=%llu dels=%llu ranges=%llu dropped=%llu kept_ins=%llu sum=%llu %s\n", what, (int)ok, (int)limit,
           v.names.size(), (unsigned long long)v.rows, (unsigned long long)v.snvs, (unsigned long long)v.insertions, (unsigned long long)v.deletions,
           (unsigned long long)v.deleted_ranges, (unsigned long long)v.dropped_points, (unsigned long long)v.n_insertions_kept(), (unsigned long long)sum, err.c_str());
    return ok;
}

int main(int argc, char** argv) {
    if (argc < 2) { fprintf(stderr, "usage: %s variants.tsv\n", argv[0]); return 2; }
    const std::string golden = slurp(argv[1]);
    if (!table_case("golden", golden)) return 1;
    {
        Variants v; std::string err; bool limit = false, io = false;
        const bool a = read_variants(argv[1], v, err, limit, io);
        const bool b = read_variants("/no/such/dir/v.tsv", v, err, limit, io);
        printf("file ok=%d rows=%llu; unreadable ok=%d io=%d %s\n", (int)a, (unsigned long long)v.rows, (int)b, (int)io, err.c_str());
        if (!a || b || !io || v.find("chr1", 4) < 0 || v.find("chr", 3) >= 0 || v.find("", 0) >= 0) return 1;
    }
    table_case("empty file", "");
    table_case("only newlines", "\n\n\n");
    table_case("only blanks", " \t\r\n\v\f");
    table_case("no trailing newline", "c 5 A\nc 7 .AC");
    table_case("truncated line", golden.substr(0, golden.size() / 2 + 3));
    table_case("one field", "c");
    table_case("two fields", "c\t5");
    table_case("two fields and blanks", "c\t5\t \n");
    table_case("more fields", "c 5 A x y z\n");
    table_case("huge POS", "c 99999999999999999999999999 A\n");
    table_case("POS above 2^31 - 1", "c 2147483648 A\n");
    table_case("largest POS", "c 2147483647 A\nc 2147483647 2147483647\nc 0 2147483647\nc 2147483647 .A\n");
    table_case("huge deletion end", "c 5 99999999999999999999999999\n");
    table_case("negative POS", "c -5 A\n");
    table_case("signed POS", "c +5 A\n");
    table_case("lone dot", "c 5 .\n");
    table_case("dot and letter", "c 5 .A\nc 5 AA\nc 5 ..\n");
    table_case("high bytes", std::string("c\xff 5 \xfe\nc\xff 5 \xfd\xfc\n") + std::string("c\0 6 \0\n", 7));
    table_case("empty deletions", "c 5 5\nc 0 0\n");
    table_case("reversed and nested", "c 9 3\nc 4 6\nc 1 4\nc 20 30\nc 30 40\nc 3 A\nc 0 A\nc 40 .T\nc 39 .T\n");
    table_case("insertion at the limit", "c 5 ." + std::string(1u << 20, 'A'));
    table_case("insertion above the limit", "c 5 ." + std::string((1u << 20) + 1, 'A'));
    {   // many contigs and rows: every vector grows
        std::string big;
        for (int i = 0; i < 20000; i++) big += "ctg" + std::to_string(i % 300) + "\t" + std::to_string((i * 7919) % 5000) + "\t" + (i % 3 == 0 ? std::to_string((i * 104729) % 5000) : i % 3 == 1 ? "G" : "TAC") + "\n";
        table_case("20000 rows on 300 contigs", big);
    }
    return 0;
}
