// AddressSanitizer + UBSan over the host-only code of transcribe (csrc/tsb_host.cpp): the GTF reader and the abundance join, which read
// user files, over the golden inputs and malformed ones.  CPU only, never loaded into Python:
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer -I tksm_amd/csrc \
//       -o /tmp/sanitize_tsb_host tools/sanitize_tsb_host.cpp tksm_amd/csrc/tsb_host.cpp
//   /tmp/sanitize_tsb_host tests/golden/transcribe/ann.gtf tests/golden/transcribe/abund_exact.tsv
// Prints one line per case; texts are copied into heap blocks of their exact size first, so that a read past the end is seen.
#include "tsb_host.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
using namespace tsb;

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

static void gtf_case(const char* what, const std::string& text, bool skip, Transcripts* keep = nullptr) {
    Exact e(text);
    Transcripts t; std::string err;
    const bool ok = parse_gtf(e.p.get(), e.n, what, skip, t, err);
    printf("gtf %-28s skip=%d ok=%d transcripts=%llu exons=%llu contigs=%zu %s\n", what, (int)skip, (int)ok, (unsigned long long)t.n(), (unsigned long long)t.n_exons(),
           t.contig_names.size(), err.c_str());
    if (keep && ok) *keep = t;
}
static void ab_case(const char* what, const std::string& text, bool whole, const Transcripts& t) {
    Exact e(text);
    Abundance a; std::string err;
    const bool ok = parse_abundance(e.p.get(), e.n, whole, t, a, err);
    uint64_t found = 0;
    for (uint32_t x : a.tx) found += x != Abundance::NONE;
    std::string c;
    for (uint64_t r = 0; r < a.rows(); r++)
        if (a.tx[r] != Abundance::NONE) append_comment(c, a.text.data() + a.cb_off[r], a.cb_len[r], t.id_pool.data() + t.id_off[a.tx[r]], t.id_len[a.tx[r]]);
    printf("abundance %-22s whole=%d ok=%d rows=%llu found=%llu missing=%zu sum=%.17g comments=%zu %s\n", what, (int)whole, (int)ok, (unsigned long long)a.rows(),
           (unsigned long long)found, a.missing_off.size(), a.sum_tpm, c.size(), err.c_str());
}

int main(int argc, char** argv) {
    if (argc < 3) { fprintf(stderr, "usage: %s ann.gtf abundance.tsv\n", argv[0]); return 2; }
    const std::string gtf = slurp(argv[1]), ab = slurp(argv[2]);
    Transcripts golden;
    gtf_case("golden", gtf, false, &golden);
    gtf_case("golden", gtf, true);
    {   // a second file into the same table: nothing new, nothing lost; an unreadable path
        Transcripts t = golden; std::string err; bool io = false;
        const bool merged = read_gtf(argv[1], false, t, err, io);
        printf("merge ok=%d transcripts=%llu exons=%llu\n", (int)merged, (unsigned long long)t.n(), (unsigned long long)t.n_exons());
        const bool read = read_gtf("/no/such/dir/x.gtf", false, t, err, io);
        printf("unreadable ok=%d io=%d %s\n", (int)read, (int)io, err.c_str());
    }
    const std::string l9 = "c1\th\ttranscript\t1\t9\t.\t+\t.\tgene_id \"g\"; transcript_id \"t\";";
    const std::string ex = "c1\th\texon\t1\t9\t.\t+\t.\tgene_id \"g\"; transcript_id \"t\";";
    gtf_case("empty file", "", false);
    gtf_case("only newlines", "\n\n\n", false);
    gtf_case("no trailing newline", l9 + "\n" + ex, false);
    gtf_case("truncated line", l9 + "\n" + ex.substr(0, 17), false);
    gtf_case("truncated attributes", l9.substr(0, l9.size() - 9) + "\n" + ex.substr(0, ex.size() - 3), false);
    gtf_case("8 fields", "c1\th\ttranscript\t1\t9\t.\t+\t.", false);
    gtf_case("10 fields", l9 + "\textra\n" + ex + "\tmore\tstill", false);
    gtf_case("huge numbers", "c1\th\ttranscript\t99999999999999999999\t9\t.\t+\t.\tx", false);
    gtf_case("huge end", "c1\th\ttranscript\t1\t2147483648\t.\t+\t.\tx", false);
    gtf_case("largest numbers", "c1\th\ttranscript\t2147483647\t2147483647\t.\t+\t.\ttranscript_id t\nc1\th\texon\t2147483647\t2147483647\t.\t-\t.\t", false);
    gtf_case("zero and negative start", "c1\th\tgene\t0\t9\t.\t+\t.\tx\n", false);
    gtf_case("non-numeric", "c1\th\tgene\tabc\t9\t.\t+\t.\tx\n", false);
    gtf_case("stoi tails", "c1\th\ttranscript\t +12abc\t34.5\t.\t+\t.\ttranscript_id \"t\"\nc1\th\texon\t12\t34\t.\t\t.\t;;; ; a;\n", false);
    gtf_case("exon first", ex + "\n" + l9 + "\n", false);
    gtf_case("attribute shapes", "c1\th\ttranscript\t1\t9\t.\t+\t.\t\"transcript_id\"  ; transcript_id; transcript_id \"\"\"; gene_biotype protein_coding x;transcript_id \"a b\" c\n" + ex + "\n", true);
    gtf_case("empty fields", "\t\t\t1\t2\t\t\t\t\n\t\ttranscript\t1\t2\t\t\t\t\n\t\texon\t1\t2\t\t\t\t\n", false);
    gtf_case("comment and CR", "#x\r\n" + l9 + "\r\n" + ex + "\r\n#", false);
    {   // many transcripts: the index grows and is rebuilt
        std::string big;
        for (int i = 0; i < 5000; i++) { big += "c" + std::to_string(i % 7) + "\th\ttranscript\t1\t9\t.\t+\t.\ttranscript_id \"t" + std::to_string(i % 4000) + "\"\n"; if (i % 3) big += ex + "\n"; }
        gtf_case("5000 transcript lines", big, false);
    }
    ab_case("golden", ab, false, golden);
    ab_case("golden", ab, true, golden);
    ab_case("empty file", "", false, golden);
    ab_case("header only", "id\ttpm\tcb", false, golden);
    ab_case("no trailing newline", "h\nT1\t2\tAC", false, golden);
    ab_case("truncated line", "h\nT1\t2\tAC\nT2\t", false, golden);
    ab_case("empty lines", "h\n\n  \t \nT1\n", false, golden);
    ab_case("huge numbers", "h\nT1 1e999 AC\nT2 -1e999 AC\nT3 99999999999999999999999999999999999999999 x\nT5 1e-999 y\n", false, golden);
    ab_case("number shapes", "h\nT1 1e AC\nT1 . AC\nT1 +.5e-3x AC\nT1 1.2.3 AC\nT1 -\nT1 nan x\nT1 0x10 x\nT1 1e+ x\nT1 00012.50000000000000000000000000000000000000000000000000000000000000000000001 x\n", false, golden);
    ab_case("dots", "h\n.\t1\t.\n..\t1\n.T1\t1\nT1.\t1\nT1.2.3\t1\n", false, golden);
    ab_case("dots", "h\n.\t1\t.\n..\t1\n.T1\t1\nT1.\t1\nT1.2.3\t1\n", true, golden);
    ab_case("long id", "h\n" + std::string(100000, 'T') + "\t1\t" + std::string(100000, 'A') + "\n", false, golden);
    const char* nums[] = {"", "1", "1.5abc", "-", "+", ".", "1e5.3", "1E+2", "1e", "1e-", "e5", "12345678901234567890123456789012345678901234567890123456789012345678901234567890"};
    for (const char* z : nums) { Exact e(z); size_t taken = 0; bool ok = false; const double v = parse_tpm(e.p.get(), e.n, &taken, &ok); printf("tpm '%s' -> %.17g taken=%zu ok=%d\n", z, v, taken, (int)ok); }
    return 0;
}
