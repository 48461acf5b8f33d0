// AddressSanitizer + UBSan over the host-only code of model-sequence (csrc/ms_host.cpp): the FASTQ reader and interner, the PAF / cg:Z:
// reader incl. truncated and garbage input, the FASTQ list loader of the three tools that read reads, and the writers of the two model files.
// CPU only, never loaded into Python:
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-omit-frame-pointer -I tksm_amd/csrc -o /tmp/sanitize_ms_host \
//       tools/sanitize_ms_host.cpp tksm_amd/csrc/ms_host.cpp tksm_amd/csrc/abund_host.cpp -lz
//   /tmp/sanitize_ms_host ref.fa reads.fq aln.paf /tmp/ms_host_out
// Prints one "key value..." line per result (tests/test_model_sequence.py compares them with the specification).
#include <algorithm>
#include <cstdio>
#include <cstring>

#include "abund_host.h"
#include "ms_host.h"
using namespace tkh;

static void paf_case(const char* label, const std::string& text, const MsReads& reads, const std::unordered_map<std::string, uint32_t>& targets,
                     const std::vector<uint64_t>& tlen, uint64_t max_aln = 0) {
    MsAlignments a; std::string err;
    std::string copy(text);                                    // (a copy: the sanitizer sees its exact end)
    const bool ok = parse_paf_ms(copy.data(), copy.size(), reads, targets, tlen, max_aln, a, err);
    printf("paf_case %s %d %zu %zu %llu %llu %llu %llu %llu %llu %s\n", label, (int)ok, a.aln.size(), a.ops.size(), (unsigned long long)a.lines, (unsigned long long)a.no_cigar,
           (unsigned long long)a.supplementary, (unsigned long long)a.unknown_read, (unsigned long long)a.unknown_target, (unsigned long long)a.cigar_op, err.c_str());
}

static bool same_reads(const MsReads& a, const MsReads& b) { return a.bases == b.bases && a.quals == b.quals && a.off == b.off && a.index == b.index; }

// the FASTQ list loader on files written into dir: "list_case label result reads same-as-`want` message"
static void list_cases(const std::string& dir) {
    const std::string a = "@a1 x\nACGT\n+\nIIII\n@a2\nGG\n+\n#I\n", b = "@b1\nTTTAA\n+\n!!!~~\n\n@b2\nC\n+\n5\n", dup = "@b3\nAC\n+\nII\n@a2\nT\n+\nI\n";
    const std::string cut = b.substr(0, b.size() - 5);                                   // ends inside the record of b2
    std::string e;
    for (const auto& f : {std::make_pair("a.fq", a), std::make_pair("b.fq", b), std::make_pair("b.fq.gz", b), std::make_pair("cut.fq", cut), std::make_pair("dup.fq", dup)})
        if (!write_abundance_file(dir + "/" + f.first, f.second, e)) { printf("error %s\n", e.c_str()); return; }
    MsReads both, first, none;
    const std::string ab = a + b;
    parse_fastq(ab.data(), ab.size(), both, e);
    parse_fastq(a.data(), a.size(), first, e);
    const std::string A = dir + "/a.fq", B = dir + "/b.fq";
    struct Case { const char* label; std::string list; const MsReads* want; uint64_t limit; };
    const Case cases[] = {{"two", A + "," + B, &both, 0}, {"empty_entries", A + ",," + B + ",", &both, 0}, {"empty", "", &none, 0}, {"comma", ",", &none, 0},
                          {"missing", A + "," + dir + "/nosuch.fq", &first, 0}, {"cut", A + "," + dir + "/cut.fq", nullptr, 0}, {"duplicate", A + "," + dir + "/dup.fq", nullptr, 0},
                          {"gz", A + "," + B + ".gz", &both, 0}, {"limit_after_second", A + "," + B, &both, 3}, {"limit_after_first", A + "," + B, &first, 2}};
    for (const Case& c : cases) {
        MsReads r; std::string err;
        const int res = load_fastq_list(c.list, r, err, c.limit);
        printf("list_case %s %d %zu %d %s\n", c.label, res, r.size(), c.want ? (int)same_reads(r, *c.want) : -1, err.c_str());
    }
    std::string text, io;
    abund_read_file(dir + "/nosuch.fq", text, io);
    printf("list_io_message %s\n", io.c_str());
    std::string names;
    for (const std::string& n : both.names()) names += n + " ";
    printf("list_names %s\n", names.c_str());
}

int main(int argc, char** argv) {
    if (argc < 5) { fprintf(stderr, "usage: %s ref.fa reads.fq aln.paf out_dir\n", argv[0]); return 2; }
    const std::string dir = argv[4];
    std::string text, e;
    // the contig names and lengths of a plain FASTA
    std::unordered_map<std::string, uint32_t> targets; std::vector<uint64_t> tlen;
    if (!abund_read_file(argv[1], text, e)) { printf("error %s\n", e.c_str()); return 1; }
    for (size_t a = 0; a < text.size();) {
        size_t b = text.find('\n', a);
        if (b == std::string::npos) b = text.size();
        if (text[a] == '>') { size_t z = a + 1; while (z < b && text[z] != ' ' && text[z] != '\t') z++; targets.emplace(text.substr(a + 1, z - a - 1), (uint32_t)tlen.size()); tlen.push_back(0); }
        else if (!tlen.empty()) tlen.back() += b - a;
        a = b + 1;
    }
    MsReads reads;
    std::string fq;
    if (!abund_read_file(argv[2], fq, e) || !parse_fastq(fq.data(), fq.size(), reads, e)) { printf("error %s\n", e.c_str()); return 1; }
    unsigned long long sum = 0;
    for (size_t i = 0; i < reads.bases.size(); i++) sum += (unsigned long long)(i % 1000 + 1) * (reads.bases[i] + 3ull * reads.quals[i]);
    printf("fastq %zu %zu %llu\n", reads.size(), reads.bases.size(), sum);
    // the same file cut at every 997th byte: parses or names a record, never reads past the end
    int ok = 0, bad = 0;
    for (size_t cut = 0; cut < fq.size(); cut += 997) {
        std::string part(fq.data(), cut);
        MsReads r; std::string err;
        if (parse_fastq(part.data(), part.size(), r, err)) ok++; else { bad++; if (err.compare(0, 13, "FASTQ record ") != 0) { printf("error %s\n", err.c_str()); return 1; } }
    }
    printf("fastq_cut %d %d\n", ok, bad);
    const char* fqs[] = {"", "\n\n", "@a\nACGT\n+\nIIII\n", "@a x y\nacgtn\n+a\n!!~~I", "@a\nACGT\n+\nIII\n", "@a\nACGT\n+\n", "@a\nACGT\n", "a\nACGT\n+\nIIII\n", "@a\nACGT\n-\nIIII\n",
                         "@a\nACGT\n+\nII\x7fI\n", "@a\nACGT\n+\nII I\n", "@a\nAC\n+\nII\n@a\nAC\n+\nII\n", "@a\r\nAC\r\n+\r\nII\r\n\r\n@b\tz\nG\n+\n#\n", "@\n\n+\n\n", "\xff\xfe\n\x01"};
    for (const char* t : fqs) {
        MsReads r; std::string err; std::string copy(t);
        const bool good = parse_fastq(copy.data(), copy.size(), r, err);
        printf("fastq_case %d %zu %zu %s\n", (int)good, r.size(), r.bases.size(), err.c_str());
    }
    {
        MsReads r; std::string err; std::string copy(fqs[3]);
        parse_fastq(copy.data(), copy.size(), r, err);
        printf("fastq_values %s %d %d %d %d %d\n", std::string(r.bases.begin(), r.bases.end()).c_str(), r.quals[0], r.quals[1], r.quals[2], r.quals[3], r.quals[4]);
    }
    MsAlignments al;
    std::string paf;
    if (!abund_read_file(argv[3], paf, e) || !parse_paf_ms(paf.data(), paf.size(), reads, targets, tlen, 0, al, e)) { printf("error %s\n", e.c_str()); return 1; }
    sum = 0;
    for (size_t i = 0; i < al.aln.size(); i++) {
        const MsAln& a = al.aln[i];
        unsigned long long cols = 0;
        for (uint32_t o = 0; o < a.n_ops; o++) cols += al.ops[a.op_off + o] >> 2;
        sum += (unsigned long long)(i + 1) * (a.qstart + 3ull * a.qend + 5ull * a.tstart + 7ull * a.tend + 11ull * a.strand + 13ull * cols + 17ull * a.tid);
    }
    printf("paf %zu %llu %llu %llu %llu %llu %llu %llu\n", al.aln.size(), (unsigned long long)al.lines, (unsigned long long)al.no_cigar, (unsigned long long)al.supplementary,
           (unsigned long long)al.unknown_read, (unsigned long long)al.unknown_target, (unsigned long long)al.cigar_op, sum);
    ok = 0; bad = 0;
    for (size_t cut = 0; cut < paf.size(); cut += 997) {
        std::string part(paf.data(), cut);
        MsAlignments t; std::string err;
        if (parse_paf_ms(part.data(), part.size(), reads, targets, tlen, 0, t, err)) ok++; else { bad++; if (err.compare(0, 9, "PAF line ") != 0) { printf("error %s\n", err.c_str()); return 1; } }
    }
    printf("paf_cut %d %d\n", ok, bad);
    // hand-made lines over a read "r" of 10 bases and a contig "t" of 20
    MsReads one; std::string err1; const std::string r1 = "@r\nACGTACGTAC\n+\nIIIIIIIIII\n";
    parse_fastq(r1.data(), r1.size(), one, err1);
    std::unordered_map<std::string, uint32_t> tg{{"t", 0u}}; std::vector<uint64_t> tl{20};
    const std::string head = "r\t10\t1\t9\t+\tt\t20\t2\t10\t8\t8\t60\t";
    paf_case("good", head + "tp:A:P\tcg:Z:8M\n", one, tg, tl);
    paf_case("mixed_ops", head + "cg:Z:2=1X1I3M1D1=\n", one, tg, tl);
    paf_case("empty", "", one, tg, tl);
    paf_case("nine_columns", "r\t10\t1\t9\t+\tt\t20\t2\t10\n", one, tg, tl);
    paf_case("wrong_read_length", head + "cg:Z:7M\n", one, tg, tl);
    paf_case("wrong_target_length", head + "cg:Z:7M1I\n", one, tg, tl);
    paf_case("no_number", head + "cg:Z:M\n", one, tg, tl);
    paf_case("trailing_number", head + "cg:Z:8M3\n", one, tg, tl);
    paf_case("empty_cigar", head + "cg:Z:\n", one, tg, tl);
    paf_case("garbage_op", head + "cg:Z:8*\n", one, tg, tl);
    paf_case("huge_op", head + "cg:Z:99999999999M\n", one, tg, tl);
    paf_case("clip", head + "cg:Z:1S8M\n", one, tg, tl);
    paf_case("no_cg", head + "tp:A:P\n", one, tg, tl);
    paf_case("supplementary", head + "tp:A:S\tcg:Z:8M\n", one, tg, tl);
    paf_case("unknown_read", "q" + head.substr(1) + "cg:Z:8M\n", one, tg, tl);
    paf_case("unknown_target", "r\t10\t1\t9\t+\tu\t20\t2\t10\t8\t8\t60\tcg:Z:8M\n", one, tg, tl);
    paf_case("not_a_number", "r\t10\tx\t9\t+\tt\t20\t2\t10\t8\t8\t60\tcg:Z:8M\n", one, tg, tl);
    paf_case("negative", "r\t10\t-1\t9\t+\tt\t20\t2\t10\t8\t8\t60\tcg:Z:8M\n", one, tg, tl);
    paf_case("two_to_the_31", "r\t10\t1\t2147483648\t+\tt\t20\t2\t10\t8\t8\t60\tcg:Z:8M\n", one, tg, tl);
    paf_case("start_after_end", "r\t10\t9\t1\t+\tt\t20\t2\t10\t8\t8\t60\tcg:Z:8M\n", one, tg, tl);
    paf_case("end_after_length", "r\t10\t1\t11\t+\tt\t20\t2\t12\t8\t8\t60\tcg:Z:10M\n", one, tg, tl);
    paf_case("target_end_after_contig", "r\t10\t1\t9\t+\tt\t20\t13\t21\t8\t8\t60\tcg:Z:8M\n", one, tg, tl);
    paf_case("column_2", "r\t11\t1\t9\t+\tt\t20\t2\t10\t8\t8\t60\tcg:Z:8M\n", one, tg, tl);
    paf_case("strand", "r\t10\t1\t9\t*\tt\t20\t2\t10\t8\t8\t60\tcg:Z:8M\n", one, tg, tl);
    paf_case("second_line_bad", head + "cg:Z:8M\n\n" + head + "cg:Z:9M\n", one, tg, tl);
    paf_case("max_alignments", head + "cg:Z:8M\n" + head + "cg:Z:8M\n" + head + "cg:Z:9M\n", one, tg, tl, 2);
    paf_case("binary", "\xff\xfe\t\x01\n", one, tg, tl);

    // the writers
    std::vector<MsErrRow> rows(64);
    rows[0].total = 4; rows[0].self = 2; rows[0].n_alt = 2; rows[0].alt[0] = 4u << 24 | 0x1u << 16; rows[0].count[0] = 1; rows[0].alt[1] = 2u << 24; rows[0].count[1] = 1;
    rows[63].total = 3; rows[63].n_alt = 1; rows[63].alt[0] = 7u << 24 | 0xFFFFFFu; rows[63].count[0] = 2;
    std::string etext;
    error_model_text(3, rows, etext);
    printf("error_lines %zu\n", (size_t)std::count(etext.begin(), etext.end(), '\n'));
    MsQRow overall, forced[3];
    overall.n = 8; overall.count[0] = 1; overall.count[10] = 4; overall.count[93] = 3;
    forced[0].key = 1ull << 58; forced[1].key = 1ull << 58 | 3ull << 56; forced[2].key = 1ull << 58 | 2ull << 56;
    forced[0].n = 5; forced[0].count[10] = 4; forced[0].count[93] = 1; forced[1].n = 1; forced[1].count[0] = 1; forced[2].n = 2; forced[2].count[93] = 2;
    std::vector<MsQRow> best(2), sel;
    best[0] = forced[0];
    best[1].key = 3ull << 58 | 0x04ull << 52; best[1].n = 3; best[1].count[7] = 3;          // "=D="
    std::string err;
    bool good = qscore_select(best, forced, 2, sel, err);
    printf("select %d %zu\n", (int)good, sel.size());
    std::string qtext;
    qscore_model_text(overall, sel, qtext);
    good = qscore_select(best, forced, 10, sel, err);
    printf("select_all %d %zu\n", (int)good, sel.size());
    forced[2].n = 0;
    good = qscore_select(best, forced, 10, sel, err);
    printf("select_missing %d %s\n", (int)good, err.c_str());
    printf("key_text %s %s %s\n", ms_key_text(best[1].key).c_str(), ms_key_text(29ull << 58 | 0x3FFFFFFFFFFFFFFull).c_str(), ms_key_text(~0ull).c_str());
    printf("write %d %d %d %d\n", (int)write_abundance_file(dir + "/e.model", etext, e), (int)write_abundance_file(dir + "/e.model.gz", etext, e),
           (int)write_abundance_file(dir + "/q.model", qtext, e), (int)write_abundance_file(dir + "/no/such/dir/q.model", qtext, e));
    std::string back;
    printf("gz_round_trip %d\n", (int)(abund_read_file(dir + "/e.model.gz", back, e) && back == etext));
    list_cases(dir);
    return 0;
}
