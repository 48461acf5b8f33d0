// tsb_host.h -- host side of transcribe (src/transcribe.cpp:119-198): the GTF reader into a transcript table and the abundance reader
// with its join.  No device code and no HIP calls: tools/sanitize_tsb_host.cpp runs these under ASan / UBSan.
//
// Reference behaviour kept (file:line into vpc-ccg/tksm), each a quirk a reader of a GTF would not expect:
//   src/transcribe.cpp:136   --default-depth is passed where read_gtf_transcripts_deep expects skip_lnc: a non-zero value drops every GTF
//                            line whose gene_biotype is not protein_coding (src/gtf.h:286); zero, the default, keeps all
//   src/transcribe.cpp:124   --non-coding is read and never used
//   src/interval.h:261-274   an attribute's value is the SECOND space-separated token of its ';' field with '"' stripped from both ends
//                            (`gene_name "A B"` is `A`); a later attribute of the same name replaces an earlier one
//   src/gtf.h:295-301        a transcript line whose transcript_id is known keeps the first line (emplace) but becomes the current
//                            transcript, so its exons are appended to the first one's; an exon goes to the current transcript whatever
//                            its own transcript_id says; exons stay in file order, each with its own strand
//   src/transcribe.cpp:136   across GTF files the first file that has an id keeps it, exons included (unordered_map::merge)
//   src/transcribe.cpp:156   only the abundance-side id is cut at its first '.', unless --use-whole-id (format_annot_id, src/util.h:203-210)
//   src/transcribe.cpp:152-155  a row is read with operator>>: any whitespace separates, a missing or unparsable tpm is 0 (and nothing
//                            is read behind it), a line without a token keeps the id "BEG"; the first line is skipped whatever it holds
// Made defined where the reference is undefined: a GTF line with fewer than 9 fields, a coordinate that is not
// a number in [1, 2^31 - 1] ([0, 2^31 - 1] for the end), an exon before any transcript line and an unreadable GTF are errors that name file
// and line; empty GTF lines are skipped; an attribute without a second token has the value "".
#pragma once
#include <stdint.h>

#include <string>
#include <vector>

namespace tsb {

// open addressing over ids that live in a pool: the one probe per GTF transcript line and per abundance row
struct IdIndex {
    std::vector<uint32_t> slot;          // transcript index + 1, 0: free
    uint32_t used = 0;
    static uint64_t hash(const char* s, size_t n);
};

struct Transcripts {
    // transcript t: id = id_pool[id_off[t], +id_len[t]), exons [exon_first[t], exon_first[t + 1])
    std::vector<uint32_t> id_off, id_len, exon_first{0};
    std::string id_pool;
    // exon e (SoA): contig = contig_names[ex_contig[e]], [ex_start, ex_end) 0-based half-open as the MDF prints them, ex_minus
    std::vector<uint32_t> ex_contig, ex_start, ex_end;
    std::vector<uint8_t> ex_minus;
    std::vector<std::string> contig_names;
    IdIndex index;
    uint64_t serial = 0;                 // set by the owner: a table that has changed is a new table with a new serial
    uint64_t n() const { return id_off.size(); }
    uint64_t n_exons() const { return ex_start.size(); }
    int find(const char* id, size_t len) const;      // -1: not there
};

// read_gtf_transcripts_deep (src/gtf.h:274-304) + the gtf line constructor (src/interval.h:252-275) over one file's text, merged into `into`
// like std::unordered_map::merge (ids already there stay).  name: for the messages.  false: err names file and line, `into` is unchanged.
bool parse_gtf(const char* text, size_t len, const std::string& name, bool skip_non_coding, Transcripts& into, std::string& err);
// false with io = true: the file cannot be read
bool read_gtf(const std::string& path, bool skip_non_coding, Transcripts& into, std::string& err, bool& io);

// the rows of one abundance table joined with the transcripts (src/transcribe.cpp:149-158, :170-179)
struct Abundance {
    static constexpr uint32_t NONE = 0xffffffffu;
    std::vector<uint32_t> tx;            // [rows] transcript index, NONE: "Isoform {} is not found in the input GTFs!"
    std::vector<double> tpm;             // [rows]
    std::vector<uint32_t> cb_off, cb_len;   // [rows] the third column, in `text`
    std::vector<uint32_t> missing_off, missing_len;   // the (trimmed) ids of the NONE rows in row order, in `text`
    std::string text;                    // the table's own bytes (ids and barcodes point into it)
    double sum_tpm = 0.0;                // left to right over every row, found or not (:170)
    uint64_t rows() const { return tx.size(); }
};
// false: more than 2^32 - 2 bytes or rows
bool parse_abundance(const char* text, size_t len, bool use_whole_id, const Transcripts& t, Abundance& out, std::string& err);

// what `istream >> double` (libstdc++ num_get) makes of the token at p[0, n): the value and how many bytes it took; *ok = false: failbit
// (the value is then 0, or +-DBL_MAX for a number beyond the range of double)
double parse_tpm(const char* p, size_t n, size_t* taken, bool* ok);

// dump_comment (src/interval.h:881-891) of {"CB": [cb], "tid": [tid]}: keys sorted, a value "." prints the bare key
void append_comment(std::string& out, const char* cb, size_t cb_len, const char* tid, size_t tid_len);

}  // namespace tsb
