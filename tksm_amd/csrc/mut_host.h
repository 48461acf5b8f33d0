// mut_host.h -- host side of mutate: the reader of a variant table (the -t/--tsv format of src/mutate.cpp:157-181, Mod::Mod :99-108) and its
// normal form.  No device code and no HIP calls: tools/sanitize_mut_host.cpp runs this under ASan / UBSan.
//
// A line is `CONTIG POS MOD`, whitespace-separated (space, \t, \v, \f, \r); lines without a field are skipped, fields behind the third are
// not read.  POS is 0-based on the plus strand.  MOD all digits: a deletion of [min(POS, MOD), max(POS, MOD)) (empty: counted, otherwise
// ignored); MOD one byte that is no digit: an SNV, the base at POS becomes that byte (a lone '.' is refused); anything else: an insertion
// `X SEQ` -- X is '.' or the letter that replaces the anchor base at POS, SEQ (the rest) goes in BEHIND the anchor, as plus-strand text.
// Made defined where the reference reads garbage or throws: fewer than three fields, a POS or a deletion end that is
// no integer in [0, 2^31 - 1] (digits only) and a lone '.' are errors that name file and line; an insertion of more than 2^20 letters and a
// table of 2^31 rows or more are limits.
//
// Normal form, per contig name: the deletions sorted and their union taken (disjoint half-open ranges, ascending; ranges that touch are
// one); the point variants -- SNVs and insertions -- sorted by (POS, line), those inside a deleted range dropped and counted.
#pragma once
#include <stdint.h>

#include <string>
#include <vector>

namespace mut {

constexpr uint32_t MAX_POS = 0x7fffffffu;
constexpr uint32_t MAX_INSERTION = 1u << 20;         // the limit polyA and tag have
// pt_info: bits 0..31 the insertion's ordinal among the kept insertions of the table, bits 32..39 the letter, bit 40 "carries a letter"
// (every SNV; an insertion whose X is not '.'), bit 41 "is an insertion"
constexpr uint64_t PT_LETTER = 1ull << 40, PT_INSERTION = 1ull << 41;

struct Variants {
    // contig k: names[k]; the contigs are sorted by (length of the name, bytes), which is the order the device searches them in
    std::vector<std::string> names;
    std::vector<uint32_t> del_first{0}, pt_first{0};      // [contigs + 1] into the arrays below
    std::vector<uint32_t> del_from, del_to;               // disjoint ranges, ascending
    std::vector<uint32_t> pt_pos;                         // ascending; equal positions in line order
    std::vector<uint64_t> pt_info;
    std::vector<uint64_t> ins_ent;                        // [kept insertions][2] {offset into ins_pool, letters}
    std::string ins_pool;
    // rows: lines with fields; snvs + insertions + deletions == rows (empty deletions included); deleted_ranges: ranges of the normal form;
    // dropped_points: SNVs and insertions inside a deleted range
    uint64_t rows = 0, snvs = 0, insertions = 0, deletions = 0, deleted_ranges = 0, dropped_points = 0;
    uint64_t serial = 0;                                  // set by the owner: every loaded table has its own
    uint64_t n_insertions_kept() const { return ins_ent.size() / 2; }
    int find(const char* name, size_t len) const;         // -1: not there
};

// name: for the messages.  false: err says why ("<name>:<line>: ..."), limit = true for a limit rather than a malformed line
bool parse_variants(const char* text, size_t len, const std::string& name, Variants& out, std::string& err, bool& limit);
// false with io = true: the file cannot be read
bool read_variants(const std::string& path, Variants& out, std::string& err, bool& limit, bool& io);

}  // namespace mut
