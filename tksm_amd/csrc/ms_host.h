// ms_host.h -- host side of model-sequence (include/tksmseq.h): the FASTQ reader and the interner of read names, the PAF reader with its
// cg:Z: tags, and the writers of the two model files.  No device code: tools/sanitize_ms_host.cpp runs these under ASan / UBSan.
#pragma once
#include <stdint.h>

#include <string>
#include <unordered_map>
#include <vector>

namespace tkh {

// the reads of every FASTQ file, in file order: bases (upper-cased) and qualities (char - 33) in one pool each
struct MsReads {
    std::vector<uint8_t> bases, quals;
    std::vector<uint64_t> off{0};                        // [n_reads + 1] into both pools
    std::unordered_map<std::string, uint32_t> index;     // name (the header up to the first white space) -> read
    size_t size() const { return off.size() - 1; }
    std::vector<std::string> names() const {             // the names in read order
        std::vector<std::string> v(size());
        for (const auto& kv : index) v[kv.second] = kv.first;
        return v;
    }
};
// appends the records of one file's text.  false with err = "FASTQ record N: ..." (a record of fewer than four lines, a header without
// '@', a third line without '+', sequence and quality of different lengths, a quality outside [0, 93], a name seen before) or
// "model-sequence: 2^32 reads or more"
bool parse_fastq(const char* text, size_t len, MsReads& out, std::string& err);
// appends the records of every file of a comma-separated list (empty entries are passed over; .gz is read as such), in list order.  What was
// read before a failure stays appended.  Returns TKSMSEQ_OK, or TKSMSEQ_EIO: err = abund_read_file's; TKSMSEQ_EINVAL: err = "<path>: FASTQ
// record N: ..."; TKSMSEQ_ELIMIT: err = "<path>: " + parse_fastq's limit, or, with read_limit > 0, no message once a file has brought the
// reads to read_limit (the callers that count word that limit themselves)
int load_fastq_list(const std::string& list, MsReads& out, std::string& err, uint64_t read_limit = 0);

// alignment column ops as the kernels read them: length << 2 | MS_OP_*
enum { MS_OP_M = 0, MS_OP_I = 1, MS_OP_D = 2 };
struct MsAln { uint32_t read, tid, qlen, qstart, qend, tstart, tend, strand /* 1: '-' */, op_off, n_ops; };
struct MsAlignments {
    std::vector<MsAln> aln;
    std::vector<uint32_t> ops;
    uint64_t lines = 0, no_cigar = 0, supplementary = 0, unknown_read = 0, unknown_target = 0, cigar_op = 0;
};
// the used lines of a PAF in file order (the rules of include/tksmseq.h, checked in this order: columns, cg:Z:, tp:A:S, read, target, ops,
// integers, ranges, read length, consumed lengths); max_alignments > 0 stops after that many used lines.  false: err = "PAF line N: ..."
// (or "model-sequence: 2^32 ops or more")
bool parse_paf_ms(const char* text, size_t len, const MsReads& reads, const std::unordered_map<std::string, uint32_t>& targets,
                  const std::vector<uint64_t>& target_len, uint64_t max_alignments, MsAlignments& out, std::string& err);

// ---- the tables the device hands back, and their text
constexpr int MS_MAX_ALT = 31, MS_MAX_ALT_LEN = 12, MS_Q = 94, MS_KEY_MAX = 29;
// one k-mer: alt = length << 24 | bases, 2 bits each, the first in bits 23..22
struct MsErrRow { uint64_t total = 0, self = 0, too_long = 0; uint32_t n_alt = 0; uint32_t alt[MS_MAX_ALT] = {}; uint64_t count[MS_MAX_ALT] = {}; };
// rows: all 4^k k-mers in ACGT order
void error_model_text(int k, const std::vector<MsErrRow>& rows, std::string& out);
// a q-score key: length << 58 | letters, 2 bits each ('=' 0, 'D' 1, 'I' 2, 'X' 3: the order of their bytes), the first in bits 57..56
struct MsQRow { uint64_t key = 0, n = 0; uint64_t count[MS_Q] = {}; };
std::string ms_key_text(uint64_t key);
// the written keys of the rule in include/tksmseq.h: `best` = the keys with n >= min_occur in file order (at least the first max_output of
// them), `forced` = the rows of "=", "I" and "X" (n = 0: never seen).  false: err names the forced key with count 0
bool qscore_select(const std::vector<MsQRow>& best, const MsQRow forced[3], uint64_t max_output, std::vector<MsQRow>& out, std::string& err);
void qscore_model_text(const MsQRow& overall, const std::vector<MsQRow>& rows, std::string& out);

}  // namespace tkh
