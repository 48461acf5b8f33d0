// abund_host.h -- host side of abundance (py/transcript_abundance.py): the PAF reader and interner, the lr-br and whitelist readers, the
// barcode and weight draws of --cb-count, and the TSV writer.  No device code: tools/sanitize_abund_host.cpp runs these under ASan / UBSan.
#pragma once
#include <stdint.h>

#include <string>
#include <unordered_map>
#include <vector>

namespace tkh {

// parse_paf (:182-203): every line counts (no tp:A filter), columns 0, 1, 5, 7, 9, 10.  Reads and transcripts are numbered in order of
// first appearance; a read's records are all lines with its name in file order, adjacent or not (CSR over the reads).
struct AbundInput {
    std::vector<std::string> tnames, rnames;
    std::vector<uint32_t> rec_off;                       // [n_reads + 1]
    std::vector<uint32_t> tid, tstart, nmatch, blen;     // [n_records], grouped by read
    std::vector<uint32_t> qlen;                          // [n_reads]: column 1 of the read's FIRST record (:224)
    uint64_t n_lines = 0;
};
// false with err = "PAF line N: ..." (fewer than 11 columns, a used column that int() refuses, a value outside [0, 2^31)) or
// "abundance: 2^31 ..." (limit: *limit set)
bool parse_paf_abund(const char* text, size_t len, AbundInput& out, std::string& err, bool* limit = nullptr);
// the file's bytes; .gz (and anything else zlib reads) decompressed
bool abund_read_file(const std::string& path, std::string& out, std::string& err);

// parse_lr_bc_matches (:166-179): exactly five columns per line (anything else: err names the line); column 2 == "1": read (column 0)
// -> barcode (column 4), a later line overwriting an earlier one
bool parse_lr_br(const char* text, size_t len, std::unordered_map<std::string, std::string>& out, std::string& err);
// parse_barcodes_txt (:153-163): one barcode per line
void parse_whitelist(const char* text, size_t len, std::vector<std::string>& out);

// the argument checks of parse_args (:121-138) with its messages; they apply when cb_count > 0 only.  sigma: the reference asserts > 0
bool abund_check_args(long long cb_count, const char* lr_br, const char* pattern, const char* txt, double dropout, double mu, double sigma, std::string& err);

// the counter-based draws of --cb-count (include/tksmseq.h): Philox4x32-10 keyed by (seed, g, stream, n), the kernels' layout
enum { ST_ABUND_BC = 57, ST_ABUND_BC_TXT = 58, ST_ABUND_WEIGHT = 59, ST_ABUND_CELL = 60 };
void abund_philox(uint64_t seed, uint64_t g, uint32_t stream, uint32_t n, uint32_t w[4]);
// the letters an IUPAC pattern letter stands for (IUPAC_nts :13-29), or null
const char* iupac_letters(char c);
// barcode b of a pattern: letter p = set[umulhi32(x, |set|)], x the first word of Philox(seed, b, ST_ABUND_BC, p); false: a letter outside IUPAC
bool barcodes_from_pattern(const std::string& pattern, uint32_t count, uint64_t seed, std::vector<std::string>& out);
// barcode b of a whitelist: list[umulhi32(x, |list|)], x the first word of Philox(seed, b, ST_ABUND_BC_TXT, 0) (with replacement)
void barcodes_from_whitelist(const std::vector<std::string>& list, uint32_t count, uint64_t seed, std::vector<std::string>& out);
// generate_rid_to_bc (:305-323): weight b = exp(mu + sigma z), z = Box-Muller of the first two words of Philox(seed, b, ST_ABUND_WEIGHT, 0);
// the dropout entry (index count) has sum(w) d / (1 - d).  cdf[k] = w[0] + ... + w[k], left to right; dropout 1: every weight 0 but the last
void cell_cdf(uint32_t count, uint64_t seed, double mu, double sigma, double dropout, std::vector<double>& cdf);

// the writer of main() (:367-389): header, then per row "name\t%.3f\tcell" of tpm = a * 1e6, skipping tpm < 0.001 and what prints as 0.000;
// gzipped when the path ends in .gz.  Written under <path>.tmp and renamed.
struct AbundRow { uint32_t tid, cell; double a; };
bool abundance_tsv(const std::vector<AbundRow>& rows, const std::vector<std::string>& tnames, const std::vector<std::string>& cells, std::string& out);
bool write_abundance_file(const std::string& path, const std::string& text, std::string& err);

}  // namespace tkh
