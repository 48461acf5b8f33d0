// bm_host.h -- host side of barcode-match (include/tksmseq.h): the whitelist reader with its 64-bit keys, the packer of the reads' two ends
// and the text of a segment.  No device code.
#pragma once
#include <stdint.h>

#include <string>
#include <vector>

#include "ms_host.h"

namespace tkh {

// A C G T -> 0..3, anything else 4
inline uint32_t bm_code(uint8_t c) { return c == 'A' ? 0u : c == 'C' ? 1u : c == 'G' ? 2u : c == 'T' ? 3u : 4u; }
// the complement of an upper-case letter; a byte outside ACGT is its own
inline uint8_t bm_complement(uint8_t c) { return c == 'A' ? 'T' : c == 'C' ? 'G' : c == 'G' ? 'C' : c == 'T' ? 'A' : c; }
// lo to hi letters, all of ACGT
bool bm_is_acgt(const std::string& s, size_t lo, size_t hi);

// the whitelist: text[b] the file's spelling, keys[b] the MATCHED spelling (its reverse complement with revcomp), letter i in bits 2i
struct BmWhitelist {
    std::vector<std::string> text;
    std::vector<uint64_t> keys;
    uint32_t L = 0;
};
// one barcode per line, empty lines skipped.  false: err = "whitelist line N: ..." (a length outside [4, 32], a length other than the
// first barcode's, a letter outside ACGT, the spelling of an earlier line), "the whitelist is empty", or (*limit set) 2^27 lines or more
bool parse_bm_whitelist(const char* text, size_t len, bool revcomp, BmWhitelist& out, std::string& err, bool* limit);

// the first `letters` letters of both orientations of reads [r0, r1), in the transposed layout of tk::BmEnds
void bm_pack_ends(const MsReads& reads, uint32_t r0, uint32_t r1, uint32_t letters, std::vector<uint32_t>& codes, std::vector<uint32_t>& valid,
                  std::vector<uint32_t>& len);
// letters [start, start + n) of read r, or of its reverse complement
void bm_oriented_slice(const MsReads& reads, uint32_t r, bool reverse, uint32_t start, uint32_t n, std::string& out);

}  // namespace tkh
