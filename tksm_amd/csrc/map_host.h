// map_host.h -- host side of map (include/tksmseq.h): the parameter checks, the packer of the reads and the tiles of the sketch, and the PAF
// line.  No device code: tools/sanitize_map_host.cpp runs these under ASan / UBSan.
#pragma once
#include <stdint.h>

#include <string>
#include <vector>

#include "../../include/tksmseq.h"
#include "ms_host.h"

namespace tkh {

constexpr uint32_t MAP_TILE_WINDOWS = 192;         // windows per workgroup of the sketch (tk::MAP_TILE)

// the tables the host shares with the kernels (described in map_kernels.h)
struct MapSeq { uint64_t voff; uint32_t len, pad; };
struct MapTile { uint32_t seq, j0; };
struct MapChain { uint32_t read, tr, score, cnt, nmatch, tstart, tend, qs, qe, kept; };

// the ranges of include/tksmseq.h; false: err says which parameter
bool map_check_params(const tksmseq_map_params& p, std::string& err);
// P = 1000 secondary_ratio, rounded half up
uint32_t map_permille(double secondary_ratio);

// the windows of a sequence of `len` letters: 0 when it has no k-mer, else max(0, n - w) + 1 with n = len - k + 1
inline uint64_t map_windows(uint64_t len, uint32_t k, uint32_t w) { return len < k ? 0 : (len - k + 1 > w ? len - k + 1 - w : 0) + 1; }
// appends the tiles of sequence `seq`
void map_add_tiles(uint32_t seq, uint64_t len, uint32_t k, uint32_t w, std::vector<MapTile>& tiles);

// reads [r0, r1) packed like the reference: every read starts a validity word (32 letters) and two code words; a letter outside ACGT has
// code 0 and a clear validity bit.  seqs[r - r0] = {first validity word, length}
void map_pack_reads(const MsReads& reads, uint32_t r0, uint32_t r1, std::vector<uint32_t>& codes, std::vector<uint32_t>& valid, std::vector<MapSeq>& seqs);

// one line of the PAF for a chain of read `qname` (qlen letters) on target `tname` (tlen letters)
void map_paf_line(const std::string& qname, uint32_t qlen, const std::string& tname, uint64_t tlen, const MapChain& c, uint32_t mapq, bool primary, std::string& out);

}  // namespace tkh
