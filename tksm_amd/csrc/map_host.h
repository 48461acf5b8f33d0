// map_host.h -- host side of map (include/tksmseq.h): the parameter checks, the packer of the reads and the tiles of the sketch, and the PAF
// line.  No device code: tools/sanitize_map_host.cpp runs these under ASan / UBSan.
#pragma once
#include <stdint.h>

#include <string>
#include <utility>
#include <vector>

#include "../../include/tksmseq.h"
#include "ms_host.h"
#include "tsb_host.h"

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
// (sn >= 2: the sn:i: and si:i: tags of "map, split reads" follow s1:i:)
void map_paf_line(const std::string& qname, uint32_t qlen, const std::string& tname, uint64_t tlen, const MapChain& c, uint32_t mapq, bool primary, std::string& out,
                  uint32_t sn = 0, uint32_t si = 0);

// ---- map -c ("map, alignment" in include/tksmseq.h; the kernels are described in map_align_kernels.h)
constexpr int32_t MAP_ALN_MAX_GAP = 65536;         // a segment's traceback store is sized by dt + dq
constexpr uint32_t MAP_ALN_TB_BYTES = 16;          // traceback bytes per anti-diagonal
constexpr uint32_t MAP_ALN_WAVES = 8192;           // waves of the alignment at the most: eight on each of 1 024 SIMDs
constexpr uint64_t MAP_ALN_BYTES_MAX = 128ull << 20;   // device bytes the alignment of one chunk may take at the most
// a line before the alignment: its chain, where its anchors go, where its columns go (words, 16 columns a word) and how many it has room for
struct MapAlnLine { uint32_t chain, seg_off, col_off, cap; };
// ... and after: its columns by kind, the runs of its CIGAR, the allowed cells computed
struct MapAlnOut { uint32_t ncols, eq, x, ins, del, runs; uint64_t cells; };

// band in [1, 63]; with alignment max_gap is at most MAP_ALN_MAX_GAP; false: err says which
bool map_check_align(const tksmseq_map_params& p, const tksmseq_align_params& a, std::string& err);
// appends the line of chain c: where its anchors and columns go in a chunk that holds `segments` anchors and `col_words` words so far
inline void map_align_add_line(uint32_t chain, const MapChain& c, uint64_t& segments, uint64_t& col_words, std::vector<MapAlnLine>& lines) {
    const uint32_t cap = (c.tend - c.tstart) + (c.qe - c.qs);
    lines.push_back({chain, (uint32_t)segments, (uint32_t)col_words, cap});
    segments += c.cnt;
    col_words += ((uint64_t)cap + 15) / 16;
}
// device bytes of a chunk's alignment without the traceback stores: lines, results, anchors, columns, run offsets and the runs (at most
// a run a column is what the first sizing assumes; the exact count is known before the runs are written)
uint64_t map_align_fixed_bytes(uint64_t lines, uint64_t segments, uint64_t col_words, uint64_t runs);
// the waves that fit beside `fixed` bytes when a segment spans up to `longest` anti-diagonals: at most min(lines, MAP_ALN_WAVES), in whole
// workgroups of four; 0: not even one workgroup fits in `budget`
uint32_t map_align_waves(uint64_t budget, uint64_t fixed, uint64_t lines, uint32_t longest);
// the aligned form of map_paf_line: columns 10 and 11 from the columns, NM:i: and cg:Z: appended.  runs[r] = first column << 2 | op.
void map_paf_line_aligned(const std::string& qname, uint32_t qlen, const std::string& tname, uint64_t tlen, const MapChain& c, uint32_t mapq, bool primary,
                          const MapAlnOut& a, const uint64_t* runs, bool eqx, std::string& out, uint32_t sn = 0, uint32_t si = 0);

// ---- map --extend ("map, end extension" in include/tksmseq.h; the kernels are described in map_extend_kernels.h)
// one end of a line (end 0: left, 1: right).  The second pass also reads where its columns go (words), the best cell and cap = ei + ej
struct MapExtTask { uint32_t chain, end, col_off, cap, ei, ej; };
// what the first pass found: the best cell, the matches on the way to it, the anti-diagonals and the allowed cells computed
struct MapExtEnd { uint32_t ei, ej, m, steps; uint64_t cells; };

// band in [1, 63], drop in [1, 1000], max_ext in [1, 32768]; false: err says which
bool map_check_extend(const tksmseq_extend_params& e, std::string& err);
// device bytes of a chunk's extension without the traceback stores: the tasks and ends of the first pass; of the second the tasks, their
// results, their lines and run offsets for the encoder, their columns and their runs
uint64_t map_extend_fixed_bytes(uint64_t tasks, uint64_t traced, uint64_t col_words, uint64_t runs);
// the chain with both corners moved
inline MapChain map_extended_chain(MapChain c, const MapExtEnd& left, const MapExtEnd& right) {
    c.tstart -= left.ei; c.qs -= left.ej; c.tend += right.ei; c.qe += right.ej;
    return c;
}
// the columns of a line with extension: the left end's (or NULL), the chain's, the right end's (or NULL), each with its runs.  The runs of
// the parts are joined where two parts meet in the same op; `runs` gets first column << 2 | op of the whole line
MapAlnOut map_join_columns(const MapAlnOut* left, const uint64_t* left_runs, const MapAlnOut& mid, const uint64_t* mid_runs, const MapAlnOut* right,
                           const uint64_t* right_runs, std::vector<uint64_t>& runs);

// ---- map --split ("map, split reads" in include/tksmseq.h; the kernels are described in map_split_kernels.h)
// chains in [1, 16], overlap in [0, 2^31), segments in [2, 64]; false: err says which
bool map_check_split(const tksmseq_split_params& s, std::string& err);
// device bytes an anchor takes more with split: its word of the list, and its share of the further chains of its group (a chained group has
// at least min_count anchors) through the key sort and the selection
uint64_t map_split_anchor_bytes(const tksmseq_split_params& s, int32_t min_count);
// rank[i] = the 0-based rank of tp:A:P line i of a read by (qstart, qend, i); iv[i] = {qstart, qend} in original read coordinates
void map_split_ranks(const std::vector<std::pair<uint32_t, uint32_t>>& iv, std::vector<uint32_t>& rank);

// ---- map -g ("map, annotated targets" in include/tksmseq.h; the kernel is described in map_targets_kernels.h)
// an exon as the splice kernel reads it: g = its first letter in the genome's global coordinate, cum = the letters of its target before it,
// len_minus = its letters | strand << 31.  Empty exons are not in the list: every tuple has at least one letter
struct MapTargetExon { uint64_t g; uint32_t cum, len_minus; };
// the kept transcripts of a table: target t is transcript tx[t], len[t] letters from validity word voff[t], exons [efirst[t], efirst[t + 1])
// of `exons` (the device tuples) and of ex_start / ex_end (their genomic intervals, for the projection); contig[t], minus[t]: of a
// projectable target
struct MapTargets {
    tksmseq_targets_info info{};
    std::vector<uint32_t> tx, len, contig;
    std::vector<uint64_t> voff{0}, efirst{0};
    std::vector<MapTargetExon> exons;
    std::vector<uint32_t> ex_start, ex_end;
    std::vector<uint8_t> minus, projectable;
    size_t n() const { return tx.size(); }
};
// the walk over the table in table order ("Which transcripts become targets").  contig_of[i]: the reference's contig for the table's contig
// name i, or -1 (unknown, or declared only); contigs: the reference's {gstart, len} pairs.  TKSMSEQ_OK, or TKSMSEQ_ELIMIT / TKSMSEQ_EINVAL
// with err
int map_targets_select(const tsb::Transcripts& T, const std::vector<int32_t>& contig_of, const std::vector<uint64_t>& contigs, MapTargets& out, std::string& err);
// the FASTA of the downloaded image: ">name\n", the letters (N where the validity bit is clear) wrapped at line_width (0: one line)
void map_targets_fasta(const MapTargets& T, const std::vector<std::string>& names, const uint32_t* codes, const uint32_t* valid, int32_t line_width, std::string& out);

// ---- map --genome-coords: the projection of a written line ("map, annotated targets": "Projection")
// line: one PAF line of target t without its '\n'; T.projectable[t].  Replaces columns 5 to 9 and the cg:Z: tag and appends tx:Z:;
// returns the N runs written, or without a cg:Z: tag the exon boundaries [tstart, tend) crosses
uint64_t map_project_line(std::string& line, const MapTargets& T, uint32_t t, const std::string& tx_name, const std::string& contig_name, uint64_t contig_len);

}  // namespace tkh
