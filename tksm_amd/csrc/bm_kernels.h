// bm_kernels.h -- device side of barcode-match (include/tksmseq.h): the adapter's infix alignment in both orientations of every read (one
// lane per read and orientation), the exact counts of the whitelist barcodes over the segments' windows (one lane per segment), the
// candidate list in whitelist order, and the match of every segment against every candidate (one lane per segment, the candidate
// wave-uniform) with its merge over the candidate splits.  Integers only: there is no floating point in this file.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace tk {

constexpr int BM_SEG_MAX = 64;                     // letters of a segment: L + 2 pad at most
constexpr int BM_LIST = 8;                         // candidates listed per read
constexpr uint32_t BM_CAND_TILE = 256;             // the candidates of one workgroup of the match are a multiple of this (mirrored in _lib.py)
constexpr uint32_t BM_TARGET_WAVES = 2048;         // the match splits the candidates until it has about this many waves

// what the adapter pass leaves per read: the segment, 2 bits per letter (A C G T = 0..3; letter j in bits 2 (j & 15) of code[j >> 4]) with
// one validity bit per letter (a byte outside ACGT: code 0, bit clear)
struct BmSeg {
    uint32_t code[4];
    uint32_t valid[2];
    uint32_t meta;          // length | orientation << 7 | has adapter << 8 | da << 16
    uint32_t start;         // the segment's first letter in the oriented read
};
constexpr uint32_t BM_META_LEN = 0x7F, BM_META_REV = 1u << 7, BM_META_ADAPTER = 1u << 8;

// the two ends of the reads of a chunk, transposed: lane = 2 * read + orientation of n2 = 2 * reads lanes; letter j of the oriented read
// in bits 2 (j & 15) of codes[(j >> 4) * n2 + lane], its validity in bit j & 31 of valid[(j >> 5) * n2 + lane]; len[read] =
// min(length, letters uploaded)
struct BmEnds {
    const uint32_t *codes, *valid, *len;
    uint32_t n_reads;
};
struct BmAdapter {
    uint32_t peq[4];        // bit i of peq[c]: adapter letter i is c
    uint32_t m;             // adapter length
    uint32_t window, max_errors, pad, L;
};

// seg[read] for every read of the chunk (a read without adapter: meta = 0)
hipError_t launch_bm_adapter(const BmEnds& E, const BmAdapter& A, BmSeg* seg, hipStream_t s);
// exact[perm[k]] += 1 for every all-ACGT window of L letters of every segment that spells keys_sorted[k] (letter i in bits 2i of the key)
hipError_t launch_bm_exact(const BmSeg* seg, uint32_t n_reads, const uint64_t* keys_sorted, const uint32_t* perm, uint32_t n_keys, uint32_t L,
                           unsigned long long* exact, hipStream_t s);
// flag[b] = exact[b] >= min_exact (scanned by the caller); then cand[rank] = b and cand_peq[rank] = the four match masks of keys[b]
hipError_t launch_bm_cand_flags(const unsigned long long* exact, uint32_t n_keys, uint64_t min_exact, uint64_t* flag, hipStream_t s);
hipError_t launch_bm_cand_write(const uint64_t* keys, const uint64_t* flag, const uint64_t* scanned, uint32_t n_keys, uint32_t L, uint32_t* cand, uint4* cand_peq,
                                hipStream_t s);
// the candidates per workgroup row of the match for this many reads and candidates: a multiple of BM_CAND_TILE
uint32_t bm_split_size(uint32_t n_reads, uint32_t n_cand);
// split y takes candidates [y * per_split, (y + 1) * per_split): part_d[y * n_reads + r] = its minimal distance, or max_errors + 1 when none
// is at most max_errors; part_n likewise the number of its candidates at that distance; part_idx[(y * n_reads + r) * BM_LIST + k] the
// first of them (candidate ranks).  Entries of part_idx from min(part_n, BM_LIST) on are not written.
hipError_t launch_bm_match(const BmSeg* seg, uint32_t n_reads, const uint4* cand_peq, uint32_t n_cand, uint32_t per_split, uint32_t L, uint32_t max_errors,
                           uint32_t* part_d, uint32_t* part_n, uint32_t* part_idx, hipStream_t s);
// the splits of a read in whitelist order: res_d, res_n, res_idx[r * BM_LIST + k] (all BM_LIST written: 0xFFFFFFFF behind the list)
hipError_t launch_bm_merge(const uint32_t* part_d, const uint32_t* part_n, const uint32_t* part_idx, uint32_t n_reads, uint32_t n_splits, uint32_t max_errors,
                           uint32_t* res_d, uint32_t* res_n, uint32_t* res_idx, hipStream_t s);

}  // namespace tk
