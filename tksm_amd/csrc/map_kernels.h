// map_kernels.h -- device side of map (include/tksmseq.h): the minimizer sketch of packed sequences (one lane per k-mer position, the window
// minimum over an LDS tile with its halo), the seeds of the read minimizers in the sorted index (one lane per read minimizer), the chain of
// every (read, target, strand) group (one wave per group, the 64 predecessors in registers) and the choice of the lines of a read (one lane
// per read).  Integers only: there is no floating point in this file.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"
#include "map_host.h"

namespace tk {

constexpr uint32_t MAP_TILE = 192;                 // windows per workgroup of the sketch: 1 + MAP_TILE + 63 positions fill its 256 lanes
constexpr uint32_t MAP_NO_PRED = 0xFFFFFFFFu;
constexpr int MAP_PRED_WINDOW = 64;                // predecessors a chain step looks at: the wave width

// a sequence in the packed arrays: validity words (32 bases a word, bit g & 31) from voff, code words (16 bases a word, base g in bits
// 2 (g & 15)) from 2 voff.  The reference has this shape already (a contig starts on a 4096-base block); the reads are packed to it.
using MapSeq = tkh::MapSeq;                        // { voff, len }
using MapTile = tkh::MapTile;                      // windows [j0, j0 + MAP_TILE) of sequence seq
static_assert(MAP_TILE == tkh::MAP_TILE_WINDOWS, "the host cuts the tiles");
struct MapSketch {
    const uint32_t *codes, *valid;
    const MapSeq* seqs;
    const MapTile* tiles;
    uint32_t n_tiles, k, w;
};
struct MapChainParams { uint32_t k, max_gap, bandwidth, min_count, min_score; };
// one chain: tr = target << 1 | rel; the query interval in the strand of the chain (qs, qe of include/tksmseq.h)
using MapChain = tkh::MapChain;

// valid[w] for the n_words validity words of the reference: all ones in a pure 2-bit block, else one bit per pool byte in ACGT
hipError_t launch_map_ref_valid(const RefView& R, uint64_t n_words, uint32_t* valid, hipStream_t s);
// the minimizers of every tile: counts[tile] (scanned by the caller), then at off[tile] in window order: hash, seq, pos << 1 | strand
hipError_t launch_map_sketch_count(const MapSketch& S, uint64_t* counts, hipStream_t s);
hipError_t launch_map_sketch_write(const MapSketch& S, const uint64_t* off, uint64_t* hash, uint32_t* seq, uint32_t* ps, hipStream_t s);
// dropped[0] = the distinct hashes with more than max_occ entries
hipError_t launch_map_dropped(const uint64_t* dcount, uint32_t n_distinct, uint64_t max_occ, unsigned long long* dropped, hipStream_t s);
// per read minimizer: run[i] = its hash's place among the distinct hashes, cnt[i] = that hash's entries (0: unknown, or over max_occ)
hipError_t launch_map_seed_count(const uint64_t* rm_hash, uint32_t n_rm, const uint64_t* dkey, const uint64_t* dcount, uint32_t n_distinct, uint64_t max_occ,
                                 uint32_t* run, uint64_t* cnt, hipStream_t s);
// the anchors at off[i]: k1 = p << 31 | qa, k2 = read << 32 | target << 1 | rel (idx_seq / idx_ps: the index in sorted order, dstart its runs)
hipError_t launch_map_seed_write(const uint32_t* rm_read, const uint32_t* rm_ps, const uint32_t* run, const uint64_t* cnt, const uint64_t* off, uint32_t n_rm,
                                 const uint32_t* dstart, const uint32_t* idx_seq, const uint32_t* idx_ps, const MapSeq* reads, uint32_t k, uint64_t* k1, uint64_t* k2,
                                 hipStream_t s);
// flag[g] = group g has at least min_count anchors (scanned by the caller); then list[rank] = g
hipError_t launch_map_group_flags(const uint32_t* gstart, uint32_t n_groups, uint32_t min_count, uint64_t* flag, hipStream_t s);
hipError_t launch_map_group_list(const uint64_t* flag, const uint64_t* scanned, uint32_t n_groups, uint32_t* list, hipStream_t s);
// chain[c] for group list[c]: anchors [gstart[g], gstart[g + 1]) of k1 / k2 in (p, qa) order; pred: one word per anchor (work space)
hipError_t launch_map_chain(const uint64_t* k1, const uint64_t* k2, const uint32_t* gstart, const uint32_t* list, uint32_t n_list, const MapChainParams& P,
                            uint32_t* pred, MapChain* chain, hipStream_t s);
// key[c] = read << 32 | (2^32 - 1 - score) for a kept chain, all ones otherwise
hipError_t launch_map_chain_keys(const MapChain* chain, uint32_t n, uint64_t* key, hipStream_t s);
// one lane per read over its kept chains in sorted order (perm: into chain): n_lines[r], mapq[r], lines[r * (max_secondary + 1) + i]
hipError_t launch_map_select(const uint64_t* key_sorted, const uint32_t* perm, uint32_t n_chains, uint32_t n_reads, uint32_t permille, uint32_t max_secondary,
                             uint32_t* n_lines, uint32_t* mapq, uint32_t* lines, hipStream_t s);

}  // namespace tk
