// map_split_kernels.h -- device side of map --split ("map, split reads" in include/tksmseq.h): the chain of a group in several rounds over a
// shrinking list of its anchors (one wave per group, all rounds in that wave, the 64 predecessors in registers as in map_kernels.h) and the
// choice of a read's lines with the supplementary ones (one lane per read, the accepted chains in LDS).  Integers only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "map_kernels.h"

namespace tk {

constexpr uint32_t MAP_SPLIT_CHAINS_MAX = 16;      // rounds of a group at the most
constexpr uint32_t MAP_SPLIT_SEGMENTS_MAX = 64;    // tp:A:P lines of a read at the most
struct MapSplitSelect { uint32_t permille, max_secondary, rounds, overlap, segments; };

// chain[c * rounds + r] for round r of group list[c]; kept = 0 and cnt = 0 for a round that did not run.  rem: one word per anchor (the
// remaining original indices of the group, work space), pred: one word per anchor, original group-relative indices
hipError_t launch_map_chain_split(const uint64_t* k1, const uint64_t* k2, const uint32_t* gstart, const uint32_t* list, uint32_t n_list, const MapChainParams& P,
                                  uint32_t rounds, uint32_t* rem, uint32_t* pred, MapChain* chain, hipStream_t s);
// listx[i] = list[i / rounds]: the group of chain i, for the kernels that look a chain's group up by the chain's index
hipError_t launch_map_split_list(const uint32_t* list, uint32_t n_list, uint32_t rounds, uint32_t* listx, hipStream_t s);
// one lane per read over its kept chains in sorted order (perm: into chain).  With slots = max_secondary + segments: n_lines[r] lines in
// lines[r * slots + i], the first n_first[r] of them the primary and its secondaries, the others supplementary in order of acceptance;
// line_mapq[r * slots + i]; rejected[r] = the candidates the overlap test refused
hipError_t launch_map_select_split(const uint64_t* key_sorted, const uint32_t* perm, const MapChain* chain, const MapSeq* reads, uint32_t n_chains, uint32_t n_reads,
                                   const MapSplitSelect& S, uint32_t* n_lines, uint32_t* n_first, uint32_t* line_mapq, uint32_t* lines, uint32_t* rejected, hipStream_t s);

}  // namespace tk
