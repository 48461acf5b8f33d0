// map_align_kernels.h -- device side of map -c (include/tksmseq.h, "map, alignment"): the anchors of every written chain from what the chain
// kernel left (one lane per line), the banded unit-cost alignment of the chain's segments with its traceback (one wave per line, lane
// i % 64 owning cell (i, s - i) of anti-diagonal s), and the run-length code of the columns (one wave per line).  Integers only: there is
// no floating point in this file.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "map_kernels.h"

namespace tk {

using MapAlnLine = tkh::MapAlnLine;                // what the host knows of a line before the alignment
using MapAlnOut = tkh::MapAlnOut;                  // what the alignment found
constexpr uint32_t MAP_ALN_TB_BYTES = tkh::MAP_ALN_TB_BYTES;   // traceback bytes per anti-diagonal: two bits for each of 64 lanes
// error bits of the flag word (all of them "cannot happen": the host reports TKSMSEQ_EDEVICE)
constexpr uint32_t MAP_ALN_E_END = 1u, MAP_ALN_E_PATH = 2u, MAP_ALN_E_SEGMENT = 4u, MAP_ALN_E_TRACE = 8u;

struct MapAlnSeqs {
    const uint32_t *tcodes, *tvalid;               // the targets: the packed reference and k_map_ref_valid's words
    const MapSeq* tseqs;
    const uint32_t *qcodes, *qvalid;               // the reads of the chunk
    const MapSeq* qseqs;
};

// path[seg_off .. seg_off + cnt) of every line = the keys (p << 31 | qa) of its chain's anchors in chain order; longest[0] = the largest
// dt + dq of a segment (at least 2 k); flags |= MAP_ALN_E_*
hipError_t launch_map_align_path(const MapAlnLine* lines, uint32_t n_lines, const MapChain* chain, const uint32_t* list, const uint32_t* gstart, const uint64_t* k1,
                                 const uint32_t* pred, uint32_t k, uint64_t* path, uint32_t* longest, uint32_t* flags, hipStream_t s);
// n_waves waves (a multiple of four) take the lines in turn; wave v owns tb[v * tb_stride .. ) 16-byte units, tb_stride > longest.
// cols: two bits a column (0 =, 1 X, 2 I, 3 D), 16 a word, line l's last column at index cap - 1 of its words from col_off
hipError_t launch_map_align(const MapAlnLine* lines, uint32_t n_lines, const MapChain* chain, const uint64_t* path, const MapAlnSeqs& Q, uint32_t k, uint32_t band,
                            uint32_t eqx, uint32_t n_waves, uint32_t tb_stride, uint64_t* tb, uint32_t* cols, MapAlnOut* out, uint32_t* flags,
                            hipStream_t s);
// runs[run_off[l] + r] = first column << 2 | op for run r of line l (op: 0 = or M, 1 X, 2 I, 3 D; without eqx = and X are one op)
hipError_t launch_map_align_encode(const MapAlnLine* lines, uint32_t n_lines, const MapAlnOut* out, const uint32_t* cols, const uint64_t* run_off, uint32_t eqx,
                                   uint64_t* runs, hipStream_t s);

}  // namespace tk
