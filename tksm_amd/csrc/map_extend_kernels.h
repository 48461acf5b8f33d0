// map_extend_kernels.h -- device side of map --extend (include/tksmseq.h, "map, end extension"): the banded X-drop extension of both ends of
// every written chain, one wave per (line, end), lane (i - j + B) >> 1 owning cell (i, j) of anti-diagonal i + j.  The first pass keeps no
// store and finds the best cell; with alignment a second pass computes the anti-diagonals up to that cell again, keeps two traceback bits
// per cell and walks them back.  Integers only: there is no floating point in this file.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "map_align_kernels.h"

namespace tk {

using MapExtTask = tkh::MapExtTask;                // one end of one line
using MapExtEnd = tkh::MapExtEnd;                  // what the first pass found for it
// error bits of the flag word (all of them "cannot happen": the host reports TKSMSEQ_EDEVICE)
constexpr uint32_t MAP_EXT_E_CORNER = 1u, MAP_EXT_E_STORE = 2u, MAP_EXT_E_TRACE = 4u;

struct MapExtParams { uint32_t band, drop, max_ext, eqx; };

// ends[e] of every task: the best cell (ei, ej), the matches m on the way to it, the anti-diagonals and allowed cells computed
hipError_t launch_map_extend(const MapExtTask* tasks, uint32_t n_tasks, const MapChain* chain, const MapAlnSeqs& Q, const MapExtParams& P, uint32_t n_waves, MapExtEnd* ends,
                             uint32_t* flags, hipStream_t s);
// the tasks whose end moved, with (ei, ej) of the first pass and cap = ei + ej: wave v owns tb[v * tb_stride .. ) 16-byte units,
// tb_stride > the largest cap.  cols: two bits a column (0 =, 1 X, 2 I, 3 D), 16 a word, in target order: a left end's columns fill its
// words from index 0 up, a right end's from index cap - 1 down.  out[e]: the columns by kind and the runs of their CIGAR (cells = 0)
hipError_t launch_map_extend_trace(const MapExtTask* tasks, uint32_t n_tasks, const MapChain* chain, const MapAlnSeqs& Q, const MapExtParams& P, uint32_t n_waves,
                                   uint32_t tb_stride, uint64_t* tb, uint32_t* cols, MapAlnOut* out, uint32_t* flags, hipStream_t s);

}  // namespace tk
