// map_targets_kernels.h -- device side of map -g ("map, annotated targets" in include/tksmseq.h): the transcripts of the table spliced from
// the genome's packed image into the image the mapper reads (code words and validity words, map_kernels.h), one lane per validity word
// of the image.  Integers only: there is no floating point in this file.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "map_host.h"
#include "map_kernels.h"

namespace tk {

using MapTargetExon = tkh::MapTargetExon;          // { g, cum, len | minus << 31 }: at least one letter
struct MapSplice {
    const uint32_t *packed, *gvalid;               // the genome: 16 letters a code word, 32 a validity word, in its global coordinate
    const MapSeq* seqs;                            // [n_targets] { voff, len }
    const uint64_t* efirst;                        // [n_targets + 1] the exons of a target
    const MapTargetExon* exons;
    uint32_t n_targets;
    uint64_t n_vwords;                             // = voff[n_targets]
};

// codes[2 w], codes[2 w + 1] and valid[w] for every validity word w of the image: the letters of the exons in file order, a `-` exon
// reverse-complemented; an invalid letter has code 0, and every bit at or behind a target's length is 0
hipError_t launch_map_splice_targets(const MapSplice& S, uint32_t* codes, uint32_t* valid, hipStream_t s);

}  // namespace tk
