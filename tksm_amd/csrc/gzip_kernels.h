// gzip_kernels.h -- launchers of the device-side BGZF encoder (gzip_kernels.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gzip_core.h"

namespace tkgz {

// what the plan kernel leaves for the encode kernel, per chunk
struct ChunkPlan {
    uint32_t dynamic;                     // 1: dynamic blocks per run of lines of a class, 0: one stored block
    uint32_t crc;                         // CRC-32 of the chunk
    uint32_t hdr_bits[NCLS];              // bits of a class's block header, 0: the class does not occur
    uint32_t payload_bytes;               // deflate bytes of the member
    uint32_t reserved[2];
    uint32_t hdr[NCLS][HDR_WORDS];
    uint32_t code[NCLS][NSYM];            // length << 16 | code, first bit lowest
};

// the GF(2) operators that move a CRC register past 255 x 2^k zero bytes (k = 0..7), and the CRC-32 of a full and of the last
// chunk's worth of zero bytes: computed on the host, like zlib's crc32_combine
struct CrcOps {
    uint32_t shift[8][32];
    uint32_t zeros_full, zeros_last;
};
void make_crc_ops(CrcOps& ops, uint32_t last_chunk_bytes);

inline uint64_t n_chunks(uint64_t bytes) { return (bytes + CHUNK - 1) / CHUNK; }

// newlines per chunk (u64[n_chunks]), for the line phase of every chunk's first byte
hipError_t launch_count(const uint8_t* src, uint64_t bytes, uint64_t* counts, hipStream_t s);
// per chunk: tokens, histograms, codes, exact member size (u64 sizes[n_chunks]), CRC-32.  nl_before: exclusive scan of the
// counts (ignored for FMT_RAW, may be null then)
hipError_t launch_plan(const uint8_t* src, uint64_t bytes, int fmt, const uint64_t* nl_before, const CrcOps& ops, ChunkPlan* plans,
                       uint64_t* sizes, hipStream_t s);
// writes every member at its final offset (exclusive scan of the sizes) into out, which must be zeroed and hold out_words
// 32-bit words, at least the total rounded up
hipError_t launch_encode(const uint8_t* src, uint64_t bytes, int fmt, const uint64_t* nl_before, const ChunkPlan* plans,
                         const uint64_t* member_off, uint32_t* out, uint64_t out_words, hipStream_t s);

}  // namespace tkgz
