// map_targets_kernels.hip -- device side of map -g (see map_targets_kernels.h; the rules are stated in include/tksmseq.h).
#include "map_targets_kernels.h"

namespace tk {

namespace {

#define DEV __device__ __forceinline__

// every bit of v doubled: bit i of v in bits 2 i and 2 i + 1
DEV uint64_t spread_pairs(uint32_t v) {
    uint64_t x = v;
    x = (x | x << 16) & 0x0000FFFF0000FFFFull;
    x = (x | x << 8) & 0x00FF00FF00FF00FFull;
    x = (x | x << 4) & 0x0F0F0F0F0F0F0F0Full;
    x = (x | x << 2) & 0x3333333333333333ull;
    x = (x | x << 1) & 0x5555555555555555ull;
    return x | x << 1;
}

// letters [p, p + take) of the genome, 1 <= take <= 32 (all inside one contig: the words read hold a letter of the range each): letter i
// in bits 2 i of c and in bit i of v, nothing above them.  A funnel shift over two or three code words and one or two validity words
DEV void genome_letters(const uint32_t* __restrict__ packed, const uint32_t* __restrict__ gvalid, uint64_t p, uint32_t take, uint64_t& c, uint32_t& v) {
    const uint64_t last = p + take - 1u, cw = p >> 4, vw = p >> 5;
    const uint32_t nc = (uint32_t)((last >> 4) - cw);                         // further code words: 0, 1 or 2
    const uint64_t w0 = packed[cw], w1 = nc >= 1u ? packed[cw + 1] : 0u, w2 = nc >= 2u ? packed[cw + 2] : 0u;
    const uint32_t sh = 2u * (uint32_t)(p & 15u);
    uint64_t x = (w0 | w1 << 32) >> sh;
    if (sh) x |= w2 << (64u - sh);
    const uint64_t v0 = gvalid[vw], v1 = (last >> 5) > vw ? gvalid[vw + 1] : 0u;
    const uint32_t y = (uint32_t)((v0 | v1 << 32) >> (uint32_t)(p & 31u));
    c = take == 32u ? x : x & ((1ull << (2u * take)) - 1ull);
    v = take == 32u ? y : y & ((1u << take) - 1u);
}

}  // namespace

// One lane per validity word of the image.  The lane finds its target (the last one that starts at or before its word), its first exon
// (the last one of the target that starts at or before its first letter) and walks the exons until its letters are filled: a word holds up
// to 32 exons of one letter.  A `-` exon gives the letters of the mirrored range: all 64 bits reversed, the two bits of a letter swapped
// back, complemented; the validity bits reversed.  Whole words are stored, the lanes of a wave to neighbouring words.
__global__ void __launch_bounds__(256) k_map_splice_targets(MapSplice S, uint32_t* __restrict__ codes, uint32_t* __restrict__ valid) {
    const uint64_t w = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (w >= S.n_vwords) return;
    uint32_t lo = 0, hi = S.n_targets - 1u;                                   // voff[lo] <= w: voff[0] = 0
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo + 1u) / 2u;
        if (S.seqs[mid].voff <= w) lo = mid; else hi = mid - 1u;
    }
    const MapSeq q = S.seqs[lo];
    const uint32_t x0 = (uint32_t)(w - q.voff) << 5;                          // the word's first letter: below len, every target fills its words
    const uint32_t n = min(32u, q.len - x0);
    const uint64_t e_end = S.efirst[lo + 1];
    uint64_t a = S.efirst[lo], b = e_end - 1u;                                // cum[a] <= x0: cum of a target's first exon is 0
    while (a < b) {
        const uint64_t mid = a + (b - a + 1u) / 2u;
        if (S.exons[mid].cum <= x0) a = mid; else b = mid - 1u;
    }
    uint64_t c = 0;
    uint32_t v = 0;
    for (uint32_t filled = 0; filled < n && a < e_end; a++) {
        const MapTargetExon e = S.exons[a];
        const uint32_t len = e.len_minus & 0x7FFFFFFFu, o = x0 + filled - e.cum;
        if (o >= len) break;                                                  // (tables that do not add up: the host builds none)
        const uint32_t take = min(n - filled, len - o);
        uint64_t ec;
        uint32_t ev;
        if (e.len_minus >> 31) {
            genome_letters(S.packed, S.gvalid, e.g + (len - o - take), take, ec, ev);
            uint64_t r = __brevll(ec);
            r = ((r >> 1) & 0x5555555555555555ull) | ((r & 0x5555555555555555ull) << 1);
            r >>= 64u - 2u * take;
            ec = take == 32u ? ~r : ~r & ((1ull << (2u * take)) - 1ull);
            ev = __brev(ev) >> (32u - take);
        } else {
            genome_letters(S.packed, S.gvalid, e.g + o, take, ec, ev);
        }
        c |= ec << (2u * filled);
        v |= ev << filled;
        filled += take;
    }
    c &= spread_pairs(v);
    reinterpret_cast<uint2*>(codes)[w] = make_uint2((uint32_t)c, (uint32_t)(c >> 32));
    valid[w] = v;
}

hipError_t launch_map_splice_targets(const MapSplice& S, uint32_t* codes, uint32_t* valid, hipStream_t s) {
    if (!S.n_vwords || !S.n_targets) return hipSuccess;
    hipLaunchKernelGGL(k_map_splice_targets, dim3((unsigned)((S.n_vwords + 255u) / 256u)), dim3(256), 0, s, S, codes, valid);
    return hipGetLastError();
}

}  // namespace tk
