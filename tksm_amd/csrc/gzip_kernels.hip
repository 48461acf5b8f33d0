// gzip_kernels.hip -- BGZF (SAM specification 4.1) on the device: every 65 280 bytes of a record stream become one gzip member.
//
// One workgroup of 256 lanes owns a chunk, staged whole in LDS; lane t owns the strip of 255 bytes [255 t, 255 t + 255).
//   k_gz_count   newlines per chunk: with their exclusive scan, (newlines before a byte) mod 4 is the line of a FASTQ record the byte
//                is in (mod 2: FASTA) -- no record walk
//   k_gz_plan    tokens (literals and distance-1 matches over byte runs, gzip_core.h) -> a histogram per line class -> one
//                length-limited Huffman code per class -> the header bits of a class's dynamic block -> the EXACT size of the member;
//                a chunk that would not shrink is stored.  Also the chunk's CRC-32: a table-driven CRC per lane over strips
//                aligned to the chunk's END (zero bytes in front change nothing), merged pairwise by the shift operators of CrcOps.
//   k_gz_encode  after the scan of the sizes: per lane the bit length of its strip, a scan, and the bits go straight to the member's
//                final place -- whole 32-bit words by plain stores, the first and last word of a strip, which neighbours share, by
//                atomicOr into the zeroed buffer (an OR commutes: the bytes do not depend on the order of arrival).
// The deflate stream of a member: for every run of lines of one class a dynamic block (BFINAL = 0) that re-states the class's code,
// then an empty fixed-Huffman block with BFINAL = 1 (10 bits), so that no header bit depends on which block comes last.
#include "gzip_kernels.h"

namespace tkgz {
namespace {

constexpr uint32_t POLY = 0xEDB88320u;

// exclusive prefix sum over the workgroup (sh: 256 words); total: the sum
__device__ inline uint32_t block_excl_scan(uint32_t v, uint32_t* sh, uint32_t& total) {
    const uint32_t t = threadIdx.x;
    sh[t] = v;
    __syncthreads();
    for (uint32_t o = 1; o < STRIPS; o <<= 1) {
        const uint32_t y = t >= o ? sh[t - o] : 0u;
        __syncthreads();
        sh[t] += y;
        __syncthreads();
    }
    const uint32_t incl = sh[t];
    total = sh[STRIPS - 1];
    __syncthreads();
    return incl - v;
}

// the chunk into LDS: 16 bytes per lane and load where the source allows
__device__ inline void stage_chunk(uint8_t* d, const uint8_t* __restrict__ src, uint32_t n) {
    const uint32_t t = threadIdx.x;
    if ((reinterpret_cast<uintptr_t>(src) & 15u) == 0) {
        const uint32_t nv = n >> 4;
        for (uint32_t i = t; i < nv; i += STRIPS) reinterpret_cast<uint4*>(d)[i] = reinterpret_cast<const uint4*>(src)[i];
        for (uint32_t i = (nv << 4) + t; i < n; i += STRIPS) d[i] = src[i];
    } else {
        for (uint32_t i = t; i < n; i += STRIPS) d[i] = src[i];
    }
}

__device__ inline uint32_t newlines_in(const uint8_t* d, uint32_t b, uint32_t e) {
    uint32_t c = 0;
    for (uint32_t i = b; i < e; i++) c += d[i] == '\n';
    return c;
}

__global__ __launch_bounds__(256) void k_gz_count(const uint8_t* __restrict__ src, uint64_t bytes, uint64_t* __restrict__ counts) {
    __shared__ uint32_t sum;
    const uint64_t base = (uint64_t)blockIdx.x * CHUNK;
    const uint32_t n = (uint32_t)(bytes - base < CHUNK ? bytes - base : CHUNK);
    const uint8_t* p = src + base;
    const uint32_t t = threadIdx.x;
    if (t == 0) sum = 0;
    __syncthreads();
    uint32_t c = 0;
    if ((reinterpret_cast<uintptr_t>(p) & 15u) == 0) {
        const uint32_t nv = n >> 4;
        for (uint32_t i = t; i < nv; i += STRIPS) {
            const uint4 v = reinterpret_cast<const uint4*>(p)[i];
            const uint32_t w[4] = {v.x, v.y, v.z, v.w};
            for (int k = 0; k < 4; k++)
                for (int b = 0; b < 32; b += 8) c += ((w[k] >> b) & 0xffu) == '\n';
        }
        for (uint32_t i = (nv << 4) + t; i < n; i += STRIPS) c += p[i] == '\n';
    } else {
        for (uint32_t i = t; i < n; i += STRIPS) c += p[i] == '\n';
    }
    atomicAdd(&sum, c);
    __syncthreads();
    if (t == 0) counts[blockIdx.x] = sum;
}

__global__ __launch_bounds__(256) void k_gz_plan(const uint8_t* __restrict__ src, uint64_t bytes, int fmt, const uint64_t* __restrict__ nl_before,
                                                 CrcOps ops, ChunkPlan* __restrict__ plans, uint64_t* __restrict__ sizes) {
    __shared__ __align__(16) uint8_t d[CHUNK + 16];
    __shared__ uint32_t hist[NCLS][NSYM];
    __shared__ uint32_t sw[NCLS][NSYM];       // weights in ascending order, then the code lengths of that order, then the codes
    __shared__ uint16_t ss[NCLS][NSYM];       // the symbols in that order
    __shared__ uint8_t ll[NCLS][NSYM];
    __shared__ uint16_t rle[NCLS][320];
    __shared__ uint32_t hdr[NCLS][HDR_WORDS];
    __shared__ uint32_t hbits[NCLS];
    __shared__ uint32_t sh[STRIPS];
    __shared__ uint32_t crct[256];
    __shared__ uint32_t acc[4];               // [0] extra + distance bits, [1] code bits, [2] a header did not fit
    const uint32_t t = threadIdx.x;
    const uint64_t chunk = blockIdx.x;
    const uint64_t base = chunk * CHUNK;
    const uint32_t n = (uint32_t)(bytes - base < CHUNK ? bytes - base : CHUNK);
    stage_chunk(d, src + base, n);
    for (uint32_t i = t; i < NCLS * NSYM; i += STRIPS) { (&hist[0][0])[i] = 0; (&ll[0][0])[i] = 0; (&sw[0][0])[i] = 0; }
    for (uint32_t i = t; i < NCLS * HDR_WORDS; i += STRIPS) (&hdr[0][0])[i] = 0;
    if (t < 4) acc[t] = 0;
    {
        uint32_t c = t;
        for (int k = 0; k < 8; k++) c = (c & 1u) ? POLY ^ (c >> 1) : c >> 1;
        crct[t] = c;
    }
    __syncthreads();
    const uint32_t b = t * STRIP < n ? t * STRIP : n, e = b + STRIP < n ? b + STRIP : n;
    uint32_t nl = 0;
    if (fmt != FMT_RAW) {
        uint32_t total;
        nl = (uint32_t)(nl_before[chunk] & 3u) + block_excl_scan(newlines_in(d, b, e), sh, total);
    }
    // tokens -> histograms; a block begins wherever the class changes: one end-of-block symbol per block
    uint32_t extra = 0;
    walk_strip(d, b, e, fmt, nl, [&](uint32_t, uint32_t cls, uint32_t pcls, uint8_t c, uint32_t run) {
        if (cls != pcls) atomicAdd(&hist[cls][256], 1u);
        if (run) {
            uint32_t sym, eb, ev;
            length_symbol(run, sym, eb, ev);
            atomicAdd(&hist[cls][sym], 1u);
            extra += eb + 1u;
        } else atomicAdd(&hist[cls][c], 1u);
    });
    if (extra) atomicAdd(&acc[0], extra);
    // CRC-32: strips of the chunk as if zero bytes in front made it full
    {
        const uint32_t pad = CHUNK - n;
        uint32_t reg = 0;
        for (uint32_t j = 0; j < STRIP; j++) {
            const uint32_t q = t * STRIP + j;
            if (q >= pad) reg = crct[(reg ^ d[q - pad]) & 0xffu] ^ (reg >> 8);
        }
        sh[t] = reg;
    }
    __syncthreads();
    for (int k = 0; k < 8; k++) {
        const uint32_t stride = 1u << k;
        if ((t & (2u * stride - 1u)) == 0) {
            const uint32_t v = sh[t];
            uint32_t m = 0;
            for (int bit = 0; bit < 32; bit++) m ^= ((v >> bit) & 1u) ? ops.shift[k][bit] : 0u;
            sh[t] = m ^ sh[t + stride];
        }
        __syncthreads();
    }
    const uint32_t crc = sh[0] ^ (n == CHUNK ? ops.zeros_full : ops.zeros_last);
    // the used symbols of every class in ascending order of (weight, symbol): each finds its own rank
    for (uint32_t i = t; i < NCLS * 286u; i += STRIPS) {
        const uint32_t c = i / 286u, s = i % 286u, f = hist[c][s];
        if (!f) continue;
        uint32_t rank = 0;
        for (uint32_t s2 = 0; s2 < 286u; s2++) {
            const uint32_t f2 = hist[c][s2];
            rank += f2 && (f2 < f || (f2 == f && s2 < s));
        }
        sw[c][rank] = f;
        ss[c][rank] = (uint16_t)s;
    }
    __syncthreads();
    // one lane per class: code lengths (at most 15 bits), the block header, the codes
    if (t < NCLS) {
        int used = 0;
        for (int s = 0; s < 286; s++) used += hist[t][s] != 0;
        uint32_t hb = 0;
        if (used) {
            limited_lengths(sw[t], ss[t], used, 15, ll[t]);
            hb = block_header(ll[t], hdr[t], rle[t]);
            if (!hb) acc[2] = 1;
        }
        hbits[t] = hb;
        canonical_codes(ll[t], NSYM, sw[t]);
    }
    __syncthreads();
    {
        uint32_t bits = 0;
        for (uint32_t i = t; i < NCLS * NSYM; i += STRIPS) bits += (&hist[0][0])[i] * (&ll[0][0])[i];
        if (bits) atomicAdd(&acc[1], bits);
    }
    __syncthreads();
    ChunkPlan& plan = plans[chunk];
    if (t == 0) {
        uint32_t bits = acc[0] + acc[1] + FINAL_BITS;
        for (int c = 0; c < NCLS; c++) bits += hist[c][256] * hbits[c];
        uint32_t payload = (bits + 7u) >> 3;
        const bool dynamic = !acc[2] && payload < n + STORED_OVERHEAD;
        if (!dynamic) payload = n + STORED_OVERHEAD;
        plan.dynamic = dynamic;
        plan.crc = crc;
        for (int c = 0; c < NCLS; c++) plan.hdr_bits[c] = hbits[c];
        plan.payload_bytes = payload;
        plan.reserved[0] = plan.reserved[1] = 0;
        sizes[chunk] = MEMBER_OVERHEAD + payload;
    }
    for (uint32_t i = t; i < NCLS * HDR_WORDS; i += STRIPS) (&plan.hdr[0][0])[i] = (&hdr[0][0])[i];
    for (uint32_t i = t; i < NCLS * NSYM; i += STRIPS) (&plan.code[0][0])[i] = (&sw[0][0])[i];
}

// the bits of a strip on their way to the member: word `w` of the output buffer is the one being filled
struct Emitter {
    uint32_t* out; uint64_t cap_words, w; uint64_t acc; uint32_t na; bool first;
    __device__ Emitter(uint32_t* o, uint64_t cap, uint64_t bit) : out(o), cap_words(cap), w(bit >> 5), acc(0), na((uint32_t)(bit & 31u)), first(true) {}
    __device__ void put(uint32_t v, uint32_t n) {
        acc |= (uint64_t)v << na;
        na += n;
        if (na >= 32) {
            if (w < cap_words) { if (first) atomicOr(&out[w], (uint32_t)acc); else out[w] = (uint32_t)acc; }
            first = false;
            w++; acc >>= 32; na -= 32;
        }
    }
    __device__ void finish() { if (na && w < cap_words) atomicOr(&out[w], (uint32_t)acc); }
};

__device__ inline void or_byte(uint32_t* out, uint64_t cap_words, uint64_t pos, uint32_t v) {
    if ((pos >> 2) < cap_words) atomicOr(&out[pos >> 2], (v & 0xffu) << (8u * (uint32_t)(pos & 3u)));
}

__global__ __launch_bounds__(256) void k_gz_encode(const uint8_t* __restrict__ src, uint64_t bytes, int fmt, const uint64_t* __restrict__ nl_before,
                                                   const ChunkPlan* __restrict__ plans, const uint64_t* __restrict__ member_off,
                                                   uint32_t* __restrict__ out, uint64_t cap_words) {
    __shared__ __align__(16) uint8_t d[CHUNK + 16];
    __shared__ uint32_t code[NCLS][NSYM];
    __shared__ uint32_t hdr[NCLS][HDR_WORDS];
    __shared__ uint32_t hbits[NCLS];
    __shared__ uint32_t sh[STRIPS];
    const uint32_t t = threadIdx.x;
    const uint64_t chunk = blockIdx.x;
    const uint64_t base = chunk * CHUNK;
    const uint32_t n = (uint32_t)(bytes - base < CHUNK ? bytes - base : CHUNK);
    const ChunkPlan& plan = plans[chunk];
    const uint64_t off = member_off[chunk];
    const uint32_t payload = plan.payload_bytes;
    stage_chunk(d, src + base, n);
    for (uint32_t i = t; i < NCLS * NSYM; i += STRIPS) (&code[0][0])[i] = (&plan.code[0][0])[i];
    for (uint32_t i = t; i < NCLS * HDR_WORDS; i += STRIPS) (&hdr[0][0])[i] = (&plan.hdr[0][0])[i];
    if (t < NCLS) hbits[t] = plan.hdr_bits[t];
    if (t == 0) {
        // gzip header with the BGZF extra field (BSIZE = member size - 1), CRC-32 and ISIZE behind the deflate bytes
        const uint32_t bsize = MEMBER_OVERHEAD + payload - 1u;
        const uint8_t h[18] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0, (uint8_t)(bsize & 0xffu), (uint8_t)(bsize >> 8)};
        for (int i = 0; i < 18; i++) or_byte(out, cap_words, off + i, h[i]);
        const uint64_t tr = off + 18u + payload;
        for (int i = 0; i < 4; i++) { or_byte(out, cap_words, tr + i, plan.crc >> (8 * i)); or_byte(out, cap_words, tr + 4 + i, n >> (8 * i)); }
    }
    __syncthreads();
    if (!plan.dynamic) {
        // one stored block: whole words of the destination by plain stores, the bytes around them like every shared word
        const uint64_t D = off + 18u + STORED_OVERHEAD;
        if (t == 0) {
            const uint32_t sb[5] = {1u, n & 0xffu, n >> 8, ~n & 0xffu, (~n >> 8) & 0xffu};
            for (int i = 0; i < 5; i++) or_byte(out, cap_words, off + 18u + i, sb[i]);
        }
        const uint64_t w0 = (D + 3u) >> 2, w1 = (D + n) >> 2;
        for (uint64_t w = w0 + t; w < w1; w += STRIPS) {
            const uint32_t p = (uint32_t)(w * 4u - D);
            if (w < cap_words) out[w] = (uint32_t)d[p] | ((uint32_t)d[p + 1] << 8) | ((uint32_t)d[p + 2] << 16) | ((uint32_t)d[p + 3] << 24);
        }
        if (t == 0) {
            const uint32_t head_end = w0 < w1 ? (uint32_t)(w0 * 4u - D) : n, tail_begin = w0 < w1 ? (uint32_t)(w1 * 4u - D) : n;
            for (uint32_t p = 0; p < head_end; p++) or_byte(out, cap_words, D + p, d[p]);
            for (uint32_t p = tail_begin; p < n; p++) or_byte(out, cap_words, D + p, d[p]);
        }
        return;
    }
    const uint32_t b = t * STRIP < n ? t * STRIP : n, e = b + STRIP < n ? b + STRIP : n;
    uint32_t nl = 0, total;
    if (fmt != FMT_RAW) nl = (uint32_t)(nl_before[chunk] & 3u) + block_excl_scan(newlines_in(d, b, e), sh, total);
    // the bits of this strip: a block's first token carries the end of the previous block and the header of its own
    uint32_t bits = 0, last_cls = 0;
    walk_strip(d, b, e, fmt, nl, [&](uint32_t, uint32_t cls, uint32_t pcls, uint8_t c, uint32_t run) {
        if (cls != pcls) bits += (pcls != ~0u ? code[pcls][256] >> 16 : 0u) + hbits[cls];
        if (run) {
            uint32_t sym, eb, ev;
            length_symbol(run, sym, eb, ev);
            bits += (code[cls][sym] >> 16) + eb + 1u;
        } else bits += code[cls][c] >> 16;
        last_cls = cls;
    });
    const bool closes = b < e && e == n;                   // the lane of the chunk's last byte ends the last block and the member
    if (closes) bits += (code[last_cls][256] >> 16) + FINAL_BITS;
    const uint32_t before = block_excl_scan(bits, sh, total);
    if (!bits) return;
    Emitter em(out, cap_words, (off + 18u) * 8u + before);
    auto put_code = [&](uint32_t cv) { em.put(cv & 0xffffu, cv >> 16); };
    walk_strip(d, b, e, fmt, nl, [&](uint32_t, uint32_t cls, uint32_t pcls, uint8_t c, uint32_t run) {
        if (cls != pcls) {
            if (pcls != ~0u) put_code(code[pcls][256]);
            const uint32_t hb = hbits[cls];
            for (uint32_t i = 0; i < (hb >> 5); i++) em.put(hdr[cls][i], 32);
            if (hb & 31u) em.put(hdr[cls][hb >> 5] & ((1u << (hb & 31u)) - 1u), hb & 31u);
        }
        if (run) {
            uint32_t sym, eb, ev;
            length_symbol(run, sym, eb, ev);
            put_code(code[cls][sym]);
            if (eb) em.put(ev, eb);
            em.put(0u, 1u);                                // distance 1: the one distance code, one bit
        } else put_code(code[cls][c]);
    });
    if (closes) { put_code(code[last_cls][256]); em.put(FINAL_VALUE, FINAL_BITS); }
    em.finish();
}

uint32_t past_zero_byte(uint32_t r) {
    for (int k = 0; k < 8; k++) r = (r & 1u) ? POLY ^ (r >> 1) : r >> 1;
    return r;
}
uint32_t crc_of_zeros(uint32_t n) {
    uint32_t r = 0xFFFFFFFFu;
    for (uint32_t i = 0; i < n; i++) r = past_zero_byte(r);
    return ~r;
}

}  // namespace

void make_crc_ops(CrcOps& ops, uint32_t last_chunk_bytes) {
    static const CrcOps fixed = [] {
        CrcOps o{};
        for (int j = 0; j < 32; j++) {
            uint32_t r = 1u << j;
            for (uint32_t i = 0; i < STRIP; i++) r = past_zero_byte(r);
            o.shift[0][j] = r;
        }
        for (int k = 1; k < 8; k++)
            for (int j = 0; j < 32; j++) {
                const uint32_t v = o.shift[k - 1][j];
                uint32_t m = 0;
                for (int bit = 0; bit < 32; bit++) if ((v >> bit) & 1u) m ^= o.shift[k - 1][bit];
                o.shift[k][j] = m;
            }
        o.zeros_full = crc_of_zeros(CHUNK);
        return o;
    }();
    ops = fixed;
    ops.zeros_last = last_chunk_bytes == CHUNK ? fixed.zeros_full : crc_of_zeros(last_chunk_bytes);
}

hipError_t launch_count(const uint8_t* src, uint64_t bytes, uint64_t* counts, hipStream_t s) {
    const uint64_t nc = n_chunks(bytes);
    if (!nc) return hipSuccess;
    hipLaunchKernelGGL(k_gz_count, dim3((unsigned)nc), dim3(STRIPS), 0, s, src, bytes, counts);
    return hipGetLastError();
}

hipError_t launch_plan(const uint8_t* src, uint64_t bytes, int fmt, const uint64_t* nl_before, const CrcOps& ops, ChunkPlan* plans,
                       uint64_t* sizes, hipStream_t s) {
    const uint64_t nc = n_chunks(bytes);
    if (!nc) return hipSuccess;
    hipLaunchKernelGGL(k_gz_plan, dim3((unsigned)nc), dim3(STRIPS), 0, s, src, bytes, fmt, nl_before, ops, plans, sizes);
    return hipGetLastError();
}

hipError_t launch_encode(const uint8_t* src, uint64_t bytes, int fmt, const uint64_t* nl_before, const ChunkPlan* plans,
                         const uint64_t* member_off, uint32_t* out, uint64_t out_words, hipStream_t s) {
    const uint64_t nc = n_chunks(bytes);
    if (!nc) return hipSuccess;
    hipLaunchKernelGGL(k_gz_encode, dim3((unsigned)nc), dim3(STRIPS), 0, s, src, bytes, fmt, nl_before, plans, member_off, out, out_words);
    return hipGetLastError();
}

}  // namespace tkgz
