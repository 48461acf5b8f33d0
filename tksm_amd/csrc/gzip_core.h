// gzip_core.h -- the serial pieces of the device-side BGZF encoder, written so that the same text runs in a
// lane of gzip_kernels.hip and in a host test: the tokeniser of a strip, length-limited Huffman code lengths, the dynamic block
// header of one line class, canonical codes.  No memory is allocated; every array is the caller's.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define TKGZ_HD __host__ __device__ inline
#else
#define TKGZ_HD inline
#endif

namespace tkgz {

constexpr uint32_t CHUNK = 65280;         // uncompressed bytes of a BGZF member (0xff00, what bgzip uses)
constexpr uint32_t STRIPS = 256;          // lanes of the workgroup that owns a chunk
constexpr uint32_t STRIP = CHUNK / STRIPS;   // 255 bytes of a chunk per lane
constexpr int NSYM = 288;                 // literal/length alphabet (286 used), padded
constexpr int NCLS = 3;                   // line classes: header, sequence (with the '+' line), quality
constexpr int HDR_WORDS = 72;             // room for a block header: 17 + 19 x 3 + 287 x 7 bits at the very most
constexpr uint32_t STORED_OVERHEAD = 5;   // BFINAL/BTYPE byte, LEN, NLEN
constexpr uint32_t MEMBER_OVERHEAD = 26;  // 18-byte BGZF header + CRC-32 + ISIZE
constexpr uint32_t FINAL_BITS = 10;       // the member's last block: fixed Huffman, BFINAL = 1, nothing but end-of-block
constexpr uint32_t FINAL_VALUE = 3;

enum { FMT_RAW = 0, FMT_FASTA = 1, FMT_FASTQ = 2 };

// the class of the line that holds a byte with `nl` newlines before it (any value congruent to the true count modulo 4 will do)
TKGZ_HD uint32_t line_class(int fmt, uint32_t nl) {
    if (fmt == FMT_FASTQ) { const uint32_t t = nl & 3u; return t == 0 ? 0u : (t == 3 ? 2u : 1u); }
    if (fmt == FMT_FASTA) return nl & 1u;
    return 0;
}

// deflate's length code of a match of 3 - 258 bytes
TKGZ_HD void length_symbol(uint32_t len, uint32_t& sym, uint32_t& ebits, uint32_t& eval) {
    const uint32_t l = len - 3;
    if (l < 8) { sym = 257 + l; ebits = 0; eval = 0; return; }
    if (len == 258) { sym = 285; ebits = 0; eval = 0; return; }
    const uint32_t e = (31u - (uint32_t)__builtin_clz(l)) - 2u;
    sym = 257 + 4 * e + 4 + ((l >> e) & 3u);
    ebits = e;
    eval = l & ((1u << e) - 1u);
}

// The tokens of bytes [begin, end) of a chunk d[0..n): a byte equal to its predecessor starts a distance-1 match of the 3 - 258
// equal bytes that follow it inside the strip, everything else is a literal -- so a run of r >= 4 equal bytes is its first byte plus
// matches, and a run that crosses a strip boundary simply goes on (the match reaches back into the previous strip's last byte).
// Outside FMT_RAW a newline never joins a match: a token lies in one line, and a block boundary is a position whose byte is in
// another class than the byte before it.  f(position, class, class of the previous token or ~0u at the chunk's first byte, byte,
// match length or 0).  nl: newlines before `begin` (modulo 4).
template <class F>
TKGZ_HD void walk_strip(const uint8_t* d, uint32_t begin, uint32_t end, int fmt, uint32_t nl, F&& f) {
    uint32_t p = begin;
    uint32_t pcls = p == 0 ? ~0u : line_class(fmt, nl - (d[p - 1] == '\n' ? 1u : 0u));
    while (p < end) {
        const uint8_t c = d[p];
        const uint32_t cls = line_class(fmt, nl);
        uint32_t run = 0;
        if (p > 0 && d[p - 1] == c && (fmt == FMT_RAW || c != '\n')) {
            run = 1;
            while (p + run < end && run < 258 && d[p + run] == c) run++;
        }
        if (run >= 3) { f(p, cls, pcls, c, run); p += run; }
        else { f(p, cls, pcls, c, 0u); if (c == '\n') nl++; p++; }
        pcls = cls;
    }
}

// Minimum-redundancy code lengths in place (Moffat & Katajainen 1995): A[0..n) holds the weights in ascending order on entry and
// the code lengths (non-increasing) on return.  n >= 2.
TKGZ_HD void huffman_depths(uint32_t* A, int n) {
    if (n == 2) { A[0] = A[1] = 1; return; }
    A[0] += A[1];
    int root = 0, leaf = 2;
    for (int next = 1; next < n - 1; next++) {
        if (leaf >= n || A[root] < A[leaf]) { A[next] = A[root]; A[root++] = (uint32_t)next; } else A[next] = A[leaf++];
        if (leaf >= n || (root < next && A[root] < A[leaf])) { A[next] += A[root]; A[root++] = (uint32_t)next; } else A[next] += A[leaf++];
    }
    A[n - 2] = 0;
    for (int next = n - 3; next >= 0; next--) A[next] = A[A[next]] + 1;
    int avbl = 1, used = 0, dpth = 0;
    root = n - 2;
    int next = n - 1;
    while (avbl > 0) {
        while (root >= 0 && (int)A[root] == dpth) { used++; root--; }
        while (avbl > used) { A[next--] = (uint32_t)dpth; avbl--; }
        avbl = 2 * used; dpth++; used = 0;
    }
}

// Code lengths of at most `limit` bits for n >= 1 symbols given in ascending order of weight (w[] is overwritten): depths beyond
// the limit are moved onto it, and the Kraft sum is brought back to one by lengthening the cheapest shorter codes -- the count of
// codes per length is what is repaired, and the lengths go back to the symbols longest-first, i.e. rarest-first.
TKGZ_HD void limited_lengths(uint32_t* w, const uint16_t* sym, int n, int limit, uint8_t* len_of_symbol) {
    if (n == 1) { len_of_symbol[sym[0]] = 1; return; }
    huffman_depths(w, n);
    uint32_t num[16];
    for (int i = 0; i <= limit; i++) num[i] = 0;
    for (int i = 0; i < n; i++) num[w[i] > (uint32_t)limit ? (uint32_t)limit : w[i]]++;
    uint32_t total = 0;
    for (int i = limit; i > 0; i--) total += num[i] << (limit - i);
    while (total > (1u << limit)) {
        num[limit]--;
        for (int i = limit - 1; i > 0; i--)
            if (num[i]) { num[i]--; num[i + 1] += 2; break; }
        total--;
    }
    int at = 0;
    for (int l = limit; l > 0; l--)
        for (uint32_t j = 0; j < num[l]; j++) len_of_symbol[sym[at++]] = (uint8_t)l;
}

TKGZ_HD uint32_t reverse_bits(uint32_t v, int n) {
    uint32_t r = 0;
    for (int i = 0; i < n; i++) { r = (r << 1) | (v & 1u); v >>= 1; }
    return r;
}

// canonical codes (RFC 1951, 3.2.2) of the lengths len[0..n), as the bit stream wants them: out[s] = length << 16 | the code with
// its first bit lowest; 0 for an unused symbol
TKGZ_HD void canonical_codes(const uint8_t* len, int n, uint32_t* out) {
    uint32_t count[16], next[16];
    for (int i = 0; i < 16; i++) count[i] = 0;
    for (int s = 0; s < n; s++) count[len[s]]++;
    count[0] = 0;
    uint32_t code = 0;
    next[0] = 0;
    for (int b = 1; b < 16; b++) { code = (code + count[b - 1]) << 1; next[b] = code; }
    for (int s = 0; s < n; s++) {
        const int l = len[s];
        out[s] = l ? ((uint32_t)l << 16) | reverse_bits(next[l]++, l) : 0u;
    }
}

struct BitSink {                          // serial writer into zeroed words
    uint32_t* w; uint32_t bits = 0, cap_bits;
    bool ok = true;
    TKGZ_HD BitSink(uint32_t* words, uint32_t n_words) : w(words), cap_bits(n_words * 32u) {}
    TKGZ_HD void put(uint32_t v, uint32_t n) {
        if (!n) return;
        if (bits + n > cap_bits) { ok = false; return; }
        const uint32_t i = bits >> 5, sh = bits & 31u;
        w[i] |= v << sh;
        if (sh + n > 32) w[i + 1] |= v >> (32u - sh);
        bits += n;
    }
};

// The header of a dynamic block (not the last of its member) whose literal/length code has the lengths ll[0..NSYM) and whose
// distance code is the single 1-bit code of distance 1: BFINAL, BTYPE, HLIT, HDIST, HCLEN, the code-length code (at most 7 bits)
// and the run-length coded lengths.  hdr[0..HDR_WORDS) must be zero; rle: scratch of 320 entries.  Returns the number of bits, 0
// if it does not fit (the caller stores the chunk instead).
TKGZ_HD uint32_t block_header(const uint8_t* ll, uint32_t* hdr, uint16_t* rle) {
    int hlit = 286;
    while (hlit > 257 && ll[hlit - 1] == 0) hlit--;
    const int total = hlit + 1;
    auto at = [&](int i) -> uint32_t { return i < hlit ? ll[i] : 1u; };
    uint32_t freq[19];
    for (int i = 0; i < 19; i++) freq[i] = 0;
    int n_rle = 0;
    auto emit = [&](uint32_t sym, uint32_t extra) { rle[n_rle++] = (uint16_t)(sym | (extra << 8)); freq[sym]++; };
    for (int i = 0; i < total;) {
        const uint32_t cur = at(i);
        int r = 1;
        while (i + r < total && at(i + r) == cur) r++;
        i += r;
        if (cur == 0) {
            while (r >= 11) { const int t = r < 138 ? r : 138; emit(18, (uint32_t)(t - 11)); r -= t; }
            if (r >= 3) { emit(17, (uint32_t)(r - 3)); r = 0; }
            while (r-- > 0) emit(0, 0);
        } else {
            emit(cur, 0); r--;
            while (r >= 3) { const int t = r < 6 ? r : 6; emit(16, (uint32_t)(t - 3)); r -= t; }
            while (r-- > 0) emit(cur, 0);
        }
    }
    // the code-length code: its used symbols in ascending order of weight (19 of them at most: insertion)
    uint32_t w[19]; uint16_t s[19];
    int n = 0;
    for (int i = 0; i < 19; i++) {
        if (!freq[i]) continue;
        int j = n++;
        while (j > 0 && w[j - 1] > freq[i]) { w[j] = w[j - 1]; s[j] = s[j - 1]; j--; }
        w[j] = freq[i]; s[j] = (uint16_t)i;
    }
    uint8_t cl[19];
    for (int i = 0; i < 19; i++) cl[i] = 0;
    limited_lengths(w, s, n, 7, cl);
    uint32_t cc[19];
    canonical_codes(cl, 19, cc);
    const uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    int hclen = 19;
    while (hclen > 4 && cl[order[hclen - 1]] == 0) hclen--;
    BitSink out(hdr, HDR_WORDS);
    out.put(4, 3);                        // BFINAL = 0, BTYPE = 10
    out.put((uint32_t)(hlit - 257), 5);
    out.put(0, 5);
    out.put((uint32_t)(hclen - 4), 4);
    for (int i = 0; i < hclen; i++) out.put(cl[order[i]], 3);
    for (int i = 0; i < n_rle; i++) {
        const uint32_t sym = rle[i] & 0xffu, extra = rle[i] >> 8;
        out.put(cc[sym] & 0xffffu, cc[sym] >> 16);
        if (sym == 16) out.put(extra, 2);
        else if (sym == 17) out.put(extra, 3);
        else if (sym == 18) out.put(extra, 7);
    }
    return out.ok ? out.bits : 0u;
}

}  // namespace tkgz
