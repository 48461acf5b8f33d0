// loop_filter.h -- the bounds table that answers most first-threshold look-ups of k_loop from LDS, written so
// that the same text runs in a lane of kernels.hip, in api.cpp's model loader and in a host test (tools/loop_filter_check.cpp).
// A draw of the error loop changes nothing where its word dw is below t0, the first threshold of the k-mer under it.  The k-mers
// are grouped by a coarse key; per key the table holds the top byte of the smallest and of the largest t0 of its group.  Then
//     (dw >> 24) <  lo   proves  dw < t0  (dw < lo << 24 <= min t0 <= t0):                     the draw changes nothing
//     (dw >> 24) >  hi   proves  dw > t0  (dw >= (hi + 1) << 24 > max t0 >= t0):               the draw changes something
// and only the draws in between need t0 itself.  Both proofs hold for any key function, as long as the table was built over all
// k-mers with the same one.  No memory is allocated; every array is the caller's.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define TKLF_HD __host__ __device__ inline
#else
#define TKLF_HD inline
#endif

namespace tklf {

constexpr int LOOP_FILTER_BITS = 11;
constexpr uint32_t LOOP_FILTER_KEYS = 1u << LOOP_FILTER_BITS;          // 2048 entries of 2 bytes: 4 KB
constexpr uint32_t LOOP_FILTER_BYTES = LOOP_FILTER_KEYS * 2u;

enum { DRAW_NOOP = 0, DRAW_CHANGE = 1, DRAW_UNDECIDED = 2 };

// the key of k-mer index kx: its last base dropped, the 11 bits above it
TKLF_HD uint32_t loop_filter_key(uint32_t kx) { return (kx >> 2) & (LOOP_FILTER_KEYS - 1u); }

// an entry: lo | hi << 8
TKLF_HD uint16_t loop_filter_entry(uint32_t lo, uint32_t hi) { return (uint16_t)(lo | (hi << 8)); }

// what entry e says about a draw with word dw
TKLF_HD int loop_filter_classify(uint32_t e, uint32_t dw) {
    const uint32_t top = dw >> 24, lo = e & 0xffu, hi = (e >> 8) & 0xffu;
    return top < lo ? DRAW_NOOP : (top > hi ? DRAW_CHANGE : DRAW_UNDECIDED);
}

// the table of thresholds t0[0..nk) into out[0..LOOP_FILTER_KEYS); a key that no k-mer maps to (small k) is never decided
inline void loop_filter_build(const uint32_t* t0, size_t nk, uint16_t* out) {
    uint8_t lo[LOOP_FILTER_KEYS], hi[LOOP_FILTER_KEYS];
    for (uint32_t q = 0; q < LOOP_FILTER_KEYS; q++) { lo[q] = 255; hi[q] = 0; }
    for (size_t i = 0; i < nk; i++) {
        const uint32_t q = loop_filter_key((uint32_t)i);
        const uint8_t b = (uint8_t)(t0[i] >> 24);
        if (b < lo[q]) lo[q] = b;
        if (b > hi[q]) hi[q] = b;
    }
    for (uint32_t q = 0; q < LOOP_FILTER_KEYS; q++) out[q] = lo[q] <= hi[q] ? loop_filter_entry(lo[q], hi[q]) : loop_filter_entry(0, 255);
}

}  // namespace tklf
