// ms_kernels.hip -- device side of model-sequence (see ms_kernels.h; the rules are stated in include/tksmseq.h).
//
// The data: per chunk of alignments three ragged arrays -- the column letters, the column of every read position and of every reference
// position -- written by one wave per alignment from the run-length ops; then one u64 key per error event and per q-score event.  Counting
// is sorting: rocprim's radix sort (through abund_sort_u64 / abund_sort_u32) and the lengths of the runs of equal keys.
#include "ms_kernels.h"

namespace tk {

namespace {

#define DEV __device__ __forceinline__

// (a reader of this file's own: kernels.hip keeps its code generation to itself)
DEV uint8_t ms_ref_base(const RefView& R, uint64_t g) {
    const uint32_t ex = R.blocktab[g >> BLOCK_SHIFT];
    if (ex != NO_BLOCK) return R.pool[((uint64_t)ex << BLOCK_SHIFT) + (g & ((1u << BLOCK_SHIFT) - 1))];
    return (uint8_t)((0x54474341u >> (8 * ((R.packed[g >> 4] >> ((g & 15) * 2)) & 3u))) & 0xFFu);      // "ACGT"
}
DEV int code2(uint8_t b) { return b == 'A' ? 0 : b == 'C' ? 1 : b == 'G' ? 2 : b == 'T' ? 3 : -1; }
DEV uint8_t complement(uint8_t b) { return b == 'A' ? 'T' : b == 'C' ? 'G' : b == 'G' ? 'C' : b == 'T' ? 'A' : b; }
// base i of the aligned part of the read, in the alignment's orientation
DEV uint8_t read_base(const uint8_t* __restrict__ bases, const MsAlnDev& a, uint32_t i) {
    return a.strand ? complement(bases[a.read_off + a.qend - 1u - i]) : bases[a.read_off + a.qstart + i];
}
// the alignment of item x of the chunk: the last a in [a0, a1) with off[a] <= x
DEV uint32_t find_aln(const uint64_t* __restrict__ off, uint32_t a0, uint32_t a1, uint64_t x) {
    uint32_t lo = a0, hi = a1 - 1;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo + 1) / 2;
        if (off[mid] <= x) lo = mid; else hi = mid - 1;
    }
    return lo;
}
DEV uint32_t wave_scan(uint32_t v, uint32_t lane) {          // inclusive, 64 lanes
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t o = __shfl_up(v, d, 64);
        if (lane >= (uint32_t)d) v += o;
    }
    return v;
}

// One wave per alignment.  A pass takes 64 ops: a wave scan of their lengths gives every op its first column, read position and reference
// position; then the lanes take the pass's columns 64 at a time and find their op by a search over the 64 starts (shuffles: no LDS).
// An alignment of any number of ops and columns takes as many passes as it needs; the running totals carry over.
__global__ void __launch_bounds__(256) k_ms_expand(const MsAlnDev* __restrict__ aln, const uint32_t* __restrict__ ops, const uint8_t* __restrict__ bases, RefView R,
                                                   MsChunk C, uint8_t* __restrict__ cols, uint32_t* __restrict__ rcol, uint32_t* __restrict__ tcol) {
    const uint32_t a = C.a0 + blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    if (a >= C.a1) return;                                                 // (whole waves leave: no shuffle reads a lane that is gone)
    const MsAlnDev A = aln[a];
    uint8_t* const my_cols = cols + (C.col_off[a] - C.col_base);
    uint32_t* const my_rcol = rcol + (C.rp_off[a] - C.rp_base);
    uint32_t* const my_tcol = tcol + (C.tp_off[a] - C.tp_base);
    const uint32_t n_read = A.qend - A.qstart;
    uint32_t carry_c = 0, carry_r = 0, carry_t = 0;
    for (uint32_t first = 0; first < A.n_ops; first += 64) {
        const uint32_t op = first + lane < A.n_ops ? ops[A.op_off + first + lane] : 0u;
        const uint32_t len = op >> 2, code = op & 3u;
        const uint32_t inc_c = wave_scan(len, lane), inc_r = wave_scan(code != 2u ? len : 0u, lane), inc_t = wave_scan(code != 1u ? len : 0u, lane);
        const uint32_t total = __shfl(inc_c, 63, 64);
        const uint32_t ex_c = inc_c - len, ex_r = carry_r + inc_r - (code != 2u ? len : 0u), ex_t = carry_t + inc_t - (code != 1u ? len : 0u);
        for (uint32_t c0 = 0; c0 < total; c0 += 64) {
            const uint32_t c = c0 + lane;
            uint32_t j = 0;                                                // the last op whose first column is <= c
#pragma unroll
            for (uint32_t step = 32; step; step >>= 1) {
                const uint32_t cand = j + step;
                const uint32_t v = __shfl(ex_c, (int)min(cand, 63u), 64), l = __shfl(len, (int)min(cand, 63u), 64);
                if (cand <= 63u && l && v <= c) j = cand;
            }
            const uint32_t d = c - __shfl(ex_c, (int)j, 64), jc = __shfl(code, (int)j, 64);
            const uint32_t i = __shfl(ex_r, (int)j, 64) + d, t = __shfl(ex_t, (int)j, 64) + d;
            if (c >= total) continue;
            const uint32_t col = carry_c + c;
            uint8_t letter;
            if (jc == 0u) {
                // (the host has checked that the ops consume exactly the two ranges: i < n_read, t < tlen)
                const uint8_t rb = i < n_read ? read_base(bases, A, i) : 0, fb = t < A.tlen ? ms_ref_base(R, A.ref_g + t) : 1;
                letter = rb == fb && code2(rb) >= 0 ? MS_EQ : MS_MIS;
            } else letter = jc == 1u ? MS_INS : MS_DEL;
            my_cols[col] = letter;
            if (jc != 2u && i < n_read) my_rcol[i] = col;
            if (jc != 1u && t < A.tlen) my_tcol[t] = col;
        }
        carry_c += total;
        carry_r += __shfl(inc_r, 63, 64);
        carry_t += __shfl(inc_t, 63, 64);
    }
}

// One lane per reference offset t of an alignment with t + k <= tlen.
__global__ void __launch_bounds__(256) k_ms_err_events(const MsAlnDev* __restrict__ aln, const uint8_t* __restrict__ bases, RefView R, MsChunk C,
                                                       const uint8_t* __restrict__ cols, const uint32_t* __restrict__ rcol, const uint32_t* __restrict__ tcol, int k,
                                                       uint64_t n_events, uint64_t* __restrict__ keys) {
    const uint64_t e = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (e >= n_events) return;
    const uint32_t a = find_aln(C.ee_off, C.a0, C.a1, C.ee_base + e);
    const MsAlnDev A = aln[a];
    const uint32_t t = (uint32_t)(C.ee_base + e - C.ee_off[a]);
    uint64_t key = MS_NO_EVENT;
    uint32_t kmer = 0;
    bool ok = t + (uint32_t)k <= A.tlen;
    for (int j = 0; ok && j < k; j++) {
        const int c = code2(ms_ref_base(R, A.ref_g + t + (uint32_t)j));
        ok = c >= 0;
        kmer = kmer << 2 | (uint32_t)(c & 3);
    }
    if (ok) {
        const uint8_t* const my_cols = cols + (C.col_off[a] - C.col_base);
        const uint32_t* const my_rcol = rcol + (C.rp_off[a] - C.rp_base);
        const uint32_t* const my_tcol = tcol + (C.tp_off[a] - C.tp_base);
        const uint32_t c0 = my_tcol[t], c1 = my_tcol[t + (uint32_t)k - 1u], n_read = A.qend - A.qstart;
        ok = my_cols[c0] == MS_EQ && my_cols[c1] == MS_EQ;
        if (ok) {
            uint32_t lo = 0, hi = n_read;                                  // the read position of column c0 (an '=' column has one)
            while (lo < hi) {
                const uint32_t mid = lo + (hi - lo) / 2;
                if (my_rcol[mid] < c0) lo = mid + 1; else hi = mid;
            }
            uint32_t i = lo, len = 0, alt = 0;
            for (uint32_t c = c0; ok && c <= c1; c++) {
                if (my_cols[c] == MS_DEL) continue;
                const int b = i < n_read ? code2(read_base(bases, A, i)) : -1;
                i++;
                ok = b >= 0;
                if (len < 12u) alt |= (uint32_t)(b & 3) << (22u - 2u * len);
                len++;
            }
            if (ok) {
                const bool self = len == (uint32_t)k && (alt >> (24 - 2 * k)) == kmer;
                if (len > (uint32_t)k + 4u) key = (uint64_t)kmer << 30 | (uint64_t)MS_CLASS_TOTAL_ONLY << 28;
                else key = (uint64_t)kmer << 30 | (uint64_t)(self ? MS_CLASS_SELF : MS_CLASS_ALT) << 28 | (uint64_t)len << 24 | alt;
            }
        }
    }
    keys[e] = key;
}

// r <= 29 'D' letters, the last one in bits 1..0
DEV uint64_t d_run(uint32_t r) { return r ? 0x5555555555555555ull >> (64u - 2u * r) : 0ull; }

// One lane per read position i of an alignment: slot 0 counts q under key 0 (the overall line), slot 1 + h the window of half-width h.
// The window grows by one read position on either side per step: the 'D' run between two neighbouring read positions is the gap of their
// columns, so the longest run and the letters are kept up in O(1) per step.
__global__ void __launch_bounds__(256) k_ms_qs_events(const MsAlnDev* __restrict__ aln, const uint8_t* __restrict__ quals, MsChunk C, const uint8_t* __restrict__ cols,
                                                      const uint32_t* __restrict__ rcol, int half, uint32_t max_del, uint64_t n_positions,
                                                      uint64_t* __restrict__ keys, uint32_t* __restrict__ subs) {
    const uint64_t p = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (p >= n_positions) return;
    const uint32_t a = find_aln(C.rp_off, C.a0, C.a1, C.rp_base + p);
    const MsAlnDev A = aln[a];
    const uint32_t i = (uint32_t)(C.rp_base + p - C.rp_off[a]), n = A.qend - A.qstart;
    const uint8_t* const my_cols = cols + (C.col_off[a] - C.col_base);
    const uint32_t* const my_rcol = rcol + (C.rp_off[a] - C.rp_base);
    const uint32_t q = quals[A.read_off + (A.strand ? A.qend - 1u - i : A.qstart + i)];
    const uint64_t slot = p * (uint64_t)(half + 2);
    keys[slot] = 0; subs[slot] = q;
    uint32_t left = my_rcol[i], right = left, len = 1, longest = 0;
    uint64_t v = my_cols[left];                                            // the letters, the last one in bits 1..0
    for (int h = 0; h <= half; h++) {
        uint64_t key = MS_NO_EVENT; uint32_t sub = 0;
        if (i >= (uint32_t)h && i + (uint32_t)h < n) {
            if (h > 0) {
                const uint32_t nl = my_rcol[i - (uint32_t)h], nr = my_rcol[i + (uint32_t)h];
                const uint32_t dl = left - nl - 1u, dr = nr - right - 1u;
                longest = max(longest, max(dl, dr));
                const uint64_t grown = (uint64_t)len + dl + dr + 2u;
                // (past 29 letters the text is never used: the length alone says so, and it only grows)
                if (grown <= 29u) {
                    v |= d_run(dl) << (2u * len);
                    v |= (uint64_t)my_cols[nl] << (2u * (len + dl));
                    v = (v << (2u * (dr + 1u))) | (d_run(dr) << 2) | my_cols[nr];
                }
                len = (uint32_t)min(grown, (uint64_t)64);
                left = nl; right = nr;
            }
            if (longest > max_del) { key = 0; sub = MS_SUB_MAX_DEL; }
            else if (len > 29u) { key = 0; sub = MS_SUB_TOO_LONG; }
            else { key = (uint64_t)len << 58 | v << (58u - 2u * len); sub = q; }
        }
        keys[slot + 1u + (uint64_t)h] = key; subs[slot + 1u + (uint64_t)h] = sub;
    }
}

__global__ void __launch_bounds__(256) k_ms_gather_u64(const uint64_t* __restrict__ in, const uint32_t* __restrict__ perm, uint32_t n, uint64_t* __restrict__ out) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < n) out[i] = in[perm[i]];
}
__global__ void __launch_bounds__(256) k_ms_gather_u32(const uint32_t* __restrict__ in, const uint32_t* __restrict__ perm, uint32_t n, uint32_t* __restrict__ out) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < n) out[i] = in[perm[i]];
}
__global__ void __launch_bounds__(256) k_ms_run_flags(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ subs, uint32_t n, uint64_t* __restrict__ flag) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < n) flag[i] = (i == 0 || keys[i] != keys[i - 1] || (subs && subs[i] != subs[i - 1])) ? 1ull : 0ull;
}
__global__ void __launch_bounds__(256) k_ms_run_starts(const uint64_t* __restrict__ keys, uint32_t n, const uint64_t* __restrict__ flag,
                                                       const uint64_t* __restrict__ scanned, uint32_t* __restrict__ start, uint64_t* __restrict__ info) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    if (flag[i]) start[(uint32_t)scanned[i]] = i;
    if (i == n - 1) { start[(uint32_t)scanned[n]] = n; info[0] = scanned[n]; info[1] = keys[i] == MS_NO_EVENT ? 1ull : 0ull; }
}
__global__ void __launch_bounds__(256) k_ms_run_write(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ subs, const uint32_t* __restrict__ start,
                                                      uint32_t n_runs, const uint64_t* __restrict__ vals, const uint32_t* __restrict__ perm,
                                                      uint64_t* __restrict__ okeys, uint32_t* __restrict__ osubs, uint64_t* __restrict__ ocounts) {
    const uint32_t g = blockIdx.x * 256u + threadIdx.x;
    if (g >= n_runs) return;
    const uint32_t b = start[g], e = start[g + 1];
    uint64_t count = e - b;
    if (vals) { count = 0; for (uint32_t j = b; j < e; j++) count += vals[perm[j]]; }
    okeys[g] = keys[b];
    if (osubs) osubs[g] = subs ? subs[b] : 0u;
    ocounts[g] = count;
}

__global__ void __launch_bounds__(256) k_ms_err_rank_keys(const uint64_t* __restrict__ keys, const uint64_t* __restrict__ counts, uint32_t n,
                                                          uint64_t* __restrict__ key2, uint32_t* bad) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const uint64_t c = counts[i];
    if (c > 0xFFFFFFFFull) atomicOr(bad, 1u);
    key2[i] = (keys[i] >> 28) << 32 | (0xFFFFFFFFull - min(c, (uint64_t)0xFFFFFFFFull));
}
DEV uint32_t lower_bound_u64(const uint64_t* __restrict__ v, uint32_t n, uint64_t x) {
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (v[mid] < x) lo = mid + 1; else hi = mid;
    }
    return lo;
}
__global__ void __launch_bounds__(256) k_ms_err_select(const uint64_t* __restrict__ key2, const uint32_t* __restrict__ perm, const uint64_t* __restrict__ keys,
                                                       const uint64_t* __restrict__ counts, uint32_t n, uint32_t n_kmers, uint32_t max_alt,
                                                       MsErrRowDev* __restrict__ rows) {
    const uint32_t kmer = blockIdx.x * 256u + threadIdx.x;
    if (kmer >= n_kmers) return;
    const uint32_t b = lower_bound_u64(key2, n, (uint64_t)kmer << 34), e = lower_bound_u64(key2, n, (uint64_t)(kmer + 1u) << 34);
    MsErrRowDev& r = rows[kmer];
    uint64_t total = 0, self = 0, too_long = 0;
    uint32_t n_alt = 0;
    for (uint32_t j = b; j < e; j++) {
        const uint32_t at = perm[j];
        const uint64_t key = keys[at], c = counts[at];
        const uint32_t cls = (uint32_t)(key >> 28) & 3u;
        total += c;
        if (cls == MS_CLASS_SELF) self += c;
        else if (cls == MS_CLASS_TOTAL_ONLY) too_long += c;
        else if (n_alt < max_alt) { r.alt[n_alt] = (uint32_t)key & 0xFFFFFFFu; r.count[n_alt] = c; n_alt++; }
    }
    r.total = total; r.self = self; r.too_long = too_long; r.n_alt = n_alt;
}

__global__ void __launch_bounds__(256) k_ms_qs_totals(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ subs, const uint64_t* __restrict__ counts,
                                                      const uint32_t* __restrict__ kstart, uint32_t n_keys, uint64_t min_occur, uint64_t* __restrict__ kkey,
                                                      uint64_t* __restrict__ kn, uint64_t* __restrict__ key2, unsigned long long* n_qual) {
    const uint32_t g = blockIdx.x * 256u + threadIdx.x;
    if (g >= n_keys) return;
    const uint32_t b = kstart[g], e = kstart[g + 1];
    uint64_t n = 0;
    for (uint32_t j = b; j < e; j++) if (subs[j] < 94u) n += counts[j];
    const uint64_t key = keys[b];
    kkey[g] = key; kn[g] = n;
    const bool qual = key != 0 && n >= min_occur && n > 0;
    key2[g] = qual ? ~n : ~0ull;
    if (qual) atomicAdd(n_qual, 1ull);
}
__global__ void __launch_bounds__(256) k_ms_qs_rows(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ subs, const uint64_t* __restrict__ counts,
                                                    const uint32_t* __restrict__ kstart, const uint32_t* __restrict__ ids, uint32_t n_ids, uint32_t n_keys,
                                                    MsQRowDev* __restrict__ rows) {
    const uint32_t j = blockIdx.x * 256u + threadIdx.x;
    if (j >= n_ids) return;
    MsQRowDev& r = rows[j];
    r.key = 0; r.n = 0;
    for (int q = 0; q < MS_SUBS; q++) r.count[q] = 0;
    const uint32_t g = ids[j];
    if (g >= n_keys) return;
    uint64_t n = 0;
    for (uint32_t x = kstart[g], e = kstart[g + 1]; x < e; x++) {
        const uint32_t sub = subs[x];
        if (sub >= (uint32_t)MS_SUBS) continue;
        r.count[sub] = counts[x];
        if (sub < 94u) n += counts[x];
    }
    r.key = keys[kstart[g]]; r.n = n;
}

inline dim3 blocks(uint64_t n) { return dim3((unsigned)((n + 255u) / 256u)); }

}  // namespace

hipError_t launch_ms_expand(const MsAlnDev* aln, const uint32_t* ops, const uint8_t* bases, const RefView& R, const MsChunk& C, uint8_t* cols, uint32_t* rcol,
                            uint32_t* tcol, hipStream_t s) {
    if (C.a1 <= C.a0) return hipSuccess;
    hipLaunchKernelGGL(k_ms_expand, dim3((C.a1 - C.a0 + 3u) / 4u), dim3(256), 0, s, aln, ops, bases, R, C, cols, rcol, tcol);
    return hipGetLastError();
}
hipError_t launch_ms_err_events(const MsAlnDev* aln, const uint8_t* bases, const RefView& R, const MsChunk& C, const uint8_t* cols, const uint32_t* rcol,
                                const uint32_t* tcol, int k, uint64_t n_events, uint64_t* keys, hipStream_t s) {
    if (!n_events) return hipSuccess;
    hipLaunchKernelGGL(k_ms_err_events, blocks(n_events), dim3(256), 0, s, aln, bases, R, C, cols, rcol, tcol, k, n_events, keys);
    return hipGetLastError();
}
hipError_t launch_ms_qs_events(const MsAlnDev* aln, const uint8_t* quals, const MsChunk& C, const uint8_t* cols, const uint32_t* rcol, int kq, int max_del,
                               uint64_t n_positions, uint64_t* keys, uint32_t* subs, hipStream_t s) {
    if (!n_positions) return hipSuccess;
    hipLaunchKernelGGL(k_ms_qs_events, blocks(n_positions), dim3(256), 0, s, aln, quals, C, cols, rcol, (kq - 1) / 2, (uint32_t)max_del, n_positions, keys, subs);
    return hipGetLastError();
}
hipError_t launch_ms_gather_u64(const uint64_t* in, const uint32_t* perm, uint32_t n, uint64_t* out, hipStream_t s) {
    if (!n) return hipSuccess;
    hipLaunchKernelGGL(k_ms_gather_u64, blocks(n), dim3(256), 0, s, in, perm, n, out);
    return hipGetLastError();
}
hipError_t launch_ms_gather_u32(const uint32_t* in, const uint32_t* perm, uint32_t n, uint32_t* out, hipStream_t s) {
    if (!n) return hipSuccess;
    hipLaunchKernelGGL(k_ms_gather_u32, blocks(n), dim3(256), 0, s, in, perm, n, out);
    return hipGetLastError();
}
hipError_t launch_ms_run_flags(const uint64_t* keys, const uint32_t* subs, uint32_t n, uint64_t* flag, hipStream_t s) {
    if (!n) return hipSuccess;
    hipLaunchKernelGGL(k_ms_run_flags, blocks(n), dim3(256), 0, s, keys, subs, n, flag);
    return hipGetLastError();
}
hipError_t launch_ms_run_starts(const uint64_t* keys, uint32_t n, const uint64_t* flag, const uint64_t* scanned, uint32_t* start, uint64_t* info, hipStream_t s) {
    if (!n) return hipMemsetAsync(info, 0, 16, s);
    hipLaunchKernelGGL(k_ms_run_starts, blocks(n), dim3(256), 0, s, keys, n, flag, scanned, start, info);
    return hipGetLastError();
}
hipError_t launch_ms_run_write(const uint64_t* keys, const uint32_t* subs, const uint32_t* start, uint32_t n_runs, const uint64_t* vals, const uint32_t* perm,
                               uint64_t* okeys, uint32_t* osubs, uint64_t* ocounts, hipStream_t s) {
    if (!n_runs) return hipSuccess;
    hipLaunchKernelGGL(k_ms_run_write, blocks(n_runs), dim3(256), 0, s, keys, subs, start, n_runs, vals, perm, okeys, osubs, ocounts);
    return hipGetLastError();
}
hipError_t launch_ms_err_rank_keys(const uint64_t* keys, const uint64_t* counts, uint32_t n, uint64_t* key2, uint32_t* bad, hipStream_t s) {
    hipError_t e = hipMemsetAsync(bad, 0, 4, s);
    if (e != hipSuccess || !n) return e;
    hipLaunchKernelGGL(k_ms_err_rank_keys, blocks(n), dim3(256), 0, s, keys, counts, n, key2, bad);
    return hipGetLastError();
}
hipError_t launch_ms_err_select(const uint64_t* key2_sorted, const uint32_t* perm, const uint64_t* keys, const uint64_t* counts, uint32_t n, int k, int max_alt,
                                MsErrRowDev* rows, hipStream_t s) {
    const uint32_t n_kmers = 1u << (2 * k);
    hipLaunchKernelGGL(k_ms_err_select, blocks(n_kmers), dim3(256), 0, s, key2_sorted, perm, keys, counts, n, n_kmers, (uint32_t)max_alt, rows);
    return hipGetLastError();
}
hipError_t launch_ms_qs_totals(const uint64_t* keys, const uint32_t* subs, const uint64_t* counts, const uint32_t* kstart, uint32_t n_keys, uint64_t min_occur,
                               uint64_t* kkey, uint64_t* kn, uint64_t* key2, unsigned long long* n_qual, hipStream_t s) {
    hipError_t e = hipMemsetAsync(n_qual, 0, 8, s);
    if (e != hipSuccess || !n_keys) return e;
    hipLaunchKernelGGL(k_ms_qs_totals, blocks(n_keys), dim3(256), 0, s, keys, subs, counts, kstart, n_keys, min_occur, kkey, kn, key2, n_qual);
    return hipGetLastError();
}
hipError_t launch_ms_qs_rows(const uint64_t* keys, const uint32_t* subs, const uint64_t* counts, const uint32_t* kstart, const uint32_t* ids, uint32_t n_ids,
                             uint32_t n_keys, MsQRowDev* rows, hipStream_t s) {
    if (!n_ids) return hipSuccess;
    hipLaunchKernelGGL(k_ms_qs_rows, blocks(n_ids), dim3(256), 0, s, keys, subs, counts, kstart, ids, n_ids, n_keys, rows);
    return hipGetLastError();
}

}  // namespace tk
