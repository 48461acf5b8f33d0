// abund_kernels.hip -- device side of abundance (see abund_kernels.h; line numbers into py/transcript_abundance.py).
//
// The data: the reads' records in CSR form (grouped by read on the host), then the HITS of the surviving reads, also CSR by read, in read
// and record order: (tid, weight).  The EM round reads them twice: by transcript through a permutation made once (the stable sort of the
// hits by tid) for the M-step, and by read for the E-step.  Sums never use floating-point atomics: a segment is cut into chunks of
// ABUND_CHUNK positions, a chunk is added by ONE wave in a fixed pattern, the chunks of a segment in chunk order, the segments' sums by
// fixed trees of 256 -- the order is a function of the input alone, not of the launch geometry or the device.
#include "abund_kernels.h"

#include <cstring>

#include <rocprim/device/device_radix_sort.hpp>

namespace tk {

namespace {

#define DEV __device__ __forceinline__

struct Ph4a { uint32_t x, y, z, w; };
DEV Ph4a philox_raw(uint64_t seed, uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3) {
    uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
#pragma unroll
    for (int r = 0; r < 10; r++) {
        const unsigned long long p0 = (unsigned long long)0xD2511F53u * c0, p1 = (unsigned long long)0xCD9E8D57u * c2;
        const uint32_t h0 = (uint32_t)(p0 >> 32), l0 = (uint32_t)p0, h1 = (uint32_t)(p1 >> 32), l1 = (uint32_t)p1;
        const uint32_t n0 = h1 ^ c1 ^ k0, n2 = h0 ^ c3 ^ k1;
        c0 = n0; c1 = l1; c2 = n2; c3 = l0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    return Ph4a{c0, c1, c2, c3};
}
enum { ST_ABUND_CELL = 60 };

constexpr uint32_t FULL_LENGTH_MIN_DISTANCE = 20;    // :213
constexpr uint32_t FL_BIT = 0x80000000u;

// the best record of a read (:229-236): more matches, or as many and full length -- so a later full-length tie replaces an earlier record
DEV void best_record(const uint32_t* tstart, const uint32_t* nmatch, const uint32_t* blen, uint32_t b, uint32_t e, uint32_t& best_m, uint32_t& best_len,
                     bool& best_fl) {
    best_m = 0; best_len = 0; best_fl = false;
    for (uint32_t i = b; i < e; i++) {
        const bool fl = tstart[i] < FULL_LENGTH_MIN_DISTANCE;
        const uint32_t m = nmatch[i];
        if (m > best_m || (m == best_m && fl)) { best_len = blen[i]; best_m = m; best_fl = fl; }
    }
}
// is_equivalent_hit (:242-245): the quotient in IEEE double, strictly above 0.95, and the same full-length flag
DEV bool is_hit(uint32_t m, uint32_t ts, uint32_t best_m, bool best_fl) {
    return (double)m / (double)best_m > 0.95 && (ts < FULL_LENGTH_MIN_DISTANCE) == best_fl;
}

__global__ void __launch_bounds__(256) k_abund_compat(const uint32_t* __restrict__ rec_off, const uint32_t* __restrict__ tstart,
                                                      const uint32_t* __restrict__ nmatch, const uint32_t* __restrict__ blen,
                                                      const uint32_t* __restrict__ qlen, uint32_t n_reads, uint32_t* __restrict__ best,
                                                      uint64_t* __restrict__ packed, uint32_t* bad_read) {
    const uint32_t r = blockIdx.x * 256u + threadIdx.x;
    if (r >= n_reads) return;
    const uint32_t b = rec_off[r], e = rec_off[r + 1];
    uint32_t best_m, best_len; bool best_fl;
    best_record(tstart, nmatch, blen, b, e, best_m, best_len, best_fl);
    best[r] = best_m | (best_fl ? FL_BIT : 0u);
    uint64_t out = 0;
    const uint32_t ql = qlen[r];
    if (ql == 0) atomicMin(bad_read, r);                                   // :238 divides by the read length
    else if (!((double)best_len / (double)ql < 0.5)) {                    // :238-240; exactly 0.5 stays
        if (best_m == 0) atomicMin(bad_read, r);                           // :243 divides by the best match count
        else {
            uint32_t hits = 0;
            for (uint32_t i = b; i < e; i++) hits += is_hit(nmatch[i], tstart[i], best_m, best_fl) ? 1u : 0u;
            out = (1ull << 32) | hits;
        }
    }
    packed[r] = out;
}

__global__ void __launch_bounds__(256) k_abund_hits(const uint32_t* __restrict__ rec_off, const uint32_t* __restrict__ tid,
                                                    const uint32_t* __restrict__ tstart, const uint32_t* __restrict__ nmatch, uint32_t n_reads,
                                                    const uint32_t* __restrict__ best, const uint64_t* __restrict__ packed,
                                                    const uint64_t* __restrict__ scanned, uint32_t* __restrict__ surv_read,
                                                    uint32_t* __restrict__ hit_off, uint32_t* __restrict__ hit_tid, uint32_t* __restrict__ hit_read,
                                                    double* __restrict__ w) {
    const uint32_t r = blockIdx.x * 256u + threadIdx.x;
    if (r >= n_reads) return;
    if (r == 0) { const uint64_t t = scanned[n_reads]; hit_off[(uint32_t)(t >> 32)] = (uint32_t)t; }
    const uint64_t pk = packed[r];
    if (!(pk >> 32)) return;
    const uint64_t at = scanned[r];
    const uint32_t k = (uint32_t)(at >> 32), hits = (uint32_t)pk;
    uint32_t h = (uint32_t)at;
    surv_read[k] = r;
    hit_off[k] = h;
    const uint32_t bm = best[r] & ~FL_BIT;
    const bool bfl = (best[r] & FL_BIT) != 0;
    const double share = 1.0 / (double)hits;                               // :255
    for (uint32_t i = rec_off[r], e = rec_off[r + 1]; i < e; i++)
        if (is_hit(nmatch[i], tstart[i], bm, bfl)) { hit_tid[h] = tid[i]; hit_read[h] = k; w[h] = share; h++; }
}

__global__ void __launch_bounds__(256) k_abund_iota(uint32_t* out, uint32_t n) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < n) out[i] = i;
}

__global__ void __launch_bounds__(256) k_abund_dense_offsets(const uint32_t* __restrict__ sorted, uint32_t n, uint32_t n_keys, uint32_t* __restrict__ off) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const uint32_t k = min(sorted[i], n_keys - 1);
    const uint32_t first = i ? min(sorted[i - 1], n_keys - 1) + 1 : 0u;
    for (uint32_t t = first; t <= k; t++) off[t] = i;
    if (i == n - 1) for (uint32_t t = k + 1; t <= n_keys; t++) off[t] = n;
}

__global__ void __launch_bounds__(256) k_abund_seg_flags(const uint64_t* __restrict__ sorted, uint32_t n, uint64_t* __restrict__ flag) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < n) flag[i] = (i == 0 || sorted[i] != sorted[i - 1]) ? 1ull : 0ull;
}
__global__ void __launch_bounds__(256) k_abund_seg_write(const uint64_t* __restrict__ sorted, uint32_t n, const uint64_t* __restrict__ flag,
                                                         const uint64_t* __restrict__ scanned, uint32_t* __restrict__ off, uint64_t* __restrict__ key) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    if (flag[i]) { const uint32_t g = (uint32_t)scanned[i]; off[g] = i; key[g] = sorted[i]; }
    if (i == n - 1) off[(uint32_t)scanned[n]] = n;
}

__global__ void __launch_bounds__(256) k_abund_chunk_counts(const uint32_t* __restrict__ off, uint32_t n_seg, uint64_t* __restrict__ counts) {
    const uint32_t g = blockIdx.x * 256u + threadIdx.x;
    if (g < n_seg) counts[g] = (uint64_t)((off[g + 1] - off[g] + ABUND_CHUNK - 1) / ABUND_CHUNK);
}
__global__ void __launch_bounds__(256) k_abund_chunk_map(const uint64_t* __restrict__ chunk_off, uint32_t n_seg, uint32_t* __restrict__ chunk_seg) {
    const uint32_t g = blockIdx.x * 256u + threadIdx.x;
    if (g >= n_seg) return;
    for (uint64_t c = chunk_off[g], e = chunk_off[g + 1]; c < e; c++) chunk_seg[c] = g;
}

// the fixed tree over the 64 lanes of a wave: 32, 16, 8, 4, 2, 1 (lane 0 holds the result)
DEV double wave_tree(double v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_down(v, d, 64);
    return v;
}
// the fixed tree over the 256 threads of a block: waves first, then the four wave results in order ((0 + 1) + (2 + 3))
DEV double block_tree(double v, double* lds) {
    v = wave_tree(v);
    if ((threadIdx.x & 63u) == 0) lds[threadIdx.x >> 6] = v;
    __syncthreads();
    return (lds[0] + lds[1]) + (lds[2] + lds[3]);
}

// one wave per chunk: lane l adds positions l, l + 64, ... of the chunk in order, then the tree
__global__ void __launch_bounds__(256) k_abund_msum(const double* __restrict__ w, const uint32_t* __restrict__ perm, const uint32_t* __restrict__ off,
                                                    const uint64_t* __restrict__ chunk_off, const uint32_t* __restrict__ chunk_seg, uint32_t n_chunks,
                                                    double* __restrict__ partial) {
    const uint32_t c = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    if (c >= n_chunks) return;                                             // (whole waves leave: no shuffle reads a lane that is gone)
    const uint32_t g = chunk_seg[c];
    const uint32_t k = c - (uint32_t)chunk_off[g];
    const uint32_t lo = off[g] + k * ABUND_CHUNK, hi = min(off[g + 1], lo + ABUND_CHUNK);
    double acc = 0.0;
    for (uint32_t i = lo + lane; i < hi; i += 64) acc += w[perm[i]];
    acc = wave_tree(acc);
    if (lane == 0) partial[c] = acc;
}

__global__ void __launch_bounds__(256) k_abund_mfinish(const double* __restrict__ partial, const uint64_t* __restrict__ chunk_off, uint32_t n_seg,
                                                       double* __restrict__ sum, double* __restrict__ block_part) {
    __shared__ double lds[4];
    const uint32_t g = blockIdx.x * 256u + threadIdx.x;
    double s = 0.0;
    if (g < n_seg) {
        for (uint64_t c = chunk_off[g], e = chunk_off[g + 1]; c < e; c++) s += partial[c];
        sum[g] = s;
    }
    const double t = block_tree(s, lds);
    if (threadIdx.x == 0) block_part[blockIdx.x] = t;
}
// ONE block: thread t adds block_part[t], [t + 256], ... in order, then the tree
__global__ void __launch_bounds__(256) k_abund_mtotal(const double* __restrict__ block_part, uint32_t n_parts, double* __restrict__ total) {
    __shared__ double lds[4];
    double s = 0.0;
    for (uint32_t i = threadIdx.x; i < n_parts; i += 256) s += block_part[i];
    const double t = block_tree(s, lds);
    if (threadIdx.x == 0) total[0] = t;
}

__global__ void __launch_bounds__(256) k_abund_estep(const uint32_t* __restrict__ hit_off, const uint32_t* __restrict__ hit_tid, uint32_t n_surv,
                                                     const double* __restrict__ sum, const double* __restrict__ total, double* __restrict__ w) {
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    if (k >= n_surv) return;
    const uint32_t b = hit_off[k], e = hit_off[k + 1];
    const double tot = total[0];
    double acc = 0.0;                                                      // :282-284: the abundances of the read's hits in hit order
    for (uint32_t i = b; i < e; i++) acc += sum[hit_tid[i]] / tot;
    for (uint32_t i = b; i < e; i++) w[i] = (sum[hit_tid[i]] / tot) / acc; // :289
}

__global__ void __launch_bounds__(256) k_abund_scale(const double* __restrict__ sum, const double* __restrict__ total, uint32_t n, double* __restrict__ out) {
    const uint32_t g = blockIdx.x * 256u + threadIdx.x;
    if (g < n) out[g] = sum[g] / total[0];
}

__global__ void __launch_bounds__(256) k_abund_gather_cells(const uint32_t* __restrict__ surv_read, const uint32_t* __restrict__ read_cell, uint32_t n_surv,
                                                            uint32_t* __restrict__ cell) {
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    if (k < n_surv) cell[k] = read_cell[surv_read[k]];
}
__global__ void __launch_bounds__(256) k_abund_cells(uint64_t seed, const double* __restrict__ cdf, const uint32_t* __restrict__ cell_of, uint32_t n_cdf,
                                                     uint32_t n_surv, uint32_t* __restrict__ cell) {
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    if (k >= n_surv) return;
    const double u = (double)philox_raw(seed, k, 0u, ST_ABUND_CELL, 0u).x * (1.0 / 4294967296.0);
    const double target = u * cdf[n_cdf - 1];
    uint32_t lo = 0, hi = n_cdf - 1;                                       // the first b with cdf[b] > target, the last entry when none
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (cdf[mid] > target) hi = mid; else lo = mid + 1;
    }
    cell[k] = cell_of[lo];
}
__global__ void __launch_bounds__(256) k_abund_keys(const uint32_t* __restrict__ hit_tid, const uint32_t* __restrict__ hit_read, const uint32_t* __restrict__ cell,
                                                    uint32_t n_hits, uint64_t* __restrict__ key) {
    const uint32_t h = blockIdx.x * 256u + threadIdx.x;
    if (h < n_hits) key[h] = ((uint64_t)hit_tid[h] << 32) | cell[hit_read[h]];
}
__global__ void __launch_bounds__(256) k_abund_ranks(const uint32_t* __restrict__ perm, const uint32_t* __restrict__ off, uint32_t n_seg, uint32_t* __restrict__ rank) {
    const uint32_t g = blockIdx.x * 256u + threadIdx.x;
    if (g < n_seg) rank[g] = off[g + 1] > off[g] ? perm[off[g]] : ABUND_NO_READ;
}

inline dim3 blocks(uint32_t n) { return dim3((n + 255u) / 256u); }

}  // namespace

hipError_t launch_abund_compat(const uint32_t* rec_off, const uint32_t* tstart, const uint32_t* nmatch, const uint32_t* blen, const uint32_t* qlen,
                               uint32_t n_reads, uint32_t* best, uint64_t* packed, uint32_t* bad_read, hipStream_t s) {
    hipError_t e = hipMemsetAsync(bad_read, 0xFF, 4, s);
    if (e != hipSuccess || !n_reads) return e;
    hipLaunchKernelGGL(k_abund_compat, blocks(n_reads), dim3(256), 0, s, rec_off, tstart, nmatch, blen, qlen, n_reads, best, packed, bad_read);
    return hipGetLastError();
}
hipError_t launch_abund_hits(const uint32_t* rec_off, const uint32_t* tid, const uint32_t* tstart, const uint32_t* nmatch, uint32_t n_reads,
                             const uint32_t* best, const uint64_t* packed, const uint64_t* scanned, uint32_t* surv_read, uint32_t* hit_off,
                             uint32_t* hit_tid, uint32_t* hit_read, double* w, hipStream_t s) {
    if (!n_reads) return hipSuccess;
    hipLaunchKernelGGL(k_abund_hits, blocks(n_reads), dim3(256), 0, s, rec_off, tid, tstart, nmatch, n_reads, best, packed, scanned, surv_read, hit_off,
                       hit_tid, hit_read, w);
    return hipGetLastError();
}
hipError_t launch_abund_iota(uint32_t* out, uint32_t n, hipStream_t s) {
    if (!n) return hipSuccess;
    hipLaunchKernelGGL(k_abund_iota, blocks(n), dim3(256), 0, s, out, n);
    return hipGetLastError();
}
hipError_t abund_sort_u32(void* temp, size_t* temp_bytes, const uint32_t* keys, uint32_t* keys_sorted, const uint32_t* vals, uint32_t* vals_sorted, uint32_t n,
                          int end_bit, hipStream_t s) {
    return rocprim::radix_sort_pairs(temp, *temp_bytes, keys, keys_sorted, vals, vals_sorted, (size_t)n, 0u, (unsigned)end_bit, s);
}
hipError_t abund_sort_u64(void* temp, size_t* temp_bytes, const uint64_t* keys, uint64_t* keys_sorted, const uint32_t* vals, uint32_t* vals_sorted, uint32_t n,
                          int end_bit, hipStream_t s) {
    return rocprim::radix_sort_pairs(temp, *temp_bytes, keys, keys_sorted, vals, vals_sorted, (size_t)n, 0u, (unsigned)end_bit, s);
}
hipError_t launch_abund_dense_offsets(const uint32_t* sorted, uint32_t n, uint32_t n_keys, uint32_t* off, hipStream_t s) {
    if (!n || !n_keys) return hipSuccess;
    hipLaunchKernelGGL(k_abund_dense_offsets, blocks(n), dim3(256), 0, s, sorted, n, n_keys, off);
    return hipGetLastError();
}
hipError_t launch_abund_seg_flags(const uint64_t* sorted, uint32_t n, uint64_t* flag, hipStream_t s) {
    if (!n) return hipSuccess;
    hipLaunchKernelGGL(k_abund_seg_flags, blocks(n), dim3(256), 0, s, sorted, n, flag);
    return hipGetLastError();
}
hipError_t launch_abund_seg_write(const uint64_t* sorted, uint32_t n, const uint64_t* flag, const uint64_t* scanned, uint32_t* off, uint64_t* key, hipStream_t s) {
    if (!n) return hipSuccess;
    hipLaunchKernelGGL(k_abund_seg_write, blocks(n), dim3(256), 0, s, sorted, n, flag, scanned, off, key);
    return hipGetLastError();
}
hipError_t launch_abund_chunk_counts(const uint32_t* off, uint32_t n_seg, uint64_t* counts, hipStream_t s) {
    if (!n_seg) return hipSuccess;
    hipLaunchKernelGGL(k_abund_chunk_counts, blocks(n_seg), dim3(256), 0, s, off, n_seg, counts);
    return hipGetLastError();
}
hipError_t launch_abund_chunk_map(const uint64_t* chunk_off, uint32_t n_seg, uint32_t* chunk_seg, hipStream_t s) {
    if (!n_seg) return hipSuccess;
    hipLaunchKernelGGL(k_abund_chunk_map, blocks(n_seg), dim3(256), 0, s, chunk_off, n_seg, chunk_seg);
    return hipGetLastError();
}
hipError_t launch_abund_msum(const double* w, const uint32_t* perm, const uint32_t* off, const uint64_t* chunk_off, const uint32_t* chunk_seg,
                             uint32_t n_chunks, double* partial, hipStream_t s) {
    if (!n_chunks) return hipSuccess;
    hipLaunchKernelGGL(k_abund_msum, dim3((n_chunks + 3u) / 4u), dim3(256), 0, s, w, perm, off, chunk_off, chunk_seg, n_chunks, partial);
    return hipGetLastError();
}
hipError_t launch_abund_mfinish(const double* partial, const uint64_t* chunk_off, uint32_t n_seg, double* sum, double* block_part, double* total, hipStream_t s) {
    if (!n_seg) return hipMemsetAsync(total, 0, 8, s);
    const uint32_t nb = (n_seg + 255u) / 256u;
    hipLaunchKernelGGL(k_abund_mfinish, dim3(nb), dim3(256), 0, s, partial, chunk_off, n_seg, sum, block_part);
    hipLaunchKernelGGL(k_abund_mtotal, dim3(1), dim3(256), 0, s, block_part, nb, total);
    return hipGetLastError();
}
hipError_t launch_abund_estep(const uint32_t* hit_off, const uint32_t* hit_tid, uint32_t n_surv, const double* sum, const double* total, double* w, hipStream_t s) {
    if (!n_surv) return hipSuccess;
    hipLaunchKernelGGL(k_abund_estep, blocks(n_surv), dim3(256), 0, s, hit_off, hit_tid, n_surv, sum, total, w);
    return hipGetLastError();
}
hipError_t launch_abund_scale(const double* sum, const double* total, uint32_t n, double* out, hipStream_t s) {
    if (!n) return hipSuccess;
    hipLaunchKernelGGL(k_abund_scale, blocks(n), dim3(256), 0, s, sum, total, n, out);
    return hipGetLastError();
}
hipError_t launch_abund_gather_cells(const uint32_t* surv_read, const uint32_t* read_cell, uint32_t n_surv, uint32_t* cell, hipStream_t s) {
    if (!n_surv) return hipSuccess;
    hipLaunchKernelGGL(k_abund_gather_cells, blocks(n_surv), dim3(256), 0, s, surv_read, read_cell, n_surv, cell);
    return hipGetLastError();
}
hipError_t launch_abund_cells(uint64_t seed, const double* cdf, const uint32_t* cell_of, uint32_t n_cdf, uint32_t n_surv, uint32_t* cell, hipStream_t s) {
    if (!n_surv || !n_cdf) return hipSuccess;
    hipLaunchKernelGGL(k_abund_cells, blocks(n_surv), dim3(256), 0, s, seed, cdf, cell_of, n_cdf, n_surv, cell);
    return hipGetLastError();
}
hipError_t launch_abund_keys(const uint32_t* hit_tid, const uint32_t* hit_read, const uint32_t* cell, uint32_t n_hits, uint64_t* key, hipStream_t s) {
    if (!n_hits) return hipSuccess;
    hipLaunchKernelGGL(k_abund_keys, blocks(n_hits), dim3(256), 0, s, hit_tid, hit_read, cell, n_hits, key);
    return hipGetLastError();
}
hipError_t launch_abund_ranks(const uint32_t* perm, const uint32_t* off, uint32_t n_seg, uint32_t* rank, hipStream_t s) {
    if (!n_seg) return hipSuccess;
    hipLaunchKernelGGL(k_abund_ranks, blocks(n_seg), dim3(256), 0, s, perm, off, n_seg, rank);
    return hipGetLastError();
}

}  // namespace tk
