// abund_kernels.h -- device side of abundance (py/transcript_abundance.py:210-302): the compatibility pass over the reads' record
// segments, the transposed (by transcript) index of the hits, the EM round as ordered sums, the split by (transcript, cell) and the
// --cb-count cell draws.  Every floating-point sum has an order that depends on the input alone: no floating-point atomics.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace tk {

constexpr uint32_t ABUND_CHUNK = 1024;             // hits per chunk partial of a segment sum (fixed: part of the order of addition)
constexpr uint32_t ABUND_NO_READ = 0xFFFFFFFFu;

// get_compatibility (:210-256), pass 1: one lane per read over its records [rec_off[r], rec_off[r + 1]).  best[r] = best num_matches |
// best_is_full_length << 31; packed[r] = kept << 32 | hits (one u64 scan ranks the surviving reads and places their hits).
// bad_read: the lowest read whose division the reference cannot do (length 0; 0 best matches behind the 0.5 gate), else ABUND_NO_READ.
hipError_t launch_abund_compat(const uint32_t* rec_off, const uint32_t* tstart, const uint32_t* nmatch, const uint32_t* blen, const uint32_t* qlen,
                               uint32_t n_reads, uint32_t* best, uint64_t* packed, uint32_t* bad_read, hipStream_t s);
// pass 2, after the scan: surv_read[k] = r, hit_off[k], and the hits (tid, 1 / hits, k) in read and record order; hit_off[n_surv] = n_hits
hipError_t launch_abund_hits(const uint32_t* rec_off, const uint32_t* tid, const uint32_t* tstart, const uint32_t* nmatch, uint32_t n_reads,
                             const uint32_t* best, const uint64_t* packed, const uint64_t* scanned, uint32_t* surv_read, uint32_t* hit_off,
                             uint32_t* hit_tid, uint32_t* hit_read, double* w, hipStream_t s);

// A stable sort of (key, value) pairs (rocprim radix sort over bits [0, end_bit) of the key): with vals = 0 .. n - 1 (launch_abund_iota),
// vals_sorted is the permutation that orders by key and keeps input order among equal keys.  temp == nullptr: only *temp_bytes is set.
hipError_t launch_abund_iota(uint32_t* out, uint32_t n, hipStream_t s);
hipError_t abund_sort_u32(void* temp, size_t* temp_bytes, const uint32_t* keys, uint32_t* keys_sorted, const uint32_t* vals, uint32_t* vals_sorted, uint32_t n,
                          int end_bit, hipStream_t s);
hipError_t abund_sort_u64(void* temp, size_t* temp_bytes, const uint64_t* keys, uint64_t* keys_sorted, const uint32_t* vals, uint32_t* vals_sorted, uint32_t n,
                          int end_bit, hipStream_t s);
// off[t] = the first position of key t in sorted[n] (the next key's when t has none), t = 0 .. n_keys; off[n_keys] = n
hipError_t launch_abund_dense_offsets(const uint32_t* sorted, uint32_t n, uint32_t n_keys, uint32_t* off, hipStream_t s);
// segments of equal 64-bit keys: flag[i] = 1 where a segment starts; after the scan, off[seg] = i, key[seg], off[n_seg] = n
hipError_t launch_abund_seg_flags(const uint64_t* sorted, uint32_t n, uint64_t* flag, hipStream_t s);
hipError_t launch_abund_seg_write(const uint64_t* sorted, uint32_t n, const uint64_t* flag, const uint64_t* scanned, uint32_t* off, uint64_t* key, hipStream_t s);
// chunks of a segmented sum: n_chunks[g] = ceil(|segment g| / ABUND_CHUNK) as u64 (scanned by the caller); chunk_seg[c] = g
hipError_t launch_abund_chunk_counts(const uint32_t* off, uint32_t n_seg, uint64_t* counts, hipStream_t s);
hipError_t launch_abund_chunk_map(const uint64_t* chunk_off, uint32_t n_seg, uint32_t* chunk_seg, hipStream_t s);

// M-step (calculate_abundance :260-275, calculate_split_abundance :292-302) over segments of perm: partial[c] = the sum of w[perm[i]] over
// chunk c -- 64 lane sums, lane l taking positions l, l + 64, ... in order, folded by the tree 32, 16, ..., 1 -- then sum[g] = the
// partials of g in chunk order, and total[0] = the sums in segment order folded by fixed trees of 256 (block_part: ceil(n_seg / 256)).
hipError_t launch_abund_msum(const double* w, const uint32_t* perm, const uint32_t* off, const uint64_t* chunk_off, const uint32_t* chunk_seg,
                             uint32_t n_chunks, double* partial, hipStream_t s);
hipError_t launch_abund_mfinish(const double* partial, const uint64_t* chunk_off, uint32_t n_seg, double* sum, double* block_part, double* total, hipStream_t s);
// E-step (update_compatibility :279-289): one lane per surviving read; a_i = sum[tid_i] / total, w_i = a_i / (a_0 + a_1 + ... in hit order)
hipError_t launch_abund_estep(const uint32_t* hit_off, const uint32_t* hit_tid, uint32_t n_surv, const double* sum, const double* total, double* w, hipStream_t s);
// out[g] = sum[g] / total
hipError_t launch_abund_scale(const double* sum, const double* total, uint32_t n, double* out, hipStream_t s);

// cells: cell[k] = read_cell[surv_read[k]] (--lr-br), or the inverse-CDF draw of --cb-count: u = x / 2^32, x the first word of
// Philox(seed, k, stream 60, 0); b = the first entry with cdf[b] > u * cdf[n_cdf - 1] (the last when none); cell[k] = cell_of[b]
hipError_t launch_abund_gather_cells(const uint32_t* surv_read, const uint32_t* read_cell, uint32_t n_surv, uint32_t* cell, hipStream_t s);
hipError_t launch_abund_cells(uint64_t seed, const double* cdf, const uint32_t* cell_of, uint32_t n_cdf, uint32_t n_surv, uint32_t* cell, hipStream_t s);
// key[h] = tid << 32 | cell of the hit's read
hipError_t launch_abund_keys(const uint32_t* hit_tid, const uint32_t* hit_read, const uint32_t* cell, uint32_t n_hits, uint64_t* key, hipStream_t s);
// first-appearance rank of a segment: its lowest hit index perm[off[g]] (stable sort), ABUND_NO_READ for an empty one
hipError_t launch_abund_ranks(const uint32_t* perm, const uint32_t* off, uint32_t n_seg, uint32_t* rank, hipStream_t s);

}  // namespace tk
