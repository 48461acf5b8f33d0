// ms_kernels.h -- device side of model-sequence (include/tksmseq.h): the alignment columns of every used PAF line (one wave each), the
// error-model and q-score events (one lane per reference offset / read position), the run lengths of the sorted events, the merge of two
// reduced tables and the selection of the rows the host prints.  Integers only: there is no floating point in this file.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"

namespace tk {

constexpr uint64_t MS_NO_EVENT = ~0ull;            // the key of an event slot that does not count (sorts last, dropped by the reduce)
constexpr int MS_SUBS = 96;                        // payload values of a q-score event: q 0..93, 94 / 95 the two counters under key 0
constexpr uint32_t MS_SUB_MAX_DEL = 94, MS_SUB_TOO_LONG = 95;
constexpr int MS_ALT_SLOTS = 31;
// column letters, in the order of their bytes ('=' < 'D' < 'I' < 'X'): a q-score key compares like its text
enum { MS_EQ = 0, MS_DEL = 1, MS_INS = 2, MS_MIS = 3 };
// classes of an error-model key: kmer << 30 | class << 28 | length << 24 | bases (the first in bits 23..22)
enum { MS_CLASS_SELF = 0, MS_CLASS_ALT = 1, MS_CLASS_TOTAL_ONLY = 2 };

struct MsAlnDev {
    uint64_t read_off;          // the read's first base in the pools
    uint64_t ref_g;             // global coordinate of reference base tstart
    uint32_t qlen, qstart, qend, strand, tlen, op_off, n_ops, pad;
};
// the offsets of alignments [a0, a1) in the ragged arrays of a chunk: scanned counts (launch_scan) minus the chunk's first
struct MsChunk {
    const uint64_t *col_off, *rp_off, *tp_off, *ee_off;     // [n_aln + 1]: columns, read positions, reference positions, error events
    uint64_t col_base, rp_base, tp_base, ee_base;
    uint32_t a0, a1;
};
struct MsErrRowDev { uint64_t total, self, too_long; uint32_t n_alt; uint32_t alt[MS_ALT_SLOTS]; uint64_t count[MS_ALT_SLOTS]; };
struct MsQRowDev { uint64_t key, n; uint64_t count[MS_SUBS]; };

// cols[column] = letter, rcol[read position] = column, tcol[reference position] = column (columns numbered within the alignment)
hipError_t launch_ms_expand(const MsAlnDev* aln, const uint32_t* ops, const uint8_t* bases, const RefView& R, const MsChunk& C, uint8_t* cols, uint32_t* rcol,
                            uint32_t* tcol, hipStream_t s);
// keys[e] for the n_events error events of the chunk
hipError_t launch_ms_err_events(const MsAlnDev* aln, const uint8_t* bases, const RefView& R, const MsChunk& C, const uint8_t* cols, const uint32_t* rcol,
                                const uint32_t* tcol, int k, uint64_t n_events, uint64_t* keys, hipStream_t s);
// slots = (kq + 1) / 2 + 1 events per read position: keys[p * slots + j], subs likewise (slot 0: the overall count under key 0)
hipError_t launch_ms_qs_events(const MsAlnDev* aln, const uint8_t* quals, const MsChunk& C, const uint8_t* cols, const uint32_t* rcol, int kq, int max_del,
                               uint64_t n_positions, uint64_t* keys, uint32_t* subs, hipStream_t s);

// pieces of the reduce (ms_api.cpp: sort by sub, then stable by key): out[i] = in[perm[i]]
hipError_t launch_ms_gather_u64(const uint64_t* in, const uint32_t* perm, uint32_t n, uint64_t* out, hipStream_t s);
hipError_t launch_ms_gather_u32(const uint32_t* in, const uint32_t* perm, uint32_t n, uint32_t* out, hipStream_t s);
// flag[i] = 1 where (key, sub) differs from the position before; subs may be null
hipError_t launch_ms_run_flags(const uint64_t* keys, const uint32_t* subs, uint32_t n, uint64_t* flag, hipStream_t s);
// after the scan: start[run] = i, start[n_runs] = n; info[0] = n_runs, info[1] = 1 when the last run is MS_NO_EVENT
hipError_t launch_ms_run_starts(const uint64_t* keys, uint32_t n, const uint64_t* flag, const uint64_t* scanned, uint32_t* start, uint64_t* info, hipStream_t s);
// one lane per run: its key, sub and count -- the run's length, or (vals != null) the sum of vals[perm[j]] over it
hipError_t launch_ms_run_write(const uint64_t* keys, const uint32_t* subs, const uint32_t* start, uint32_t n_runs, const uint64_t* vals, const uint32_t* perm,
                               uint64_t* okeys, uint32_t* osubs, uint64_t* ocounts, hipStream_t s);

// error model: key2[i] = (key >> 28) << 32 | (2^32 - 1 - count); bad[0] |= 1 for a count of 2^32 or more
hipError_t launch_ms_err_rank_keys(const uint64_t* keys, const uint64_t* counts, uint32_t n, uint64_t* key2, uint32_t* bad, hipStream_t s);
// one lane per k-mer over the table ordered by key2 (perm: into keys / counts)
hipError_t launch_ms_err_select(const uint64_t* key2_sorted, const uint32_t* perm, const uint64_t* keys, const uint64_t* counts, uint32_t n, int k, int max_alt,
                                MsErrRowDev* rows, hipStream_t s);
// q-score model: one lane per key run [kstart[g], kstart[g + 1]) of the (key, sub, count) table: kkey[g], kn[g] (the counts with sub < 94),
// key2[g] = ~n for a key other than 0 with n >= min_occur, else all ones; n_qual[0] counts the former
hipError_t launch_ms_qs_totals(const uint64_t* keys, const uint32_t* subs, const uint64_t* counts, const uint32_t* kstart, uint32_t n_keys, uint64_t min_occur,
                               uint64_t* kkey, uint64_t* kn, uint64_t* key2, unsigned long long* n_qual, hipStream_t s);
// rows[j] = key run ids[j] as a dense row
hipError_t launch_ms_qs_rows(const uint64_t* keys, const uint32_t* subs, const uint64_t* counts, const uint32_t* kstart, const uint32_t* ids, uint32_t n_ids,
                             uint32_t n_keys, MsQRowDev* rows, hipStream_t s);

}  // namespace tk
