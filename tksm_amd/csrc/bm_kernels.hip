// bm_kernels.hip -- device side of barcode-match (see bm_kernels.h; the rules are stated in include/tksmseq.h).  Both alignments are the
// bit-parallel column step of Myers (1999) in its search form (row 0 all zeros), the pattern in one 32-bit word: bits above the pattern's
// last row hold garbage that never reaches the rows below, because carries and shifts only move upwards.
#include "bm_kernels.h"

namespace tk {

namespace {

// one text column: eq = the pattern rows that match the column's letter.  Returns the change of the bottom row's score (top: its bit).
__device__ __forceinline__ int bm_column(uint32_t eq, uint32_t& pv, uint32_t& mv, uint32_t top_shift) {
    const uint32_t xv = eq | mv;
    const uint32_t xh = (((eq & pv) + pv) ^ pv) | eq;
    uint32_t ph = mv | ~(xh | pv);
    uint32_t mh = pv & xh;
    const int delta = (int)((ph >> top_shift) & 1u) - (int)((mh >> top_shift) & 1u);
    ph <<= 1;
    mh <<= 1;
    pv = mh | ~(xv | ph);
    mv = ph & xv;
    return delta;
}

__device__ __forceinline__ uint32_t bm_pick(uint32_t c, uint32_t p0, uint32_t p1, uint32_t p2, uint32_t p3) {
    return (c & 2u) ? ((c & 1u) ? p3 : p2) : ((c & 1u) ? p1 : p0);
}

}  // namespace

__global__ void __launch_bounds__(256) k_bm_adapter(BmEnds E, BmAdapter A, BmSeg* __restrict__ seg) {
    const uint32_t n2 = 2u * E.n_reads;
    const uint32_t lane = blockIdx.x * 256u + threadIdx.x;
    const bool live = lane < n2;
    const uint32_t me = live ? lane : 0u;
    const uint32_t len = live ? E.len[me >> 1] : 0u;
    const uint32_t ncol = min(A.window, len);
    const uint32_t top_shift = A.m - 1u;
    uint32_t pv = ~0u, mv = 0u, cw = 0u, vw = 0u;
    int score = (int)A.m, best = (int)A.m;
    uint32_t end = 0u;
    for (uint32_t j = 0; j < ncol; j++) {
        if ((j & 15u) == 0u) cw = E.codes[(size_t)(j >> 4) * n2 + me];
        if ((j & 31u) == 0u) vw = E.valid[(size_t)(j >> 5) * n2 + me];
        const uint32_t eq = (vw & 1u) ? bm_pick(cw & 3u, A.peq[0], A.peq[1], A.peq[2], A.peq[3]) : 0u;
        cw >>= 2; vw >>= 1;
        score += bm_column(eq, pv, mv, top_shift);
        if (score < best) { best = score; end = j + 1u; }
    }
    // the two orientations of a read sit in neighbouring lanes of one wave (every lane of the wave gets here)
    const int other = __shfl_xor(best, 1);
    const bool wins = (me & 1u) ? best < other : best <= other;
    if (!live || !wins) return;
    BmSeg out{};
    if ((uint32_t)best <= A.max_errors) {
        const uint32_t start = end > A.pad ? end - A.pad : 0u;
        const uint32_t stop = min(len, end + A.L + A.pad);
        const uint32_t n = stop - start;              // at most L + 2 pad <= BM_SEG_MAX
        uint64_t lo = 0, hi = 0, ok = 0;
        for (uint32_t k = 0; k < n; k++) {
            const uint32_t pos = start + k;
            const uint64_t c = (E.codes[(size_t)(pos >> 4) * n2 + me] >> ((pos & 15u) * 2u)) & 3u;
            const uint64_t v = (E.valid[(size_t)(pos >> 5) * n2 + me] >> (pos & 31u)) & 1u;
            if (k < 32u) lo |= c << (2u * k); else hi |= c << (2u * (k - 32u));
            ok |= v << k;
        }
        out.code[0] = (uint32_t)lo; out.code[1] = (uint32_t)(lo >> 32); out.code[2] = (uint32_t)hi; out.code[3] = (uint32_t)(hi >> 32);
        out.valid[0] = (uint32_t)ok; out.valid[1] = (uint32_t)(ok >> 32);
        out.meta = n | ((me & 1u) ? BM_META_REV : 0u) | BM_META_ADAPTER | (uint32_t)best << 16;
        out.start = start;
    }
    seg[me >> 1] = out;
}

__global__ void __launch_bounds__(256) k_bm_exact(const BmSeg* __restrict__ seg, uint32_t n_reads, const uint64_t* __restrict__ keys_sorted,
                                                  const uint32_t* __restrict__ perm, uint32_t n_keys, uint32_t L, unsigned long long* __restrict__ exact) {
    const uint32_t r = blockIdx.x * 256u + threadIdx.x;
    if (r >= n_reads) return;
    const BmSeg sg = seg[r];
    const uint32_t len = sg.meta & BM_META_LEN;
    if (!(sg.meta & BM_META_ADAPTER) || len < L) return;
    uint64_t lo = (uint64_t)sg.code[1] << 32 | sg.code[0], hi = (uint64_t)sg.code[3] << 32 | sg.code[2], ok = (uint64_t)sg.valid[1] << 32 | sg.valid[0];
    uint64_t key = 0;
    uint32_t run = 0;
    const uint32_t put = 2u * (L - 1u);
    for (uint32_t j = 0; j < len; j++) {
        key = (key >> 2) | ((lo & 3ull) << put);
        run = (ok & 1ull) ? run + 1u : 0u;
        lo = (lo >> 2) | (hi << 62); hi >>= 2; ok >>= 1;
        if (run < L) continue;
        uint32_t a = 0, b = n_keys;                   // lower bound
        while (a < b) {
            const uint32_t mid = a + (b - a) / 2u;
            if (keys_sorted[mid] < key) a = mid + 1u; else b = mid;
        }
        if (a < n_keys && keys_sorted[a] == key) atomicAdd(&exact[perm[a]], 1ull);
    }
}

__global__ void __launch_bounds__(256) k_bm_cand_flags(const unsigned long long* __restrict__ exact, uint32_t n_keys, uint64_t min_exact, uint64_t* __restrict__ flag) {
    const uint32_t b = blockIdx.x * 256u + threadIdx.x;
    if (b < n_keys) flag[b] = exact[b] >= min_exact ? 1ull : 0ull;
}

__global__ void __launch_bounds__(256) k_bm_cand_write(const uint64_t* __restrict__ keys, const uint64_t* __restrict__ flag, const uint64_t* __restrict__ scanned,
                                                       uint32_t n_keys, uint32_t L, uint32_t* __restrict__ cand, uint4* __restrict__ cand_peq) {
    const uint32_t b = blockIdx.x * 256u + threadIdx.x;
    if (b >= n_keys || !flag[b]) return;
    const uint64_t key = keys[b];
    uint4 p = make_uint4(0u, 0u, 0u, 0u);
    for (uint32_t i = 0; i < L; i++) {
        const uint32_t c = (uint32_t)(key >> (2u * i)) & 3u, bit = 1u << i;
        if (c == 0u) p.x |= bit; else if (c == 1u) p.y |= bit; else if (c == 2u) p.z |= bit; else p.w |= bit;
    }
    const uint64_t rank = scanned[b];
    cand[rank] = b;
    cand_peq[rank] = p;
}

// The hot path.  A lane holds its segment (four code words, two validity words) and the column state in registers; the candidate's four match
// masks are the same for the whole wave and come through scalar loads.  The list of a read goes straight to memory: a store happens only
// when a candidate reaches the read's running minimum, which is rare next to the column steps.
__global__ void __launch_bounds__(256) k_bm_match(const BmSeg* __restrict__ seg, uint32_t n_reads, const uint4* __restrict__ cand_peq, uint32_t n_cand,
                                                  uint32_t per_split, uint32_t L, uint32_t max_errors, uint32_t* __restrict__ part_d,
                                                  uint32_t* __restrict__ part_n, uint32_t* __restrict__ part_idx) {
    const uint32_t r = blockIdx.x * 256u + threadIdx.x;
    const bool live = r < n_reads;
    BmSeg sg{};
    if (live) sg = seg[r];
    const uint32_t len = (sg.meta & BM_META_ADAPTER) ? (sg.meta & BM_META_LEN) : 0u;
    const uint32_t b0 = blockIdx.y * per_split, b1 = min(n_cand, b0 + per_split);
    const size_t slot = (size_t)blockIdx.y * n_reads + r;
    const uint32_t top_shift = L - 1u;
    uint32_t dmin = max_errors + 1u, cnt = 0u;
    // (a wave whose lanes all lack a segment has nothing to compare)
    uint32_t wave_cols = len;
    for (int d = 1; d < 64; d <<= 1) wave_cols = max(wave_cols, (uint32_t)__shfl_xor((int)wave_cols, d));
    wave_cols = (uint32_t)__builtin_amdgcn_readfirstlane((int)wave_cols);
    for (uint32_t b = b0; b < b1 && wave_cols; b++) {
        const uint4 m = cand_peq[b];
        uint32_t pv = ~0u, mv = 0u;
        int score = (int)L, best = (int)L;
#pragma unroll
        for (uint32_t w = 0; w < 4u; w++) {
            uint32_t cw = sg.code[w], vw = sg.valid[w >> 1] >> ((w & 1u) * 16u);
            if (w * 16u >= wave_cols) break;
            const uint32_t cols = min(16u, wave_cols - w * 16u);
            for (uint32_t k = 0; k < cols; k++) {
                const uint32_t eq = (vw & 1u) ? bm_pick(cw & 3u, m.x, m.y, m.z, m.w) : 0u;
                cw >>= 2; vw >>= 1;
                score += bm_column(eq, pv, mv, top_shift);
                if (w * 16u + k < len) best = min(best, score);
            }
        }
        if (!live) continue;
        if ((uint32_t)best < dmin) { dmin = (uint32_t)best; cnt = 1u; part_idx[slot * BM_LIST] = b; }
        else if ((uint32_t)best == dmin && dmin <= max_errors) { if (cnt < (uint32_t)BM_LIST) part_idx[slot * BM_LIST + cnt] = b; cnt++; }
    }
    if (live) { part_d[slot] = dmin; part_n[slot] = cnt; }
}

__global__ void __launch_bounds__(256) k_bm_merge(const uint32_t* __restrict__ part_d, const uint32_t* __restrict__ part_n, const uint32_t* __restrict__ part_idx,
                                                  uint32_t n_reads, uint32_t n_splits, uint32_t max_errors, uint32_t* __restrict__ res_d,
                                                  uint32_t* __restrict__ res_n, uint32_t* __restrict__ res_idx) {
    const uint32_t r = blockIdx.x * 256u + threadIdx.x;
    if (r >= n_reads) return;
    uint32_t dmin = max_errors + 1u, cnt = 0u, k = 0u;
    for (uint32_t y = 0; y < n_splits; y++) {
        const size_t slot = (size_t)y * n_reads + r;
        const uint32_t d = part_d[slot], n = part_n[slot];
        if (!n) continue;
        if (d < dmin) { dmin = d; cnt = 0u; k = 0u; }
        if (d != dmin) continue;
        for (uint32_t i = 0; i < min(n, (uint32_t)BM_LIST) && k < (uint32_t)BM_LIST; i++) res_idx[(size_t)r * BM_LIST + k++] = part_idx[slot * BM_LIST + i];
        cnt += n;
    }
    for (; k < (uint32_t)BM_LIST; k++) res_idx[(size_t)r * BM_LIST + k] = 0xFFFFFFFFu;
    res_d[r] = dmin;
    res_n[r] = cnt;
}

static inline uint32_t bm_blocks(uint64_t n) { return (uint32_t)((n + 255u) / 256u); }

hipError_t launch_bm_adapter(const BmEnds& E, const BmAdapter& A, BmSeg* seg, hipStream_t s) {
    if (!E.n_reads) return hipSuccess;
    k_bm_adapter<<<bm_blocks(2ull * E.n_reads), 256, 0, s>>>(E, A, seg);
    return hipGetLastError();
}
hipError_t launch_bm_exact(const BmSeg* seg, uint32_t n_reads, const uint64_t* keys_sorted, const uint32_t* perm, uint32_t n_keys, uint32_t L,
                           unsigned long long* exact, hipStream_t s) {
    if (!n_reads || !n_keys) return hipSuccess;
    k_bm_exact<<<bm_blocks(n_reads), 256, 0, s>>>(seg, n_reads, keys_sorted, perm, n_keys, L, exact);
    return hipGetLastError();
}
hipError_t launch_bm_cand_flags(const unsigned long long* exact, uint32_t n_keys, uint64_t min_exact, uint64_t* flag, hipStream_t s) {
    if (!n_keys) return hipSuccess;
    k_bm_cand_flags<<<bm_blocks(n_keys), 256, 0, s>>>(exact, n_keys, min_exact, flag);
    return hipGetLastError();
}
hipError_t launch_bm_cand_write(const uint64_t* keys, const uint64_t* flag, const uint64_t* scanned, uint32_t n_keys, uint32_t L, uint32_t* cand, uint4* cand_peq,
                                hipStream_t s) {
    if (!n_keys) return hipSuccess;
    k_bm_cand_write<<<bm_blocks(n_keys), 256, 0, s>>>(keys, flag, scanned, n_keys, L, cand, cand_peq);
    return hipGetLastError();
}
uint32_t bm_split_size(uint32_t n_reads, uint32_t n_cand) {
    const uint32_t read_waves = (n_reads + 63u) / 64u;
    const uint32_t want = read_waves >= BM_TARGET_WAVES ? 1u : BM_TARGET_WAVES / (read_waves ? read_waves : 1u);
    const uint32_t per = (n_cand + want - 1u) / want;
    return ((per ? per : 1u) + BM_CAND_TILE - 1u) / BM_CAND_TILE * BM_CAND_TILE;
}
hipError_t launch_bm_match(const BmSeg* seg, uint32_t n_reads, const uint4* cand_peq, uint32_t n_cand, uint32_t per_split, uint32_t L, uint32_t max_errors,
                           uint32_t* part_d, uint32_t* part_n, uint32_t* part_idx, hipStream_t s) {
    if (!n_reads || !n_cand) return hipSuccess;
    const uint32_t n_splits = (n_cand + per_split - 1u) / per_split;
    k_bm_match<<<dim3(bm_blocks(n_reads), n_splits), 256, 0, s>>>(seg, n_reads, cand_peq, n_cand, per_split, L, max_errors, part_d, part_n, part_idx);
    return hipGetLastError();
}
hipError_t launch_bm_merge(const uint32_t* part_d, const uint32_t* part_n, const uint32_t* part_idx, uint32_t n_reads, uint32_t n_splits, uint32_t max_errors,
                           uint32_t* res_d, uint32_t* res_n, uint32_t* res_idx, hipStream_t s) {
    if (!n_reads) return hipSuccess;
    k_bm_merge<<<bm_blocks(n_reads), 256, 0, s>>>(part_d, part_n, part_idx, n_reads, n_splits, max_errors, res_d, res_n, res_idx);
    return hipGetLastError();
}

}  // namespace tk
