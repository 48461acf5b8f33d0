// map_align_kernels.hip -- device side of map -c (see map_align_kernels.h; the rules are stated in include/tksmseq.h, "map, alignment").
#include "map_align_kernels.h"

namespace tk {

namespace {

#define DEV __device__ __forceinline__

constexpr int ALN_INF = 1 << 29;                   // an allowed cell nothing reaches (adding 1 stays in range; every real cost is below 2^18)

DEV int uni(int v) { return __builtin_amdgcn_readfirstlane(v); }
DEV uint64_t lane_u64(uint64_t v, int l) {         // the value of lane l, l the same in the whole wave
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, l), hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), l);
    return (uint64_t)hi << 32 | lo;
}
// letter g of a packed sequence: its code, or 4 when it is outside ACGT
DEV uint32_t aln_letter(const uint32_t* __restrict__ codes, const uint32_t* __restrict__ valid, uint64_t voff, uint32_t g) {
    const uint32_t ok = (valid[voff + (g >> 5)] >> (g & 31u)) & 1u;
    return ok ? (codes[2ull * voff + (g >> 4)] >> (2u * (g & 15u))) & 3u : 4u;
}
// i in [lo, lo + 64) with i % 64 = lane
DEV int owned(int lo, uint32_t lane) { return lo + (int)((lane - (uint32_t)lo) & 63u); }

}  // namespace

// One lane per line.  The end anchor is found by its key in the sorted group; the predecessors lead back from it, and the anchors are
// written from the line's last slot down, which leaves them in chain order.
__global__ void __launch_bounds__(256) k_map_align_path(const MapAlnLine* __restrict__ lines, uint32_t n_lines, const MapChain* __restrict__ chain,
                                                        const uint32_t* __restrict__ list, const uint32_t* __restrict__ gstart, const uint64_t* __restrict__ k1,
                                                        const uint32_t* __restrict__ pred, uint32_t k, uint64_t* __restrict__ path, uint32_t* __restrict__ longest,
                                                        uint32_t* __restrict__ flags) {
    const uint32_t l = blockIdx.x * 256u + threadIdx.x;
    if (l >= n_lines) return;
    const MapAlnLine L = lines[l];
    const MapChain c = chain[L.chain];
    const uint32_t g = list[L.chain], b = gstart[g], n = gstart[g + 1] - b;
    const uint64_t want = (uint64_t)(c.tend - k) << 31 | (c.qe - k);
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (k1[b + mid] < want) lo = mid + 1u; else hi = mid;
    }
    if (lo >= n || k1[b + lo] != want) { atomicOr(flags, MAP_ALN_E_END); return; }
    uint32_t i = lo, left = c.cnt, widest = 2u * k;
    uint64_t key = want;
    for (;;) {
        path[L.seg_off + --left] = key;
        if (!left) break;
        const uint32_t j = pred[b + i];
        if (j == MAP_NO_PRED || j >= i) break;
        const uint64_t kj = k1[b + j];
        widest = max(widest, (uint32_t)((key >> 31) - (kj >> 31)) + (uint32_t)((key & 0x7FFFFFFFu) - (kj & 0x7FFFFFFFu)));
        i = j; key = kj;
    }
    // the chain kernel counted cnt anchors on this very walk, and it starts at (tstart, qs)
    if (left || pred[b + i] < i || key != ((uint64_t)c.tstart << 31 | c.qs)) atomicOr(flags, MAP_ALN_E_PATH);
    atomicMax(longest, widest);
}

// One wave per line, the segments of the line from the last to the first, so that the columns, which a traceback gives from the end, fill
// the line's words from the top down.  In a segment lane i % 64 owns cell (i, s - i) of anti-diagonal s: the allowed cells of one
// anti-diagonal have consecutive i and there are at most 64 of them, so the lane's own value of step s - 1 is (i, j - 1), lane - 1's value
// of step s - 1 is (i - 1, j) and what the lane fetched from lane - 1 one step ago is (i - 1, j - 1).  lo, the first i the window
// [lo, lo + 64) holds, follows the lower edge of the band by at most one a step; e = lo (dt + dq) - s dt places it without a division.
__global__ void __launch_bounds__(256) k_map_align(const MapAlnLine* __restrict__ lines, uint32_t n_lines, const MapChain* __restrict__ chain,
                                                   const uint64_t* __restrict__ path, MapAlnSeqs Q, uint32_t k, uint32_t band, uint32_t eqx, uint32_t tb_stride,
                                                   uint64_t* tb_all, uint32_t* __restrict__ cols, MapAlnOut* __restrict__ out, uint32_t* __restrict__ flags) {
    const uint32_t lane = threadIdx.x & 63u, below = (lane + 63u) & 63u, n_waves = gridDim.x * 4u;
    const uint32_t wave = (uint32_t)uni((int)(blockIdx.x * 4u + (threadIdx.x >> 6)));     // (said to be one value in the wave: the line's tables are then read once, not by every lane)
    uint64_t* tb = tb_all + 2ull * tb_stride * wave;
    // (the lines go round the waves: a line counter fetched by lane 0 and handed round would need the wave to be back together at the fetch,
    // which nothing promises after the lane-0 stores that end a line)
    for (uint32_t l = wave; l < n_lines; l += n_waves) {
        const MapAlnLine L = lines[l];
        const MapChain c = chain[L.chain];
        const uint32_t rel = c.tr & 1u;
        const MapSeq ts = Q.tseqs[c.tr >> 1], qs = Q.qseqs[c.read];
        uint32_t* lcols = cols + L.col_off;
        // the state of the line's columns: x is the next (lower) column to write
        uint32_t x = L.cap, acc = 0, n_eq = 0, n_x = 0, n_ins = 0, n_del = 0, runs = 0, last_op = 4, err = 0;
        uint64_t cells = 0;
        for (uint32_t sg = c.cnt; sg-- > 0 && !err;) {
            const uint64_t a0 = path[L.seg_off + sg], a1 = sg + 1u < c.cnt ? path[L.seg_off + sg + 1u] : a0 + ((uint64_t)k << 31 | k);
            const int p0 = uni((int)(a0 >> 31)), q0 = uni((int)(a0 & 0x7FFFFFFFu));
            const int dt = uni((int)(a1 >> 31)) - p0, dq = uni((int)(a1 & 0x7FFFFFFFu)) - q0;
            if (dt <= 0 || dq <= 0 || (uint32_t)dt > 65536u || (uint32_t)dq > 65536u || (uint32_t)(dt + dq) >= tb_stride || (uint32_t)(dt + dq) > x ||
                (uint32_t)(p0 + dt) > ts.len || (uint32_t)(q0 + dq) > qs.len) { err = MAP_ALN_E_SEGMENT; break; }
            const int S = dt + dq;
            const int64_t width = (int64_t)band * S;
            // ---- the cells, anti-diagonal by anti-diagonal
            int lo = 0, lo1 = 0, lo2 = 0;                                    // the window of this step and of the two before it
            int64_t e = 0;
            int v1 = ALN_INF, fetched = ALN_INF;                             // the lane's value of step s - 1; lane - 1's of step s - 2
            int t_at = -1, q_at = -1;                                        // what tl and the read words hold
            uint32_t tl = 4, qv = 0;
            uint64_t qw = 0;
            for (int s = 0; s <= S; s++) {
                const int i = owned(lo, lane), j = s - i;
                const int64_t ei = e + (int64_t)(i - lo) * S;
                const bool allowed = i <= min(dt, s) && 2 * (ei < 0 ? -ei : ei) <= width;
                const int up = __shfl(v1, (int)below, 64);                    // (i - 1, j) when lane - 1 owned i - 1 one step ago
                int val = ALN_INF;
                uint32_t code = 0;
                if (allowed) {
                    if (s == 0) val = 0;
                    else {
                        int d = ALN_INF, u = ALN_INF, w = ALN_INF;
                        uint32_t miss = 1;
                        if (i > 0 && j > 0) {
                            if (t_at != i) { tl = aln_letter(Q.tcodes, Q.tvalid, ts.voff, (uint32_t)(p0 + i - 1)); t_at = i; }
                            const uint32_t at = (uint32_t)(q0 + j - 1), r = rel ? qs.len - 1u - at : at;
                            if (q_at != (int)(r >> 5)) {
                                q_at = (int)(r >> 5);
                                qw = *reinterpret_cast<const uint64_t*>(Q.qcodes + 2ull * qs.voff + 2u * (r >> 5));
                                qv = Q.qvalid[qs.voff + (r >> 5)];
                            }
                            const uint32_t qc = (uint32_t)(qw >> (2u * (r & 31u))) & 3u;
                            miss = ((qv >> (r & 31u)) & 1u) && tl == (rel ? 3u - qc : qc) ? 0u : 1u;
                            if (owned(lo2, below) == i - 1) d = fetched + (int)miss;
                        }
                        if (i > 0 && owned(lo1, below) == i - 1) u = up + 1;
                        if (j > 0 && owned(lo1, lane) == i) w = v1 + 1;
                        val = min(min(d, u), min(w, ALN_INF));
                        code = d == val ? miss : u == val ? 3u : 2u;
                    }
                }
                const unsigned long long b0 = __ballot(allowed && (code & 1u)), b1 = __ballot(allowed && (code & 2u));
                cells += (uint32_t)__popcll(__ballot(allowed));
                if (lane == 0) { tb[2 * s] = b0; tb[2 * s + 1] = b1; }
                fetched = up; v1 = val;
                lo2 = lo1; lo1 = lo;
                e -= dt;
                if (2 * e < -width || lo < s + 1 - dq) { lo++; e += S; }
            }
            if (uni(__shfl(v1, dt & 63, 64)) >= ALN_INF) { err = MAP_ALN_E_TRACE; break; }
            __threadfence();
            // ---- the way back (the same in every lane; lane 0 writes).  Lane t holds the bits of anti-diagonal top - t.
            int i = dt, j = dq, top = -1;
            uint64_t t0 = 0, t1 = 0;
            while (i > 0 || j > 0) {
                const int s = i + j;
                if (top < 0 || top - s > 63) {
                    top = s;
                    const int mine = s - (int)lane;
                    if (mine >= 0) {                                          // (read past the vector L1: the wave has just written them)
                        t0 = __hip_atomic_load(tb + 2 * mine, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        t1 = __hip_atomic_load(tb + 2 * mine + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    }
                }
                const uint32_t code = (uint32_t)((lane_u64(t0, top - s) >> (i & 63)) & 1u) | (uint32_t)((lane_u64(t1, top - s) >> (i & 63)) & 1u) << 1;
                if (code < 2u ? (i <= 0 || j <= 0) : code == 3u ? i <= 0 : j <= 0) { err = MAP_ALN_E_TRACE; break; }
                if (code < 2u) { i--; j--; } else if (code == 3u) i--; else j--;
                const uint32_t op = eqx || code >= 2u ? code : 0u;
                n_eq += code == 0u; n_x += code == 1u; n_ins += code == 2u; n_del += code == 3u;
                runs += op != last_op ? 1u : 0u;
                last_op = op;
                x--;                                                          // (x > 0: a segment has at most dt + dq columns, checked against x above)
                acc |= code << (2u * (x & 15u));
                if ((x & 15u) == 0u) { if (lane == 0) lcols[x >> 4] = acc; acc = 0; }
            }
        }
        if ((x & 15u) != 0u && lane == 0) lcols[x >> 4] = acc;
        if (lane == 0) {
            if (err) atomicOr(flags, err);
            MapAlnOut o;
            o.ncols = L.cap - x; o.eq = n_eq; o.x = n_x; o.ins = n_ins; o.del = n_del; o.runs = err ? 0u : runs; o.cells = cells;
            out[l] = o;
        }
    }
}

// One wave per line, 64 columns a step: a column that differs from the one before it starts a run.
__global__ void __launch_bounds__(256) k_map_align_encode(const MapAlnLine* __restrict__ lines, uint32_t n_lines, const MapAlnOut* __restrict__ out,
                                                          const uint32_t* __restrict__ cols, const uint64_t* __restrict__ run_off, uint32_t eqx, uint64_t* __restrict__ runs) {
    const uint32_t l = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    if (l >= n_lines) return;
    const MapAlnLine L = lines[l];
    const uint32_t n = out[l].ncols, first = L.cap - n, n_runs = (uint32_t)(run_off[l + 1] - run_off[l]);
    const uint32_t* lcols = cols + L.col_off;
    uint64_t* o = runs + run_off[l];
    uint32_t before = 4, done = 0;                                            // the op of the column before this step; runs written
    for (uint32_t base = 0; base < n; base += 64u) {
        const uint32_t at = base + lane;
        uint32_t op = 4;
        if (at < n) {
            const uint32_t xx = first + at, code = (lcols[xx >> 4] >> (2u * (xx & 15u))) & 3u;
            op = eqx || code >= 2u ? code : 0u;
        }
        const uint32_t prev_lane = (uint32_t)__shfl((int)op, (int)((lane + 63u) & 63u), 64);
        const uint32_t prev = lane ? prev_lane : before;
        const bool start = at < n && op != prev;
        const unsigned long long ballot = __ballot(start);
        const uint32_t rank = done + (uint32_t)__popcll(ballot & ((1ull << lane) - 1ull));
        if (start && rank < n_runs) o[rank] = (uint64_t)at << 2 | op;
        done += (uint32_t)__popcll(ballot);
        before = (uint32_t)__shfl((int)op, 63, 64);
    }
}

hipError_t launch_map_align_path(const MapAlnLine* lines, uint32_t n_lines, const MapChain* chain, const uint32_t* list, const uint32_t* gstart, const uint64_t* k1,
                                 const uint32_t* pred, uint32_t k, uint64_t* path, uint32_t* longest, uint32_t* flags, hipStream_t s) {
    if (!n_lines) return hipSuccess;
    hipLaunchKernelGGL(k_map_align_path, dim3((n_lines + 255u) / 256u), dim3(256), 0, s, lines, n_lines, chain, list, gstart, k1, pred, k, path, longest, flags);
    return hipGetLastError();
}
hipError_t launch_map_align(const MapAlnLine* lines, uint32_t n_lines, const MapChain* chain, const uint64_t* path, const MapAlnSeqs& Q, uint32_t k, uint32_t band,
                            uint32_t eqx, uint32_t n_waves, uint32_t tb_stride, uint64_t* tb, uint32_t* cols, MapAlnOut* out, uint32_t* flags,
                            hipStream_t s) {
    if (!n_lines || !n_waves) return hipSuccess;
    // whole workgroups of four waves: the caller's store holds n_waves rounded up to four
    hipLaunchKernelGGL(k_map_align, dim3((n_waves + 3u) / 4u), dim3(256), 0, s, lines, n_lines, chain, path, Q, k, band, eqx, tb_stride, tb, cols, out, flags);
    return hipGetLastError();
}
hipError_t launch_map_align_encode(const MapAlnLine* lines, uint32_t n_lines, const MapAlnOut* out, const uint32_t* cols, const uint64_t* run_off, uint32_t eqx,
                                   uint64_t* runs, hipStream_t s) {
    if (!n_lines) return hipSuccess;
    hipLaunchKernelGGL(k_map_align_encode, dim3((n_lines + 3u) / 4u), dim3(256), 0, s, lines, n_lines, out, cols, run_off, eqx, runs);
    return hipGetLastError();
}

}  // namespace tk
