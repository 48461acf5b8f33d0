// map_extend_kernels.hip -- device side of map --extend (see map_extend_kernels.h; the rules are stated in include/tksmseq.h, "map, end extension").
#include "map_extend_kernels.h"

namespace tk {

namespace {

#define DEV __device__ __forceinline__

constexpr int EXT_NEG = -(1 << 29);                // a cell that is not allowed (every real score lies above -2^18)
constexpr int EXT_MATCH = 1, EXT_MISS = -2, EXT_GAP = -2;

DEV int uni(int v) { return __builtin_amdgcn_readfirstlane(v); }
DEV uint64_t lane_u64(uint64_t v, int l) {         // the value of lane l, l the same in the whole wave
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, l), hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), l);
    return (uint64_t)hi << 32 | lo;
}
DEV int wave_max(int v) {
    for (int d = 32; d > 0; d >>= 1) v = max(v, __shfl_xor(v, d, 64));
    return v;
}

// sixteen letters of a packed sequence at a time: the code word and the validity word that hold letter g stay in registers while the
// lane walks on (forwards at a right end, backwards at a left one)
struct Letters {
    const uint32_t *codes, *valid;
    uint64_t voff;
    uint32_t at = 0xFFFFFFFFu, cw = 0, vw = 0;
    DEV Letters(const uint32_t* c, const uint32_t* v, uint64_t o) : codes(c), valid(v), voff(o) {}
    // letter g: its code, or 4 when it is outside ACGT
    DEV uint32_t operator()(uint32_t g) {
        if (at != (g >> 4)) { at = g >> 4; cw = codes[2ull * voff + at]; vw = valid[voff + (g >> 5)]; }
        return (vw >> (g & 31u)) & 1u ? (cw >> (2u * (g & 15u))) & 3u : 4u;
    }
};

// what a task is cut to: the corner in the target and in the read (in the strand of rel), and the letters beyond it
struct Cut { uint32_t tc, qc, lt, lq, rel, right, bad; };
DEV Cut cut_of(const MapExtTask& K, const MapChain& c, const MapSeq& ts, const MapSeq& qs, uint32_t max_ext) {
    Cut x;
    x.rel = c.tr & 1u; x.right = K.end & 1u;
    x.bad = c.tstart > c.tend || c.tend > ts.len || c.qs > c.qe || c.qe > qs.len ? 1u : 0u;
    x.tc = x.right ? c.tend : c.tstart; x.qc = x.right ? c.qe : c.qs;
    x.lt = x.bad ? 0u : min(max_ext, x.right ? ts.len - c.tend : c.tstart);
    x.lq = x.bad ? 0u : min(max_ext, x.right ? qs.len - c.qe : c.qs);
    return x;
}

// The cells of one task, anti-diagonal by anti-diagonal.  With par = (s + B) & 1 the lane's cell has d = i - j = 2 lane - B + par: the
// diagonal predecessor is the lane's own value of step s - 2; (i - 1, j) is lane - 1's value of step s - 1 when par = 0 and the lane's own
// when par = 1; (i, j - 1) is the lane's own when par = 0 and lane + 1's when par = 1.  A cell outside the band or the rectangle holds
// EXT_NEG, so a predecessor that is not allowed never wins.  TRACE: the anti-diagonals 1 .. s_end, two bits per cell to tb; else until
// the stop rule says so, and the best cell to `best`.
template <bool TRACE>
DEV void extend_cells(const Cut& x, const MapSeq& ts, const MapSeq& qs, const MapAlnSeqs& Q, int B, int Z, int s_end, uint32_t lane, uint64_t* tb, MapExtEnd& best) {
    const int Lt = (int)x.lt, Lq = (int)x.lq;
    Letters tl(Q.tcodes, Q.tvalid, ts.voff), ql(Q.qcodes, Q.qvalid, qs.voff);
    int h1 = (int)lane == (B >> 1) ? 0 : EXT_NEG, h2 = EXT_NEG, m1 = 0, m2 = 0;          // the lane's values of steps s - 1 and s - 2
    int top = 0, prev_mx = 0;
    best.ei = best.ej = best.m = best.steps = 0; best.cells = 0;
    const int last = TRACE ? s_end : Lt + Lq;
    for (int s = 1; s <= last; s++) {
        const int par = (s + B) & 1, d = 2 * (int)lane - B + par, i = (s + d) >> 1, j = s - i;
        const bool allowed = (int)lane <= B - par && i >= 0 && j >= 0 && i <= Lt && j <= Lq;
        const unsigned long long any = __ballot(allowed);
        if (!any) break;
        const int from = par ? (int)((lane + 1u) & 63u) : (int)((lane + 63u) & 63u);
        int nh = __shfl(h1, from, 64);
        const int nm = __shfl(m1, from, 64);
        if (par ? lane == 63u : lane == 0u) nh = EXT_NEG;
        int val = EXT_NEG, m = 0;
        uint32_t code = 0;
        if (allowed) {
            int dg = EXT_NEG;
            uint32_t miss = 1;
            if (i > 0 && j > 0) {
                const uint32_t t = tl(x.right ? x.tc + (uint32_t)(i - 1) : x.tc - (uint32_t)i);
                const uint32_t at = x.right ? x.qc + (uint32_t)(j - 1) : x.qc - (uint32_t)j;
                const uint32_t q = ql(x.rel ? qs.len - 1u - at : at);
                miss = t < 4u && q < 4u && t == (x.rel ? 3u - q : q) ? 0u : 1u;
                dg = h2 + (miss ? EXT_MISS : EXT_MATCH);
            }
            const int up = (par ? h1 : nh) + EXT_GAP, left = (par ? nh : h1) + EXT_GAP;       // (i - 1, j): a D column; (i, j - 1): an I column
            val = max(dg, max(up, left));
            code = dg == val ? miss : up == val ? 3u : 2u;
            m = dg == val ? m2 + (int)(1u - miss) : up == val ? (par ? m1 : nm) : (par ? nm : m1);
        }
        if (TRACE) {
            const unsigned long long b0 = __ballot(allowed && (code & 1u)), b1 = __ballot(allowed && (code & 2u));
            if (lane == 0) { tb[2 * s] = b0; tb[2 * s + 1] = b1; }
        } else {
            const int mx = uni(wave_max(val));
            best.steps++;
            best.cells += (uint32_t)__popcll(any);
            if (mx > 0 && mx >= top) {                                         // the later anti-diagonal wins, within it the smallest i
                const int l = __ffsll((long long)__ballot(allowed && val == mx)) - 1;
                top = mx;
                best.ei = (uint32_t)__builtin_amdgcn_readlane(i, l);
                best.ej = (uint32_t)s - best.ei;
                best.m = (uint32_t)__builtin_amdgcn_readlane(m, l);
            }
            if (max(mx, prev_mx) < top - Z) break;
            prev_mx = mx;
        }
        h2 = h1; m2 = m1; h1 = val; m1 = m;
    }
}

}  // namespace

// One wave per task, the tasks going round the waves.
__global__ void __launch_bounds__(256) k_map_extend(const MapExtTask* __restrict__ tasks, uint32_t n_tasks, const MapChain* __restrict__ chain, MapAlnSeqs Q, MapExtParams P,
                                                    MapExtEnd* __restrict__ ends, uint32_t* __restrict__ flags) {
    const uint32_t lane = threadIdx.x & 63u, n_waves = gridDim.x * 4u;
    const uint32_t wave = (uint32_t)uni((int)(blockIdx.x * 4u + (threadIdx.x >> 6)));
    for (uint32_t e = wave; e < n_tasks; e += n_waves) {
        const MapExtTask K = tasks[e];
        const MapChain c = chain[K.chain];
        const MapSeq ts = Q.tseqs[c.tr >> 1], qs = Q.qseqs[c.read];
        const Cut x = cut_of(K, c, ts, qs, P.max_ext);
        MapExtEnd best;
        best.ei = best.ej = best.m = best.steps = 0; best.cells = 0;
        if (x.lt && x.lq) extend_cells<false>(x, ts, qs, Q, (int)P.band, (int)P.drop, 0, lane, nullptr, best);
        if (lane == 0) {
            if (x.bad) atomicOr(flags, MAP_EXT_E_CORNER);
            ends[e] = best;
        }
    }
}

// The second pass of the tasks whose end moved: the same cells up to anti-diagonal ei + ej with their traceback bits, and the way back from
// (ei, ej) (the same in every lane; lane 0 writes).  On the way back lane t holds the bits of anti-diagonal top - t.
__global__ void __launch_bounds__(256) k_map_extend_trace(const MapExtTask* __restrict__ tasks, uint32_t n_tasks, const MapChain* __restrict__ chain, MapAlnSeqs Q,
                                                          MapExtParams P, uint32_t tb_stride, uint64_t* tb_all, uint32_t* __restrict__ cols, MapAlnOut* __restrict__ out,
                                                          uint32_t* __restrict__ flags) {
    const uint32_t lane = threadIdx.x & 63u, n_waves = gridDim.x * 4u;
    const uint32_t wave = (uint32_t)uni((int)(blockIdx.x * 4u + (threadIdx.x >> 6)));
    uint64_t* tb = tb_all + 2ull * tb_stride * wave;
    const int B = (int)P.band;
    for (uint32_t e = wave; e < n_tasks; e += n_waves) {
        const MapExtTask K = tasks[e];
        const MapChain c = chain[K.chain];
        const MapSeq ts = Q.tseqs[c.tr >> 1], qs = Q.qseqs[c.read];
        const Cut x = cut_of(K, c, ts, qs, P.max_ext);
        uint32_t* lcols = cols + K.col_off;
        uint32_t err = 0, n = 0, acc = 0, n_eq = 0, n_x = 0, n_ins = 0, n_del = 0, runs = 0, last_op = 4;
        // (the store holds anti-diagonals 0 .. cap, and the cell must be one the first pass could have found)
        if (x.bad || K.cap >= tb_stride || K.ei + K.ej != K.cap || K.ei > x.lt || K.ej > x.lq || !K.cap) err = MAP_EXT_E_STORE;
        if (!err) {
            MapExtEnd unused;
            extend_cells<true>(x, ts, qs, Q, B, (int)P.drop, (int)K.cap, lane, tb, unused);
            __threadfence();
            int i = (int)K.ei, j = (int)K.ej, top = -1;
            uint64_t t0 = 0, t1 = 0;
            uint32_t at = x.right ? K.cap : 0u;                                // a right end's columns come last column first
            while (i > 0 || j > 0) {
                const int s = i + j, l = (i - j + B) >> 1;
                if (top < 0 || top - s > 63) {
                    top = s;
                    const int mine = s - (int)lane;
                    if (mine >= 1) {                                          // (read past the vector L1: the wave has just written them)
                        t0 = __hip_atomic_load(tb + 2 * mine, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        t1 = __hip_atomic_load(tb + 2 * mine + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    }
                }
                if (i - j > B || j - i > B) { err = MAP_EXT_E_TRACE; break; }
                const uint32_t code = (uint32_t)((lane_u64(t0, top - s) >> l) & 1u) | (uint32_t)((lane_u64(t1, top - s) >> l) & 1u) << 1;
                if (code < 2u ? (i <= 0 || j <= 0) : code == 3u ? i <= 0 : j <= 0) { err = MAP_EXT_E_TRACE; break; }
                if (code < 2u) { i--; j--; } else if (code == 3u) i--; else j--;
                const uint32_t op = P.eqx || code >= 2u ? code : 0u;
                n_eq += code == 0u; n_x += code == 1u; n_ins += code == 2u; n_del += code == 3u;
                runs += op != last_op ? 1u : 0u;
                last_op = op;
                n++;
                if (x.right) {                                                // (at > 0: a way back has at most ei + ej = cap columns)
                    at--;
                    acc |= code << (2u * (at & 15u));
                    if ((at & 15u) == 0u) { if (lane == 0) lcols[at >> 4] = acc; acc = 0; }
                } else {
                    acc |= code << (2u * (at & 15u));
                    at++;
                    if ((at & 15u) == 0u) { if (lane == 0) lcols[(at - 1u) >> 4] = acc; acc = 0; }
                }
            }
            if ((at & 15u) != 0u && lane == 0) lcols[at >> 4] = acc;
        }
        if (lane == 0) {
            if (err) atomicOr(flags, err);
            MapAlnOut o;
            o.ncols = err ? 0u : n; o.eq = n_eq; o.x = n_x; o.ins = n_ins; o.del = n_del; o.runs = err ? 0u : runs; o.cells = 0;
            out[e] = o;
        }
    }
}

hipError_t launch_map_extend(const MapExtTask* tasks, uint32_t n_tasks, const MapChain* chain, const MapAlnSeqs& Q, const MapExtParams& P, uint32_t n_waves, MapExtEnd* ends,
                             uint32_t* flags, hipStream_t s) {
    if (!n_tasks || !n_waves) return hipSuccess;
    hipLaunchKernelGGL((k_map_extend), dim3((n_waves + 3u) / 4u), dim3(256), 0, s, tasks, n_tasks, chain, Q, P, ends, flags);
    return hipGetLastError();
}
hipError_t launch_map_extend_trace(const MapExtTask* tasks, uint32_t n_tasks, const MapChain* chain, const MapAlnSeqs& Q, const MapExtParams& P, uint32_t n_waves,
                                   uint32_t tb_stride, uint64_t* tb, uint32_t* cols, MapAlnOut* out, uint32_t* flags, hipStream_t s) {
    if (!n_tasks || !n_waves) return hipSuccess;
    // whole workgroups of four waves: the caller's store holds n_waves rounded up to four
    hipLaunchKernelGGL((k_map_extend_trace), dim3((n_waves + 3u) / 4u), dim3(256), 0, s, tasks, n_tasks, chain, Q, P, tb_stride, tb, cols, out, flags);
    return hipGetLastError();
}

}  // namespace tk
