// map_split_kernels.hip -- device side of map --split (see map_split_kernels.h; the rules are stated in include/tksmseq.h, "map, split reads").
#include "map_split_kernels.h"

namespace tk {

namespace {

#define DEV __device__ __forceinline__

DEV uint64_t wave_max_u64(uint64_t v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const uint64_t o = __shfl_xor(v, d, 64);
        v = o > v ? o : v;
    }
    return v;
}

// a word this wave wrote earlier in the launch, read past the vector L1
DEV uint32_t load_own(const uint32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// the letters two half-open intervals share
DEV uint32_t shared_letters(uint32_t a0, uint32_t a1, uint32_t b0, uint32_t b1) {
    const uint32_t lo = max(a0, b0), hi = min(a1, b1);
    return hi > lo ? hi - lo : 0u;
}

}  // namespace

// One wave per group, all its rounds.  A round is k_map_chain's loop over the list of the remaining anchors: position x of the list holds
// the original group-relative index rem[x] (round 1: x itself, rem is not read).  Lane l keeps the anchor at list position x with
// x % 64 = l of the last 64 (p, qa, f and its original index in registers); the best candidate is one wave-wide maximum over
// score << 6 | slot, and the predecessor's original index comes from the lane that holds it.  pred is written at original indices and only
// for the anchors of the list, so the anchors of an earlier round's chain, which all left the list, keep their predecessors.  The walk
// back is done by all lanes alike (every lane reads the same words): the wave stays together for the next round.  After a kept round the
// list is compacted in place, tile by tile: a tile is loaded whole before its survivors are stored at or below its own positions.
__global__ void __launch_bounds__(256) k_map_chain_split(const uint64_t* __restrict__ k1, const uint64_t* __restrict__ k2, const uint32_t* __restrict__ gstart,
                                                         const uint32_t* __restrict__ list, uint32_t n_list, MapChainParams P, uint32_t rounds, uint32_t* rem, uint32_t* pred,
                                                         MapChain* __restrict__ chain) {
    const uint32_t c = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    if (c >= n_list) return;                                                  // (whole waves leave)
    const uint32_t g = list[c], b = gstart[g], n = gstart[g + 1] - b;
    const int k = (int)P.k;
    const uint64_t who = k2[b];
    uint32_t m = n, r = 0;                                                    // the anchors of the list, the round
    while (r < rounds) {
        int rp = 0, rq = 0, rf = 0;
        uint32_t ro = 0;
        int best_f = -1;
        uint32_t best_o = 0;
        for (uint32_t base = 0; base < m; base += 64u) {
            const uint32_t pos = base + lane;
            const bool live = pos < m;
            uint32_t no = pos;
            if (r && live) no = load_own(rem + b + pos);
            const uint64_t key = live ? k1[b + no] : 0ull;
            const int np = (int)(key >> 31), nq = (int)(key & 0x7FFFFFFFu);
            uint32_t my_pred = MAP_NO_PRED;
            const uint32_t tile = min(64u, m - base);
            for (uint32_t t = 0; t < tile; t++) {
                const int pi = __shfl(np, (int)t, 64), qi = __shfl(nq, (int)t, 64);
                const uint32_t oi = __shfl(no, (int)t, 64);
                uint64_t cand = 0;
                if (lane < t || base > 0u) {                                  // this lane holds a predecessor
                    const int dt = pi - rp, dq = qi - rq;
                    if (dt > 0 && dq > 0 && (uint32_t)dt <= P.max_gap && (uint32_t)dq <= P.max_gap) {
                        const uint32_t gap = (uint32_t)(dt > dq ? dt - dq : dq - dt);
                        if (gap <= P.bandwidth) {
                            const int64_t cost = gap ? (int64_t)gap * k / 100 + (31 - __clz((int)gap)) / 2 : 0;
                            const int64_t sc = (int64_t)rf + min(k, min(dt, dq)) - cost;
                            if (sc > k) cand = (uint64_t)sc << 6 | (lane < t ? 64u - t + lane : lane - t);
                        }
                    }
                }
                const uint64_t top = wave_max_u64(cand);
                // list position base + t - 64 + slot lies in lane (t + slot) % 64
                const uint32_t po = __shfl(ro, (int)((t + (uint32_t)(top & 63u)) & 63u), 64);
                int f = k;
                uint32_t pr = MAP_NO_PRED;
                if (top) { f = (int)(top >> 6); pr = po; }
                if (lane == t) { rp = np; rq = nq; rf = f; ro = no; my_pred = pr; }
                if (f > best_f) { best_f = f; best_o = oi; }
            }
            if (live) pred[b + no] = my_pred;
        }
        __threadfence();
        // the walk back through the predecessors the wave has just written, the same in every lane
        uint32_t i = best_o, cnt = 1, nmatch = (uint32_t)k;
        uint64_t key = k1[b + i];
        int p = (int)(key >> 31), q = (int)(key & 0x7FFFFFFFu);
        const int p_last = p, q_last = q;
        for (;;) {
            const uint32_t j = load_own(pred + b + i);
            if (j == MAP_NO_PRED || j >= i) break;                            // (j < i always: the second test only bounds the walk)
            key = k1[b + j];
            const int pj = (int)(key >> 31), qj = (int)(key & 0x7FFFFFFFu);
            nmatch += (uint32_t)min(k, min(p - pj, q - qj));
            cnt++;
            i = j; p = pj; q = qj;
        }
        MapChain o;
        o.read = (uint32_t)(who >> 32); o.tr = (uint32_t)who;
        o.score = (uint32_t)best_f; o.cnt = cnt; o.nmatch = nmatch;
        o.tstart = (uint32_t)p; o.tend = (uint32_t)p_last + P.k;
        o.qs = (uint32_t)q; o.qe = (uint32_t)q_last + P.k;
        o.kept = cnt >= P.min_count && o.score >= P.min_score ? 1u : 0u;
        if (lane == 0) chain[(uint64_t)c * rounds + r] = o;
        r++;
        if (!o.kept || r == rounds) break;
        // the anchors whose k-mer meets [qs, qe) leave the list
        uint32_t w = 0;
        for (uint32_t base = 0; base < m; base += 64u) {
            const uint32_t pos = base + lane;
            const bool live = pos < m;
            uint32_t no = pos;
            if (r > 1u && live) no = load_own(rem + b + pos);
            const uint32_t qa = live ? (uint32_t)(k1[b + no] & 0x7FFFFFFFu) : 0u;
            const bool stays = live && !(qa < o.qe && qa + P.k > o.qs);
            const unsigned long long ballot = __ballot(stays);
            if (stays) rem[b + w + (uint32_t)__popcll(ballot & ((1ull << lane) - 1ull))] = no;
            w += (uint32_t)__popcll(ballot);
        }
        __threadfence();
        m = w;
        if (m < P.min_count) break;
    }
    MapChain none;
    none.read = (uint32_t)(who >> 32); none.tr = (uint32_t)who;
    none.score = 0; none.cnt = 0; none.nmatch = 0; none.tstart = 0; none.tend = 0; none.qs = 0; none.qe = 0; none.kept = 0;
    for (uint32_t x = r + lane; x < rounds; x += 64u) chain[(uint64_t)c * rounds + x] = none;
}

__global__ void __launch_bounds__(256) k_map_split_list(const uint32_t* __restrict__ list, uint32_t n, uint32_t rounds, uint32_t* __restrict__ listx) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < n) listx[i] = list[i / rounds];
}

// One lane per read, 64 reads a workgroup.  Step A is k_map_select's loop over the round-1 chains of the read (chain index % rounds = 0).
// Step B walks the kept chains of all rounds that step A did not write; the accepted chains are kept in LDS, entry j of lane l at [j][l]
// (16 KB at 64 segments), and their read intervals are read again from chain[].  The mapq pass walks the read's chains once more: the first chain that is not written as tp:A:P and shares
// more than `overlap` letters with a supplementary line is that line's s2 (the chains come by descending score).
__global__ void __launch_bounds__(64) k_map_select_split(const uint64_t* __restrict__ key_sorted, const uint32_t* __restrict__ perm, const MapChain* __restrict__ chain,
                                                         const MapSeq* __restrict__ reads, uint32_t n_chains, uint32_t n_reads, MapSplitSelect S,
                                                         uint32_t* __restrict__ n_lines, uint32_t* __restrict__ n_first, uint32_t* __restrict__ line_mapq,
                                                         uint32_t* __restrict__ lines, uint32_t* __restrict__ rejected) {
    extern __shared__ uint32_t s_acc[];                                       // [segments - 1][64]: the accepted chains
    const uint32_t lane = threadIdx.x, r = blockIdx.x * 64u + lane;
    if (r >= n_reads) return;                                                 // (no barrier in this kernel)
    const uint32_t room = S.segments - 1u, slots = S.max_secondary + S.segments;
    uint32_t* s_chain = s_acc + lane;
    uint32_t lo = 0, hi = n_chains;                                           // the first key of read r or later
    const uint64_t want = (uint64_t)r << 32;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (key_sorted[mid] < want) lo = mid + 1u; else hi = mid;
    }
    uint32_t* out = lines + (uint64_t)r * slots;
    uint32_t* mq_out = line_mapq + (uint64_t)r * slots;
    const uint32_t qlen = reads[r].len;
    uint32_t count = 0, first = 0, rej = 0;
    // ---- step A: the round-1 chains alone
    {
        uint64_t s1 = 0, s2 = 0;
        uint32_t seen = 0;
        for (uint32_t c = lo; c < n_chains && (key_sorted[c] >> 32) == r; c++) {
            const uint32_t cc = perm[c];
            if (cc % S.rounds) continue;
            const uint64_t sc = 0xFFFFFFFFu - (uint32_t)key_sorted[c];
            if (!seen++) { s1 = sc; out[count++] = cc; continue; }
            if (seen == 2u) s2 = sc;
            if (count > S.max_secondary || sc * 1000ull < (uint64_t)S.permille * s1) break;
            out[count++] = cc;
        }
        first = count;
        if (first) mq_out[0] = (uint32_t)min((uint64_t)60, 60ull * (s1 - s2) / s1);        // (s1 >= k: never 0)
        for (uint32_t i = 1; i < first; i++) mq_out[i] = 0u;
    }
    // ---- step B: the other kept chains of all rounds against the primary and the accepted ones
    uint32_t nacc = 0;
    if (first) {
        const uint32_t primary = out[0];
        const MapChain pc = chain[primary];
        const uint32_t pa = (pc.tr & 1u) ? qlen - pc.qe : pc.qs, pb = (pc.tr & 1u) ? qlen - pc.qs : pc.qe;
        uint32_t in_a = 0;
        for (uint32_t c = lo; c < n_chains && (key_sorted[c] >> 32) == r && nacc < room; c++) {
            const uint32_t cc = perm[c];
            if (cc % S.rounds == 0u && in_a++ < first) continue;              // (step A wrote the first `first` round-1 chains)
            const MapChain x = chain[cc];
            const uint32_t a = (x.tr & 1u) ? qlen - x.qe : x.qs, e = (x.tr & 1u) ? qlen - x.qs : x.qe;
            bool ok = shared_letters(a, e, pa, pb) <= S.overlap;
            for (uint32_t j = 0; j < nacc && ok; j++) {
                const MapChain y = chain[s_chain[j * 64u]];
                ok = shared_letters(a, e, (y.tr & 1u) ? qlen - y.qe : y.qs, (y.tr & 1u) ? qlen - y.qs : y.qe) <= S.overlap;
            }
            if (!ok) { rej++; continue; }
            s_chain[nacc * 64u] = cc;
            out[count++] = cc;
            nacc++;
        }
        // ---- mapq of the supplementary lines
        uint64_t open = nacc ? ~0ull >> (64u - nacc) : 0ull;
        for (uint32_t c = lo; open && c < n_chains && (key_sorted[c] >> 32) == r; c++) {
            const uint32_t cc = perm[c];
            bool written = cc == primary;
            for (uint32_t j = 0; j < nacc && !written; j++) written = s_chain[j * 64u] == cc;
            if (written) continue;
            const MapChain x = chain[cc];
            const uint32_t a = (x.tr & 1u) ? qlen - x.qe : x.qs, e = (x.tr & 1u) ? qlen - x.qs : x.qe;
            for (uint32_t j = 0; j < nacc; j++) {
                if (!(open >> j & 1ull)) continue;
                const MapChain y = chain[s_chain[j * 64u]];
                if (shared_letters(a, e, (y.tr & 1u) ? qlen - y.qe : y.qs, (y.tr & 1u) ? qlen - y.qs : y.qe) <= S.overlap) continue;
                const uint64_t sj = y.score, s2 = x.score;
                mq_out[first + j] = s2 >= sj ? 0u : (uint32_t)min((uint64_t)60, 60ull * (sj - s2) / sj);
                open &= ~(1ull << j);
            }
        }
        for (uint32_t j = 0; j < nacc; j++)
            if (open >> j & 1ull) mq_out[first + j] = 60u;
    }
    n_lines[r] = count;
    n_first[r] = first;
    rejected[r] = rej;
}

hipError_t launch_map_chain_split(const uint64_t* k1, const uint64_t* k2, const uint32_t* gstart, const uint32_t* list, uint32_t n_list, const MapChainParams& P,
                                  uint32_t rounds, uint32_t* rem, uint32_t* pred, MapChain* chain, hipStream_t s) {
    if (!n_list) return hipSuccess;
    if (!rounds || rounds > MAP_SPLIT_CHAINS_MAX) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_map_chain_split, dim3((n_list + 3u) / 4u), dim3(256), 0, s, k1, k2, gstart, list, n_list, P, rounds, rem, pred, chain);
    return hipGetLastError();
}
hipError_t launch_map_split_list(const uint32_t* list, uint32_t n_list, uint32_t rounds, uint32_t* listx, hipStream_t s) {
    const uint64_t n = (uint64_t)n_list * rounds;
    if (!n) return hipSuccess;
    if (n >= (1ull << 32)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_map_split_list, dim3((unsigned)((n + 255u) / 256u)), dim3(256), 0, s, list, (uint32_t)n, rounds, listx);
    return hipGetLastError();
}
hipError_t launch_map_select_split(const uint64_t* key_sorted, const uint32_t* perm, const MapChain* chain, const MapSeq* reads, uint32_t n_chains, uint32_t n_reads,
                                   const MapSplitSelect& S, uint32_t* n_lines, uint32_t* n_first, uint32_t* line_mapq, uint32_t* lines, uint32_t* rejected, hipStream_t s) {
    if (!n_reads) return hipSuccess;
    if (S.segments < 2u || S.segments > MAP_SPLIT_SEGMENTS_MAX || !S.rounds) return hipErrorInvalidValue;
    const size_t lds = (size_t)(S.segments - 1u) * 64u * sizeof(uint32_t);
    hipLaunchKernelGGL(k_map_select_split, dim3((n_reads + 63u) / 64u), dim3(64), lds, s, key_sorted, perm, chain, reads, n_chains, n_reads, S, n_lines, n_first,
                       line_mapq, lines, rejected);
    return hipGetLastError();
}

}  // namespace tk
