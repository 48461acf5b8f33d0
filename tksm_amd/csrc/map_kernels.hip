// map_kernels.hip -- device side of map (see map_kernels.h; the rules are stated in include/tksmseq.h).
#include "map_kernels.h"

namespace tk {

namespace {

#define DEV __device__ __forceinline__

DEV uint64_t map_mix(uint64_t x) {                 // the finaliser of splitmix64
    x ^= x >> 30; x *= 0xbf58476d1ce4e5b9ull;
    x ^= x >> 27; x *= 0x94d049bb133111ebull;
    x ^= x >> 31;
    return x;
}

// the k-mer at position p of a sequence (p + k <= len: the words read lie inside the sequence): its letters from two or three code words
// and its validity from one or two validity words.  ok: all letters ACGT and the k-mer is not its own reverse complement.
DEV bool map_kmer(const uint32_t* __restrict__ codes, const uint32_t* __restrict__ valid, uint64_t voff, uint32_t p, uint32_t k, uint64_t& hash, uint32_t& strand) {
    const uint64_t cw = 2ull * voff + (p >> 4), vw = voff + (p >> 5);
    const uint32_t last = p + k - 1u;
    const uint32_t nc = (last >> 4) - (p >> 4);                               // further code words: 0, 1 or 2
    const uint64_t w0 = codes[cw], w1 = nc >= 1u ? codes[cw + 1] : 0u, w2 = nc >= 2u ? codes[cw + 2] : 0u;
    const uint32_t sh = 2u * (p & 15u);
    uint64_t x = (w0 | w1 << 32) >> sh;
    if (sh) x |= w2 << (64u - sh);
    const uint64_t mask = (1ull << (2u * k)) - 1ull;                            // k <= 28
    x &= mask;                                                                // letter i in bits 2i
    const uint64_t v0 = valid[vw], v1 = (last >> 5) > (p >> 5) ? valid[vw + 1] : 0u;
    const uint64_t kbits = (1ull << k) - 1ull;
    const bool all_acgt = (((v0 | v1 << 32) >> (p & 31u)) & kbits) == kbits;
    // fwd: the first letter highest.  Reversing all 64 bits reverses the letters and swaps the two bits of each; swap those back.
    uint64_t r = __brevll(x);
    r = ((r >> 1) & 0x5555555555555555ull) | ((r & 0x5555555555555555ull) << 1);
    const uint64_t fwd = r >> (64u - 2u * k);
    const uint64_t rev = ~x & mask;                                           // letter j of the reverse complement is 3 - letter k - 1 - j
    strand = rev < fwd ? 1u : 0u;
    hash = map_mix(rev < fwd ? rev : fwd);
    return all_acgt && fwd != rev;
}

DEV uint64_t wave_max_u64(uint64_t v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const uint64_t o = __shfl_xor(v, d, 64);
        v = o > v ? o : v;
    }
    return v;
}

inline dim3 blocks(uint64_t n) { return dim3((unsigned)((n + 255u) / 256u)); }

}  // namespace

__global__ void __launch_bounds__(256) k_map_ref_valid(RefView R, uint64_t n_words, uint32_t* __restrict__ valid) {
    const uint64_t w = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (w >= n_words) return;
    const uint64_t g = w << 5;
    const uint32_t ex = R.blocktab[g >> BLOCK_SHIFT];
    uint32_t bits = ~0u;
    if (ex != NO_BLOCK) {
        const uint4* src = reinterpret_cast<const uint4*>(R.pool + ((uint64_t)ex << BLOCK_SHIFT) + (g & ((1u << BLOCK_SHIFT) - 1)));      // 32 bytes, 32-byte aligned
        bits = 0u;
#pragma unroll
        for (int q = 0; q < 2; q++) {
            const uint4 v = src[q];
            const uint32_t word[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int i = 0; i < 16; i++) {
                const uint32_t c = (word[i >> 2] >> (8 * (i & 3))) & 0xFFu;
                bits |= (uint32_t)(c == 'A' || c == 'C' || c == 'G' || c == 'T') << (16 * q + i);
            }
        }
    }
    valid[w] = bits;
}

// One workgroup per tile of MAP_TILE windows.  Lane t hashes position j0 - 1 + t into LDS (the tile's positions, the w - 1 behind its last
// window and the one before its first); lanes 0 .. MAP_TILE then take window j0 - 1 + t and walk its w hashes in LDS.  The selected
// positions never decrease from one window to the next, so a window adds a minimizer exactly when it selects another position than the
// window before it; lane 0's window is only that predecessor.
template <bool WRITE>
__global__ void __launch_bounds__(256) k_map_sketch(MapSketch S, const uint64_t* __restrict__ off, uint64_t* __restrict__ counts, uint64_t* __restrict__ o_hash,
                                                    uint32_t* __restrict__ o_seq, uint32_t* __restrict__ o_ps) {
    __shared__ uint64_t s_hash[256];
    __shared__ uint32_t s_info[256];              // bit 0: valid, bit 1: strand
    __shared__ uint32_t s_wave[4];
    const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6;
    const MapTile tile = S.tiles[blockIdx.x];
    const MapSeq q = S.seqs[tile.seq];
    const uint32_t n = q.len - S.k + 1u;                                      // positions: at least one (the host makes no tile otherwise)
    const uint32_t last_window = n > S.w ? n - S.w : 0u;
    const int64_t base = (int64_t)tile.j0 - 1;
    const int64_t p = base + t;
    uint64_t h = 0;
    uint32_t info = 0;
    if (p >= 0 && p < (int64_t)n) {
        uint32_t strand;
        const bool ok = map_kmer(S.codes, S.valid, q.voff, (uint32_t)p, S.k, h, strand);
        info = (ok ? 1u : 0u) | strand << 1;
    }
    s_hash[t] = h;
    s_info[t] = info;
    __syncthreads();
    uint32_t sel = 0;                                                         // the window's choice: its offset in the tile + 1, or 0 for none
    const bool window = t <= MAP_TILE && p >= 0 && p <= (int64_t)last_window;
    if (window) {
        const uint32_t m = min(S.w, n - (uint32_t)p);
        uint64_t best = 0;
        for (uint32_t i = 0; i < m; i++) {
            const uint64_t hi = s_hash[t + i];
            if ((s_info[t + i] & 1u) && (!sel || hi < best)) { best = hi; sel = t + i + 1u; }
        }
    }
    __shared__ uint32_t s_sel[256];
    s_sel[t] = sel;
    __syncthreads();
    const bool mine = window && t >= 1u && sel && sel != s_sel[t - 1];
    const unsigned long long ballot = __ballot(mine);
    if (lane == 0) s_wave[wave] = (uint32_t)__popcll(ballot);
    __syncthreads();
    if (!WRITE) {
        if (t == 0) counts[blockIdx.x] = (uint64_t)s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
        return;
    }
    if (mine) {
        uint32_t rank = (uint32_t)__popcll(ballot & ((1ull << lane) - 1ull));
        for (uint32_t v = 0; v < wave; v++) rank += s_wave[v];
        const uint64_t o = off[blockIdx.x] + rank;
        o_hash[o] = s_hash[sel - 1u];
        o_seq[o] = tile.seq;
        o_ps[o] = (uint32_t)(base + (sel - 1u)) << 1 | (s_info[sel - 1u] >> 1);
    }
}

__global__ void __launch_bounds__(256) k_map_dropped(const uint64_t* __restrict__ dcount, uint32_t n, uint64_t max_occ, unsigned long long* __restrict__ dropped) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    const bool over = i < n && dcount[i] > max_occ;
    const unsigned long long ballot = __ballot(over);
    if ((threadIdx.x & 63u) == 0 && ballot) atomicAdd(dropped, (unsigned long long)__popcll(ballot));
}

__global__ void __launch_bounds__(256) k_map_seed_count(const uint64_t* __restrict__ rm_hash, uint32_t n_rm, const uint64_t* __restrict__ dkey,
                                                        const uint64_t* __restrict__ dcount, uint32_t n_distinct, uint64_t max_occ, uint32_t* __restrict__ run,
                                                        uint64_t* __restrict__ cnt) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n_rm) return;
    const uint64_t h = rm_hash[i];
    uint32_t lo = 0, hi = n_distinct;                                         // the first distinct hash >= h
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (dkey[mid] < h) lo = mid + 1u; else hi = mid;
    }
    uint64_t c = 0;
    if (lo < n_distinct && dkey[lo] == h) { c = dcount[lo]; if (c > max_occ) c = 0; }
    run[i] = lo;
    cnt[i] = c;
}

__global__ void __launch_bounds__(256) k_map_seed_write(const uint32_t* __restrict__ rm_read, const uint32_t* __restrict__ rm_ps, const uint32_t* __restrict__ run,
                                                        const uint64_t* __restrict__ cnt, const uint64_t* __restrict__ off, uint32_t n_rm,
                                                        const uint32_t* __restrict__ dstart, const uint32_t* __restrict__ idx_seq, const uint32_t* __restrict__ idx_ps,
                                                        const MapSeq* __restrict__ reads, uint32_t k, uint64_t* __restrict__ k1, uint64_t* __restrict__ k2) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n_rm) return;
    const uint32_t c = (uint32_t)cnt[i];
    if (!c) return;
    const uint32_t read = rm_read[i], q = rm_ps[i] >> 1, sr = rm_ps[i] & 1u;
    const uint32_t q_rev = reads[read].len - k - q;
    const uint32_t e0 = dstart[run[i]];
    const uint64_t o = off[i];
    for (uint32_t e = 0; e < c; e++) {
        const uint32_t t = idx_seq[e0 + e], ps = idx_ps[e0 + e];
        const uint32_t rel = sr ^ (ps & 1u);
        k1[o + e] = (uint64_t)(ps >> 1) << 31 | (rel ? q_rev : q);
        k2[o + e] = (uint64_t)read << 32 | (uint64_t)t << 1 | rel;
    }
}

__global__ void __launch_bounds__(256) k_map_group_flags(const uint32_t* __restrict__ gstart, uint32_t n_groups, uint32_t min_count, uint64_t* __restrict__ flag) {
    const uint32_t g = blockIdx.x * 256u + threadIdx.x;
    if (g < n_groups) flag[g] = gstart[g + 1] - gstart[g] >= min_count ? 1ull : 0ull;
}
__global__ void __launch_bounds__(256) k_map_group_list(const uint64_t* __restrict__ flag, const uint64_t* __restrict__ scanned, uint32_t n_groups,
                                                        uint32_t* __restrict__ list) {
    const uint32_t g = blockIdx.x * 256u + threadIdx.x;
    if (g < n_groups && flag[g]) list[(uint32_t)scanned[g]] = g;
}

// One wave per group.  Lane l keeps anchor j with j % 64 = l of the last 64 anchors (p, qa and f in registers): at step i these are
// exactly the predecessors i - 64 .. i - 1, and lane i % 64 takes anchor i over once the step is decided.  The anchors come in tiles of
// 64, one per lane, and the current one is broadcast from its lane.  The best candidate is one wave-wide maximum over
// score << 6 | (j - (i - 64)): the largest score, and among equal scores the largest j.
__global__ void __launch_bounds__(256) k_map_chain(const uint64_t* __restrict__ k1, const uint64_t* __restrict__ k2, const uint32_t* __restrict__ gstart,
                                                   const uint32_t* __restrict__ list, uint32_t n_list, MapChainParams P, uint32_t* pred, MapChain* __restrict__ chain) {
    const uint32_t c = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    if (c >= n_list) return;                                                  // (whole waves leave)
    const uint32_t g = list[c], b = gstart[g], n = gstart[g + 1] - b;
    const int k = (int)P.k;
    int rp = 0, rq = 0, rf = 0;
    int best_f = -1;
    uint32_t best_i = 0;
    for (uint32_t base = 0; base < n; base += 64u) {
        const uint32_t idx = base + lane;
        const bool live = idx < n;
        const uint64_t key = live ? k1[b + idx] : 0ull;
        const int np = (int)(key >> 31), nq = (int)(key & 0x7FFFFFFFu);
        uint32_t my_pred = MAP_NO_PRED;
        const uint32_t m = min(64u, n - base);
        for (uint32_t t = 0; t < m; t++) {
            const int pi = __shfl(np, (int)t, 64), qi = __shfl(nq, (int)t, 64);
            uint64_t cand = 0;
            if (lane < t || base > 0u) {                                      // this lane holds a predecessor
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
            int f = k;
            uint32_t pr = MAP_NO_PRED;
            if (top) { f = (int)(top >> 6); pr = base + t - 64u + (uint32_t)(top & 63u); }
            if (lane == t) { rp = np; rq = nq; rf = f; my_pred = pr; }
            if (f > best_f) { best_f = f; best_i = base + t; }
        }
        if (live) pred[b + idx] = my_pred;
    }
    __threadfence();
    if (lane != 0) return;
    // the walk back through the predecessors the wave has just written (read past the vector L1)
    uint32_t i = best_i, cnt = 1, nmatch = (uint32_t)k;
    uint64_t key = k1[b + i];
    int p = (int)(key >> 31), q = (int)(key & 0x7FFFFFFFu);
    const int p_last = p, q_last = q;
    for (;;) {
        const uint32_t j = __hip_atomic_load(pred + b + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (j == MAP_NO_PRED || j >= i) break;                                // (j < i always: the second test only bounds the walk)
        key = k1[b + j];
        const int pj = (int)(key >> 31), qj = (int)(key & 0x7FFFFFFFu);
        nmatch += (uint32_t)min(k, min(p - pj, q - qj));
        cnt++;
        i = j; p = pj; q = qj;
    }
    MapChain o;
    const uint64_t who = k2[b];
    o.read = (uint32_t)(who >> 32); o.tr = (uint32_t)who;
    o.score = (uint32_t)best_f; o.cnt = cnt; o.nmatch = nmatch;
    o.tstart = (uint32_t)p; o.tend = (uint32_t)p_last + P.k;
    o.qs = (uint32_t)q; o.qe = (uint32_t)q_last + P.k;
    o.kept = cnt >= P.min_count && o.score >= P.min_score ? 1u : 0u;
    chain[c] = o;
}

__global__ void __launch_bounds__(256) k_map_chain_keys(const MapChain* __restrict__ chain, uint32_t n, uint64_t* __restrict__ key) {
    const uint32_t c = blockIdx.x * 256u + threadIdx.x;
    if (c < n) key[c] = chain[c].kept ? (uint64_t)chain[c].read << 32 | (0xFFFFFFFFu - chain[c].score) : ~0ull;
}

__global__ void __launch_bounds__(256) k_map_select(const uint64_t* __restrict__ key_sorted, const uint32_t* __restrict__ perm, uint32_t n_chains, uint32_t n_reads,
                                                    uint32_t permille, uint32_t max_secondary, uint32_t* __restrict__ n_lines, uint32_t* __restrict__ mapq,
                                                    uint32_t* __restrict__ lines) {
    const uint32_t r = blockIdx.x * 256u + threadIdx.x;
    if (r >= n_reads) return;
    uint32_t lo = 0, hi = n_chains;                                           // the first key of read r or later
    const uint64_t want = (uint64_t)r << 32;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (key_sorted[mid] < want) lo = mid + 1u; else hi = mid;
    }
    uint32_t count = 0, mq = 0;
    if (lo < n_chains && (key_sorted[lo] >> 32) == r) {
        uint32_t* out = lines + (uint64_t)r * (max_secondary + 1u);
        const uint64_t s1 = 0xFFFFFFFFu - (uint32_t)key_sorted[lo];
        out[count++] = perm[lo];
        uint64_t s2 = 0;
        for (uint32_t c = lo + 1u; c < n_chains && (key_sorted[c] >> 32) == r; c++) {
            const uint64_t sc = 0xFFFFFFFFu - (uint32_t)key_sorted[c];
            if (c == lo + 1u) s2 = sc;
            if (count > max_secondary || sc * 1000ull < (uint64_t)permille * s1) break;
            out[count++] = perm[c];
        }
        mq = (uint32_t)min((uint64_t)60, 60ull * (s1 - s2) / s1);               // (s1 >= k: never 0)
    }
    n_lines[r] = count;
    mapq[r] = mq;
}

hipError_t launch_map_ref_valid(const RefView& R, uint64_t n_words, uint32_t* valid, hipStream_t s) {
    if (!n_words) return hipSuccess;
    hipLaunchKernelGGL(k_map_ref_valid, blocks(n_words), dim3(256), 0, s, R, n_words, valid);
    return hipGetLastError();
}
hipError_t launch_map_sketch_count(const MapSketch& S, uint64_t* counts, hipStream_t s) {
    if (!S.n_tiles) return hipSuccess;
    hipLaunchKernelGGL(k_map_sketch<false>, dim3(S.n_tiles), dim3(256), 0, s, S, (const uint64_t*)nullptr, counts, (uint64_t*)nullptr, (uint32_t*)nullptr, (uint32_t*)nullptr);
    return hipGetLastError();
}
hipError_t launch_map_sketch_write(const MapSketch& S, const uint64_t* off, uint64_t* hash, uint32_t* seq, uint32_t* ps, hipStream_t s) {
    if (!S.n_tiles) return hipSuccess;
    hipLaunchKernelGGL(k_map_sketch<true>, dim3(S.n_tiles), dim3(256), 0, s, S, off, (uint64_t*)nullptr, hash, seq, ps);
    return hipGetLastError();
}
hipError_t launch_map_dropped(const uint64_t* dcount, uint32_t n_distinct, uint64_t max_occ, unsigned long long* dropped, hipStream_t s) {
    hipError_t e = hipMemsetAsync(dropped, 0, 8, s);
    if (e != hipSuccess || !n_distinct) return e;
    hipLaunchKernelGGL(k_map_dropped, blocks(n_distinct), dim3(256), 0, s, dcount, n_distinct, max_occ, dropped);
    return hipGetLastError();
}
hipError_t launch_map_seed_count(const uint64_t* rm_hash, uint32_t n_rm, const uint64_t* dkey, const uint64_t* dcount, uint32_t n_distinct, uint64_t max_occ,
                                 uint32_t* run, uint64_t* cnt, hipStream_t s) {
    if (!n_rm) return hipSuccess;
    hipLaunchKernelGGL(k_map_seed_count, blocks(n_rm), dim3(256), 0, s, rm_hash, n_rm, dkey, dcount, n_distinct, max_occ, run, cnt);
    return hipGetLastError();
}
hipError_t launch_map_seed_write(const uint32_t* rm_read, const uint32_t* rm_ps, const uint32_t* run, const uint64_t* cnt, const uint64_t* off, uint32_t n_rm,
                                 const uint32_t* dstart, const uint32_t* idx_seq, const uint32_t* idx_ps, const MapSeq* reads, uint32_t k, uint64_t* k1, uint64_t* k2,
                                 hipStream_t s) {
    if (!n_rm) return hipSuccess;
    hipLaunchKernelGGL(k_map_seed_write, blocks(n_rm), dim3(256), 0, s, rm_read, rm_ps, run, cnt, off, n_rm, dstart, idx_seq, idx_ps, reads, k, k1, k2);
    return hipGetLastError();
}
hipError_t launch_map_group_flags(const uint32_t* gstart, uint32_t n_groups, uint32_t min_count, uint64_t* flag, hipStream_t s) {
    if (!n_groups) return hipSuccess;
    hipLaunchKernelGGL(k_map_group_flags, blocks(n_groups), dim3(256), 0, s, gstart, n_groups, min_count, flag);
    return hipGetLastError();
}
hipError_t launch_map_group_list(const uint64_t* flag, const uint64_t* scanned, uint32_t n_groups, uint32_t* list, hipStream_t s) {
    if (!n_groups) return hipSuccess;
    hipLaunchKernelGGL(k_map_group_list, blocks(n_groups), dim3(256), 0, s, flag, scanned, n_groups, list);
    return hipGetLastError();
}
hipError_t launch_map_chain(const uint64_t* k1, const uint64_t* k2, const uint32_t* gstart, const uint32_t* list, uint32_t n_list, const MapChainParams& P,
                            uint32_t* pred, MapChain* chain, hipStream_t s) {
    if (!n_list) return hipSuccess;
    hipLaunchKernelGGL(k_map_chain, dim3((n_list + 3u) / 4u), dim3(256), 0, s, k1, k2, gstart, list, n_list, P, pred, chain);
    return hipGetLastError();
}
hipError_t launch_map_chain_keys(const MapChain* chain, uint32_t n, uint64_t* key, hipStream_t s) {
    if (!n) return hipSuccess;
    hipLaunchKernelGGL(k_map_chain_keys, blocks(n), dim3(256), 0, s, chain, n, key);
    return hipGetLastError();
}
hipError_t launch_map_select(const uint64_t* key_sorted, const uint32_t* perm, uint32_t n_chains, uint32_t n_reads, uint32_t permille, uint32_t max_secondary,
                             uint32_t* n_lines, uint32_t* mapq, uint32_t* lines, hipStream_t s) {
    if (!n_reads) return hipSuccess;
    hipLaunchKernelGGL(k_map_select, blocks(n_reads), dim3(256), 0, s, key_sorted, perm, n_chains, n_reads, permille, max_secondary, n_lines, mapq, lines);
    return hipGetLastError();
}

}  // namespace tk
