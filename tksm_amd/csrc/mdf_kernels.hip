// mdf_kernels.hip -- PCR amplification and truncation of molecule descriptions on the device (gfx950).
//
// Reference behaviour restated (file:line into vpc-ccg/tksm):
//   PCR::do_pcr / perform        src/pcr.cpp:40-89     branching amplification, per-copy substitutions, capture by sequencing
//   molecule_descriptor::add_error  src/interval.h:866-874  molecule position -> (segment, offset)
//   truncate()                   src/truncate.cpp:23-65   keep the first L bases in segment order
//   einterval::truncate          src/interval.h:708-735   cut segment: new bounds, substitutions re-based and filtered
//   custom_distribution / 2D     src/truncate.cpp:77-227  empirical samplers of the KDE truncation model
//   truncate_transformer(_kde)   src/truncate.cpp:322-351 3' truncation, then 5' truncation of the flipped molecule
//   add_polyA                    src/polyA.cpp:133-148    append "A" x len, len ~ gamma / poisson / weibull / normal, clamped
//   TAG_module::run              src/tag.cpp:70-113       prepend / append a tag drawn from an IUPAC format (fmt2seq, src/util.h:53-92)
//   SingleCellBarcoder::run      src/scb.cpp:57-80        append the CB barcode of the header comment
//   flip_molecule                src/interval.h:908-920   reverse the segment order, toggle every strand
//   RWGS_module::run             src/random_wgs.cpp:181-207 whole-genome fragments: position, length and strand draws, no input
//   NoiseAdder::operator()       src/append_noise.cpp:83-128 tail noise: a random literal, or the last segments again as a hairpin
//   Splicer_module::run          src/transcribe.cpp:170-197 an abundance row becomes `depth` copies of its transcript's exons, no input batch
//   Unsegment_module::run        src/unsegment.cpp:88-105  a molecule is glued behind its predecessor with a probability (concat, src/interval.h:893-896)
//   Shuffle_module::shuffle_stream  src/shuffle.cpp:23-44  the molecules in a random order, whole or through a buffer of B slots
//   Mutate_module (table format) src/mutate.cpp:99-108, :157-181 SNVs, insertions, deletions; the transform itself is defined in DESIGN.md ("mutate")
// Integer / byte work, one LANE per molecule (tail-noise alone spreads its per-base work: one wave per molecule, or a flat grid): the tables of a molecule are a few dozen bytes, the work per molecule is a short
// serial walk (tree of copies; list of segments).  The reference draws from a sequential Mersenne Twister; here every
// decision has its own Philox counter (template molecule, path of copy cycles, purpose), so the result does not depend on
// the order molecules are processed in, and the CPU oracle (oracle/mdf_ops_oracle.py) reproduces it bit for bit.
#include "mdf_kernels.h"

namespace tk {

#define DEV __device__ __forceinline__

struct Ph4m { uint32_t x, y, z, w; };
enum { ST_PCR_PICK = 16, ST_PCR_EMIT = 17, ST_PCR_CHILD = 18, ST_PCR_MUT = 19, ST_TRC_LEN = 24, ST_TRC_SIDE = 25,
       ST_PLA_LEN = 26, ST_TAG5 = 27, ST_TAG3 = 28, ST_FLIP = 29, ST_GLUE = 30, ST_SHF_KEY = 31, ST_WGS_POS = 32, ST_WGS_LEN = 33, ST_WGS_STRAND = 34,
       ST_SHF_SLOT = 35,
       ST_NOISE_LEN = 40, ST_NOISE_SEQ = 41, ST_NOISE_ERR = 42, ST_TSB = 56 };

DEV Ph4m philox_raw(uint64_t seed, uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3) {
    uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
#pragma unroll
    for (int r = 0; r < 10; r++) {
        const unsigned long long p0 = (unsigned long long)0xD2511F53u * c0, p1 = (unsigned long long)0xCD9E8D57u * c2;
        const uint32_t h0 = (uint32_t)(p0 >> 32), l0 = (uint32_t)p0, h1 = (uint32_t)(p1 >> 32), l1 = (uint32_t)p1;
        const uint32_t n0 = h1 ^ c1 ^ k0, n2 = h0 ^ c3 ^ k1;
        c0 = n0; c1 = l1; c2 = n2; c3 = l0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    return Ph4m{c0, c1, c2, c3};
}
// a decision about the copy with path `mask` of template molecule u
DEV Ph4m philox_node(uint64_t seed, uint32_t u, uint64_t mask, uint32_t stream, uint32_t n) {
    return philox_raw(seed, u, (uint32_t)mask, stream | ((uint32_t)(mask >> 32) << 8), n);
}
// per-molecule streams (same counter layout as the Seq kernels: read index, stream, n)
DEV Ph4m philox_mol(uint64_t seed, uint64_t g, uint32_t stream, uint32_t n) {
    return philox_raw(seed, (uint32_t)g, (uint32_t)(g >> 32), stream, n);
}
DEV double u01(uint32_t x) { return (double)x * (1.0 / 4294967296.0); }

// nominal size of a segment (ginterval::size, end - start; the Seq kernels clamp to the contig, PCR / Trc do not)
DEV uint32_t seg_size(const uint32_t* iv) { return iv[2] > iv[1] ? iv[2] - iv[1] : 0u; }
DEV uint32_t mol_size(const BatchView& B, uint32_t r) {
    const uint32_t ib = B.reads[2 * r], ic = B.reads[2 * r + 1];
    uint32_t t = 0;
    for (uint32_t i = 0; i < ic; i++) t += seg_size(B.intervals + 4ull * (ib + i));
    return t;
}
DEV uint32_t mol_mods(const BatchView& B, uint32_t r) {
    const uint32_t ib = B.reads[2 * r], ic = B.reads[2 * r + 1];
    return (B.intervals[4ull * (ib + ic) + 3] & 0x7fffffffu) - (B.intervals[4ull * ib + 3] & 0x7fffffffu);
}
DEV int ndig(uint32_t v) { int d = 1; while (v >= 10) { v /= 10; d++; } return d; }
DEV int put_dec(uint8_t* o, uint32_t v) { const int d = ndig(v); for (int i = d - 1; i >= 0; i--) { o[i] = (uint8_t)('0' + v % 10); v /= 10; } return d; }

// ------------------------------------------------------------------------------------------------
// PCR.  The reference walks the whole tree of copies of a template (every copy made in cycle s is a template in the cycles
// after s: src/pcr.cpp:62-64) and lets each copy be captured by the sequencing with probability drop_ratio (:59).  The tree has
// (1 + efficiency)^cycles nodes, of which a fraction drop_ratio is written; here only the branches that lead to a written
// copy are walked: P(no copy is written in the subtree of an existing copy made in cycle t) = q[t] is known in closed
// form (PcrParams), so "the copy exists AND its subtree writes something" is decided first, and inside such a subtree
// the events {this copy is written, the copy made from it in cycle t leads to a written copy} are drawn one after the other
// conditioned on at least one of them happening.  The distribution of the written set (with its ancestry, hence shared
// substitutions) is the reference's; the cost is proportional to what is written.
// visit(): calls out(mask) for every written copy of template u, in the reference's order (a copy, then the copies made
// from it cycle by cycle: depth first).
// ------------------------------------------------------------------------------------------------
template <class F>
DEV void pcr_walk(const PcrParams& P, uint32_t u, F&& out) {
    // explicit stack: node mask, next cycle to try, "an emission has already happened in this subtree"
    unsigned long long smask[PCR_MAX_CYCLES + 1]; int snext[PCR_MAX_CYCLES + 1]; bool ssat[PCR_MAX_CYCLES + 1];
    int sp = 0;
    smask[0] = 0ull; snext[0] = 0; ssat[0] = true;                    // the template itself: nothing required of its subtree
    while (sp >= 0) {
        const unsigned long long R = smask[sp];
        const int t = snext[sp];
        if (t >= P.cycles) { sp--; continue; }
        snext[sp] = t + 1;
        const double pm = P.efficiency * (1.0 - P.q[t]);                // the copy made in cycle t exists and leads to an emission
        const double p = ssat[sp] ? pm : pm / (1.0 - P.A[t]);
        const unsigned long long C = R | (1ull << t);
        if (!(u01(philox_node(P.seed, u, C, ST_PCR_CHILD, 0).x) < p)) continue;
        ssat[sp] = true;
        // enter the copy: is it written itself?
        const double pe = P.drop / (1.0 - P.q[t]);                      // given that its subtree writes something
        const bool emit = u01(philox_node(P.seed, u, C, ST_PCR_EMIT, 0).x) < pe;
        if (emit) out(C);
        sp++;
        smask[sp] = C; snext[sp] = t + 1; ssat[sp] = emit;
    }
}

// substitutions of the copy event that made node `mask` (src/pcr.cpp:44-56): count = floor(rate * size) + Bernoulli(fraction),
// distinct positions (std::sample: in increasing order), bases from "ACTG"
DEV int pcr_mutations(const PcrParams& P, uint32_t u, unsigned long long mask, uint32_t size, uint32_t* pos, uint8_t* base) {
    const double expected = P.rate * (double)size;
    int cnt = (int)expected;
    cnt += u01(philox_node(P.seed, u, mask, ST_PCR_MUT, 0).x) < (expected - (double)cnt) ? 1 : 0;
    cnt = min(min(cnt, PCR_MAX_MUT), (int)size);
    uint32_t attempt = 1;
    for (int j = 0; j < cnt; j++) {
        for (;;) {
            const Ph4m w = philox_node(P.seed, u, mask, ST_PCR_MUT, attempt++);
            const uint32_t p = __umulhi(w.x, size);
            bool dup = false;
            for (int q = 0; q < j; q++) dup |= pos[q] == p;
            if (dup) continue;
            // insertion sort by position
            int q = j;
            while (q > 0 && pos[q - 1] > p) { pos[q] = pos[q - 1]; base[q] = base[q - 1]; q--; }
            pos[q] = p; base[q] = (uint8_t)((0x47544341u >> (8 * (w.y & 3u))) & 0xffu);   // "ACTG"
            break;
        }
    }
    return cnt;
}

DEV uint32_t pcr_template(const MolView& M, uint64_t i) { return M.keep ? M.keep[i] : (uint32_t)i; }

__global__ void k_pcr_count(MolView M, PcrParams P, uint64_t* __restrict__ n_out, uint32_t* __restrict__ status) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= M.n_kept) return;
    const uint32_t u = pcr_template(M, i);
    unsigned long long n = 0;
    pcr_walk(P, u, [&](unsigned long long) { n++; });
    n_out[i] = n;
    if ((double)mol_size(M.B, u) * P.rate >= (double)PCR_MAX_MUT) atomicOr(status, 1u);
}

// id of a copy: template id [+ "_" + index among the unrolled copies] + "." + cycle for every copy event on its path
DEV uint32_t pcr_id_len(const MolView& M, uint32_t u, unsigned long long mask) {
    uint32_t n = M.B.ids[2 * u + 1];
    if (M.dup && (M.dup[u] >> 31)) n += 1 + ndig(M.dup[u] & 0x7fffffffu);
    for (unsigned long long m = mask; m; m &= m - 1) n += 1 + ndig((uint32_t)__builtin_ctzll(m));
    return n;
}

__global__ void k_pcr_list(MolView M, PcrParams P, const uint64_t* __restrict__ out_off, uint32_t* __restrict__ node_mol,
                           uint64_t* __restrict__ node_mask, MolCounts C) {
    uint64_t* __restrict__ node_ivls = C.ivl; uint64_t* __restrict__ node_mods = C.mod; uint64_t* __restrict__ node_idlen = C.id;
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= M.n_kept) return;
    const uint32_t u = pcr_template(M, i);
    const uint32_t size = mol_size(M.B, u), base_mods = mol_mods(M.B, u), ic = M.B.reads[2 * u + 1];
    uint64_t at = out_off[i];
    pcr_walk(P, u, [&](unsigned long long mask) {
        // substitutions accumulated along the path: one count per copy event (prefix of the path)
        uint32_t nm = base_mods;
        unsigned long long pre = 0ull;
        for (unsigned long long m = mask; m; m &= m - 1) {
            pre |= m & (~m + 1ull);
            const double expected = P.rate * (double)size;
            int cnt = (int)expected;
            cnt += u01(philox_node(P.seed, u, pre, ST_PCR_MUT, 0).x) < (expected - (double)cnt) ? 1 : 0;
            nm += (uint32_t)min(min(cnt, PCR_MAX_MUT), (int)size);
        }
        node_mol[at] = u; node_mask[at] = mask; node_ivls[at] = ic; node_mods[at] = nm; node_idlen[at] = pcr_id_len(M, u, mask);
        at++;
    });
}

__global__ void k_pcr_write(MolView M, PcrParams P, uint64_t n_nodes, const uint32_t* __restrict__ node_mol,
                            const uint64_t* __restrict__ node_mask, MolOffsets F, MolOut O) {
    const uint64_t* __restrict__ ivl_off = F.ivl; const uint64_t* __restrict__ mod_off = F.mod; const uint64_t* __restrict__ id_off = F.id;
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n_nodes) return;
    const uint32_t u = node_mol[j];
    const unsigned long long mask = node_mask[j];
    const BatchView& B = M.B;
    const uint32_t ib = B.reads[2 * u], ic = B.reads[2 * u + 1];
    const uint32_t size = mol_size(B, u);
    const uint64_t io = ivl_off[j];
    uint64_t mo = mod_off[j];
    O.reads[2 * j] = (uint32_t)io; O.reads[2 * j + 1] = ic;
    // id
    {
        uint8_t* d = O.idpool + id_off[j];
        const uint32_t so = B.ids[2 * u], sl = B.ids[2 * u + 1];
        uint32_t k = 0;
        for (; k < sl; k++) d[k] = B.idpool[so + k];
        if (M.dup && (M.dup[u] >> 31)) { d[k++] = '_'; k += (uint32_t)put_dec(d + k, M.dup[u] & 0x7fffffffu); }
        for (unsigned long long m = mask; m; m &= m - 1) { d[k++] = '.'; k += (uint32_t)put_dec(d + k, (uint32_t)__builtin_ctzll(m)); }
        O.ids[2 * j] = (uint32_t)id_off[j]; O.ids[2 * j + 1] = k;
    }
    // segments with their substitutions: the template's own first, then those of every copy event on the path, oldest first
    // (do_pcr appends to the copy it was handed: src/pcr.cpp:52-56)
    uint32_t cum = 0;
    for (uint32_t i = 0; i < ic; i++) {
        const uint32_t* iv = B.intervals + 4ull * (ib + i);
        const uint32_t sz = seg_size(iv);
        uint32_t* ov = O.intervals + 4ull * (io + i);
        ov[0] = iv[0]; ov[1] = iv[1]; ov[2] = iv[2]; ov[3] = (uint32_t)mo | (iv[3] & 0x80000000u);
        const uint32_t mb = iv[3] & 0x7fffffffu, me = iv[7] & 0x7fffffffu;
        for (uint32_t q = mb; q < me; q++) { O.mods[2 * mo] = B.mods[2ull * q]; O.mods[2 * mo + 1] = B.mods[2ull * q + 1]; mo++; }
        unsigned long long pre = 0ull;
        for (unsigned long long m = mask; m; m &= m - 1) {
            pre |= m & (~m + 1ull);
            uint32_t pos[PCR_MAX_MUT]; uint8_t base[PCR_MAX_MUT];
            const int cnt = pcr_mutations(P, u, pre, size, pos, base);
            for (int q = 0; q < cnt; q++)
                // add_error: the segment whose cumulative size first exceeds the position (empty segments are skipped)
                if (pos[q] >= cum && pos[q] < cum + sz) { O.mods[2 * mo] = pos[q] - cum; O.mods[2 * mo + 1] = base[q]; mo++; }
        }
        cum += sz;
    }
}

// ------------------------------------------------------------------------------------------------
// truncation
// ------------------------------------------------------------------------------------------------
// double -> int as the reference's implicit conversion at the call truncate(md, <double>) does it (toward zero); clamped
DEV int to_int(double v) { return v >= 2147483647.0 ? 2147483647 : (v <= -2147483648.0 ? (-2147483647 - 1) : (int)v); }

// truncate() as a window computation: what [0, size) shrinks to when the first L bases are kept.  Returns the new size;
// cut = false when the call changes nothing (L == size, or fewer bases than L).
DEV int trc_keep(int size, int L, int min_val, bool& cut) {
    cut = false;
    if (L == size) return size;
    if (min_val > L) L = min_val;
    if (size < L) return size;
    cut = true;                                                        // (L == size here: a cut that removes nothing)
    return L;
}

// first index with cdf[idx] >= u (std::lower_bound), cdf has n entries
DEV int lower_bound_d(const double* cdf, int n, double u) {
    int lo = 0, hi = n;
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (cdf[mid] < u) lo = mid + 1; else hi = mid; }
    return lo;
}

// custom_distribution<double, long>::operator()(g, u) on row `row` of the 2-D model: bin by the row's cumulative sums,
// then a uniform integer in [previous label (0 for the first bin), label] (src/truncate.cpp:128-134, :107-114)
DEV double trc_row_draw(const TrcParams& T, int row, double u, uint32_t w) {
    const double* cdf = T.cdf + (size_t)row * (T.nx + 1);
    int bin = lower_bound_d(cdf, T.row_n[row] + 1, u) - 1;
    bin = max(0, min(bin, T.nx - 1));
    const long long lo = bin == 0 ? 0ll : T.xlab[bin - 1], hi = T.xlab[bin];
    const unsigned long long span = (unsigned long long)(hi - lo) + 1ull;
    return (double)(lo + (long long)(((unsigned long long)w * span) >> 32));
}

__global__ void k_trc_plan(MolView M, TrcParams T, uint64_t first_index, uint32_t* __restrict__ keep_from, uint32_t* __restrict__ keep_to,
                           double* __restrict__ tr_len, double* __restrict__ tr_side, MolCounts C) {
    uint64_t* __restrict__ n_ivls = C.ivl; uint64_t* __restrict__ n_mods = C.mod; uint64_t* __restrict__ n_idlen = C.id;
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= M.B.n_reads) return;
    const BatchView& B = M.B;
    const int size = (int)mol_size(B, (uint32_t)r);
    const uint64_t g = first_index + r;
    int w0 = 0, w1 = size;
    bool cut3 = false, cut5 = false;
    double tl = 0.0, side = 1.0;
    if (T.mode != 2) {
        // normal / lognormal post-truncation length (src/truncate.cpp:335-345): Box-Muller on one Philox draw
        const Ph4m w = philox_mol(T.seed, g, ST_TRC_LEN, 0);
        const double u1 = ((double)w.x + 1.0) * (1.0 / 4294967296.0), u2 = u01(w.y);
        const double z = sqrt(-2.0 * log(u1)) * cos(6.283185307179586 * u2);
        double v = T.mu + T.sigma * z;
        if (T.mode == 1) v = exp(v);
        tl = v;
        w1 = trc_keep(size, to_int(v), T.min_len, cut3);
    } else {
        // KDE model (src/truncate.cpp:322-351): truncation length from the row nearest to the molecule's size, averaged with the
        // next row's draw at the same quantile; share of the 3' end from the end-ratio histogram
        const Ph4m w = philox_mol(T.seed, g, ST_TRC_LEN, 0);
        int d = 0;
        {
            int lo = 0, hi = T.ny;                                     // lower_bound(y labels, size)
            while (lo < hi) { const int mid = (lo + hi) >> 1; if (T.ylab[mid] < (long long)size) lo = mid + 1; else hi = mid; }
            d = min(lo, T.ny - 1);
            if (lo < T.ny && d > 0 && llabs(T.ylab[d] - (long long)size) > llabs(T.ylab[d - 1] - (long long)size)) d--;
        }
        const double u = u01(w.x);
        double val = trc_row_draw(T, d, u, w.y);
        if (d + 1 < T.ny) val = (val + trc_row_draw(T, d + 1, u, w.z)) / 2.0;
        tl = T.models_length ? (double)size - val : val;
        if (T.always_end && !T.have_sider) side = 1.0;
        else {
            const Ph4m s = philox_mol(T.seed, g, ST_TRC_SIDE, 0);
            int bin = lower_bound_d(T.scdf, T.ns + 1, u01(s.x)) - 1;
            bin = max(0, min(bin, T.ns - 1));
            const double lo = bin == 0 ? 0.0 : T.slab[bin - 1], hi = T.slab[bin];
            side = lo + (hi - lo) * u01(s.y);
        }
        w1 = trc_keep(size, to_int((double)size - tl * side), T.min_len, cut3);
        const int s1 = w1;
        const int l2 = trc_keep(s1, to_int((double)s1 - tl * (1.0 - side)), T.min_len, cut5);
        w0 = s1 - l2;
    }
    keep_from[r] = (uint32_t)w0 | (cut5 ? 0x80000000u : 0u);
    keep_to[r] = (uint32_t)w1 | (cut3 ? 0x80000000u : 0u);
    tr_len[r] = tl; tr_side[r] = side;
    // sizes of the truncated molecule
    const uint32_t ib = B.reads[2 * r], ic = B.reads[2 * r + 1];
    uint64_t ni = 0, nm = 0;
    int c = 0;
    for (uint32_t i = 0; i < ic; i++) {
        const uint32_t* iv = B.intervals + 4ull * (ib + i);
        const int sz = (int)seg_size(iv);
        const int lo = max(w0, c), hi = min(w1, c + sz);
        const bool keep = sz > 0 ? hi > lo : ((!cut3 || c < w1) && (!cut5 || c > w0));
        if (keep) {
            ni++;
            const bool minus = iv[3] >> 31;
            const int fx = minus ? c + sz - hi : lo - c, fy = minus ? c + sz - lo : hi - c;     // forward offsets kept
            const uint32_t mb = iv[3] & 0x7fffffffu, me = iv[7] & 0x7fffffffu;
            for (uint32_t q = mb; q < me; q++) { const int p = (int)B.mods[2ull * q]; nm += (sz == 0 || (p >= fx && p < fy)) ? 1 : 0; }
        }
        c += sz;
    }
    n_ivls[r] = ni; n_mods[r] = nm;
    // the molecules come out of the MDF reader unrolled (stream_mdf(..., true), src/mdf.h:97-105): copies of a depth > 1
    // molecule are named id_0, id_1, ...
    n_idlen[r] = B.ids[2 * r + 1] + ((M.dup && (M.dup[r] >> 31)) ? 1u + (uint32_t)ndig(M.dup[r] & 0x7fffffffu) : 0u);
}

__global__ void k_trc_write(MolView M, const uint32_t* __restrict__ keep_from, const uint32_t* __restrict__ keep_to, MolOffsets F, MolOut O) {
    const uint64_t* __restrict__ ivl_off = F.ivl; const uint64_t* __restrict__ mod_off = F.mod; const uint64_t* __restrict__ id_off = F.id;
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= M.B.n_reads) return;
    const BatchView& B = M.B;
    const int w0 = (int)(keep_from[r] & 0x7fffffffu), w1 = (int)(keep_to[r] & 0x7fffffffu);
    const bool cut5 = keep_from[r] >> 31, cut3 = keep_to[r] >> 31;
    const uint32_t ib = B.reads[2 * r], ic = B.reads[2 * r + 1];
    uint64_t io = ivl_off[r], mo = mod_off[r];
    O.reads[2 * r] = (uint32_t)io; O.reads[2 * r + 1] = (uint32_t)(ivl_off[r + 1] - io);
    {
        uint8_t* d = O.idpool + id_off[r];
        const uint32_t so = B.ids[2 * r], sl = B.ids[2 * r + 1];
        uint32_t k = 0;
        for (; k < sl; k++) d[k] = B.idpool[so + k];
        if (M.dup && (M.dup[r] >> 31)) { d[k++] = '_'; k += (uint32_t)put_dec(d + k, M.dup[r] & 0x7fffffffu); }
        O.ids[2 * r] = (uint32_t)id_off[r]; O.ids[2 * r + 1] = k;
    }
    int c = 0;
    for (uint32_t i = 0; i < ic; i++) {
        const uint32_t* iv = B.intervals + 4ull * (ib + i);
        const int sz = (int)seg_size(iv);
        const int lo = max(w0, c), hi = min(w1, c + sz);
        const bool keep = sz > 0 ? hi > lo : ((!cut3 || c < w1) && (!cut5 || c > w0));
        if (keep) {
            const bool minus = iv[3] >> 31;
            const int fx = minus ? c + sz - hi : lo - c, fy = minus ? c + sz - lo : hi - c;
            uint32_t* ov = O.intervals + 4ull * io;
            ov[0] = iv[0];
            ov[1] = sz > 0 ? iv[1] + (uint32_t)fx : iv[1];
            ov[2] = sz > 0 ? iv[1] + (uint32_t)fy : iv[2];
            ov[3] = (uint32_t)mo | (iv[3] & 0x80000000u);
            const uint32_t mb = iv[3] & 0x7fffffffu, me = iv[7] & 0x7fffffffu;
            // truncate() sorts the substitutions of THE cut segment -- the first whose end reaches the kept length, even when
            // the cut falls on its boundary -- in the 3' pass and, on the flipped molecule, in the 5' pass
            const int szk = min(c + sz, w1) - c;                      // size after the 3' pass
            const bool was_cut = sz > 0 && ((cut3 && c < w1 && c + sz >= w1) || (cut5 && c <= w0 && w0 < c + szk));
            const uint64_t m_first = mo;
            for (uint32_t q = mb; q < me; q++) {
                const int p = (int)B.mods[2ull * q];
                if (sz == 0 || (p >= fx && p < fy)) { O.mods[2 * mo] = (uint32_t)(sz == 0 ? p : p - fx); O.mods[2 * mo + 1] = B.mods[2ull * q + 1]; mo++; }
            }
            if (was_cut) {
                // einterval::truncate sorts the substitutions of a cut segment by position (stable here)
                for (uint64_t a = m_first + 1; a < mo; a++) {
                    const uint32_t kp = O.mods[2 * a], kb = O.mods[2 * a + 1];
                    uint64_t b = a;
                    while (b > m_first && O.mods[2 * (b - 1)] > kp) { O.mods[2 * b] = O.mods[2 * (b - 1)]; O.mods[2 * b + 1] = O.mods[2 * (b - 1) + 1]; b--; }
                    O.mods[2 * b] = kp; O.mods[2 * b + 1] = kb;
                }
            }
            io++;
        }
        c += sz;
    }
}

// ------------------------------------------------------------------------------------------------
// polyA / tag / scb / flip: one generic segment edit.  A plan kernel per module decides, per molecule, a literal to put in front
// (pre), a literal to put behind (post) -- EDIT_NONE for none -- and whether the segments are flipped; k_edit_count sizes the
// result, k_edit_write copies it.  New literal intervals are {0x80000000 | literal, 0, len, mod_begin | plus}.
// ------------------------------------------------------------------------------------------------
DEV double u01o(uint32_t x) { return ((double)x + 1.0) * (1.0 / 4294967296.0); }       // (0, 1]
DEV double box_muller(uint32_t a, uint32_t b) { return sqrt(-2.0 * log(u01o(a))) * cos(6.283185307179586 * u01(b)); }

// std::poisson_distribution<int>: multiplication for lambda < 10 (uniforms: the words of blocks 0, 1, ... of the stream in order),
// PTRS (Hoermann 1993, "The transformed rejection method for generating Poisson random variables") above, one block per attempt
DEV double pla_poisson(uint64_t seed, uint64_t g, double lam) {
    if (lam < 10.0) {
        const double enlam = exp(-lam);
        double prod = 1.0, k = 0.0;
        for (uint32_t n = 0; n < PLA_MAX_ATTEMPTS * 4; n++) {
            const Ph4m w = philox_mol(seed, g, ST_PLA_LEN, n);
            const uint32_t ws[4] = {w.x, w.y, w.z, w.w};
            for (int j = 0; j < 4; j++) {
                prod *= u01(ws[j]);
                if (prod > enlam) k += 1.0; else return k;
            }
        }
        return k;
    }
    const double slam = sqrt(lam), loglam = log(lam);
    const double b = 0.931 + 2.53 * slam, a = -0.059 + 0.02483 * b;
    const double invalpha = 1.1239 + 1.1328 / (b - 3.4), vr = 0.9277 - 3.6224 / (b - 2.0);
    for (uint32_t n = 0; n < PLA_MAX_ATTEMPTS; n++) {
        const Ph4m w = philox_mol(seed, g, ST_PLA_LEN, n);
        const double U = u01(w.x) - 0.5, V = u01(w.y);
        const double us = 0.5 - fabs(U);
        const double k = floor((2.0 * a / us + b) * U + lam + 0.43);
        if (us >= 0.07 && V <= vr) return k;
        if (k < 0.0 || (us < 0.013 && V > us)) continue;
        if (log(V) + log(invalpha) - log(a / (us * us) + b) <= -lam + k * loglam - lgamma(k + 1.0)) return k;
    }
    return floor(lam);
}

DEV double pla_draw(const PlaParams& P, uint64_t g) {
    if (P.dist == PLA_POISSON) return pla_poisson(P.seed, g, P.a);
    if (P.dist == PLA_NORMAL) { const Ph4m w = philox_mol(P.seed, g, ST_PLA_LEN, 0); return P.a + P.b * box_muller(w.x, w.y); }
    if (P.dist == PLA_WEIBULL) { const Ph4m w = philox_mol(P.seed, g, ST_PLA_LEN, 0); return P.b * pow(-log(u01o(w.x)), 1.0 / P.a); }
    // gamma(shape a, scale b): Marsaglia & Tsang 2000 on shape a (a >= 1) or a + 1 (a < 1, times u^(1/a)); attempt n uses block n:
    // x, y -> the normal deviate, z -> the acceptance uniform, w -> the boost
    const double al = P.a < 1.0 ? P.a + 1.0 : P.a;
    const double d = al - 1.0 / 3.0, c = 1.0 / sqrt(9.0 * d);
    for (uint32_t n = 0; n < PLA_MAX_ATTEMPTS; n++) {
        const Ph4m w = philox_mol(P.seed, g, ST_PLA_LEN, n);
        const double z = box_muller(w.x, w.y);
        const double t = 1.0 + c * z;
        if (t <= 0.0) continue;
        const double v = t * t * t;
        if (log(u01o(w.z)) < 0.5 * z * z + d - d * v + d * log(v)) {
            double x = d * v;
            if (P.a < 1.0) x = x * pow(u01o(w.w), 1.0 / P.a);
            return x * P.b;
        }
    }
    return d * P.b;
}

// add_polyA (src/polyA.cpp:133-148): the draw, clamped to [min, max] in double (NaN -> min), then truncated toward zero
DEV int pla_length(const PlaParams& P, uint64_t g) {
    const double v = pla_draw(P, g);
    if (!(v >= (double)P.min_len)) return P.min_len;
    if (v > (double)P.max_len) return P.max_len;
    return (int)v;
}

__global__ void k_pla_plan(uint64_t n, PlaParams P, uint64_t first_index, uint32_t* __restrict__ post) {
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n) return;
    const int len = pla_length(P, first_index + r);
    post[r] = len > 0 ? P.lit_base + (uint32_t)(len - 1) : EDIT_NONE;     // literal lit_base + L - 1 is "A" x L
}

// fmt2seq's table (src/util.h:62-80): the choices of an IUPAC letter, packed a byte each, and their number (0: not in the table)
DEV uint32_t iupac(uint8_t c, int& k) {
    k = 1;
    switch (c) {
        case 'A': return 'A'; case 'G': return 'G'; case 'T': return 'T'; case 'C': return 'C'; case 'U': return 'U';
        case 'R': k = 2; return 'G' | 'A' << 8;                 case 'Y': k = 2; return 'T' | 'C' << 8;
        case 'K': k = 2; return 'G' | 'T' << 8;                 case 'M': k = 2; return 'A' | 'C' << 8;
        case 'S': k = 2; return 'G' | 'C' << 8;                 case 'W': k = 2; return 'A' | 'T' << 8;
        case 'B': k = 3; return 'G' | 'T' << 8 | 'C' << 16;     case 'D': k = 3; return 'G' | 'A' << 8 | 'T' << 16;
        case 'H': k = 3; return 'A' | 'C' << 8 | 'T' << 16;     case 'V': k = 3; return 'G' | 'C' << 8 | 'A' << 16;
        case 'N': k = 4; return 'A' | 'G' << 8 | 'C' << 16 | (uint32_t)'T' << 24;
        default: k = 0; return 0u;
    }
}

// one tag: character j of the (table-only) format is choice umulhi(word j of the stream, k) -- word j = component j % 4 of block j / 4
DEV void tag_draw(uint64_t seed, uint64_t g, uint32_t stream, const uint8_t* fmt, int len, uint8_t* dst) {
    Ph4m w{};
    for (int j = 0; j < len; j++) {
        if ((j & 3) == 0) w = philox_mol(seed, g, stream, (uint32_t)j >> 2);
        const uint32_t word = (j & 3) == 0 ? w.x : (j & 3) == 1 ? w.y : (j & 3) == 2 ? w.z : w.w;
        int k;
        const uint32_t opts = iupac(fmt[j], k);
        dst[j] = (uint8_t)(opts >> (8 * __umulhi(word, (uint32_t)k)));
    }
}

__global__ void k_tag_plan(uint64_t n, TagParams T, uint64_t first_index, uint32_t* __restrict__ pre, uint32_t* __restrict__ post,
                           uint64_t* __restrict__ lits, uint8_t* __restrict__ pool) {
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n) return;
    const uint64_t g = first_index + r;
    for (int e = 0; e < 2; e++) {
        const TagEnd& E = T.end[e];
        uint32_t li = E.shared;
        if (li == EDIT_NONE && E.len > 0) {
            // a literal of its own: entry lit_base + r, bytes at pool_base + r x len
            li = E.lit_base + (uint32_t)r;
            const uint64_t off = E.pool_base + r * (uint64_t)E.len;
            tag_draw(T.seed, g, e == 0 ? ST_TAG5 : ST_TAG3, E.fmt, E.len, pool + off);
            lits[2ull * li] = off; lits[2ull * li + 1] = (uint64_t)E.len;
        }
        (e == 0 ? pre : post)[r] = li;
    }
}

__global__ void k_flip_plan(uint64_t n, uint64_t seed, double p, uint64_t first_index, uint8_t* __restrict__ flip) {
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n) return;
    flip[r] = u01(philox_mol(seed, first_index + r, ST_FLIP, 0).x) < p ? 1 : 0;
}

DEV uint32_t unrolled_id_len(const MolView& M, uint64_t r) {
    return M.B.ids[2 * r + 1] + ((M.dup && (M.dup[r] >> 31)) ? 1u + (uint32_t)ndig(M.dup[r] & 0x7fffffffu) : 0u);
}

__global__ void k_edit_count(MolView M, const uint32_t* __restrict__ pre, const uint32_t* __restrict__ post, MolCounts C) {
    uint64_t* __restrict__ n_ivls = C.ivl; uint64_t* __restrict__ n_mods = C.mod; uint64_t* __restrict__ n_idlen = C.id;
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= M.B.n_reads) return;
    n_ivls[r] = M.B.reads[2 * r + 1] + ((pre && pre[r] != EDIT_NONE) ? 1u : 0u) + ((post && post[r] != EDIT_NONE) ? 1u : 0u);
    n_mods[r] = mol_mods(M.B, (uint32_t)r);
    n_idlen[r] = unrolled_id_len(M, r);
}

__global__ void k_edit_write(MolView M, const uint32_t* __restrict__ pre, const uint32_t* __restrict__ post, const uint8_t* __restrict__ flip,
                             const uint64_t* __restrict__ lits, MolOffsets F, MolOut O) {
    const uint64_t* __restrict__ ivl_off = F.ivl; const uint64_t* __restrict__ mod_off = F.mod; const uint64_t* __restrict__ id_off = F.id;
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= M.B.n_reads) return;
    const BatchView& B = M.B;
    const uint32_t ib = B.reads[2 * r], ic = B.reads[2 * r + 1];
    uint64_t io = ivl_off[r], mo = mod_off[r];
    O.reads[2 * r] = (uint32_t)io; O.reads[2 * r + 1] = (uint32_t)(ivl_off[r + 1] - io);
    {
        uint8_t* d = O.idpool + id_off[r];
        const uint32_t so = B.ids[2 * r], sl = B.ids[2 * r + 1];
        uint32_t k = 0;
        for (; k < sl; k++) d[k] = B.idpool[so + k];
        if (M.dup && (M.dup[r] >> 31)) { d[k++] = '_'; k += (uint32_t)put_dec(d + k, M.dup[r] & 0x7fffffffu); }
        O.ids[2 * r] = (uint32_t)id_off[r]; O.ids[2 * r + 1] = k;
    }
    auto put_literal = [&](uint32_t li) {
        uint32_t* ov = O.intervals + 4ull * io++;
        ov[0] = 0x80000000u | li; ov[1] = 0u; ov[2] = (uint32_t)lits[2ull * li + 1]; ov[3] = (uint32_t)mo;
    };
    if (pre && pre[r] != EDIT_NONE) put_literal(pre[r]);
    const bool fl = flip && flip[r];
    for (uint32_t q = 0; q < ic; q++) {
        const uint32_t i = fl ? ic - 1 - q : q;
        const uint32_t* iv = B.intervals + 4ull * (ib + i);
        uint32_t* ov = O.intervals + 4ull * io++;
        ov[0] = iv[0]; ov[1] = iv[1]; ov[2] = iv[2]; ov[3] = (uint32_t)mo | ((iv[3] ^ (fl ? 0x80000000u : 0u)) & 0x80000000u);
        const uint32_t mb = iv[3] & 0x7fffffffu, me = iv[7] & 0x7fffffffu;
        for (uint32_t m = mb; m < me; m++) { O.mods[2 * mo] = B.mods[2ull * m]; O.mods[2 * mo + 1] = B.mods[2ull * m + 1]; mo++; }
    }
    if (post && post[r] != EDIT_NONE) put_literal(post[r]);
}

// ------------------------------------------------------------------------------------------------
// random-wgs (src/random_wgs.cpp:181-207): molecules made here, not read.  One lane per CANDIDATE c (0, 1, 2, ... over the whole run): a
// uniform position on the concatenated contigs, a length from the named distribution clipped to the contig end, a strand.  A candidate
// whose clipped length is at least 1 is emitted; the run's output is the prefix of the emitted candidates whose bases before them are
// below base_count.  k_wgs_plan draws; launch_scan ranks the emitted ones and sums their bases; k_wgs_cut finds the end of the prefix and
// sizes the ids (the molecule index is the rank: known only after the scan); k_wgs_write fills the tables.
// ------------------------------------------------------------------------------------------------
DEV double u53(uint32_t hi, uint32_t lo) { return (double)(((unsigned long long)hi << 21) | (lo >> 11)) * (1.0 / 9007199254740992.0); }            // [0, 1)
DEV double u53o(uint32_t hi, uint32_t lo) { return ((double)(((unsigned long long)hi << 21) | (lo >> 11)) + 1.0) * (1.0 / 9007199254740992.0); }   // (0, 1]
DEV int ndig64(unsigned long long v) { int d = 1; while (v >= 10ull) { v /= 10ull; d++; } return d; }
DEV int put_dec64(uint8_t* o, unsigned long long v) { const int d = ndig64(v); for (int i = d - 1; i >= 0; i--) { o[i] = (uint8_t)('0' + v % 10ull); v /= 10ull; } return d; }

// the raw fragment length of candidate g (std:: parameterisation of a, b)
DEV double wgs_draw(const WgsParams& W, uint64_t g) {
    const Ph4m w = philox_mol(W.seed, g, ST_WGS_LEN, 0);
    if (W.dist == WGS_UNIFORM) return W.a + (W.b - W.a) * u53(w.x, w.y);
    if (W.dist == WGS_EXPONENTIAL) return -log(u53o(w.x, w.y)) / W.a;
    const double v = W.a + W.b * box_muller(w.x, w.y);
    return W.dist == WGS_LOGNORMAL ? exp(v) : v;
}
// double -> int toward zero, clamped to the int range in double first; NaN gives 0
DEV int wgs_to_int(double v) { return !(v == v) ? 0 : v >= 2147483647.0 ? 2147483647 : (v <= -2147483648.0 ? (-2147483647 - 1) : (int)v); }

// so_far: [n_contigs] running sums of the contig lengths.  The table is searched in LDS when it fits (WGS_LDS_CONTIGS entries), in
// global memory otherwise: first i with pos <= so_far[i] (the reference's while loop, :190-193)
__global__ void __launch_bounds__(256) k_wgs_plan(WgsParams W, const uint64_t* __restrict__ so_far, uint64_t first, uint64_t n,
                                                  uint4* __restrict__ plan, uint64_t* __restrict__ flag, uint64_t* __restrict__ bases) {
    __shared__ uint64_t tab[WGS_LDS_CONTIGS];
    const bool in_lds = W.n_contigs <= (uint32_t)WGS_LDS_CONTIGS;
    if (in_lds) {
        for (uint32_t i = threadIdx.x; i < W.n_contigs; i += blockDim.x) tab[i] = so_far[i];
        __syncthreads();
    }
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    const uint64_t g = first + t;
    const Ph4m wp = philox_mol(W.seed, g, ST_WGS_POS, 0);
    const unsigned long long pos = __umul64hi(((unsigned long long)wp.x << 32) | wp.y, W.ref_length);
    uint32_t lo = 0, hi = W.n_contigs - 1;                            // pos < ref_length = so_far[n_contigs - 1]: the answer is in [0, n_contigs)
    if (in_lds) { while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; if (tab[mid] < pos) lo = mid + 1; else hi = mid; } }
    else { while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; if (so_far[mid] < pos) lo = mid + 1; else hi = mid; } }
    const unsigned long long end = in_lds ? tab[lo] : so_far[lo], begin = lo ? (in_lds ? tab[lo - 1] : so_far[lo - 1]) : 0ull;
    const long long len = (long long)(end - begin);
    const long long ref_pos = (long long)(pos - end) + len;           // (:194) == pos - begin: 1 .. len, or 0 .. len on the first contig
    long long fl = wgs_to_int(wgs_draw(W, g));
    if (fl > len - ref_pos) fl = len - ref_pos;                       // (:196-198)
    const bool minus = (philox_mol(W.seed, g, ST_WGS_STRAND, 0).x & 1u) != 0u;
    const bool emit = fl >= 1;
    plan[t] = make_uint4(lo, (uint32_t)ref_pos, emit ? (uint32_t)fl : 0u, minus ? 1u : 0u);
    flag[t] = emit ? 1ull : 0ull;
    bases[t] = emit ? (unsigned long long)fl : 0ull;
}

// rank / bsum: exclusive scans of flag / bases ([n + 1]).  Candidate t is kept when it is emitted and the bases of the emitted candidates
// before it -- of this call and of the calls before (bases_before) -- are below base_count.  idlen[t]: bytes of the id of a kept candidate,
// "{index}_{contig}:{ref_pos}-{end}{+|-}", 0 otherwise.  The kept candidate that reaches base_count (at most one: emitted lengths are
// positive) reports the end of the run: cut = {molecules kept, bases kept, candidates consumed, 1}
__global__ void k_wgs_cut(uint64_t n, const uint4* __restrict__ plan, const uint64_t* __restrict__ rank, const uint64_t* __restrict__ bsum,
                          const uint32_t* __restrict__ name_len, uint64_t mols_before, uint64_t bases_before, uint64_t base_count,
                          uint64_t* __restrict__ idlen, uint64_t* __restrict__ cut) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    const uint4 p = plan[t];
    const unsigned long long before = bases_before + bsum[t];
    const bool keep = p.z != 0u && before < base_count;
    idlen[t] = keep ? (uint64_t)(ndig64(mols_before + rank[t]) + 1 + (int)name_len[p.x] + 1 + ndig(p.y) + 1 + ndig(p.y + p.z) + 1) : 0ull;
    if (keep && before + p.z >= base_count) { cut[0] = rank[t] + 1ull; cut[1] = bsum[t] + p.z; cut[2] = t + 1ull; cut[3] = 1ull; }
}

__global__ void k_wgs_write(uint64_t n, const uint4* __restrict__ plan, const uint64_t* __restrict__ rank, const uint64_t* __restrict__ idlen,
                            const uint64_t* __restrict__ id_off, const uint32_t* __restrict__ name_off, const uint32_t* __restrict__ name_len,
                            const uint8_t* __restrict__ names, uint64_t mols_before, MolOut O) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n || idlen[t] == 0ull) return;
    const uint4 p = plan[t];
    const uint64_t j = rank[t];
    O.reads[2 * j] = (uint32_t)j; O.reads[2 * j + 1] = 1u;
    uint32_t* ov = O.intervals + 4ull * j;
    ov[0] = p.x; ov[1] = p.y; ov[2] = p.y + p.z; ov[3] = p.w << 31;   // no substitutions: mod_begin 0
    uint8_t* d = O.idpool + id_off[t];
    uint32_t k = (uint32_t)put_dec64(d, mols_before + j);
    d[k++] = '_';
    const uint8_t* nm = names + name_off[p.x];
    const uint32_t nl = name_len[p.x];
    for (uint32_t q = 0; q < nl; q++) d[k + q] = nm[q];
    k += nl;
    d[k++] = ':'; k += (uint32_t)put_dec(d + k, p.y);
    d[k++] = '-'; k += (uint32_t)put_dec(d + k, p.y + p.z);
    d[k++] = p.w ? '-' : '+';
    O.ids[2 * j] = (uint32_t)id_off[t]; O.ids[2 * j + 1] = k;
}

// ------------------------------------------------------------------------------------------------
// tail-noise (src/append_noise.cpp:83-128).  k_noise_plan: one lane per molecule draws the noise length L (Box-Muller on block 0 of
// ST_NOISE_LEN, exp for the lognormal; clamped in double, NaN -> 0, toward zero) and, for the palindromic mode, walks the segment sizes
// from the last one backwards until their sum is strictly above L (:93-107).
// Random mode (:118-126): letter j of molecule g is alphabet[umulhi(word j, k)], word j = component j % 4 of block j / 4 of
// ST_NOISE_SEQ -- the tag rule.  k_noise_fill is a FLAT grid, one lane per 4-letter Philox block of the whole batch, the owner found by
// binary search in the scan of the block counts: lengths vary from molecule to molecule (lognormal: by orders of magnitude), so a wave
// per molecule would idle most lanes on a 50-letter literal (13 blocks) and serialise a 10^6-letter one; the flat grid's work is even
// whatever the lengths are, at the price of ~21 probes of a table that stays in L2.  The literal then goes through k_edit_count /
// k_edit_write like an ambiguous tag.
// Palindromic mode: k_edit_count / k_edit_write size and write the molecule itself; k_pal_count / k_pal_write, ONE WAVE PER MOLECULE,
// add the hairpin behind it.  Lanes stride over the bases of a new segment 64 at a time; base t of the hairpin (t counts over the new
// segments in the order they are appended) draws components (0, 1) of block t / 2 of ST_NOISE_ERR when t is even, (2, 3) when odd:
// u01(first) < error_rate puts alphabet[umulhi(second, k)] at that position of its segment.  New substitutions are counted with ballot +
// popcount; the write pass recomputes the draws and places a new substitution at (running count) + (its rank in the ballot) + (copied
// substitutions at or before its position), a copied one at (its stable rank among the copied) + (new ones before its position): the
// segment's list comes out sorted by position, a copied substitution before a new one at the same position.  The copied substitutions
// of the cut copy are re-based to the kept range and those outside dropped (einterval::truncate); a copy cut to nothing is not written.
// ------------------------------------------------------------------------------------------------
DEV int noise_length(const NoiseParams& P, uint64_t g) {
    const Ph4m w = philox_mol(P.seed, g, ST_NOISE_LEN, 0);
    const double v = P.mu + P.sigma * box_muller(w.x, w.y);
    return wgs_to_int(P.dist == NOISE_LOGNORMAL ? exp(v) : v);
}

__global__ void k_noise_plan(MolView M, NoiseParams P, uint64_t first_index, uint32_t* __restrict__ len, uint64_t* __restrict__ nblk,
                             unsigned long long* __restrict__ over, uint4* __restrict__ plan) {
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= M.B.n_reads) return;
    const int L = noise_length(P, first_index + r);
    if (!plan) {
        uint32_t l = L > 0 ? (uint32_t)L : 0u;
        if (l > (uint32_t)NOISE_MAX_LEN) { atomicMin(over, (unsigned long long)r); l = 0u; }
        len[r] = l; nblk[r] = (l + 3u) >> 2;
        return;
    }
    uint32_t ncopy = 0, extra = 0;
    unsigned long long total = 0ull;
    if (L > 0) {
        const uint32_t ib = M.B.reads[2 * r], ic = M.B.reads[2 * r + 1];
        for (uint32_t q = 0; q < ic; q++) {
            total += seg_size(M.B.intervals + 4ull * (ib + ic - 1 - q));
            ncopy++;
            if (total > (unsigned long long)L) { extra = (uint32_t)(total - (unsigned long long)L); break; }
        }
    }
    plan[r] = make_uint4(ncopy, extra, (uint32_t)(total - extra), 0u);
}

__global__ void k_noise_fill(uint64_t n, uint64_t n_blocks, NoiseParams P, uint64_t first_index, const uint32_t* __restrict__ len,
                             const uint64_t* __restrict__ blk_off, uint32_t lit_base, uint64_t pool_base, uint64_t* __restrict__ lits,
                             uint8_t* __restrict__ pool, uint32_t* __restrict__ post) {
    const uint64_t b = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= n_blocks) return;
    uint64_t lo = 0, hi = n;                                          // the owner: the last r with blk_off[r] <= b (blk_off[n] = n_blocks > b)
    while (lo + 1 < hi) { const uint64_t mid = (lo + hi) >> 1; if (blk_off[mid] <= b) lo = mid; else hi = mid; }
    const uint64_t r = lo, at = pool_base + 4ull * blk_off[r];
    const uint32_t jb = (uint32_t)(b - blk_off[r]), L = len[r];
    if (jb == 0u) {
        const uint32_t li = lit_base + (uint32_t)r;
        lits[2ull * li] = at; lits[2ull * li + 1] = L;
        post[r] = li;
    }
    const Ph4m w = philox_mol(P.seed, first_index + r, ST_NOISE_SEQ, jb);
    const uint32_t ws[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
    for (int c = 0; c < 4; c++) {
        const uint32_t j = 4u * jb + (uint32_t)c;
        if (j < L) pool[at + j] = P.alphabet[__umulhi(ws[c], P.k)];
    }
}

// copy q (0: of the last segment) of the hairpin of a molecule with plan pl
struct PalSeg {
    const uint32_t* iv;
    uint32_t nsz, fx, mb, me;             // bases of the copy; first forward offset kept (substitutions are re-based by it); the original's substitutions
    bool cut;
};
DEV PalSeg pal_seg(const BatchView& B, uint32_t ib, uint32_t ic, uint32_t q, const uint4& pl) {
    PalSeg s;
    s.iv = B.intervals + 4ull * (ib + ic - 1 - q);
    const uint32_t sz = seg_size(s.iv);
    s.cut = q + 1 == pl.x && pl.y > 0u;
    s.nsz = s.cut ? sz - pl.y : sz;
    s.fx = (s.cut && (s.iv[3] >> 31)) ? pl.y : 0u;                    // original on the plus strand: end -= extra; on the minus strand: start += extra
    s.mb = s.iv[3] & 0x7fffffffu; s.me = s.iv[7] & 0x7fffffffu;
    return s;
}
DEV bool pal_kept(const PalSeg& s, uint32_t p) { return !s.cut || (p >= s.fx && p - s.fx < s.nsz); }
DEV uint32_t pal_kept_count(const BatchView& B, const PalSeg& s, uint32_t lane) {
    if (!s.cut) return s.me - s.mb;
    uint32_t n = 0;
    for (uint32_t m0 = s.mb; m0 < s.me; m0 += 64u) {
        const uint32_t m = m0 + lane;
        n += (uint32_t)__popcll(__ballot(m < s.me && pal_kept(s, B.mods[2ull * m])));
    }
    return n;
}
DEV bool noise_hit(const NoiseParams& P, uint64_t g, uint32_t t, uint32_t& pick) {
    const Ph4m w = philox_mol(P.seed, g, ST_NOISE_ERR, t >> 1);
    pick = __umulhi((t & 1u) ? w.w : w.y, P.k);
    return u01((t & 1u) ? w.z : w.x) < P.error_rate;
}

__global__ void __launch_bounds__(256) k_pal_count(MolView M, NoiseParams P, uint64_t first_index, const uint4* __restrict__ plan, MolCounts C) {
    uint64_t* __restrict__ n_ivls = C.ivl; uint64_t* __restrict__ n_mods = C.mod;
    const uint64_t r = (uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6);
    if (r >= M.B.n_reads) return;
    const uint32_t lane = threadIdx.x & 63u;
    const uint4 pl = plan[r];
    if (pl.x == 0u) return;
    const BatchView& B = M.B;
    const uint32_t ib = B.reads[2 * r], ic = B.reads[2 * r + 1];
    const uint64_t g = first_index + r;
    const bool draws = P.error_rate > 0.0;                            // (<= 0: no draw is below it)
    uint32_t t0 = 0, nseg = 0;
    uint64_t nm = 0;
    for (uint32_t q = 0; q < pl.x; q++) {
        const PalSeg s = pal_seg(B, ib, ic, q, pl);
        if (s.cut && s.nsz == 0u) continue;
        nseg++;
        nm += pal_kept_count(B, s, lane);
        if (draws)
            for (uint64_t c0 = 0; c0 < s.nsz; c0 += 64u) {
                const uint64_t j = c0 + lane;
                uint32_t pick;
                nm += (uint64_t)__popcll(__ballot(j < s.nsz && noise_hit(P, g, t0 + (uint32_t)j, pick)));
            }
        t0 += s.nsz;
    }
    if (lane == 0u) { n_ivls[r] += nseg; n_mods[r] += nm; }
}

__global__ void __launch_bounds__(256) k_pal_write(MolView M, NoiseParams P, uint64_t first_index, const uint4* __restrict__ plan, MolOffsets F,
                                                   MolOut O) {
    const uint64_t* __restrict__ ivl_off = F.ivl; const uint64_t* __restrict__ mod_off = F.mod;
    const uint64_t r = (uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6);
    if (r >= M.B.n_reads) return;
    const uint32_t lane = threadIdx.x & 63u;
    const uint4 pl = plan[r];
    if (pl.x == 0u) return;
    const BatchView& B = M.B;
    const uint32_t ib = B.reads[2 * r], ic = B.reads[2 * r + 1];
    const uint64_t g = first_index + r;
    const bool draws = P.error_rate > 0.0;
    uint64_t io = ivl_off[r] + ic, mo = mod_off[r] + mol_mods(B, (uint32_t)r);      // behind what k_edit_write wrote
    uint32_t t0 = 0;
    for (uint32_t q = 0; q < pl.x; q++) {
        const PalSeg s = pal_seg(B, ib, ic, q, pl);
        if (s.cut && s.nsz == 0u) continue;
        if (lane == 0u) {
            const bool minus = s.iv[3] >> 31;
            uint32_t* ov = O.intervals + 4ull * io;
            ov[0] = s.iv[0];
            ov[1] = s.iv[1] + s.fx;
            ov[2] = (s.cut && !minus) ? s.iv[2] - pl.y : s.iv[2];
            ov[3] = (uint32_t)mo | (minus ? 0u : 0x80000000u);        // strand toggled
        }
        io++;
        const uint32_t kept = pal_kept_count(B, s, lane);
        // stable rank of the copied substitution m among the kept ones, by re-based position
        auto srank = [&](uint32_t m, uint32_t pr) {
            uint32_t k = 0;
            for (uint32_t x = s.mb; x < s.me; x++) {
                const uint32_t px = B.mods[2ull * x];
                if (pal_kept(s, px)) k += (px - s.fx < pr || (px - s.fx == pr && x < m)) ? 1u : 0u;
            }
            return k;
        };
        uint32_t n_new = 0;
        uint64_t c0 = 0;
        for (; c0 < s.nsz; c0 += 64u) {
            const uint64_t j = c0 + lane;
            uint32_t pick = 0;
            const bool hit = draws && j < s.nsz && noise_hit(P, g, t0 + (uint32_t)j, pick);
            const unsigned long long mask = __ballot(hit);
            if (hit) {
                uint32_t before = 0;                                  // copied substitutions at or before position j
                for (uint32_t x = s.mb; x < s.me; x++) { const uint32_t px = B.mods[2ull * x]; before += (pal_kept(s, px) && px - s.fx <= (uint32_t)j) ? 1u : 0u; }
                const uint64_t at = mo + n_new + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull)) + before;
                O.mods[2 * at] = (uint32_t)j; O.mods[2 * at + 1] = P.alphabet[pick];
            }
            for (uint32_t m = s.mb + lane; m < s.me; m += 64u) {       // copied substitutions whose position falls into this run of 64
                const uint32_t p = B.mods[2ull * m];
                if (!pal_kept(s, p)) continue;
                const uint32_t pr = p - s.fx;
                if (pr < c0 || pr >= c0 + 64u) continue;
                const uint64_t at = mo + srank(m, pr) + n_new + (uint32_t)__popcll(mask & ((1ull << (pr - (uint32_t)c0)) - 1ull));
                O.mods[2 * at] = pr; O.mods[2 * at + 1] = B.mods[2ull * m + 1];
            }
            n_new += (uint32_t)__popcll(mask);
        }
        for (uint32_t m = s.mb + lane; m < s.me; m += 64u) {           // positions beyond the segment (an uncut copy keeps them, as the reference does)
            const uint32_t p = B.mods[2ull * m];
            if (!pal_kept(s, p) || p - s.fx < c0) continue;
            const uint64_t at = mo + srank(m, p - s.fx) + n_new;
            O.mods[2 * at] = p - s.fx; O.mods[2 * at + 1] = B.mods[2ull * m + 1];
        }
        mo += kept + n_new;
        t0 += s.nsz;
    }
}

// ------------------------------------------------------------------------------------------------
// transcribe (src/transcribe.cpp:170-197): molecules made here from the transcript table of the context and the rows of an abundance
// table.  k_tsb_count, one lane per ROW: count = ((W x tpm) x molecule_count) / sum_tpm in double, in this order (:181; sum_tpm is the
// host's left-to-right sum, :170); carry = count - int(count); one uniform of Philox(seed, row index, ST_TSB, 0) below the carry adds 1
// (:182-186); depth = int(count), with the clamp-in-double and NaN -> 0 rule of wgs_to_int for both conversions.  A row is emitted when its
// transcript was found and depth >= 1.  launch_scan ranks the emitted rows (the molecule index of :195 is the rank), k_tsb_size then
// knows every row's id length, and three more scans give each row's first molecule, first interval and first id byte.
// k_tsb_write fills the tables of any slice of the unrolled molecule range.  A row owns between one and 10^6 molecules and a transcript one
// to several hundred exons, so neither a lane nor a wave per row (or per molecule) has even work: one would serialise a million copies
// behind one lane, the other idle 63 lanes on a single-exon transcript.  The grid is FLAT over the OUTPUT instead (the k_noise_fill
// argument): lane t writes molecule t of the slice -- its reads entry, id and dup word -- and interval t of the slice, each owner found by
// a binary search in the scans (~22 probes for 4 M rows; the upper levels of the search are the same lines for every lane and stay in L2,
// the last ones are shared by neighbouring lanes).  The stores are what matters: lane t stores the 16 bytes of interval t, so a wave
// writes 1 KB in one piece whatever the exon counts are, and the exon tuples it copies come from a table that is small next to the
// output (8 exons per transcript on average: read once from HBM, then from L2).  Nothing is staged in LDS: no element is used by a
// second lane.
// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_tsb_count(uint64_t n, TsbCount P, const uint32_t* __restrict__ tx, const double* __restrict__ tpm,
                                                   uint64_t* __restrict__ depth, uint64_t* __restrict__ flag) {
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n) return;
    double c = ((P.weight * tpm[r]) * P.molecule_count) / P.sum_tpm;
    const double carry = c - (double)wgs_to_int(c);
    const Ph4m w = philox_mol(P.seed, P.first_row + r, ST_TSB, 0);
    if (u53(w.x, w.y) < carry) c += 1.0;
    const int d = wgs_to_int(c);
    const bool emit = tx[r] != 0xffffffffu && d >= 1;
    depth[r] = emit ? (uint64_t)d : 0ull;
    flag[r] = emit ? 1ull : 0ull;
}

__global__ void __launch_bounds__(256) k_tsb_size(uint64_t n, const uint32_t* __restrict__ tx, const uint32_t* __restrict__ exon_first,
                                                  const uint64_t* __restrict__ depth, const uint64_t* __restrict__ rank, uint32_t prefix_len,
                                                  uint64_t* __restrict__ n_ivl, uint64_t* __restrict__ id_bytes) {
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n) return;
    const uint64_t d = depth[r];
    const uint32_t t = tx[r];
    n_ivl[r] = d ? d * (uint64_t)(exon_first[t + 1] - exon_first[t]) : 0ull;
    id_bytes[r] = d ? d * (uint64_t)(prefix_len + (uint32_t)ndig64(rank[r])) : 0ull;
}

// the owner of element v: the last r in [0, n) with first[r] <= v (first[0] = 0; rows without elements share their successor's start and
// are never the last)
DEV uint64_t tsb_owner(const uint64_t* __restrict__ first, uint64_t n, uint64_t v) {
    uint64_t lo = 0, hi = n;
    while (lo + 1 < hi) { const uint64_t mid = (lo + hi) >> 1; if (first[mid] <= v) lo = mid; else hi = mid; }
    return lo;
}

__global__ void __launch_bounds__(256) k_tsb_write(TsbPlanView V, uint64_t first_mol, uint64_t n_mol, uint64_t ivl_base, uint64_t n_ivl, uint64_t id_base,
                                                   MolOut O, uint32_t* __restrict__ dup) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t < n_mol) {
        const uint64_t m = first_mol + t;
        const uint64_t r = tsb_owner(V.mol_first, V.n_rows, m);
        const uint64_t copy = m - V.mol_first[r], depth = V.mol_first[r + 1] - V.mol_first[r];
        const uint32_t tr = V.tx[r], ec = V.exon_first[tr + 1] - V.exon_first[tr];
        O.reads[2 * t] = (uint32_t)(V.ivl_first[r] + copy * ec - ivl_base); O.reads[2 * t + 1] = ec;
        const uint64_t index = V.rank[r];
        const uint32_t idl = V.prefix_len + (uint32_t)ndig64(index);
        const uint64_t at = V.id_first[r] + copy * idl - id_base;
        uint8_t* d = O.idpool + at;
        for (uint32_t q = 0; q < V.prefix_len; q++) d[q] = V.prefix[q];
        put_dec64(d + V.prefix_len, index);
        O.ids[2 * t] = (uint32_t)at; O.ids[2 * t + 1] = idl;
        dup[t] = depth > 1ull ? (0x80000000u | (uint32_t)copy) : 0u;
    }
    if (t < n_ivl) {
        const uint64_t g = ivl_base + t;
        const uint64_t r = tsb_owner(V.ivl_first, V.n_rows, g);
        const uint32_t tr = V.tx[r], e0 = V.exon_first[tr], ec = V.exon_first[tr + 1] - e0;
        const uint64_t within = g - V.ivl_first[r];
        reinterpret_cast<uint4*>(O.intervals)[t] = V.exons[e0 + (uint32_t)(within % ec)];      // (mod_begin 0: no substitutions)
    }
}

// ------------------------------------------------------------------------------------------------
// filter (Flt, src/filter.cpp:21-117, :196-212) and concat (Mrg: `cat` of MDF files).  Both move whole molecules and draw nothing.
// k_flt_pred: one lane per unrolled molecule evaluates the conjunction -- `info` comes in as a byte per molecule (the host reads the
// comments), `size` and `locus` are computed here -- and writes the molecule's side, its rank flag and its three counts into the
// arrays of its side (0 into the other side's).  The scans of those give every molecule its slot; k_flt_write copies it there.
// k_cat_write copies one input of a concatenation behind the inputs before it: every index it carries is re-based.
// Kept quirk of the reference: interval::overlap (src/interval.h:38-58) has six branches and falls through to 0 for a range that
// shares exactly one end with the segment and sticks out on the other side (range.start < seg.start && range.end == seg.end;
// range.start == seg.start && range.end > seg.end), so `locus` misses those two overlaps.
// ------------------------------------------------------------------------------------------------
// this = [s, e) the segment, other = [os, oe) the range of the condition
DEV long long flt_overlap(long long s, long long e, long long os, long long oe) {
    if (oe <= s) return 0;                                            // BEFORE
    else if (os >= e) return 0;                                       // AFTER
    else if (os >= s && oe <= e) return oe - os;                      // IN
    else if (os < s && oe > e) return e - s;                          // AROUND
    else if (os < s && oe < e && oe > s) return oe - s;               // LEFT OVERLAP
    else if (os > s && os < e && oe > e) return e - os;               // RIGHT OVERLAP
    return 0;
}

// seg.chr == chr: a contig by its index, a literal by its text (the reference compares strings)
DEV bool flt_on_contig(const BatchView& B, uint32_t c, const FltCond& C) {
    if (!(c >> 31)) return c == C.contig;
    const uint32_t li = c & 0x7fffffffu;
    if (B.literals[2ull * li + 1] != (uint64_t)C.name_len) return false;
    const uint8_t* t = B.litpool + B.literals[2ull * li];
    for (uint32_t k = 0; k < C.name_len; k++) if (t[k] != C.name[k]) return false;
    return true;
}

DEV bool flt_holds(const BatchView& B, uint32_t r, const FltCond& C) {
    const uint32_t ib = B.reads[2 * r], ic = B.reads[2 * r + 1];
    if (C.kind == FLT_SIZE) {
        unsigned long long sz = 0;                                     // molecule_descriptor::size, src/interval.h:876
        for (uint32_t i = 0; i < ic; i++) sz += seg_size(B.intervals + 4ull * (ib + i));
        const unsigned long long v = (unsigned long long)C.value;
        switch (C.cmp) {
            case FLT_LT: return sz < v;   case FLT_LE: return sz <= v;   case FLT_GT: return sz > v;
            case FLT_GE: return sz >= v;  case FLT_EQ: return sz == v;   default: return sz != v;
        }
    }
    for (uint32_t i = 0; i < ic; i++) {                               // FLT_LOCUS: any segment (src/filter.cpp:89-112)
        const uint32_t* iv = B.intervals + 4ull * (ib + i);
        if (!flt_on_contig(B, iv[0], C)) continue;
        if (!C.ranged || flt_overlap((long long)iv[1], (long long)iv[2], C.start, C.end) > 0) return true;
    }
    return false;
}

__global__ void k_flt_pred(MolView M, const FltCond* __restrict__ conds, uint32_t n_conds, const uint8_t* __restrict__ info, int negate,
                           uint8_t* __restrict__ side, uint64_t* __restrict__ flag, MolCounts T, MolCounts F) {
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= M.B.n_reads) return;
    bool ok = info ? info[r] != 0 : true;
    for (uint32_t c = 0; c < n_conds && ok; c++) ok = flt_holds(M.B, (uint32_t)r, conds[c]);
    if (negate) ok = !ok;
    side[r] = ok ? 1 : 0;
    flag[r] = ok ? 1ull : 0ull;
    const uint64_t ni = M.B.reads[2 * r + 1], nm = mol_mods(M.B, (uint32_t)r), nd = unrolled_id_len(M, r);
    T.ivl[r] = ok ? ni : 0ull; T.mod[r] = ok ? nm : 0ull; T.id[r] = ok ? nd : 0ull;
    if (F.ivl) { F.ivl[r] = ok ? 0ull : ni; F.mod[r] = ok ? 0ull : nm; F.id[r] = ok ? 0ull : nd; }
}

// the id of molecule r of M (with the unroll suffix) becomes the id of molecule j of O, its bytes at id_at
DEV void copy_id(const MolView& M, uint64_t r, uint64_t j, uint64_t id_at, const MolOut& O) {
    const BatchView& B = M.B;
    uint8_t* d = O.idpool + id_at;
    const uint32_t so = B.ids[2 * r], sl = B.ids[2 * r + 1];
    uint32_t k = 0;
    for (; k < sl; k++) d[k] = B.idpool[so + k];
    if (M.dup && (M.dup[r] >> 31)) { d[k++] = '_'; k += (uint32_t)put_dec(d + k, M.dup[r] & 0x7fffffffu); }
    O.ids[2 * j] = (uint32_t)id_at; O.ids[2 * j + 1] = k;
}
// the segments of molecule r of M become the intervals of O from io on, their substitutions from mo on; literal indices move up by lit_shift
DEV void copy_segments(const MolView& M, uint64_t r, uint64_t io, uint64_t mo, uint32_t lit_shift, const MolOut& O) {
    const BatchView& B = M.B;
    const uint32_t ib = B.reads[2 * r], ic = B.reads[2 * r + 1];
    for (uint32_t i = 0; i < ic; i++) {
        const uint32_t* iv = B.intervals + 4ull * (ib + i);
        uint32_t* ov = O.intervals + 4ull * io++;
        ov[0] = (iv[0] >> 31) ? iv[0] + lit_shift : iv[0]; ov[1] = iv[1]; ov[2] = iv[2]; ov[3] = (uint32_t)mo | (iv[3] & 0x80000000u);
        const uint32_t mb = iv[3] & 0x7fffffffu, me = iv[7] & 0x7fffffffu;
        for (uint32_t m = mb; m < me; m++) { O.mods[2 * mo] = B.mods[2ull * m]; O.mods[2 * mo + 1] = B.mods[2ull * m + 1]; mo++; }
    }
}
// molecule r of M becomes molecule j of O: intervals from io, substitutions from mo, id bytes (with the unroll suffix) at id_at;
// literal indices move up by lit_shift
DEV void copy_molecule(const MolView& M, uint64_t r, uint64_t j, uint64_t io, uint64_t mo, uint64_t id_at, uint32_t lit_shift, const MolOut& O) {
    O.reads[2 * j] = (uint32_t)io; O.reads[2 * j + 1] = M.B.reads[2 * r + 1];
    copy_id(M, r, j, id_at, O);
    copy_segments(M, r, io, mo, lit_shift, O);
}

// rank: exclusive scan of flag (molecules of the true side before r); T / F: the scans of the counts; OF is not touched without F
__global__ void k_flt_write(MolView M, const uint8_t* __restrict__ side, const uint64_t* __restrict__ rank, MolOffsets T, MolOffsets F, MolOut OT, MolOut OF) {
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= M.B.n_reads) return;
    if (side[r]) copy_molecule(M, r, rank[r], T.ivl[r], T.mod[r], T.id[r], 0u, OT);
    else if (F.ivl) copy_molecule(M, r, r - rank[r], F.ivl[r], F.mod[r], F.id[r], 0u, OF);
}

// one input of a concatenation: its molecules (lanes below n_reads) and its literal entries (lanes below n_literals)
__global__ void k_cat_write(MolView M, MolOffsets F, CatBase base, uint64_t* __restrict__ lits, MolOut O) {
    const uint64_t* __restrict__ ivl_off = F.ivl; const uint64_t* __restrict__ mod_off = F.mod; const uint64_t* __restrict__ id_off = F.id;
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r < M.B.n_reads) copy_molecule(M, r, base.mol + r, base.ivl + ivl_off[r], base.mod + mod_off[r], base.id + id_off[r], base.lit, O);
    if (r < M.B.n_literals) { lits[2ull * (base.lit + r)] = M.B.literals[2 * r] + base.pool; lits[2ull * (base.lit + r) + 1] = M.B.literals[2 * r + 1]; }
}

// ------------------------------------------------------------------------------------------------
// unsegment (Glu, src/unsegment.cpp:88-105 with molecule_descriptor::concat, src/interval.h:893-896): a molecule is glued behind its
// predecessor with a probability.  Unrolled molecule g of the whole input joins when g > 0 and u01(Philox(seed, g, ST_GLUE, 0).x) <
// probability; the first molecule of a call is a head whatever it draws.  A chain -- a head and the joiners behind it -- becomes ONE
// molecule: the head's id, the segments of all members in order.  Chains are contiguous, so the output's interval and substitution
// tables are the input's unrolled ones in the same order: every lane copies its own molecule's segments to the offsets the scans give
// it, however long its chain is, and only the heads write a reads entry and an id.  A head finds the end of its chain without walking
// it: rank is the exclusive scan of the head flags, non-decreasing, so the next head is the last index whose rank is still this head's
// rank + 1 (n when there is none) -- a binary search, the same whether the chain has two members or spans many blocks.
// Two departures from the reference, both deliberate: the last chain IS written (the reference's loop never writes its
// last `current`), and every unrolled molecule draws for itself (the reference glues records, so a depth-3 head gives three equal
// chimeras and a joiner's depth is lost).
// ------------------------------------------------------------------------------------------------
__global__ void k_glue_plan(MolView M, uint64_t seed, double p, uint64_t first_index, uint8_t* __restrict__ join, uint64_t* __restrict__ head,
                            MolCounts C) {
    uint64_t* __restrict__ n_ivls = C.ivl; uint64_t* __restrict__ n_mods = C.mod; uint64_t* __restrict__ n_idlen = C.id;
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= M.B.n_reads) return;
    const bool j = r > 0 && u01(philox_mol(seed, first_index + r, ST_GLUE, 0).x) < p;      // (NaN compares false: nothing joins)
    join[r] = j ? 1 : 0;
    head[r] = j ? 0ull : 1ull;
    n_ivls[r] = M.B.reads[2 * r + 1];
    n_mods[r] = mol_mods(M.B, (uint32_t)r);
    n_idlen[r] = j ? 0ull : (uint64_t)unrolled_id_len(M, r);
}

// rank: exclusive scan of head ([n + 1]); ivl_off / mod_off / id_off: the scans of the counts
__global__ void k_glue_write(MolView M, const uint8_t* __restrict__ join, const uint64_t* __restrict__ rank, MolOffsets F, MolOut O) {
    const uint64_t* __restrict__ ivl_off = F.ivl; const uint64_t* __restrict__ mod_off = F.mod; const uint64_t* __restrict__ id_off = F.id;
    const uint64_t n = M.B.n_reads;
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n) return;
    copy_segments(M, r, ivl_off[r], mod_off[r], 0u, O);
    if (join[r]) return;
    const uint64_t j = rank[r];
    uint64_t lo = r + 1, hi = n;                                      // the last index in [r + 1, n] with rank <= j + 1 (rank[r + 1] = j + 1)
    while (lo < hi) { const uint64_t mid = (lo + hi + 1) >> 1; if (rank[mid] <= j + 1) lo = mid; else hi = mid - 1; }
    O.reads[2 * j] = (uint32_t)ivl_off[r]; O.reads[2 * j + 1] = (uint32_t)(ivl_off[lo] - ivl_off[r]);
    copy_id(M, r, j, id_off[r], O);
}

// ------------------------------------------------------------------------------------------------
// shuffle (Shf, Shuffle_module::shuffle_stream, src/shuffle.cpp:23-44).  The reference keeps a buffer of B molecules: molecule t >= B
// draws a slot, the slot's occupant is written and t takes its place; at the end the buffer is shuffled and written.  Here the draws are
// counter-based -- slot_t = umulhi(Philox(seed, t, ST_SHF_SLOT, 0).x, B), and the final order of the slots is that of (key(s), s) with
// key(s) = x << 32 | y of Philox(seed, s, ST_SHF_KEY, 0) -- so the loop need not be run in sequence: after a STABLE sort of the arrivals
// (slot_t, t) by slot the arrivals of one slot stand together in t order, the molecule written at step t is the arrival before it in
// that run (the molecule numbered slot_t, the slot's first occupant, when t opens the run), and the slot's final occupant is the last
// arrival of its run (s itself for a slot nothing arrived in).  Without a buffer size (or B >= n) every molecule has a slot of its
// own, there are no arrivals, and the output is the order of (key(i), i): a uniformly random permutation up to key collisions.
// k_shf_key: one lane per slot; k_shf_slot: one lane per arrival; the sorts are rocprim's radix sort (launch_abund_iota / abund_sort_*);
// k_shf_evict: one lane per sorted arrival fills src[0, n - B); k_shf_occupant: one lane per slot in key order fills src[n - B, n).
// src[j] is the input molecule that becomes output molecule j; k_gather_count / k_gather_write size and copy in that order.
// ------------------------------------------------------------------------------------------------
__global__ void k_shf_key(uint64_t n_slots, uint64_t seed, uint64_t* __restrict__ key) {
    const uint64_t s = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n_slots) return;
    const Ph4m w = philox_mol(seed, s, ST_SHF_KEY, 0);
    key[s] = ((uint64_t)w.x << 32) | w.y;
}

// arrival a is molecule t = B + a
__global__ void k_shf_slot(uint64_t n_arrivals, uint32_t B, uint64_t seed, uint32_t* __restrict__ slot) {
    const uint64_t a = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (a >= n_arrivals) return;
    slot[a] = __umulhi(philox_mol(seed, (uint64_t)B + a, ST_SHF_SLOT, 0).x, B);
}

// slot_s / arr_s: the arrivals' slots and indices after the stable sort by slot
__global__ void k_shf_evict(uint64_t n_arrivals, uint32_t B, const uint32_t* __restrict__ slot_s, const uint32_t* __restrict__ arr_s,
                            uint32_t* __restrict__ src) {
    const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n_arrivals) return;
    const uint32_t s = slot_s[k];
    src[arr_s[k]] = (k > 0 && slot_s[k - 1] == s) ? B + arr_s[k - 1] : s;
}

// order[q]: the slot at place q of the (key, slot) order; src_tail = src + n_arrivals
__global__ void k_shf_occupant(uint64_t n_slots, uint64_t n_arrivals, uint32_t B, const uint32_t* __restrict__ order, const uint32_t* __restrict__ slot_s,
                               const uint32_t* __restrict__ arr_s, uint32_t* __restrict__ src_tail) {
    const uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n_slots) return;
    const uint32_t s = order[q];
    uint64_t lo = 0, hi = n_arrivals;                                 // the first sorted arrival whose slot is above s
    while (lo < hi) { const uint64_t mid = (lo + hi) >> 1; if (slot_s[mid] <= s) lo = mid + 1; else hi = mid; }
    src_tail[q] = (lo > 0 && slot_s[lo - 1] == s) ? B + arr_s[lo - 1] : s;
}

__global__ void k_gather_count(MolView M, const uint32_t* __restrict__ src, uint64_t n, MolCounts C) {
    uint64_t* __restrict__ n_ivls = C.ivl; uint64_t* __restrict__ n_mods = C.mod; uint64_t* __restrict__ n_idlen = C.id;
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const uint32_t r = src[j];
    n_ivls[j] = M.B.reads[2 * r + 1]; n_mods[j] = mol_mods(M.B, r); n_idlen[j] = unrolled_id_len(M, r);
}

__global__ void k_gather_write(MolView M, const uint32_t* __restrict__ src, uint64_t n, MolOffsets F, MolOut O) {
    const uint64_t* __restrict__ ivl_off = F.ivl; const uint64_t* __restrict__ mod_off = F.mod; const uint64_t* __restrict__ id_off = F.id;
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    copy_molecule(M, src[j], j, ivl_off[j], mod_off[j], id_off[j], 0u, O);
}

// ------------------------------------------------------------------------------------------------
// mutate: a variant table -- SNVs, insertions, deletions -- applied to every segment ("mutate"; the reference's src/mutate.cpp is
// unfinished, so the transform is specified there and in include/tksmseq.h).  The table comes in its normal form (mut_host.h): per contig
// the disjoint deleted ranges [del_from, del_to) ascending, and the point variants (SNVs and insertions outside every deleted range) by
// (position, table line).  k_mut_resolve: one lane per literal entry of the input finds the table contig whose NAME is the literal's text (a
// batch parsed without a reference knows its contigs as literals), by binary search over the names sorted by (length, bytes).
// k_mut_count / k_mut_write: one lane per molecule walks its segments.  A segment [s, e) on a table contig finds its deleted ranges (the first
// with del_to > s, up to the first with del_from >= e) and its points (lower bounds of s and e) by binary search -- a table of millions of
// rows is a few tens of MB that stay in L2 -- and then, if there is a range or an insertion among them, merges the two lists by position:
// a range ends the running piece in front of it and moves on behind it, an insertion ends the piece behind its anchor and puts the
// insertion's literal (entry lit_base + ordinal of the output's literal table, shared by all molecules) after it.  A piece [a, b) carries the
// segment's own substitutions that fall into it, re-based, then ALL of the table's letters with a <= POS < b in table order.  Without an
// event the segment is copied whole, its own substitutions untouched, the table's letters behind them.  A minus-strand segment comes out
// back to front: the write pass sizes the segment first (the same walk, counting), then fills intervals and substitutions from the end.
// ------------------------------------------------------------------------------------------------
DEV uint32_t mut_lower(const uint32_t* a, uint32_t lo, uint32_t hi, uint32_t key) {      // first index in [lo, hi) with a[index] >= key
    while (lo < hi) { const uint32_t mid = lo + ((hi - lo) >> 1); if (a[mid] < key) lo = mid + 1; else hi = mid; }
    return lo;
}

__global__ void k_mut_resolve(BatchView B, MutView V, uint32_t* __restrict__ lit_ctg, uint64_t* __restrict__ out_lits, uint32_t lit_base, uint64_t pool_base) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < B.n_literals) {
        const uint64_t len = B.literals[2 * i + 1];
        const uint8_t* t = B.litpool + B.literals[2 * i];
        uint32_t lo = 0, hi = V.n_contigs, found = MUT_NONE;
        while (lo < hi) {
            const uint32_t mid = lo + ((hi - lo) >> 1);
            const uint32_t no = V.name_off[mid], nl = V.name_off[mid + 1] - no;
            int c = (uint64_t)nl < len ? -1 : ((uint64_t)nl > len ? 1 : 0);
            for (uint32_t k = 0; c == 0 && k < nl; k++) c = (int)V.names[no + k] - (int)t[k];
            if (c == 0) { found = mid; break; }
            if (c < 0) lo = mid + 1; else hi = mid;
        }
        lit_ctg[i] = found;
    }
    if (i < V.n_ins) { out_lits[2ull * (lit_base + i)] = pool_base + V.ins_ent[2 * i]; out_lits[2ull * (lit_base + i) + 1] = V.ins_ent[2 * i + 1]; }
}

// One segment `iv` of the input.  WRITE false: io / mo are advanced by the intervals / substitutions the segment becomes.  WRITE true: they
// are written from io / mo on as well.
template <bool WRITE>
DEV void mut_segment(const BatchView& B, const MutView& V, const uint32_t* __restrict__ lit_ctg, const uint32_t* iv, uint32_t lit_base, uint64_t& io, uint64_t& mo,
                     const MolOut& O) {
    const uint32_t s = iv[1], e = iv[2], mb = iv[3] & 0x7fffffffu, me = iv[7] & 0x7fffffffu, strand = iv[3] & 0x80000000u;
    const uint32_t tc = (iv[0] >> 31) ? lit_ctg[iv[0] & 0x7fffffffu] : (iv[0] < V.n_ref ? V.ref_ctg[iv[0]] : MUT_NONE);
    uint32_t d0 = 0, d1 = 0, p0 = 0, p1 = 0;
    bool events = false;
    if (tc != MUT_NONE && e > s) {
        const uint32_t db = V.del_first[tc], de = V.del_first[tc + 1], pb = V.pt_first[tc], pe = V.pt_first[tc + 1];
        d0 = mut_lower(V.del_to, db, de, s + 1u);                     // the first range with del_to > s
        d1 = mut_lower(V.del_from, d0, de, e);                        // ... up to the first with del_from >= e
        p0 = mut_lower(V.pt_pos, pb, pe, s);
        p1 = mut_lower(V.pt_pos, p0, pe, e);
        events = d0 < d1;
        for (uint32_t q = p0; q < p1 && !events; q++) events = (V.pt_info[q] & MUT_PT_INSERTION) != 0ull;
    }
    if (!events) {
        if (WRITE) {
            uint32_t* ov = O.intervals + 4ull * io;
            ov[0] = iv[0]; ov[1] = s; ov[2] = e; ov[3] = (uint32_t)mo | strand;
            for (uint32_t m = mb; m < me; m++) { O.mods[2 * (mo + (m - mb))] = B.mods[2ull * m]; O.mods[2 * (mo + (m - mb)) + 1] = B.mods[2ull * m + 1]; }
        }
        io++; mo += me - mb;
        for (uint32_t q = p0; q < p1; q++) {                           // SNVs only: appended, as add_error appends
            const uint64_t info = V.pt_info[q];
            if (!(info & MUT_PT_LETTER)) continue;
            if (WRITE) { O.mods[2 * mo] = V.pt_pos[q] - s; O.mods[2 * mo + 1] = (uint32_t)(info >> 32) & 0xffu; }
            mo++;
        }
        return;
    }
    const bool back = WRITE && strand != 0u;                          // minus strand: filled from the end
    uint64_t hi_i = 0, hi_m = 0, seg_i = 0, seg_m = 0;
    if (back) { mut_segment<false>(B, V, lit_ctg, iv, lit_base, seg_i, seg_m, O); hi_i = io + seg_i; hi_m = mo + seg_m; }
    uint32_t cur = s, d = d0, q = p0, qs = p0;
    auto piece = [&](uint32_t a, uint32_t b) {
        const uint32_t fa = a - s, fb = b - s;
        uint32_t nm = 0;
        for (uint32_t m = mb; m < me; m++) { const uint32_t p = B.mods[2ull * m]; nm += (p >= fa && p < fb) ? 1u : 0u; }
        while (qs < p1 && V.pt_pos[qs] < a) qs++;
        uint32_t qe = qs;
        for (; qe < p1 && V.pt_pos[qe] < b; qe++) nm += (V.pt_info[qe] & MUT_PT_LETTER) ? 1u : 0u;
        if (WRITE) {
            if (back) hi_m -= nm;
            uint64_t at = back ? hi_m : mo;
            uint32_t* ov = O.intervals + 4ull * (back ? --hi_i : io);
            ov[0] = iv[0]; ov[1] = a; ov[2] = b; ov[3] = (uint32_t)at | strand;
            for (uint32_t m = mb; m < me; m++) {
                const uint32_t p = B.mods[2ull * m];
                if (p >= fa && p < fb) { O.mods[2 * at] = p - fa; O.mods[2 * at + 1] = B.mods[2ull * m + 1]; at++; }
            }
            for (uint32_t x = qs; x < qe; x++) {
                const uint64_t info = V.pt_info[x];
                if (info & MUT_PT_LETTER) { O.mods[2 * at] = V.pt_pos[x] - a; O.mods[2 * at + 1] = (uint32_t)(info >> 32) & 0xffu; at++; }
            }
        }
        if (!back) { io++; mo += nm; }
        qs = qe;
    };
    for (;;) {
        while (q < p1 && !(V.pt_info[q] & MUT_PT_INSERTION)) q++;     // the next insertion
        const bool hd = d < d1, hq = q < p1;
        if (!hd && !hq) break;
        if (hd && (!hq || V.del_from[d] <= V.pt_pos[q])) {            // (a kept point lies in no range)
            const uint32_t f = V.del_from[d], t = V.del_to[d];
            if (f > cur) piece(cur, f);
            cur = t < e ? t : e;
            d++;
        } else {
            const uint32_t p = V.pt_pos[q];
            if (p + 1u > cur) piece(cur, p + 1u);                     // (empty for a second insertion at the same anchor)
            if (WRITE) {
                const uint32_t li = (uint32_t)V.pt_info[q];
                uint32_t* ov = O.intervals + 4ull * (back ? --hi_i : io);
                ov[0] = 0x80000000u | (lit_base + li); ov[1] = 0u; ov[2] = (uint32_t)V.ins_ent[2ull * li + 1]; ov[3] = (uint32_t)(back ? hi_m : mo) | strand;
            }
            if (!back) io++;
            cur = p + 1u;
            q++;
        }
    }
    if (cur < e) piece(cur, e);
    if (back) { io += seg_i; mo += seg_m; }
}

__global__ void k_mut_count(MolView M, MutView V, const uint32_t* __restrict__ lit_ctg, MolCounts C) {
    uint64_t* __restrict__ n_ivls = C.ivl; uint64_t* __restrict__ n_mods = C.mod; uint64_t* __restrict__ n_idlen = C.id;
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= M.B.n_reads) return;
    const BatchView& B = M.B;
    const uint32_t ib = B.reads[2 * r], ic = B.reads[2 * r + 1];
    uint64_t ni = 0, nm = 0;
    for (uint32_t i = 0; i < ic; i++) mut_segment<false>(B, V, lit_ctg, B.intervals + 4ull * (ib + i), 0u, ni, nm, MolOut{});
    n_ivls[r] = ni; n_mods[r] = nm; n_idlen[r] = unrolled_id_len(M, r);
}

__global__ void k_mut_write(MolView M, MutView V, const uint32_t* __restrict__ lit_ctg, uint32_t lit_base, MolOffsets F, MolOut O) {
    const uint64_t* __restrict__ ivl_off = F.ivl; const uint64_t* __restrict__ mod_off = F.mod; const uint64_t* __restrict__ id_off = F.id;
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= M.B.n_reads) return;
    const BatchView& B = M.B;
    const uint32_t ib = B.reads[2 * r], ic = B.reads[2 * r + 1];
    uint64_t io = ivl_off[r], mo = mod_off[r];
    O.reads[2 * r] = (uint32_t)io; O.reads[2 * r + 1] = (uint32_t)(ivl_off[r + 1] - io);
    copy_id(M, r, r, id_off[r], O);
    for (uint32_t i = 0; i < ic; i++) mut_segment<true>(B, V, lit_ctg, B.intervals + 4ull * (ib + i), lit_base, io, mo, O);
}

// ------------------------------------------------------------------------------------------------
// launchers
// ------------------------------------------------------------------------------------------------
static inline unsigned nblk(uint64_t n) { return (unsigned)((n + 127) / 128); }

hipError_t launch_pcr_count(const MolView& m, const PcrParams& p, uint64_t* n_out, uint32_t* status, hipStream_t s) {
    if (!m.n_kept) return hipSuccess;
    hipLaunchKernelGGL(k_pcr_count, dim3(nblk(m.n_kept)), dim3(128), 0, s, m, p, n_out, status);
    return hipGetLastError();
}
hipError_t launch_pcr_list(const MolView& m, const PcrParams& p, const uint64_t* out_off, uint32_t* node_mol, uint64_t* node_mask, const MolCounts& c,
                           hipStream_t s) {
    if (!m.n_kept) return hipSuccess;
    hipLaunchKernelGGL(k_pcr_list, dim3(nblk(m.n_kept)), dim3(128), 0, s, m, p, out_off, node_mol, node_mask, c);
    return hipGetLastError();
}
hipError_t launch_pcr_write(const MolView& m, const PcrParams& p, uint64_t n_nodes, const uint32_t* node_mol, const uint64_t* node_mask,
                            const MolOffsets& f, const MolOut& o, hipStream_t s) {
    if (!n_nodes) return hipSuccess;
    hipLaunchKernelGGL(k_pcr_write, dim3(nblk(n_nodes)), dim3(128), 0, s, m, p, n_nodes, node_mol, node_mask, f, o);
    return hipGetLastError();
}
hipError_t launch_trc_plan(const MolView& m, const TrcParams& p, uint64_t first_index, uint32_t* keep_from, uint32_t* keep_to, double* tr_len,
                           double* tr_side, const MolCounts& c, hipStream_t s) {
    if (!m.B.n_reads) return hipSuccess;
    hipLaunchKernelGGL(k_trc_plan, dim3(nblk(m.B.n_reads)), dim3(128), 0, s, m, p, first_index, keep_from, keep_to, tr_len, tr_side, c);
    return hipGetLastError();
}
hipError_t launch_trc_write(const MolView& m, const uint32_t* keep_from, const uint32_t* keep_to, const MolOffsets& f, const MolOut& o, hipStream_t s) {
    if (!m.B.n_reads) return hipSuccess;
    hipLaunchKernelGGL(k_trc_write, dim3(nblk(m.B.n_reads)), dim3(128), 0, s, m, keep_from, keep_to, f, o);
    return hipGetLastError();
}

hipError_t launch_pla_plan(uint64_t n, const PlaParams& p, uint64_t first_index, uint32_t* post, hipStream_t s) {
    if (!n) return hipSuccess;
    hipLaunchKernelGGL(k_pla_plan, dim3(nblk(n)), dim3(128), 0, s, n, p, first_index, post);
    return hipGetLastError();
}
hipError_t launch_tag_plan(uint64_t n, const TagParams& p, uint64_t first_index, uint32_t* pre, uint32_t* post, uint64_t* lits, uint8_t* pool,
                           hipStream_t s) {
    if (!n) return hipSuccess;
    hipLaunchKernelGGL(k_tag_plan, dim3(nblk(n)), dim3(128), 0, s, n, p, first_index, pre, post, lits, pool);
    return hipGetLastError();
}
hipError_t launch_flip_plan(uint64_t n, uint64_t seed, double p, uint64_t first_index, uint8_t* flip, hipStream_t s) {
    if (!n) return hipSuccess;
    hipLaunchKernelGGL(k_flip_plan, dim3(nblk(n)), dim3(128), 0, s, n, seed, p, first_index, flip);
    return hipGetLastError();
}
hipError_t launch_edit_count(const MolView& m, const uint32_t* pre, const uint32_t* post, const MolCounts& c, hipStream_t s) {
    if (!m.B.n_reads) return hipSuccess;
    hipLaunchKernelGGL(k_edit_count, dim3(nblk(m.B.n_reads)), dim3(128), 0, s, m, pre, post, c);
    return hipGetLastError();
}
hipError_t launch_edit_write(const MolView& m, const uint32_t* pre, const uint32_t* post, const uint8_t* flip, const uint64_t* lits,
                             const MolOffsets& f, const MolOut& o, hipStream_t s) {
    if (!m.B.n_reads) return hipSuccess;
    hipLaunchKernelGGL(k_edit_write, dim3(nblk(m.B.n_reads)), dim3(128), 0, s, m, pre, post, flip, lits, f, o);
    return hipGetLastError();
}

hipError_t launch_flt_pred(const MolView& m, const FltCond* conds, uint32_t n_conds, const uint8_t* info, int negate, uint8_t* side, uint64_t* flag,
                           const MolCounts& t, const MolCounts& f, hipStream_t s) {
    if (!m.B.n_reads) return hipSuccess;
    hipLaunchKernelGGL(k_flt_pred, dim3(nblk(m.B.n_reads)), dim3(128), 0, s, m, conds, n_conds, info, negate, side, flag, t, f);
    return hipGetLastError();
}
hipError_t launch_flt_write(const MolView& m, const uint8_t* side, const uint64_t* rank, const MolOffsets& t, const MolOffsets& f, const MolOut& ot,
                            const MolOut& of, hipStream_t s) {
    if (!m.B.n_reads) return hipSuccess;
    hipLaunchKernelGGL(k_flt_write, dim3(nblk(m.B.n_reads)), dim3(128), 0, s, m, side, rank, t, f, ot, of);
    return hipGetLastError();
}
hipError_t launch_cat_write(const MolView& m, const MolOffsets& f, const CatBase& base, uint64_t* lits, const MolOut& o, hipStream_t s) {
    const uint64_t n = m.B.n_reads > m.B.n_literals ? m.B.n_reads : (uint64_t)m.B.n_literals;
    if (!n) return hipSuccess;
    hipLaunchKernelGGL(k_cat_write, dim3(nblk(n)), dim3(128), 0, s, m, f, base, lits, o);
    return hipGetLastError();
}

hipError_t launch_glue_plan(const MolView& m, uint64_t seed, double p, uint64_t first_index, uint8_t* join, uint64_t* head, const MolCounts& c,
                            hipStream_t s) {
    if (!m.B.n_reads) return hipSuccess;
    hipLaunchKernelGGL(k_glue_plan, dim3(nblk(m.B.n_reads)), dim3(128), 0, s, m, seed, p, first_index, join, head, c);
    return hipGetLastError();
}
hipError_t launch_glue_write(const MolView& m, const uint8_t* join, const uint64_t* rank, const MolOffsets& f, const MolOut& o, hipStream_t s) {
    if (!m.B.n_reads) return hipSuccess;
    hipLaunchKernelGGL(k_glue_write, dim3(nblk(m.B.n_reads)), dim3(128), 0, s, m, join, rank, f, o);
    return hipGetLastError();
}
hipError_t launch_shf_key(uint64_t n_slots, uint64_t seed, uint64_t* key, hipStream_t s) {
    if (!n_slots) return hipSuccess;
    hipLaunchKernelGGL(k_shf_key, dim3(nblk(n_slots)), dim3(128), 0, s, n_slots, seed, key);
    return hipGetLastError();
}
hipError_t launch_shf_slot(uint64_t n_arrivals, uint32_t n_slots, uint64_t seed, uint32_t* slot, hipStream_t s) {
    if (!n_arrivals) return hipSuccess;
    hipLaunchKernelGGL(k_shf_slot, dim3(nblk(n_arrivals)), dim3(128), 0, s, n_arrivals, n_slots, seed, slot);
    return hipGetLastError();
}
hipError_t launch_shf_evict(uint64_t n_arrivals, uint32_t n_slots, const uint32_t* slot_sorted, const uint32_t* arrival_sorted, uint32_t* src, hipStream_t s) {
    if (!n_arrivals) return hipSuccess;
    hipLaunchKernelGGL(k_shf_evict, dim3(nblk(n_arrivals)), dim3(128), 0, s, n_arrivals, n_slots, slot_sorted, arrival_sorted, src);
    return hipGetLastError();
}
hipError_t launch_shf_occupant(uint32_t n_slots, uint64_t n_arrivals, const uint32_t* order, const uint32_t* slot_sorted, const uint32_t* arrival_sorted,
                               uint32_t* src_tail, hipStream_t s) {
    if (!n_slots) return hipSuccess;
    hipLaunchKernelGGL(k_shf_occupant, dim3(nblk(n_slots)), dim3(128), 0, s, (uint64_t)n_slots, n_arrivals, n_slots, order, slot_sorted, arrival_sorted, src_tail);
    return hipGetLastError();
}
hipError_t launch_gather_count(const MolView& m, const uint32_t* src, uint64_t n, const MolCounts& c, hipStream_t s) {
    if (!n) return hipSuccess;
    hipLaunchKernelGGL(k_gather_count, dim3(nblk(n)), dim3(128), 0, s, m, src, n, c);
    return hipGetLastError();
}
hipError_t launch_gather_write(const MolView& m, const uint32_t* src, uint64_t n, const MolOffsets& f, const MolOut& o, hipStream_t s) {
    if (!n) return hipSuccess;
    hipLaunchKernelGGL(k_gather_write, dim3(nblk(n)), dim3(128), 0, s, m, src, n, f, o);
    return hipGetLastError();
}

hipError_t launch_mut_resolve(const BatchView& b, const MutView& v, uint32_t* lit_ctg, uint64_t* out_lits, uint32_t lit_base, uint64_t pool_base, hipStream_t s) {
    const uint64_t n = b.n_literals > v.n_ins ? b.n_literals : v.n_ins;
    if (!n) return hipSuccess;
    hipLaunchKernelGGL(k_mut_resolve, dim3(nblk(n)), dim3(128), 0, s, b, v, lit_ctg, out_lits, lit_base, pool_base);
    return hipGetLastError();
}
hipError_t launch_mut_count(const MolView& m, const MutView& v, const uint32_t* lit_ctg, const MolCounts& c, hipStream_t s) {
    if (!m.B.n_reads) return hipSuccess;
    hipLaunchKernelGGL(k_mut_count, dim3(nblk(m.B.n_reads)), dim3(128), 0, s, m, v, lit_ctg, c);
    return hipGetLastError();
}
hipError_t launch_mut_write(const MolView& m, const MutView& v, const uint32_t* lit_ctg, uint32_t lit_base, const MolOffsets& f, const MolOut& o,
                            hipStream_t s) {
    if (!m.B.n_reads) return hipSuccess;
    hipLaunchKernelGGL(k_mut_write, dim3(nblk(m.B.n_reads)), dim3(128), 0, s, m, v, lit_ctg, lit_base, f, o);
    return hipGetLastError();
}

hipError_t launch_wgs_plan(const WgsParams& p, const uint64_t* so_far, uint64_t first, uint64_t n, uint4* plan, uint64_t* flag, uint64_t* bases, hipStream_t s) {
    if (!n) return hipSuccess;
    hipLaunchKernelGGL(k_wgs_plan, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, p, so_far, first, n, plan, flag, bases);
    return hipGetLastError();
}
hipError_t launch_wgs_cut(uint64_t n, const uint4* plan, const uint64_t* rank, const uint64_t* bsum, const uint32_t* name_len, uint64_t mols_before,
                          uint64_t bases_before, uint64_t base_count, uint64_t* idlen, uint64_t* cut, hipStream_t s) {
    if (!n) return hipSuccess;
    hipLaunchKernelGGL(k_wgs_cut, dim3(nblk(n)), dim3(128), 0, s, n, plan, rank, bsum, name_len, mols_before, bases_before, base_count, idlen, cut);
    return hipGetLastError();
}
hipError_t launch_wgs_write(uint64_t n, const uint4* plan, const uint64_t* rank, const uint64_t* idlen, const uint64_t* id_off, const uint32_t* name_off,
                            const uint32_t* name_len, const uint8_t* names, uint64_t mols_before, const MolOut& o, hipStream_t s) {
    if (!n) return hipSuccess;
    hipLaunchKernelGGL(k_wgs_write, dim3(nblk(n)), dim3(128), 0, s, n, plan, rank, idlen, id_off, name_off, name_len, names, mols_before, o);
    return hipGetLastError();
}

hipError_t launch_tsb_count(uint64_t n_rows, const TsbCount& p, const uint32_t* tx, const double* tpm, uint64_t* depth, uint64_t* flag, hipStream_t s) {
    if (!n_rows) return hipSuccess;
    hipLaunchKernelGGL(k_tsb_count, dim3((unsigned)((n_rows + 255) / 256)), dim3(256), 0, s, n_rows, p, tx, tpm, depth, flag);
    return hipGetLastError();
}
hipError_t launch_tsb_size(uint64_t n_rows, const uint32_t* tx, const uint32_t* exon_first, const uint64_t* depth, const uint64_t* rank, uint32_t prefix_len,
                           uint64_t* n_ivl, uint64_t* id_bytes, hipStream_t s) {
    if (!n_rows) return hipSuccess;
    hipLaunchKernelGGL(k_tsb_size, dim3((unsigned)((n_rows + 255) / 256)), dim3(256), 0, s, n_rows, tx, exon_first, depth, rank, prefix_len, n_ivl, id_bytes);
    return hipGetLastError();
}
hipError_t launch_tsb_write(const TsbPlanView& v, uint64_t first_mol, uint64_t n_mol, uint64_t ivl_base, uint64_t n_ivl, uint64_t id_base, const MolOut& o,
                            uint32_t* dup, hipStream_t s) {
    const uint64_t n = n_mol > n_ivl ? n_mol : n_ivl;
    if (!n || !v.n_rows) return hipSuccess;
    hipLaunchKernelGGL(k_tsb_write, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, v, first_mol, n_mol, ivl_base, n_ivl, id_base, o, dup);
    return hipGetLastError();
}

hipError_t launch_noise_plan(const MolView& m, const NoiseParams& p, uint64_t first_index, uint32_t* len, uint64_t* n_blk, unsigned long long* over,
                             uint4* plan, hipStream_t s) {
    if (!m.B.n_reads) return hipSuccess;
    hipLaunchKernelGGL(k_noise_plan, dim3(nblk(m.B.n_reads)), dim3(128), 0, s, m, p, first_index, len, n_blk, over, plan);
    return hipGetLastError();
}
hipError_t launch_noise_fill(uint64_t n, uint64_t n_blocks, const NoiseParams& p, uint64_t first_index, const uint32_t* len, const uint64_t* blk_off,
                             uint32_t lit_base, uint64_t pool_base, uint64_t* lits, uint8_t* pool, uint32_t* post, hipStream_t s) {
    if (!n || !n_blocks) return hipSuccess;
    hipLaunchKernelGGL(k_noise_fill, dim3((unsigned)((n_blocks + 255) / 256)), dim3(256), 0, s, n, n_blocks, p, first_index, len, blk_off, lit_base, pool_base,
                       lits, pool, post);
    return hipGetLastError();
}
// one wave per molecule: 4 molecules per block of 256
hipError_t launch_pal_count(const MolView& m, const NoiseParams& p, uint64_t first_index, const uint4* plan, const MolCounts& c, hipStream_t s) {
    if (!m.B.n_reads) return hipSuccess;
    hipLaunchKernelGGL(k_pal_count, dim3((unsigned)((m.B.n_reads + 3) / 4)), dim3(256), 0, s, m, p, first_index, plan, c);
    return hipGetLastError();
}
hipError_t launch_pal_write(const MolView& m, const NoiseParams& p, uint64_t first_index, const uint4* plan, const MolOffsets& f, const MolOut& o,
                            hipStream_t s) {
    if (!m.B.n_reads) return hipSuccess;
    hipLaunchKernelGGL(k_pal_write, dim3((unsigned)((m.B.n_reads + 3) / 4)), dim3(256), 0, s, m, p, first_index, plan, f, o);
    return hipGetLastError();
}

}  // namespace tk
