// mdf_kernels.h -- device side of the molecule-description transforms upstream of Seq in BASELINE config 5:
// PCR amplification (src/pcr.cpp:22-89) and truncation (src/truncate.cpp:23-65, :77-227, :322-351), and the segment edits of polyA,
// tag, scb and flip.  All read a molecule batch in the binary layout of include/tksmseq.h and write a new one, on the device.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"

namespace tk {

constexpr int PCR_MAX_CYCLES = 56;        // path masks are 56-bit (the RNG counter carries them)
constexpr double PCR_TABLE_REL_ERR = 0x1p-24;   // bound on the relative error of 1 - q[t], 1 - A[t] above which a call is refused (pcr_setup)
constexpr int PCR_MAX_MUT = 32;           // mutations of one copy event (rate x length is ~0.3 for Taq on 1 kb)

struct PcrParams {
    uint64_t seed;
    int cycles;
    double efficiency, rate;              // rate = 4 * error_rate / 3 (src/pcr.cpp:36)
    double drop;                          // target / ((1 + efficiency)^cycles * molecules)
    double q[PCR_MAX_CYCLES + 1];         // q[t]: P(no molecule is emitted in the subtree of an existing copy made in cycle t)
    double A[PCR_MAX_CYCLES + 2];         // A[t]: P(none of the copies made in cycles t .. cycles-1 from one template leads to an emission)
};

// input batch plus what PCR / truncation need beyond the Seq view
struct MolView {
    BatchView B;
    const uint32_t* dup;                  // [n_reads] bit 31: the molecule had depth > 1, bits 0..30: its index among the copies (MDF unroll, src/mdf.h:97-105); may be null
    uint64_t n_intervals, n_mods;
    const uint32_t* keep;                 // optional [n_kept] molecule indices to amplify (more than 2 x target molecules: src/pcr.cpp:217-220)
    uint64_t n_kept;
};

// output tables (sized by the count pass)
struct MolOut {
    uint32_t* reads; uint32_t* intervals; uint32_t* mods; uint32_t* ids; uint8_t* idpool;
};
// what a count pass writes and a write pass reads, one entry per output molecule
struct MolCounts { uint64_t *ivl, *mod, *id; };           // intervals, substitutions, id bytes
struct MolOffsets { const uint64_t *ivl, *mod, *id; };    // their exclusive scans, [n + 1]

// PCR: pass 1 counts the emitted copies of every template; pass 2 lists them (template, path mask) with their sizes;
// pass 3 writes the molecules
hipError_t launch_pcr_count(const MolView& m, const PcrParams& p, uint64_t* n_out /* [n_kept] */, uint32_t* status, hipStream_t s);
hipError_t launch_pcr_list(const MolView& m, const PcrParams& p, const uint64_t* out_off /* [n_kept + 1] */, uint32_t* node_mol,
                           uint64_t* node_mask, const MolCounts& c, hipStream_t s);
hipError_t launch_pcr_write(const MolView& m, const PcrParams& p, uint64_t n_nodes, const uint32_t* node_mol, const uint64_t* node_mask,
                            const MolOffsets& f, const MolOut& o, hipStream_t s);

// truncation
struct TrcParams {
    uint64_t seed;
    int mode;                             // 0 normal(mu, sigma), 1 lognormal(mu, sigma), 2 KDE model
    double mu, sigma;
    int min_len;                          // truncate()'s min_val (100)
    // KDE model (custom_distribution2D / custom_distribution, src/truncate.cpp:77-227)
    int nx, ny;                           // x labels (bins), y labels (rows)
    const long long* xlab; const long long* ylab;
    const double* cdf;                    // [ny][nx + 1] running sums of row i's first i + 1 entries (the rest repeat the last)
    const int* row_n;                     // [ny] entries of row i that belong to its distribution (i + 1, at most nx)
    int have_sider, ns;                   // end_mtx: which share of the truncation goes to the 3' end
    const double* slab; const double* scdf;   // [ns] labels, [ns + 1] running sums
    int always_end, models_length;
};
// per molecule: the kept part [cut5, total - cut3) of its bases in segment order, plus what the TR comment shows
hipError_t launch_trc_plan(const MolView& m, const TrcParams& p, uint64_t first_index, uint32_t* keep_from, uint32_t* keep_to,
                           double* tr_len, double* tr_side, const MolCounts& c, hipStream_t s);
hipError_t launch_trc_write(const MolView& m, const uint32_t* keep_from, const uint32_t* keep_to, const MolOffsets& f, const MolOut& o, hipStream_t s);


// polyA / tag / scb / flip (src/polyA.cpp:133-148, src/tag.cpp:70-113, src/scb.cpp:57-80, src/interval.h:908-920): a plan per molecule
// (literal in front, literal behind, flip), then one generic count + write pass
constexpr uint32_t EDIT_NONE = 0xffffffffu;
constexpr uint32_t PLA_MAX_ATTEMPTS = 64;   // rejection attempts of the gamma / PTRS samplers (blocks of 4 words for the multiplication method)
enum { PLA_GAMMA = 0, PLA_POISSON = 1, PLA_WEIBULL = 2, PLA_NORMAL = 3 };
struct PlaParams {
    uint64_t seed;
    int dist;                             // PLA_*
    double a, b;                          // gamma / weibull (shape, scale), poisson (lambda, -), normal (mu, sigma)
    int min_len, max_len;
    uint32_t lit_base;                    // literal lit_base + L - 1 is "A" x L, L = 1 .. max_len
};
hipError_t launch_pla_plan(uint64_t n, const PlaParams& p, uint64_t first_index, uint32_t* post, hipStream_t s);
struct TagEnd {
    const uint8_t* fmt;                   // the format's letters that fmt2seq's table knows, upper case (device)
    int len;
    uint32_t shared;                      // a format without ambiguous letters: its one literal; EDIT_NONE otherwise
    uint32_t lit_base;                    // otherwise molecule r gets literal lit_base + r, bytes at pool_base + r x len
    uint64_t pool_base;
};
struct TagParams { uint64_t seed; TagEnd end[2]; };     // [0] 5' (prepended), [1] 3' (appended)
hipError_t launch_tag_plan(uint64_t n, const TagParams& p, uint64_t first_index, uint32_t* pre, uint32_t* post, uint64_t* lits, uint8_t* pool,
                           hipStream_t s);
hipError_t launch_flip_plan(uint64_t n, uint64_t seed, double p, uint64_t first_index, uint8_t* flip, hipStream_t s);
// pre / post / flip: [n_reads], any may be null (nothing of that kind); lits: the OUTPUT literal table (new literals' lengths)
hipError_t launch_edit_count(const MolView& m, const uint32_t* pre, const uint32_t* post, const MolCounts& c, hipStream_t s);
hipError_t launch_edit_write(const MolView& m, const uint32_t* pre, const uint32_t* post, const uint8_t* flip, const uint64_t* lits, const MolOffsets& f,
                             const MolOut& o, hipStream_t s);

// filter (src/filter.cpp:21-117, :196-212): a two-way partition of a batch by a conjunction of conditions; see mdf_kernels.hip
enum { FLT_SIZE = 1, FLT_LOCUS = 2 };     // (`info` conditions are read off the comments by the host: a byte per molecule)
enum { FLT_LT = 0, FLT_LE = 1, FLT_GT = 2, FLT_GE = 3, FLT_EQ = 4, FLT_NE = 5 };
struct FltCond {
    int kind, cmp;                        // FLT_SIZE: cmp is FLT_LT .. FLT_NE, against value
    long long value;
    uint32_t contig;                      // FLT_LOCUS: the context's contig of that name, ~0: none
    uint32_t name_len;                    // ... and the name itself, which a literal segment's text may equal (device)
    const uint8_t* name;
    int ranged;                           // 0: any segment on the contig; 1: one whose overlap with [start, end) is positive
    long long start, end;
};
// side[r]: 1 when the conjunction (inverted by negate) holds; flag[r] the same as a scan input; t / f: per INPUT molecule its counts on
// that side, 0 on the other; f.ivl null: no false side is sized
hipError_t launch_flt_pred(const MolView& m, const FltCond* conds, uint32_t n_conds, const uint8_t* info, int negate, uint8_t* side, uint64_t* flag,
                           const MolCounts& t, const MolCounts& f, hipStream_t s);
// rank: exclusive scan of flag; f.ivl null: molecules of the false side are not written (of is not touched)
hipError_t launch_flt_write(const MolView& m, const uint8_t* side, const uint64_t* rank, const MolOffsets& t, const MolOffsets& f, const MolOut& ot,
                            const MolOut& of, hipStream_t s);
// concat: where one input's molecules, intervals, substitutions, id bytes, literal entries and literal pool bytes start in the output
struct CatBase { uint64_t mol, ivl, mod, id; uint32_t lit; uint64_t pool; };
// f: scans of the input's own counts (launch_edit_count without literals); lits: the output's literal table
hipError_t launch_cat_write(const MolView& m, const MolOffsets& f, const CatBase& base, uint64_t* lits, const MolOut& o, hipStream_t s);

// unsegment (src/unsegment.cpp:88-105): glue a molecule behind its predecessor with probability p; see mdf_kernels.hip
// join[r]: 1 when molecule r (index first_index + r of the whole input) joins its predecessor, never for r = 0; head[r] = 1 - join[r] as a scan
// input; the three counts of molecule r on its own, the id length 0 for a joiner
hipError_t launch_glue_plan(const MolView& m, uint64_t seed, double p, uint64_t first_index, uint8_t* join, uint64_t* head, const MolCounts& c, hipStream_t s);
// rank: exclusive scan of head ([n_reads + 1]); the offsets: scans of the counts.  Output molecule rank[r] is the chain that head r opens
hipError_t launch_glue_write(const MolView& m, const uint8_t* join, const uint64_t* rank, const MolOffsets& f, const MolOut& o, hipStream_t s);

// shuffle (src/shuffle.cpp:23-44): the buffer of n_slots molecules as a sort; see mdf_kernels.hip.  n_arrivals = n - n_slots
hipError_t launch_shf_key(uint64_t n_slots, uint64_t seed, uint64_t* key, hipStream_t s);                       // key[s] of slot s
hipError_t launch_shf_slot(uint64_t n_arrivals, uint32_t n_slots, uint64_t seed, uint32_t* slot, hipStream_t s);   // slot[a] of molecule n_slots + a
// slot_sorted / arrival_sorted: the arrivals after a stable sort by slot; src[a]: the molecule written when arrival a comes
hipError_t launch_shf_evict(uint64_t n_arrivals, uint32_t n_slots, const uint32_t* slot_sorted, const uint32_t* arrival_sorted, uint32_t* src, hipStream_t s);
// order: the slots sorted by (key, slot); src_tail[q] (= src[n_arrivals + q]): the final occupant of slot order[q]
hipError_t launch_shf_occupant(uint32_t n_slots, uint64_t n_arrivals, const uint32_t* order, const uint32_t* slot_sorted, const uint32_t* arrival_sorted,
                               uint32_t* src_tail, hipStream_t s);
// a gather: output molecule j is input molecule src[j] (unrolled: ids with their suffix); counts, then -- with their scans -- the copy
hipError_t launch_gather_count(const MolView& m, const uint32_t* src, uint64_t n, const MolCounts& c, hipStream_t s);
hipError_t launch_gather_write(const MolView& m, const uint32_t* src, uint64_t n, const MolOffsets& f, const MolOut& o, hipStream_t s);

// mutate (a variant table applied to every segment; the transform is this build's own, DESIGN.md "mutate"): see mdf_kernels.hip
constexpr uint32_t MUT_NONE = 0xffffffffu;
constexpr uint64_t MUT_PT_LETTER = 1ull << 40, MUT_PT_INSERTION = 1ull << 41;     // pt_info (mut_host.h): ordinal | letter << 32 | flags
struct MutView {                          // the device form of a variant table in its normal form, for one context
    uint32_t n_contigs, n_ref, n_ins;     // contigs of the table; contigs of the context's reference; kept insertions
    const uint32_t* ref_ctg;              // [n_ref] the table's contig of a context contig, MUT_NONE: not in the table
    const uint32_t* name_off;             // [n_contigs + 1] the table's contig names in `names`, sorted by (length, bytes)
    const uint8_t* names;
    const uint32_t *del_first, *pt_first; // [n_contigs + 1]
    const uint32_t *del_from, *del_to;    // disjoint deleted ranges, ascending per contig
    const uint32_t* pt_pos;               // SNVs and insertions, ascending per contig, equal positions in table order
    const uint64_t* pt_info;
    const uint64_t* ins_ent;              // [n_ins][2] {offset in the table's insertion pool, letters}
};
// one lane per literal entry of the input: lit_ctg[l] = the table's contig whose name is the literal's text, MUT_NONE: none; and one lane per
// kept insertion k: entry lit_base + k of the OUTPUT literal table = {pool_base + its offset, its letters}
hipError_t launch_mut_resolve(const BatchView& b, const MutView& v, uint32_t* lit_ctg, uint64_t* out_lits, uint32_t lit_base, uint64_t pool_base, hipStream_t s);
hipError_t launch_mut_count(const MolView& m, const MutView& v, const uint32_t* lit_ctg, const MolCounts& c, hipStream_t s);
hipError_t launch_mut_write(const MolView& m, const MutView& v, const uint32_t* lit_ctg, uint32_t lit_base, const MolOffsets& f, const MolOut& o, hipStream_t s);

// random-wgs (src/random_wgs.cpp:181-207): fragments of the whole genome, one lane per candidate; see mdf_kernels.hip
constexpr int WGS_LDS_CONTIGS = 2048;       // running sums of that many contigs are searched in LDS (16 KB), more in global memory
enum { WGS_NORMAL = 0, WGS_UNIFORM = 1, WGS_LOGNORMAL = 2, WGS_EXPONENTIAL = 3 };
struct WgsParams {
    uint64_t seed;
    int dist;                             // WGS_*
    double a, b;                          // normal / lognormal (mean, sigma), uniform [a, b), exponential (rate, -)
    uint64_t ref_length;                  // sum of the contig lengths (> 0)
    uint32_t n_contigs;
};
// plan[t] = {contig, ref_pos, clipped length (0: not emitted), strand minus}; flag / bases: what launch_scan ranks and sums
hipError_t launch_wgs_plan(const WgsParams& p, const uint64_t* so_far, uint64_t first, uint64_t n, uint4* plan, uint64_t* flag, uint64_t* bases, hipStream_t s);
// idlen[t]: id bytes of a candidate inside the run's prefix (0: outside, or not emitted); cut[4] (zeroed by the caller) = {molecules, bases,
// candidates consumed, 1} when base_count is reached inside the call
hipError_t launch_wgs_cut(uint64_t n, const uint4* plan, const uint64_t* rank, const uint64_t* bsum, const uint32_t* name_len, uint64_t mols_before,
                          uint64_t bases_before, uint64_t base_count, uint64_t* idlen, uint64_t* cut, hipStream_t s);
hipError_t launch_wgs_write(uint64_t n, const uint4* plan, const uint64_t* rank, const uint64_t* idlen, const uint64_t* id_off, const uint32_t* name_off,
                            const uint32_t* name_len, const uint8_t* names, uint64_t mols_before, const MolOut& o, hipStream_t s);

// transcribe (src/transcribe.cpp:170-197): an abundance row becomes `depth` copies of its transcript; see mdf_kernels.hip
struct TsbCount {
    uint64_t seed, first_row;             // row r draws from Philox(seed, first_row + r, ST_TSB, 0)
    double weight, molecule_count, sum_tpm;   // c = ((weight x tpm) x molecule_count) / sum_tpm
};
// depth[r]: molecules of row r (0: transcript not found, or a count below 1); flag[r]: 1 when depth[r] >= 1.  tx[r]: transcript, ~0: none
hipError_t launch_tsb_count(uint64_t n_rows, const TsbCount& p, const uint32_t* tx, const double* tpm, uint64_t* depth, uint64_t* flag, hipStream_t s);
// rank: exclusive scan of flag ([n_rows + 1]); n_ivl[r] = depth x exons of the transcript, id_bytes[r] = depth x (prefix_len + digits of rank)
hipError_t launch_tsb_size(uint64_t n_rows, const uint32_t* tx, const uint32_t* exon_first, const uint64_t* depth, const uint64_t* rank, uint32_t prefix_len,
                           uint64_t* n_ivl, uint64_t* id_bytes, hipStream_t s);
struct TsbPlanView {                      // the plan's device arrays: per row, and their exclusive scans ([n_rows + 1])
    uint64_t n_rows;
    const uint32_t* tx;
    const uint64_t *mol_first, *rank, *ivl_first, *id_first;
    const uint32_t* exon_first;           // [n_transcripts + 1]
    const uint4* exons;                   // {contig (bit 31: literal), start, end, minus << 31}: an interval of the batch layout
    const uint8_t* prefix; uint32_t prefix_len;
};
// molecules [first_mol, first_mol + n_mol) of the unrolled range; their intervals are [ivl_base, ivl_base + n_ivl) and their id bytes start
// at id_base of the whole run's.  dup: [n_mol] bit 31 for a copy of a row with depth > 1, low bits the copy's index
hipError_t launch_tsb_write(const TsbPlanView& v, uint64_t first_mol, uint64_t n_mol, uint64_t ivl_base, uint64_t n_ivl, uint64_t id_base, const MolOut& o,
                            uint32_t* dup, hipStream_t s);

// tail-noise (src/append_noise.cpp:83-128, NoiseAdder::operator()): a noise length L per molecule from normal / lognormal(mu, sigma);
// random mode appends a literal of L letters of the alphabet, palindromic mode appends the molecule's last segments again, strands
// toggled, the last copy cut so that the hairpin has min(L, molecule size) bases, then a Bernoulli(error_rate) substitution per hairpin
// base.  The plan is one lane per molecule; the per-base work is spread: letters over a flat grid of 4-letter Philox blocks, hairpin
// bases over the 64 lanes of one wave per molecule (k_pal_count / k_pal_write).  See mdf_kernels.hip.
constexpr int NOISE_MAX_LEN = 1 << 20;      // random mode: letters of one literal (the limit polyA and tag have)
enum { NOISE_NORMAL = 0, NOISE_LOGNORMAL = 1 };
struct NoiseParams {
    uint64_t seed;
    int dist;                             // NOISE_*
    double mu, sigma, error_rate;
    const uint8_t* alphabet;              // [k] (device); repeated letters weight the draw
    uint32_t k;
};
// random mode (plan != null is the palindromic one): len[r] = L (0 for L <= 0), nblk[r] = ceil(L / 4), *over = the smallest r whose
// L is above NOISE_MAX_LEN (its len is 0; the caller sets *over to ~0 first).  Palindromic mode: plan[r] = {segments copied (the cut
// one included; 0: the molecule stays as it is), bases cut off the last copy, hairpin bases H = min(L, molecule size), 0}.
hipError_t launch_noise_plan(const MolView& m, const NoiseParams& p, uint64_t first_index, uint32_t* len, uint64_t* nblk, unsigned long long* over,
                             uint4* plan, hipStream_t s);
// blk_off: exclusive scan of nblk ([n + 1]), n_blocks its total.  Molecule r with L > 0 gets literal lit_base + r = L letters at
// pool_base + 4 x blk_off[r] and post[r] = that literal; post (all EDIT_NONE) and the new entries of lits (zero) are set by the caller.
hipError_t launch_noise_fill(uint64_t n, uint64_t n_blocks, const NoiseParams& p, uint64_t first_index, const uint32_t* len, const uint64_t* blk_off,
                             uint32_t lit_base, uint64_t pool_base, uint64_t* lits, uint8_t* pool, uint32_t* post, hipStream_t s);
// palindromic mode, after launch_edit_count / launch_edit_write without literals or flip: the count ADDS the hairpin's segments and
// substitutions to c.ivl / c.mod, the write puts them behind the molecule's own (f.ivl / f.mod: scans of the sums); the id members are not read
hipError_t launch_pal_count(const MolView& m, const NoiseParams& p, uint64_t first_index, const uint4* plan, const MolCounts& c, hipStream_t s);
hipError_t launch_pal_write(const MolView& m, const NoiseParams& p, uint64_t first_index, const uint4* plan, const MolOffsets& f, const MolOut& o, hipStream_t s);

}  // namespace tk
