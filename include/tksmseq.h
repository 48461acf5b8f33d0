/*
 * tksmseq.h -- C-ABI of the MI355X-native TKSM `Seq` hot path (libtksmseq.so).
 *
 * This is the drop-in boundary for the path BASELINE.json names: TKSM's Seq exit module,
 *   src/sequence.cpp:21-57  (Sequencer_module::impl::run -> embedded Python)
 *   py/sequence.py:323-376  (main block: load reference + models, per-molecule loop, write)
 *   py/tksm_badread.py      (Badread identity / error / q-score model)
 * Every entry point below names the reference code it replaces (file:line into vpc-ccg/tksm).
 * Plain pointers and sizes only; no C++ or torch types; no exceptions cross this boundary.
 * All functions return TKSMSEQ_OK (0) or a TKSMSEQ_E* code; tksmseq_last_error() gives the text.
 * A context is used from one host thread at a time and owns one HIP device + stream.  Contexts are independent:
 * several may be driven from different threads on the same device (each on its own stream), and that is how batches
 * are streamed at full rate -- the kernels of concurrent runs fill each other's gaps (instruction-bound error loop next
 * to memory-bound alignment, the latency-bound last rounds of one batch underneath the bulk of the next).
 *
 * There is no CPU fallback: every compute entry point runs HIP kernels on gfx950 and fails with
 * TKSMSEQ_EDEVICE when no device is usable.
 *
 * Environment.  Results never depend on any of these: they choose between kernel variants that produce the same bytes (the GPU tests
 * use them to reach every variant) or print diagnostics.  Read when a context is created unless noted.  This list names everything the library reads.
 *   TKSM_MODELS            colon list of model directories searched after the built-in one (src/sequence.cpp:38-52, py/sequence.py:17-31)
 *   TKSMSEQ_BUILTIN_MODELS the built-in model directory (default: models/ next to the library)
 *   TKSMSEQ_VERBOSE=1|2    per-run statistics on stderr (rounds, slow-path reads, full-width redo jobs, alignment fall-backs by reason);
 *                          2: per-batch stage times as well (also read by the CLI).  Read at the start of every run
 *   TKSMSEQ_FORCE_SLOW=1   every read through the exact wave-wide kernel (k_simulate) instead of the fast pipeline
 *   TKSMSEQ_SMALL_ALN=N    rounds with at most N alignment jobs store all 64 band rows in one launch (default 131072; 0: always the
 *                          14-row pass + redo list)
 *   TKSMSEQ_WAVE_LOOP=N    rounds with at most N reads left run the error loop one wave per read (k_loopw; default 16384, 0: never)
 *   TKSMSEQ_TAIL_WAVE=N    once at most N reads are left (and each can have a wave of its own at once) they finish in ONE launch that runs
 *                          every remaining visit of a read on one wave, alignments included (k_loopw<true>; default 4096, 0: never)
 *   TKSMSEQ_LOOP_WL=W      words (16 bases each) of a read's packed fragment that k_loop keeps in LDS per lane (default 64, multiple of 4);
 *                          read once per process, at the first k_loop launch
 *   TKSMSEQ_EARLY_TAIL=N   at most N reads whose length x (1 - target identity) exceeds 4 x the batch's median get their straggler waves at
 *                          round 0, on a stream of their own underneath the regular rounds (default 1024, at most 4096; 0: never)
 *   TKSMSEQ_TAIL_WCAP=C    columns of a window the straggler kernel aligns on its wave (default and maximum 2048; a wider window takes the
 *                          regular route for that visit; the tests force that with a small value)
 *   TKSMSEQ_HBM_STATE_LEN=L fragments longer than L are edited in HBM by the last visit instead of being staged in LDS (default 2304)
 *   TKSMSEQ_DEFER_LEN=L    reads longer than L wait with their q-score alignment until the regular rounds are over (default 0: all)
 *   TKSMSEQ_BUCKETS=N      length buckets of the last visit's launches (default 16)
 *   TKSMSEQ_TAIL_CUT=N     diagnostic: once fewer than N reads are left, they finish in the wave-wide kernel (default 0: off)
 *   TKSMSEQ_FULL_ROWS_CAP=N diagnostic: the full-width alignment pass sees a pool of at most N rows (a multiple of 64, at least 64; default 0:
 *                          no cap).  Which rounds align at full width does not change, so a round with more jobs than rows leaves waves without
 *                          rows: their jobs are counted as fall-backs (reason bit 0x02) and their reads finish in the exact kernel
 *   TKSMSEQ_FULL_POOL_MB=M memory for the unbanded alignment fallback of the wave-wide kernel (default 1024)
 *   TKSMSEQ_POISON=W       diagnostic: W a 32-bit word in hex (1 - 8 digits).  Every device block and page-locked buffer the library's allocator
 *                          hands out, fresh or recycled, is filled with W first (a grown buffer: behind the bytes it keeps), each fill
 *                          waited for, and every context prints `poison W: <blocks> blocks, <bytes> bytes` on stderr as it is destroyed: what
 *                          the process has filled since the line before.  The same bytes must come out whatever W is
 *                          (tests/test_history_gpu.py).  Read once per process, at the first allocation
 *   TKSMSEQ_STATS_FILE=P   (CLI) `tksm sequence` writes one JSON object with the run's stage clocks to P: reads, batches, MDF bytes in, record
 *                          bytes out, seconds of set-up (devices, references, models), of streaming (first chunk read -> last record byte
 *                          written) and, summed over the threads of a stage, of parsing, running, device-side staging copies, waiting for
 *                          device-to-host pieces, write calls, waiting for the writer, reading + counting (bench.py's end-to-end leg)
 *   TKSMSEQ_PIECE_BYTES=B  (CLI) size of the page-locked pieces a batch's records pass through (default 64 MB; the tests use 4 KB)
 *   TKSMSEQ_LIB=NAME       (Python package) file name of the library to load instead of libtksmseq.so, next to it: diagnostic builds
 *   TKSMSEQ_ABLATE=N       only in the diagnostic build (`make ablate`, -DTKSM_ABLATE): timing experiments on the last visit's q-score loop
 *                          (40 - 45, tools/ablate_err.sh) and k_loop's prologue (33)
 *   GPU_MAX_HW_QUEUES      (HIP runtime) the CLI and bench.py set 16 when unset: a hardware queue per context in flight -- INTEGRATION.md
 */
#ifndef TKSMSEQ_H
#define TKSMSEQ_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TKSMSEQ_OK 0
#define TKSMSEQ_EINVAL 1    /* bad argument / malformed input (reference: Python exception -> exit 1) */
#define TKSMSEQ_EIO 2       /* file could not be read / written */
#define TKSMSEQ_EDEVICE 3   /* HIP error or no device */
#define TKSMSEQ_ENOMEM 4
#define TKSMSEQ_ESTATE 5    /* call order violated (e.g. run before models are set) */
#define TKSMSEQ_ELIMIT 6    /* input exceeds a documented limit of this build (molecule too long) */

typedef struct tksmseq_ctx tksmseq_ctx;
typedef struct tksmseq_batch tksmseq_batch;

/* ---- lifetime ------------------------------------------------------------------------------
 * Replaces Py_Initialize + module globals (src/python_runner.h:44-73, py/sequence.py:323-345). */
int tksmseq_create(int device, tksmseq_ctx** out);
void tksmseq_destroy(tksmseq_ctx* ctx);
const char* tksmseq_last_error(const tksmseq_ctx* ctx);   /* ctx may be NULL: last create() error */
const char* tksmseq_version(void);
/* Launch on a caller-owned hipStream_t (e.g. torch's current stream); NULL = library stream. */
int tksmseq_set_stream(tksmseq_ctx* ctx, void* hip_stream);
/* A second context on the same device that SHARES src's packed reference and model tables (read-only views; it gets
 * its own stream and work buffers).  Replaces what the reference's worker processes inherit by fork from the module
 * globals (multiprocessing.Pool, py/sequence.py:354-366; reference_seqs / error_model / qscore_model, :336-345).
 * Destroy clones before src.  Loading another model or contig into a clone gives that clone a private copy. */
int tksmseq_clone(const tksmseq_ctx* src, tksmseq_ctx** out);
/* Page-locked host memory for tksmseq_result_download destinations (a pageable destination halves the copy rate). */
int tksmseq_host_alloc(uint64_t bytes, void** out);
void tksmseq_host_free(void* p);
int tksmseq_synchronize(tksmseq_ctx* ctx);
/* Device memory of the caller's own (on ctx's device) and copies out of it on ctx's stream: what a writer needs to keep a batch's
 * records (tksmseq_result_copy_device into such a buffer) while the context that made them runs its next batch.  async != 0:
 * returns once the copy is queued (tksmseq_synchronize before the bytes are read). */
int tksmseq_device_alloc(tksmseq_ctx* ctx, uint64_t bytes, void** out);
void tksmseq_device_free(tksmseq_ctx* ctx, void* p);
int tksmseq_copy_to_host(tksmseq_ctx* ctx, void* dst_host, const void* src_device, uint64_t bytes, int async);

/* ---- reference genome (S0) -------------------------------------------------------------------
 * get_reference_seqs / generate_fasta, py/sequence.py:168-194: name = header up to the first
 * space; later contigs with the same name replace earlier ones.  The library packs to 2 bit/base
 * on the device (upper-cased; 4096-base blocks holding any non-ACGT byte are kept as bytes). */
int tksmseq_reference_add_fasta(tksmseq_ctx* ctx, const char* path /* .fa / .fa.gz */);
/* ascii: host pointer (on_device = 0) or device pointer (on_device = 1); caller keeps ownership. */
int tksmseq_reference_add_contig(tksmseq_ctx* ctx, const char* name, const uint8_t* ascii, uint64_t len,
                                 int on_device);
int tksmseq_reference_contig_id(const tksmseq_ctx* ctx, const char* name);   /* -1 if absent */
/* A contig known by name and length only -- what `<reference>.fai` gives (src/random_wgs.cpp:139-161 reads nothing else).  tksmseq_wgs and
 * the MDF writer work on a context with declared contigs; tksmseq_run on it fails with TKSMSEQ_ESTATE (there are no bases to read).
 * A later tksmseq_reference_add_contig of the same name supplies the bases. */
int tksmseq_reference_declare_contig(tksmseq_ctx* ctx, const char* name, uint64_t len);
int tksmseq_reference_info(const tksmseq_ctx* ctx, uint64_t* n_contigs, uint64_t* total_bases,
                           uint64_t* device_bytes);

/* ---- models ----------------------------------------------------------------------------------
 * ErrorModel.__init__/load_from_file + align_kmers, py/tksm_badread.py:76-117, :146-197.
 * QScoreModel.__init__/load_from_file/random/ideal, py/tksm_badread.py:464-582.
 * name_or_path: "random" (both), "ideal" (q-score), a model name resolved through $TKSM_MODELS
 * (colon list, <dir>/badread/<name>.{error,qscore}.gz, py/sequence.py:17-31) or a file path. */
int tksmseq_load_error_model(tksmseq_ctx* ctx, const char* name_or_path);
int tksmseq_load_qscore_model(tksmseq_ctx* ctx, const char* name_or_path);
/* Tail noise, TAIL_NOISE_MODEL_PY.KDE_noise_generator (py/tksm_badread.py:886-962; sampled at :335, appended to the
 * fragment before the k-base pads at :336-341).  name_or_path: "no_noise" (the default: nothing is appended), a name
 * resolved through $TKSM_MODELS (<dir>/badread/<name>.tail.gz) or a JSON[.gz] file in the layout
 * KDE_noise_generator.save writes (:935-942).  The tail's bases count towards `length=` but not towards
 * `error_free_length=` (py/sequence.py:253-254).  --perfect output never carries a tail. */
int tksmseq_load_tail_model(tksmseq_ctx* ctx, const char* name_or_path);
typedef struct tksmseq_tail_model {
    uint32_t n_lx, n_ly;
    const double* lx;      /* [n_lx] tail lengths (Custom2Dist.lx) */
    const double* ly;      /* [n_ly] fragment-length labels, sorted (Custom2Dist.ly) */
    const double* grid;    /* [n_ly][n_lx] densities, >= 0, every row with a positive sum */
    double trans[16];      /* [4][4] transition weights of the base chain (transition_matrix[1]) */
    double ratio;          /* probability that a read gets a tail */
    uint8_t bases[4];      /* output byte of each chain state (default "AGTC") */
    uint8_t pad[4];
} tksmseq_tail_model;
/* the same from tables in memory; NULL switches the tail off */
int tksmseq_set_tail_model(tksmseq_ctx* ctx, const tksmseq_tail_model* model);
/* Identities.__init__ + beta_parameters, py/tksm_badread.py:703-757 (percent units, as the CLI). */
int tksmseq_set_identity(tksmseq_ctx* ctx, double mean, double max, double stdev);

/* Table read-back (host copies) so tests can compare the packed layouts with the oracle's.
 * Pass NULL for an array to query sizes only. */
int tksmseq_get_error_model(const tksmseq_ctx* ctx, int32_t* type, int32_t* k, int32_t* max_alts,
                            uint32_t* cdf, uint64_t* alts, uint8_t* nalts);
int tksmseq_get_qscore_model(const tksmseq_ctx* ctx, int32_t* n_slots, int32_t* kmer_size, uint64_t* pool_len,
                             uint64_t* keys, uint32_t* row_off, uint32_t* row_cnt, uint32_t* cdf_pool,
                             uint8_t* q_pool);
int tksmseq_get_identity(const tksmseq_ctx* ctx, int32_t* constant, double* value, double* beta_a,
                         double* beta_b, double* qtab /* [65537] or NULL */);

/* ---- molecule batches (MDF) ------------------------------------------------------------------
 * mdf_generator, py/sequence.py:197-221: header '+id\tdepth\tcomment', interval lines with exactly
 * 5 tab fields 'contig\tstart\tend\tstrand\tmods'; a molecule is emitted `depth` times.  A contig
 * name absent from the reference is a literal sequence (py/sequence.py:307).
 * Binary layout (what the kernels read; "algorithmic bytes" 8 + 16 S + 8 M per read):
 *   reads      [n_reads]      {u32 ivl_begin, u32 ivl_count}
 *   intervals  [n_intervals]  {u32 contig (bit31: literal index), u32 start, u32 end,
 *                              u32 mod_begin | strand_minus << 31}
 *   mods       [n_mods]       {u32 pos, u32 chr}
 *   literals   [n_literals]   {u64 off, u64 len} into literal_pool
 *   ids        [n_reads]      {u32 off, u32 len} into id_pool                                   */
typedef struct {
    uint64_t n_reads, n_intervals, n_mods, n_literals, literal_bytes, id_bytes;
    const uint32_t* reads;        /* [n_reads][2] */
    const uint32_t* intervals;    /* [n_intervals][4]; mods of interval i are [mod_begin_i, mod_begin_{i+1}) */
    const uint32_t* mods;         /* [n_mods][2] */
    const uint64_t* literals;     /* [n_literals][2] */
    const uint8_t* literal_pool;
    const uint32_t* ids;          /* [n_reads][2] */
    const uint8_t* id_pool;
} tksmseq_batch_desc;

/* Copies host arrays to the device (validated first). */
int tksmseq_batch_create(tksmseq_ctx* ctx, const tksmseq_batch_desc* host_desc, tksmseq_batch** out);
/* Parses MDF text (whole file or a chunk ending at a molecule boundary) and uploads it. */
int tksmseq_batch_from_mdf_text(tksmseq_ctx* ctx, const char* text, uint64_t len, tksmseq_batch** out);
/* The same for the MDF -> MDF modules (tksmseq_pcr, tksmseq_truncate), which the reference runs without a FASTA: contig names
 * the context does not know stay what they are (the writer prints them back), substitution positions are not checked. */
int tksmseq_molecules_from_mdf_text(tksmseq_ctx* ctx, const char* text, uint64_t len, tksmseq_batch** out);
int tksmseq_batch_info(const tksmseq_batch* b, uint64_t* n_reads, uint64_t* n_intervals, uint64_t* n_mods);
/* Releases a batch.  `ctx`: the context that last ran / transformed the batch -- its stream is drained first, then the batch's device
 * tables go back to the library's per-process cache of device blocks (not to the driver: hipFree waits for the whole device), from
 * which the next batch of about that size takes them.  A caller that used the batch on SEVERAL contexts frees it through the last one
 * after the others have been synchronised (tksmseq_synchronize).  ctx may be NULL once every context has been destroyed. */
void tksmseq_batch_free(tksmseq_ctx* ctx, tksmseq_batch* b);

/* ---- the hot path ----------------------------------------------------------------------------
 * One call = the body of the reference's per-molecule loop for every read of the batch:
 * mdf_to_seq (py/sequence.py:303-320) -> perfect (:261-270) or badread (:242-258) ->
 * sequence_fragment / get_qscores (py/tksm_badread.py:324-451, :607-655) -> fastq/fasta
 * formatter (py/sequence.py:273-288).  Output records are concatenated in read order.
 * Randomness is counter-based: it depends only on (seed, global read index), where
 * global index = first_read_index + i * read_index_stride for read i of the batch. */
#define TKSMSEQ_MODE_PERFECT 0
#define TKSMSEQ_MODE_BADREAD 1
typedef struct {
    uint64_t seed;
    uint64_t first_read_index;
    uint64_t read_index_stride;   /* 0 is treated as 1 */
    int32_t mode;                 /* TKSMSEQ_MODE_* */
    int32_t fastq;                /* 1: '@id info\nSEQ\n+\nQUAL\n'   0: '>id info\nSEQ\n' */
    int32_t compute_qual;         /* badread only: 0 = all 'K' (--skip-qual-compute) */
    int32_t collect_stats;        /* 1: fill the per-read debug statistics (tests) */
    int32_t perfect_of_badread;   /* badread only: format the badread sequence the way perfect() does (quals 'K',
                                     error_free_length = length, identity 100.00%).  This is what the reference
                                     writes to --perfect when -o is given too (py/sequence.py:317-319 rebinds
                                     `seq`); the CLI uses it to reproduce that behaviour. */
    int32_t reserved;
} tksmseq_run_params;

typedef struct {
    const void* records;          /* device pointer, records_bytes bytes */
    const void* record_offsets;   /* device u64[n_reads + 1] */
    uint64_t records_bytes;
    uint64_t n_reads;
    uint64_t bases_in;            /* error-free bases (sum of spliced lengths) */
    uint64_t bases_out;           /* emitted bases */
    float kernel_ms[8];           /* device time of this call by HIP events on its stream, 0 if timing is off: [0] lengths + scan,
                                     [1] the simulate stage as a whole, [2] record offsets, [3] k_emit / k_perfect, [4] everything;
                                     Badread: summed launch durations of [5] the error-loop kernels (k_loop, k_loopw, the straggler launch), [6] the
                                     alignment kernel k_alnf (all passes), [7] the launches around k_qjobs (rounds 1 - 2: k_job); the rest of [1]:
                                     k_init, the final-stage k_err, host gaps between rounds */
} tksmseq_result;

int tksmseq_run(tksmseq_ctx* ctx, const tksmseq_batch* batch, const tksmseq_run_params* params,
                tksmseq_result* result);
/* Caller-provided device buffer for the record stream (e.g. a torch tensor); NULL restores the
 * library-owned buffer.  tksmseq_run fails with TKSMSEQ_ENOMEM if it is too small. */
int tksmseq_set_output_buffer(tksmseq_ctx* ctx, void* device_ptr, uint64_t capacity);
/* Host threads used to parse MDF text in tksmseq_batch_from_mdf_text (default 1).  The reference's parallel knob is
 * -t/--threads: multiprocessing.Pool(args.threads) over molecules, py/sequence.py:360-368; here the device does the per-molecule
 * work and the threads go to the text -> binary batch conversion. */
int tksmseq_set_host_threads(tksmseq_ctx* ctx, int n);
/* 1 if `name` resolves to a model file of `kind` ("error", "qscore", "tail") in the built-in directory or $TKSM_MODELS
 * (set_tksm_models_dicts, py/sequence.py:17-31): the CLI's default-model rule "nanopore2020 if discoverable else random"
 * (py/sequence.py:86-107). */
int tksmseq_model_available(const char* name, const char* kind);
/* Host only, no context, callable from any thread: parses a model file ("error" / "qscore") or computes the identity quantile
 * table now and keeps the result for the process, so that a later tksmseq_load_*_model / tksmseq_set_identity with the same
 * file / parameters copies it instead of parsing again.  The CLI calls these on threads of their own while the device is set up
 * and the reference packed (the reference's Python loads its models serially at import, py/sequence.py:323-345). */
int tksmseq_prefetch_model(const char* name_or_path, const char* kind);
int tksmseq_prefetch_identity(double mean, double max, double stdev);
int tksmseq_set_timing(tksmseq_ctx* ctx, int enable);   /* hipEvent per stage, read via result.kernel_ms */
/* Diagnostics of the last Badread tksmseq_run on this context (no reference counterpart: the lane-per-alignment kernels fall back
 * to an exact wave-wide kernel for what their fixed-size queues / stored rows cannot hold, with the same results -- so a defect that
 * only shows as fall-backs is invisible to parity tests; tests/test_gpu_parity.py watches these counts instead).  out[16]:
 *  [0] rounds of the host loop            [1] reads finished by the exact wave-wide kernel (non-ACGT bytes, band exits, fall-backs)
 *  [2] predicted stragglers (own stream)   [3] alignment jobs of the rounds whose first pass stores 14 rows
 *  [4] of those, jobs redone at full width (path left the stored rows)       [5] fused-alignment fall-backs (job given up by k_alnf)
 *  [6] the fall-backs' reasons, or-ed (bit 0 column-queue / reservoir overflow, 3 window shift > 31, 4 shift > 14 in the 14-row
 *      pass, 5 end cell outside the band, 6 walk left the stored rows)        [7] fall-backs among q-score jobs
 *  [8] fall-backs in the full-width list pass                                 [9] alignment jobs of all rounds
 *  [10] reads whose alignment left the 64-row band (exact kernel)            [11..15] reserved (0) */
int tksmseq_run_diagnostics(tksmseq_ctx* ctx, uint32_t* out);
/* Copies the last result to host memory (records: records_bytes, offsets: n_reads + 1). */
int tksmseq_result_download(tksmseq_ctx* ctx, uint8_t* records, uint64_t* offsets);
/* A slice [offset, offset + bytes) of the last result's record stream to host memory -- for callers that stream a large result
 * through a small page-locked buffer (tksmseq_host_alloc) instead of holding it whole.  async != 0: returns once the copy is
 * queued on the context's stream (tksmseq_synchronize before the bytes are read). */
int tksmseq_result_download_range(tksmseq_ctx* ctx, uint8_t* dst, uint64_t offset, uint64_t bytes, int async);
/* Device-to-device copies of the last result into caller buffers (either may be NULL): records_bytes bytes and
 * n_reads + 1 u64 offsets.  Asynchronous on the context's stream. */
int tksmseq_result_copy_device(tksmseq_ctx* ctx, void* records_dst, void* offsets_dst);
/* ---- BGZF on the device ------------------------------------------------------------------------
 * A record stream compressed where it was made: a sequence of BGZF members (SAM specification 4.1, what `bgzip` writes -- gzip members
 * with the 'BC' extra subfield), member c holding bytes [65280 c, 65280 (c + 1)) of the input whatever the record boundaries, at most
 * 65536 bytes each.  Every gzip reader reads the result; the members of several calls concatenate, and a file is closed by the 28
 * bytes of tksmseq_gzip_eof (never appended here).  The encoder is FASTQ-aware Huffman coding plus byte runs, not LZ77: header,
 * sequence and quality lines get deflate blocks and code tables of their own.  The bytes are a pure function of the
 * input bytes and the format.  The compressed buffer lives until the next tksmseq_run or gzip call on the context. */
#define TKSMSEQ_GZIP_RAW 0      /* any bytes: one code table per member */
#define TKSMSEQ_GZIP_FASTA 1    /* records of two lines */
#define TKSMSEQ_GZIP_FASTQ 2    /* records of four lines */
typedef struct {
    const void* data;             /* device pointer, `bytes` bytes */
    const void* member_offsets;   /* device u64[n_members + 1] */
    uint64_t bytes;
    uint64_t n_members;
    float device_ms;              /* device time of the call by HIP events, 0 if timing is off */
    float reserved;
} tksmseq_gzip_result;
/* Compresses the records of the last tksmseq_run on the context's stream; line classes follow that run's `fastq` flag. */
int tksmseq_result_gzip(tksmseq_ctx* ctx, tksmseq_gzip_result* out);
/* The same for any device bytes (e.g. an interleaved multi-GPU stream); format: TKSMSEQ_GZIP_*. */
int tksmseq_gzip_device(tksmseq_ctx* ctx, const void* src_device, uint64_t bytes, int format, tksmseq_gzip_result* out);
/* A slice of the last compressed stream to host memory, like tksmseq_result_download_range; member offsets (n_members + 1) if asked for. */
int tksmseq_gzip_download_range(tksmseq_ctx* ctx, uint8_t* dst, uint64_t offset, uint64_t bytes, int async);
int tksmseq_gzip_download_offsets(tksmseq_ctx* ctx, uint64_t* offsets);
/* Device-to-device copy of the last compressed stream (asynchronous on the context's stream): what a writer keeps while the context
 * runs its next batch. */
int tksmseq_gzip_copy_device(tksmseq_ctx* ctx, void* dst);
/* The empty member that ends a BGZF file. */
int tksmseq_gzip_eof(uint8_t out[28]);

/* Per-read debug statistics of the last badread run with collect_stats = 1: int32[n_reads][16]
 * {n_draws, change_count, n_aligns, frag_len, new_len, start_trim, end_trim, status, ...} +
 * double[n_reads][2] {errors, target_identity}. */
int tksmseq_stats_download(tksmseq_ctx* ctx, int32_t* istats, double* dstats);

/* ---- multi-GPU record ordering (S7) ----------------------------------------------------------
 * Interleaves P per-rank record streams (rank p holds global reads p, p+P, p+2P, ...) into global
 * read order on the device: dst gets sum(len) bytes.  Used after an RCCL gather on rank 0.
 * streams[p] / offsets[p] are device pointers (u64 offsets[n_p + 1]). */
int tksmseq_interleave_records(tksmseq_ctx* ctx, int n_ranks, const void* const* streams,
                               const void* const* offsets, const uint64_t* n_reads_per_rank,
                               void* dst, uint64_t dst_capacity, uint64_t* dst_bytes);

/* ---- the module entry point ------------------------------------------------------------------
 * int Sequencer_module::run() (src/sequence.cpp:30-54, src/pimpl.h:5-9) with the CLI of
 * py/sequence.py:34-165; argv[0] is "sequence" as in src/tksm.cpp:164-166.  Returns the process
 * exit code (0 ok, 1 argument / input error). */
/* ---- molecule-description transforms upstream of Seq (BASELINE config 5), on the device ----------------------------------
 * Both take a batch and return a new one (free with tksmseq_batch_free) that tksmseq_run accepts directly: the molecule
 * tables never leave the device between PCR, truncation and sequencing.  Molecules are taken depth-unrolled, as every
 * C++ module of the reference reads them (stream_mdf(..., true), src/mdf.h:97-105): copies of a depth > 1 molecule
 * become id_0, id_1, ...  Results depend only on (seed, molecule index), not on batching or the device.
 *
 * tksmseq_pcr replaces PCR::perform / do_pcr (src/pcr.cpp:40-89; module src/pcr.cpp:91-260): every cycle copies each
 * molecule present with probability `efficiency`; a copy gets floor(4/3 error_rate x size) (+1 with the fractional
 * probability) substitutions at distinct positions, bases uniform in "ACTG", on top of its template's; each copy is
 * written with probability target_count / ((1 + efficiency)^cycles x molecules); id = template id + "." + cycle.
 * More than 2 x target_count input molecules: 2 x target_count of them are used, a uniformly random ORDERED subset as :217-220's
 * std::shuffle + resize gives (the molecules with the smallest Philox keys, in key order); their copies are written in that order. */
/* flags of both transforms.  TKSMSEQ_MOL_NO_COMMENTS: the output batch carries no header comments.  Comments ("truncated=...", "TR=...",
 * the template's own) are host-side text per molecule; a caller whose next step is tksmseq_run -- which never reads them, like the
 * reference's Seq (mdf_generator, py/sequence.py:206-213, drops the comment column) -- saves that work: the chained `tksm sequence
 * --pcr-... --truncate-...` sets it, `tksm pcr` / `tksm truncate` (MDF text out) do not. */
#define TKSMSEQ_MOL_NO_COMMENTS 1
typedef struct {
    uint64_t seed;
    uint64_t target_count;        /* --molecule-count */
    int32_t cycles;               /* --cycles (at most 56) */
    int32_t flags;                /* TKSMSEQ_MOL_NO_COMMENTS or 0 */
    double error_rate;            /* --error-rate, before the 4/3 adjustment of src/pcr.cpp:36 */
    double efficiency;            /* --efficiency */
    /* the copies of the templates at positions template_begin <= i < template_end of the PROCESSING ORDER only (0, 0: all of them):
     * input order, or the subsample's key order when more than 2 x target_count molecules come in.  The drop ratio and the subsample
     * are those of the WHOLE input either way, and a copy depends on (seed, its template, its path of cycles) alone, so the outputs
     * of consecutive slices, one after the other, are the output of the whole: how `tksm pcr` streams 200 M molecules through
     * bounded memory and spreads them over several devices */
    uint64_t template_begin, template_end;
} tksmseq_pcr_params;
/* written copies per template, by position in the processing order (counts[n_reads of the batch]; positions beyond the subsample:
 * 0): what a caller needs to number the molecules of a slice's output before the slices before it have been made */
int tksmseq_pcr_template_counts(tksmseq_ctx* ctx, const tksmseq_batch* in, const tksmseq_pcr_params* params, uint64_t* counts);
int tksmseq_pcr_preset(const char* name, double* error_rate, double* efficiency);   /* -x/--preset, src/pcr.cpp:136-140 */
int tksmseq_pcr(tksmseq_ctx* ctx, const tksmseq_batch* in, const tksmseq_pcr_params* params, tksmseq_batch** out);

/* tksmseq_truncate replaces truncate() + truncate_transformer / truncate_transformer_kde (src/truncate.cpp:23-65, :322-351):
 * NORMAL / LOGNORMAL: keep the first (int)X bases in segment order, X ~ Normal(mu, sigma) / exp(Normal(mu, sigma)), at least
 * 100 (min_val); KDE: truncation length from the 2-D model of <kde_model_path> (custom_distribution2D, :163-203), split
 * between the 3' end and the 5' end by the model's end-ratio histogram (or all at the 3' end with always_end when the
 * model has none).  A cut segment keeps its substitutions re-based, sorted by position (einterval::truncate). */
#define TKSMSEQ_TRC_NORMAL 0
#define TKSMSEQ_TRC_LOGNORMAL 1
#define TKSMSEQ_TRC_KDE 2
typedef struct {
    uint64_t seed;
    uint64_t first_molecule_index;   /* index of the batch's first molecule in the whole input (RNG key) */
    int32_t mode;                    /* TKSMSEQ_TRC_* */
    int32_t always_end;              /* --always-end */
    int32_t kde_models_length;       /* --kde-models-length */
    int32_t flags;                   /* TKSMSEQ_MOL_NO_COMMENTS or 0 */
    double mu, sigma;                /* --normal / --lognormal */
    const char* kde_model_path;      /* --kde-model */
} tksmseq_trc_params;
int tksmseq_truncate(tksmseq_ctx* ctx, const tksmseq_batch* in, const tksmseq_trc_params* params, tksmseq_batch** out);

/* ---- segment edits: polyA, tag, scb, flip (the single-cell route of the reference README: plA -> Tag -> SCB -> Tag -> PCR -> Flp ->
 * Tag -> Seq) ------------------------------------------------------------------------------------------------------------------
 * Each takes a batch and returns a new one on the device, like tksmseq_truncate: molecules depth-unrolled (id_0, id_1, ...), written in
 * input order with depth 1; randomness depends only on (seed, first_molecule_index + i); comments carried through (re-serialised
 * like dump_comment), none with TKSMSEQ_MOL_NO_COMMENTS.  A new segment is a literal (contig name = its sequence) on the plus strand;
 * the output literal table is the input's followed by the new entries (TKSMSEQ_ELIMIT at 2^31 entries).
 *
 * tksmseq_polya replaces add_polyA / polya_transformer (src/polyA.cpp:133-148; module src/polyA.cpp:17-237): appends "A" x L,
 * L = the draw truncated toward zero, clamped to [min_length, max_length] (clamped in double first: huge and NaN draws are defined);
 * L = 0 appends nothing.  Gamma / Weibull: a = shape, b = scale (std:: parameterisation); Poisson: a = lambda; normal: a = mu,
 * b = sigma.  Exact samplers.  Parameters for which the std:: distribution is undefined (a, b, lambda or
 * sigma <= 0, non-finite values) are TKSMSEQ_EINVAL -- the reference's behaviour there is undefined; max_length above 2^20 is
 * TKSMSEQ_ELIMIT. */
#define TKSMSEQ_PLA_GAMMA 0
#define TKSMSEQ_PLA_POISSON 1
#define TKSMSEQ_PLA_WEIBULL 2
#define TKSMSEQ_PLA_NORMAL 3
typedef struct {
    uint64_t seed;
    uint64_t first_molecule_index;   /* index of the batch's first molecule in the whole input (RNG key) */
    int32_t dist;                    /* TKSMSEQ_PLA_* (--gamma / --poisson / --weibull / --normal) */
    int32_t flags;                   /* TKSMSEQ_MOL_NO_COMMENTS or 0 */
    double a, b;                     /* the distribution's parameters (b unused for Poisson) */
    int32_t min_length, max_length;  /* --min-length (0), --max-length (5000) */
} tksmseq_polya_params;
int tksmseq_polya(tksmseq_ctx* ctx, const tksmseq_batch* in, const tksmseq_polya_params* params, tksmseq_batch** out);

/* tksmseq_tag replaces TAG_module::run (src/tag.cpp:70-113): prepends a tag drawn from format5 and appends one drawn from format3,
 * each letter uniform over fmt2seq's IUPAC choices (src/util.h:53-92); letters outside that table (lower case included) add nothing,
 * an empty tag adds no segment.  The formats are taken as they are: the CLI's digit rule ("10" -> "NNNNNNNNNN", src/tag.cpp:84-91)
 * is applied by the caller.  A format without ambiguous letters (an adapter) is one literal shared by every molecule. */
typedef struct {
    uint64_t seed;
    uint64_t first_molecule_index;
    const char* format5;             /* -5/--format5, NULL or "" for none */
    const char* format3;             /* -3/--format3 */
    int32_t flags;                   /* TKSMSEQ_MOL_NO_COMMENTS or 0 */
    int32_t reserved;
} tksmseq_tag_params;
int tksmseq_tag(tksmseq_ctx* ctx, const tksmseq_batch* in, const tksmseq_tag_params* params, tksmseq_batch** out);

/* tksmseq_scb replaces SingleCellBarcoder_module::run (src/scb.cpp:57-80): appends the first value of the CB comment (unless it is
 * ".") as a literal segment and drops the CB key unless keep_meta_barcodes.  A molecule without CB (the reference's meta.at throws)
 * and a batch without comments are TKSMSEQ_EINVAL.  No randomness. */
typedef struct {
    int32_t keep_meta_barcodes;      /* --keep-meta-barcodes */
    int32_t flags;                   /* TKSMSEQ_MOL_NO_COMMENTS or 0 (CB is still read from the input's comments) */
} tksmseq_scb_params;
int tksmseq_scb(tksmseq_ctx* ctx, const tksmseq_batch* in, const tksmseq_scb_params* params, tksmseq_batch** out);

/* tksmseq_flip replaces StrandMan_module (src/strand_man.cpp:37-46, flip_molecule src/interval.h:908-920): molecule i is flipped --
 * segment order reversed, every strand toggled, substitutions and comments kept -- when u01(Philox(seed, i, 29)) < flip_probability.
 * Any probability is accepted (the reference only logs a value outside [0, 1]): <= 0 flips nothing, >= 1 everything. */
typedef struct {
    uint64_t seed;
    uint64_t first_molecule_index;
    double flip_probability;         /* -p/--flip-probability */
    int32_t flags;                   /* TKSMSEQ_MOL_NO_COMMENTS or 0 */
    int32_t reserved;
} tksmseq_flip_params;
int tksmseq_flip(tksmseq_ctx* ctx, const tksmseq_batch* in, const tksmseq_flip_params* params, tksmseq_batch** out);

/* ---- filter and concat: split and join molecule batches on the device --------------------------------------------------------------------
 * tksmseq_filter replaces the loop of Filter_module::run (src/filter.cpp:196-212) with FilterCondition (:21-117): a molecule of `in`
 * (depth-unrolled, like every transform here; the predicate depends on the record alone, so the output is the unrolling of the
 * reference's) goes to *out_true when ALL conditions hold -- inverted by negate -- and to *out_false otherwise, each side in input order,
 * ids with their unroll suffix, each side with the input's literal table and its molecules' comments (none with
 * TKSMSEQ_MOL_NO_COMMENTS).  out_false may be NULL: the false side is then neither sized nor written.  A side without molecules is an
 * ordinary empty batch.  Conditions:
 *   info KEY      the header comment has KEY with at least one value, the first of which is not "." (a bare key reads as ".");
 *                 a batch without comments has no key
 *   size OP N     OP one of < <= > >= == !=, against the sum of end - start over the molecule's segments (src/interval.h:876)
 *   locus CHR     any segment's contig is CHR: a contig of the context, or a literal segment whose text is CHR
 *   locus CHR:S-E, locus CHR:S   any segment on CHR with seg.overlap([S, E)) > 0, [S, S + 1) for the short form.  interval::overlap is
 *                 kept as written (src/interval.h:38-58): a range that shares exactly one end with the segment and extends past the
 *                 other (S < seg.start && E == seg.end, or S == seg.start && E > seg.end) overlaps by 0
 * A condition is given parsed (kind INFO / SIZE / LOCUS) or as the reference's text (kind TEXT, e.g. "size >=200").  TKSMSEQ_EINVAL with
 * "Invalid condition: <text>": a text that is not two space-separated fields, an unknown kind, a size expression shorter than two
 * characters or with an unknown operator, a number std::stoi would not take, a negative size value or coordinate. */
#define TKSMSEQ_FLT_TEXT 0
#define TKSMSEQ_FLT_INFO 1
#define TKSMSEQ_FLT_SIZE 2
#define TKSMSEQ_FLT_LOCUS 3
#define TKSMSEQ_FLT_LT 0
#define TKSMSEQ_FLT_LE 1
#define TKSMSEQ_FLT_GT 2
#define TKSMSEQ_FLT_GE 3
#define TKSMSEQ_FLT_EQ 4
#define TKSMSEQ_FLT_NE 5
typedef struct {
    int32_t kind;                    /* TKSMSEQ_FLT_* */
    int32_t cmp;                     /* SIZE: TKSMSEQ_FLT_LT .. TKSMSEQ_FLT_NE */
    const char* text;                /* TEXT: the condition; INFO: the key; LOCUS: the contig name */
    int64_t value;                   /* SIZE: N (0 .. 2^31 - 1) */
    int64_t start, end;              /* LOCUS with ranged: [start, end) */
    int32_t ranged;                  /* LOCUS: 0 any segment on the contig, 1 the range */
    int32_t reserved;
} tksmseq_filter_cond;
typedef struct {
    const tksmseq_filter_cond* conditions;
    uint64_t n_conditions;           /* 0: every molecule is true (false with negate) */
    int32_t negate;                  /* --negate */
    int32_t flags;                   /* TKSMSEQ_MOL_NO_COMMENTS or 0 (`info` is still read from the input's comments) */
} tksmseq_filter_params;
int tksmseq_filter(tksmseq_ctx* ctx, const tksmseq_batch* in, const tksmseq_filter_params* params, tksmseq_batch** out_true, tksmseq_batch** out_false);
/* tksmseq_concat is what the Snakefile's Mrg rule does with `cat`: the molecules of in[0], then in[1], ... in one batch.  All inputs
 * are batches of ctx.  Interval, substitution, literal and id indices are re-based, ids get their unroll suffix (the output has no
 * depth > 1 molecule), the literal tables are concatenated.  Comments are concatenated unless flags has TKSMSEQ_MOL_NO_COMMENTS; an
 * input without comments contributes empty ones when another input has them.  n_in 0 is TKSMSEQ_EINVAL, n_in 1 a copy; empty inputs
 * may stand anywhere.  TKSMSEQ_ELIMIT: a result beyond the table limits of a batch. */
int tksmseq_concat(tksmseq_ctx* ctx, const tksmseq_batch* const* in, uint64_t n_in, int32_t flags, tksmseq_batch** out);
/* `tksm filter` (Filter_module src/filter.cpp:119-231): -i/--input, -t/--true-output, -f/--false-output, -c/--condition (repeatable,
 * comma-separated), --negate; "Missing parameter: ..." and the help for a missing -i / -t / -c, exit codes 0 and 1; streamed in batches
 * of --batch-bytes over --devices like `tksm polyA`.  There is no `tksm merge`: on files Mrg is `cat`. */
int tksmseq_filter_main(int argc, char** argv);

/* ---- unsegment and shuffle: glue and reorder molecules on the device -------------------------------------------------------------------
 * tksmseq_glue replaces the loop of Unsegment_module::run (src/unsegment.cpp:88-105) and molecule_descriptor::concat (src/interval.h:893-896).
 * Molecule i of `in` (depth-unrolled, like every transform here) joins its predecessor iff i > 0 and joins(first_molecule_index + i), with
 *   joins(g) = g > 0 && Philox(seed, g, stream 30, block 0).x / 2^32 < probability
 * (g: the molecule's index in the whole input; the first molecule of a call is always a head).  Any probability is taken: <= 0 and NaN glue
 * nothing, >= 1 glues the batch into one molecule.  A chain -- a head and the maximal run of joiners behind it -- becomes one molecule with the
 * head's id, depth 1, and the segments of all members in order, strands and substitutions unchanged.  Comments: the head's is parsed, the
 * written id of every joiner is appended to key Cat in order (add_comment("Cat", md.get_id()), :99), and the result is dumped key-sorted
 * (a head with a bare "Cat;" keeps "Cat;", one with "Cat=x;" gets "Cat=x,<ids>;"); a joiner's own comment is dropped, as in the reference;
 * a head without joiners keeps its comment; an input without comments still gets "Cat=...;" on glued heads; none, and no id fetch, with
 * TKSMSEQ_MOL_NO_COMMENTS.  An empty input gives an empty batch.  TKSMSEQ_ELIMIT ("glue: ..."): a result beyond the table limits of a batch.
 * Two deliberate departures from the reference:
 *   - the last chain is written.  The reference never writes its last `current` (there is no `output << current` behind the loop at :91-105),
 *     so every run of it silently loses its final molecule or chain;
 *   - unrolled molecules draw for themselves.  The reference glues records: a depth-3 head gives three identical chimeras and a joiner's depth
 *     is lost.  Here every unrolled molecule draws for itself, as in every other transform.
 * The reference draws from one mt19937, so agreement with it is distributional only. */
typedef struct {
    uint64_t seed;
    uint64_t first_molecule_index;   /* index of molecule 0 of `in` in the whole input (streaming in pieces) */
    double probability;              /* -p/--probability */
    int32_t flags;                   /* TKSMSEQ_MOL_NO_COMMENTS or 0 */
    int32_t reserved;
} tksmseq_glue_params;
int tksmseq_glue(tksmseq_ctx* ctx, const tksmseq_batch* in, const tksmseq_glue_params* params, tksmseq_batch** out);
/* joins(g) on the host: 1 / 0, the device's draw bit for bit (needs no context) */
int tksmseq_glue_joins(uint64_t seed, double probability, uint64_t molecule_index);
/* tksmseq_shuffle replaces Shuffle_module::shuffle_stream (src/shuffle.cpp:23-44) on the n unrolled molecules of `in`; one call is one stream.
 * key(s) = x << 32 | y of Philox(seed, s, stream 31, block 0).  buffer_size 0 or >= n: the molecules in the order of (key(i), i) ascending, a
 * uniformly random permutation.  1 <= buffer_size = B < n: the reference's buffer, step for step -- slots 0 .. B-1 hold molecules 0 .. B-1; for
 * t = B .. n-1, slot = umulhi(Philox(seed, t, stream 35, block 0).x, B), output t - B is the occupant of slot, and t takes the slot; the last B
 * outputs are the slots' final occupants in the order of (key(s), s) over the slots -- computed with two sorts, not a sequential loop.  B = 1
 * is the identity.  buffer_size chooses the ORDER the reference would give; it does not bound memory.  Ids get their unroll suffix; comments
 * follow their molecules (none with TKSMSEQ_MOL_NO_COMMENTS).  TKSMSEQ_ELIMIT ("shuffle: ...") as above. */
typedef struct {
    uint64_t seed;
    uint64_t buffer_size;            /* --buffer-size; 0: the whole input */
    int32_t flags;                   /* TKSMSEQ_MOL_NO_COMMENTS or 0 */
    int32_t reserved;
} tksmseq_shuffle_params;
int tksmseq_shuffle(tksmseq_ctx* ctx, const tksmseq_batch* in, const tksmseq_shuffle_params* params, tksmseq_batch** out);
/* `tksm unsegment` (Unsegment_module src/unsegment.cpp:22-116): -i, -o, -p/--probability; "<name> is required!" per missing one, the help, exit
 * 1; streamed in batches of --batch-bytes over --devices, a piece ending only in front of a record whose first molecule does not join, so the
 * output depends on neither.  `tksm shuffle` (Shuffle_module src/shuffle.cpp:22-125): -i, -o, --buffer-size B (long only; 0 is refused); the
 * whole input is one batch on the first entry of --devices. */
int tksmseq_unsegment_main(int argc, char** argv);
int tksmseq_shuffle_main(int argc, char** argv);

/* ---- mutate: SNVs, insertions and deletions of a variant table applied on the device -------------------------------------------------------
 * The reference's own mutate (src/mutate.cpp) is unfinished -- an insertion loses its anchor, nothing knows about strands, a deletion that
 * shares an end with a segment deletes it whole, segments on contigs without variants are dropped (DESIGN.md section 7 lists the defects) --
 * so only its TABLE FORMAT is taken (-t/--tsv, :157-181, Mod::Mod :99-108) and the transform is defined here.  It is pinned by this: a perfect
 * read of a mutated molecule equals the same slice of the mutated contig.
 *
 * tksmseq_variants_load reads a table from `path`, or (path NULL) from text[0, len); ctx may be NULL (the message of a failure is then
 * tksmseq_last_error(NULL)'s); no device is touched.  One variant per line, three whitespace-separated fields CONTIG POS MOD, lines without
 * a field skipped, POS 0-based on the plus strand.  MOD all digits: a deletion of [min(POS, MOD), max(POS, MOD)) (empty: counted, no effect);
 * one byte that is no digit: an SNV, the base at POS becomes that byte (a plus-strand letter, like an MDF substitution); anything else an
 * insertion `X SEQ`: X is '.' or the letter that replaces the anchor base at POS, SEQ goes in BEHIND the anchor as plus-strand text.
 * TKSMSEQ_EINVAL, naming file and line: fewer than three fields, a POS or deletion end that is no integer in [0, 2^31 - 1], a lone '.';
 * TKSMSEQ_ELIMIT: an insertion of more than 2^20 letters, a table of 2^31 rows or more; TKSMSEQ_EIO: an unreadable file.
 * Normal form, per contig name: the union of the deletions as disjoint ascending ranges (ranges that touch are one); the point variants
 * (SNVs, insertions) by (POS, line), those inside a deleted range dropped.  tksmseq_variants_info: rows = snvs + insertions + deletions as
 * read, deleted_ranges and dropped_points of the normal form.  A table is immutable and may be used from several contexts and threads.
 *
 * tksmseq_mutate: every molecule of `in`, depth-unrolled (ids get _k, comments kept unless TKSMSEQ_MOL_NO_COMMENTS), segment by segment.  A
 * contig segment matches a table contig by name, a literal segment by its text; a segment that matches none, or with end <= start, is copied.
 * For a segment [s, e) on a table contig: its events are the deleted ranges [f, t) with t > s && f < e and the insertions with s <= POS < e; its
 * table substitutions the SNVs and the insertions with a letter X, s <= POS < e, in table order.  Without events the segment is copied with
 * all its own substitutions, the table's follow at POS - s.  With events, in ascending position from cur = s: a range emits the piece
 * [cur, f) if f > cur, then cur = min(t, e); an insertion at p emits [cur, p + 1) unless it is empty (a second insertion at one anchor), then
 * the literal {SEQ, 0, |SEQ|} on the segment's strand, then cur = p + 1; at the end [cur, e) if not empty.  A piece [a, b) carries the segment's
 * own substitutions with a - s <= position < b - s, in their order, re-based by a - s (the others are dropped, as einterval::truncate drops
 * them), then ALL table substitutions with a <= POS < b in table order at POS - a.  A minus-strand segment gives the same pieces and literals
 * in reverse order, all on the minus strand, the literal's text as the table has it (the splice reverse-complements it).  A molecule all of
 * whose segments are deleted stays, without segments.  The output's literal table is the input's followed by one entry per kept insertion.
 * No random numbers: the result does not depend on batching or devices.  The device form of the table is kept by the context and rebuilt
 * when another table is used or the context's reference has changed.  Known limit: a literal whose text equals a contig name becomes that
 * contig once it is written as text and parsed again.  TKSMSEQ_ELIMIT ("mutate: ..."): a result beyond the table limits of a batch. */
typedef struct tksmseq_variants tksmseq_variants;
int tksmseq_variants_load(tksmseq_ctx* ctx, const char* path, const char* text, uint64_t len, tksmseq_variants** out);
int tksmseq_variants_info(const tksmseq_variants* v, uint64_t* rows, uint64_t* snvs, uint64_t* insertions, uint64_t* deletions, uint64_t* deleted_ranges,
                          uint64_t* dropped_points);
void tksmseq_variants_free(tksmseq_variants* v);
typedef struct {
    int32_t flags;                   /* TKSMSEQ_MOL_NO_COMMENTS or 0 */
    int32_t reserved;
} tksmseq_mutate_params;
int tksmseq_mutate(tksmseq_ctx* ctx, const tksmseq_batch* in, const tksmseq_variants* v, const tksmseq_mutate_params* params, tksmseq_batch** out);
/* `tksm mutate`: -i, -o, -t/--tsv; "input is required!" / "output is required!" / "tsv is required!" per missing one, the help, exit 1
 * (src/mutate.cpp:217-233).  The table is read and checked before any context is made: a bad table is exit 1 with the line named.  Streamed
 * in batches of --batch-bytes over --devices; the output depends on neither. */
int tksmseq_mutate_main(int argc, char** argv);

/* ---- tail-noise: random and hairpin noise appended on the device ----------------------------------------------------------------------
 * tksmseq_append_noise replaces NoiseAdder::operator() (src/append_noise.cpp:83-128; module AppendNoise_module :131-229) -- not to be
 * confused with the Badread tail-noise MODEL of tksmseq_load_tail_model.  Molecule i (depth-unrolled, like every segment edit; the
 * reference's module reads without unrolling and gives all copies one draw) draws a noise length L from normal(mu, sigma) or
 * lognormal(mu, sigma) = exp of the normal, keyed by (seed, first_molecule_index + i), clamped in double to the int range (NaN: 0) and
 * truncated toward zero; L <= 0 leaves the molecule as it is.
 *   random mode: one literal of L letters on the plus strand is appended, each letter uniform over the positions of `alphabet` (a
 *     repeated letter is that much more likely);
 *   palindromic mode: the segments are walked from the last to the first, each copied with its strand toggled and its substitutions,
 *     until the copied bases are strictly above L; the last copy is then cut back to L bases in all (original on the plus strand:
 *     end -= extra, on the minus strand: start += extra; a total that equals L copies the next segment and cuts it to nothing).  Every
 *     base of the hairpin (min(L, molecule size) bases) then gets, with probability error_rate, a substitution by a letter of the
 *     alphabet.  Any error rate runs: <= 0 adds nothing, >= 1 substitutes every base.  The substitutions of a new segment are written
 *     sorted by position, a copied one before a new one at the same position.
 * Deviations from the reference: the copied substitutions of the cut copy are re-based to the kept range and those outside it dropped
 * (the reference keeps them at positions that no longer exist); a copy cut to length 0 is not written; depth-unrolled input.
 * TKSMSEQ_EINVAL: an empty alphabet, a non-finite mu, sigma <= 0 or non-finite, a NaN error rate, an unknown distribution (undefined
 * behaviour or an exit in the reference); TKSMSEQ_ELIMIT: in random mode a drawn L above 2^20 (the message names the molecule). */
#define TKSMSEQ_NOISE_NORMAL 0
#define TKSMSEQ_NOISE_LOGNORMAL 1
typedef struct {
    uint64_t seed;
    uint64_t first_molecule_index;
    int32_t dist;                    /* TKSMSEQ_NOISE_* (--length-dist NAME,MU,SIGMA) */
    int32_t palindromic;             /* --palindromic */
    double mu, sigma;
    double error_rate;               /* --error-rate (0.5), palindromic mode */
    const char* alphabet;            /* --alphabet ("AGTC") */
    int32_t flags;                   /* TKSMSEQ_MOL_NO_COMMENTS or 0 */
    int32_t reserved;
} tksmseq_noise_params;
int tksmseq_append_noise(tksmseq_ctx* ctx, const tksmseq_batch* in, const tksmseq_noise_params* params, tksmseq_batch** out);

/* ---- random-wgs: whole-genome fragments made on the device ---------------------------------------------------------------------------
 * tksmseq_wgs replaces the loop of RWGS_module::run (src/random_wgs.cpp:181-207; position_dist / frag_length_dist / strand_dist, the
 * contig look-up :190-194, the clip to the contig end :195-198, the molecule :200-204, the stop rule :188, :205).  There is no input
 * batch: CANDIDATE c = 0, 1, 2, ... of the run draws, from Philox keyed by (seed, c), a position uniform on [0, ref_length - 1] (the
 * contig is the first whose running sum of lengths reaches it, ref_pos = pos - so_far + len, as the reference computes them), a length
 * from the named distribution (std:: parameterisation: normal(a, b), uniform real on [a, b), lognormal(a, b) = exp of the normal,
 * exponential(a)), clamped in double to the int range (NaN: 0), truncated toward zero and clipped to the contig end, and a strand.  A
 * candidate is EMITTED when its clipped length is at least 1 (the reference also writes empty and inverted intervals, which no later
 * module handles).  Candidates are taken in order while the bases of the emitted candidates before them are below base_count: the output
 * of a run is a prefix of its emitted candidates, its total at least base_count and below it without the last molecule; base_count <= 0
 * gives nothing.  Molecule: id "{index}_{contig}:{ref_pos}-{ref_pos + len}{+|-}" (index: position among the emitted molecules of the
 * whole run), depth 1, no comment, one segment without substitutions.
 * A call covers candidates [first_candidate, first_candidate + n_candidates) and carries the run's state in and out, so that consecutive
 * calls, one after the other, give the output of one call over the whole range: results depend on (seed, candidate index) and on prefix
 * sums only.  The contig table is the context's reference in the order its contigs were added (with or without bases).  *out is an
 * ordinary batch (possibly empty; free with tksmseq_batch_free).  A call whose candidates emit nothing returns normally (progress shows
 * it): a caller that loops must stop by itself when whole calls stay empty (`exponential 1000`: every draw below one base).
 * TKSMSEQ_EINVAL: unknown distribution, non-finite a or b, a <= 0 or b < 0 (refused by the reference, :122), uniform with b < a;
 * TKSMSEQ_ESTATE: no contigs, or none with a base; TKSMSEQ_ELIMIT: a contig of 2^31 bases or more, more than 2^28 candidates per call. */
#define TKSMSEQ_WGS_NORMAL 0
#define TKSMSEQ_WGS_UNIFORM 1
#define TKSMSEQ_WGS_LOGNORMAL 2
#define TKSMSEQ_WGS_EXPONENTIAL 3
typedef struct {
    uint64_t seed;
    int32_t dist;                    /* TKSMSEQ_WGS_* (--frag-len-dist "NAME A [B]") */
    int32_t reserved;
    double a, b;
    int64_t base_count;              /* --base-count, or (int64)(depth x ref_length) for --depth */
    uint64_t first_candidate;        /* index of this call's first candidate in the whole run (RNG key) */
    uint64_t n_candidates;
    uint64_t molecules_before;       /* carried state: molecules and bases emitted by the calls before this one (0, 0 at the start) */
    uint64_t bases_before;
} tksmseq_wgs_params;
typedef struct {
    uint64_t next_candidate;         /* the first candidate the next call takes (reached: one past the run's last molecule) */
    uint64_t molecules, bases;       /* carried state after this call */
    int32_t reached;                 /* 1: base_count was reached inside (or before) this call -- the run is complete */
    int32_t reserved;
} tksmseq_wgs_progress;
int tksmseq_wgs(tksmseq_ctx* ctx, const tksmseq_wgs_params* params, tksmseq_batch** out, tksmseq_wgs_progress* progress);

/* ---- transcribe: GTF + abundance tables to molecules, expanded on the device -------------------------------------------------------------
 * Replaces Splicer_module::run (src/transcribe.cpp:119-198) without its fusion submodule (src/fusion.cpp: not built).  The entry module of
 * every transcriptome route: a row "transcript_id tpm cell-barcode" of an abundance table becomes `depth` copies of its transcript's exons
 * with the comment "CB=<barcode>;tid=<id>;".
 *
 * tksmseq_transcripts_add_gtf replaces read_gtf_transcripts_deep + the gtf line constructor + the merge of :134-137 (src/gtf.h:274-304,
 * src/interval.h:252-275): the transcripts of one more GTF go into the context's table; an id the table already has keeps what it has.
 * skip_non_coding is what the reference passes --default-depth as (:136): non-zero drops every line whose gene_biotype is not
 * protein_coding.  The reference's quirks are kept and listed in csrc/tsb_host.h; where it is undefined this is an error: TKSMSEQ_EINVAL
 * for a line with fewer than 9 fields, a coordinate that is no number in [1, 2^31 - 1], an exon before any transcript (the message names
 * file and line), TKSMSEQ_EIO for a file that cannot be read (the reference reads nothing, silently).  A failed call leaves the table as
 * it was.  Clones made afterwards share the table; plans keep the table they were made with. */
typedef struct tksmseq_tsb_plan tksmseq_tsb_plan;
int tksmseq_transcripts_add_gtf(tksmseq_ctx* ctx, const char* path, int skip_non_coding);
int tksmseq_transcripts_info(const tksmseq_ctx* ctx, uint64_t* n_transcripts, uint64_t* n_exons);
int tksmseq_transcripts_clear(tksmseq_ctx* ctx);
/* tksmseq_transcribe_plan_create replaces the abundance reader and the count loop (:149-158, :168-190) for ONE abundance table, read from
 * abundance_path, or (path NULL) from text[0, len).  Rows are read as operator>> reads them, the first line is skipped, only the row's id is
 * cut at its first '.' unless use_whole_id (format_annot_id, src/util.h:203-210).  For data row i, in IEEE double and in this order:
 * c = ((weight x tpm_i) x molecule_count) / sum_tpm, sum_tpm the left-to-right sum over all rows; carry = c - int(c); if a uniform of
 * Philox(seed, first_row_index + i, stream 56) is below carry, c += 1; depth = int(c); int() clamps in double first and takes NaN to 0.
 * A row is emitted when its id is in the transcript table and depth >= 1 (the reference also writes negative depths); the molecule id is
 * prefix + the row's rank among the emitted rows of this table (:168, :195: the index restarts with every table).  weight: the caller's
 * share of this table (process_file_weights, :65-77: one weight w is w / n_files for every table, several are normalised to sum 1);
 * first_row_index: the data rows of the tables before this one.  The counts and their prefix sums are computed on the device and stay
 * there.  TKSMSEQ_ESTATE: no GTF added; TKSMSEQ_EIO: "Could not open abundance file X!" (:146); TKSMSEQ_ELIMIT: a table of 4 GB or 2^32 - 2 rows. */
typedef struct {
    uint64_t seed;
    int64_t molecule_count;          /* --molecule-count */
    double weight;
    uint64_t first_row_index;
    int32_t use_whole_id;            /* --use-whole-id */
    int32_t reserved;
    const char* prefix;              /* --molecule-prefix (NULL: "M") */
} tksmseq_tsb_params;
int tksmseq_transcribe_plan_create(tksmseq_ctx* ctx, const char* abundance_path, const char* text, uint64_t len, const tksmseq_tsb_params* params,
                                   tksmseq_tsb_plan** out);
/* the same plan for another context that holds the same transcript table (a clone): the parsed rows are shared, the counts computed again */
int tksmseq_transcribe_plan_clone(tksmseq_ctx* ctx, const tksmseq_tsb_plan* src, tksmseq_tsb_plan** out);
/* rows: data rows; records: emitted rows; molecules: the sum of their depths; missing: rows whose id the table lacks, whose ids
 * tksmseq_transcribe_plan_missing gives in row order (not NUL-terminated: *len bytes) for "Isoform {} is not found in the input GTFs!" (:177) */
int tksmseq_transcribe_plan_info(const tksmseq_tsb_plan* plan, uint64_t* rows, uint64_t* records, uint64_t* molecules, uint64_t* missing);
int tksmseq_transcribe_plan_missing(const tksmseq_tsb_plan* plan, uint64_t i, const char** id, uint64_t* len);
void tksmseq_transcribe_plan_free(tksmseq_tsb_plan* plan);
/* tksmseq_transcribe replaces the molecule of :180, :192-196 read back with unroll (src/mdf.h:97-105): molecules [first_molecule,
 * first_molecule + n_molecules) of the plan's records unrolled (clipped to the end: a slice past it is an empty batch) as an ordinary batch
 * on ctx, the context the plan was made for.  Copies of a record with depth > 1 print as id_0, id_1, ... and sequence as molecule_id=id,
 * like the copies of a parsed depth > 1 molecule.  A contig the context's reference knows is that contig, any other name a literal, as the
 * MDF parser has it.  flags: TKSMSEQ_MOL_NO_COMMENTS or 0.  Results depend on (seed, row index) and prefix sums only, never on the slicing
 * or the device.  TKSMSEQ_ELIMIT: more than 2^28 molecules per call (checked first), a batch beyond the table limits of a batch;
 * TKSMSEQ_ESTATE: a plan of another context, a transcript table that has changed. */
int tksmseq_transcribe(tksmseq_ctx* ctx, const tksmseq_tsb_plan* plan, uint64_t first_molecule, uint64_t n_molecules, int32_t flags, tksmseq_batch** out);
/* Device time by HIP events (0 unless tksmseq_set_timing is on) of the context's last plan -- count, size and the four scans -- and of its
 * last tksmseq_transcribe -- the write kernel alone, without the batch finalisation every device-made batch goes through. */
int tksmseq_transcribe_device_ms(const tksmseq_ctx* ctx, float* plan_ms, float* write_ms);
/* outfile << molecule (:196; operator<< and dump_comment, src/interval.h:881-905) for records [first_record, first_record + n_records):
 * "+id<TAB>depth<TAB>CB=..;tid=..;" and one line per exon -- the reference's own compact output.  Release with tksmseq_text_free. */
int tksmseq_transcribe_text(const tksmseq_tsb_plan* plan, uint64_t first_record, uint64_t n_records, char** text, uint64_t* len);
/* `tksm transcribe` (Splicer_module src/transcribe.cpp:19-218): -g/--gtf, -a/--abundance (repeatable, comma-separated), --use-whole-id,
 * --molecule-count, -o/--output, --non-coding (no effect, :124), --default-depth (see above), --molecule-prefix, -w/--weights, -s/--seed,
 * --verbosity, --log-file; here also --devices (the first entry is used) and --batch-molecules.  The --fusion-* options are not taken. */
int tksmseq_transcribe_main(int argc, char** argv);

/* ---- model-truncation: the KDE truncation model built on the device ---------------------------------------------------------------------
 * Replaces py/truncate_kde.py (behind src/model_truncation.cpp), which needs scikit-learn: the 2-D model that tksmseq_truncate's KDE mode
 * and `tksm truncate --kde-model` read.
 *
 * tksmseq_kde_grid replaces KernelDensity(bandwidth).fit(xy).score_samples + exp (ComputeKDELikelihoods, :245-287; also the grid of
 * KDE_noise_generator.from_data, py/tksm_badread.py:888-901): out[i * gy + j] = 1 / (n 2 pi h^2) sum over the samples of
 * exp(-((x - px[i])^2 + (y - py[j])^2) / 2 h^2), the EXACT Gaussian density in the linear domain (scikit-learn's tree is approximate in
 * the tails: DESIGN.md section 7).  xy[n][2], px[gx], py[gy] and out are host arrays; the axis points are arbitrary doubles.  The sum is
 * one fp64 matrix product over chunks of samples whose partial grids are added in chunk order: the same input gives the same bytes on
 * every run.  TKSMSEQ_EINVAL: bandwidth <= 0 or non-finite, n = 0, an empty axis, a coordinate that is not finite (or above 1e150);
 * TKSMSEQ_ELIMIT: gx or gy above 4096, n >= 2^31.
 *
 * tksmseq_kde_cv_bandwidth replaces CV_KDE_bandwidth (:223-242), made reproducible: for repeat r = 0, 1, 2, cv_samples indices are drawn
 * WITH replacement as umul64hi(x << 32 | y, n), (x, y) the first words of Philox(seed, draw t, stream 48, r); the draw is cut into three
 * contiguous folds (KFold(3): the first cv_samples % 3 one longer); for each bandwidth of 50, 150, ..., 950 the score is the mean over
 * the folds of the sum over a fold's points of the exact log density of the other two folds; the repeat's bandwidth is the first maximum,
 * *bandwidth the median of the three.  scores (may be NULL): [3][10] mean scores.  TKSMSEQ_EINVAL: n = 0, cv_samples < 3, a coordinate
 * that is not finite; TKSMSEQ_ELIMIT: n >= 2^31, cv_samples above 2^24.
 *
 * tksmseq_model_truncation is main() of the script (:323-352): reads the primary alignments (lines with tp:A:P) of a PAF -- default: pairs
 * (truncation length = tstart + tlen - tend, tlen); model_lengths: (tlen, tend - tstart) -- and the end ratios, searches the bandwidth if
 * params->bandwidth <= 0, evaluates the grid at the cell centres (idx[k] + idx[k + 1]) // 2 of idx = arange(grid_start, grid_end + 1,
 * grid_step), and writes printModelJson's file (:298-320): KDE_mtx (data = P.T flattened, labels idx[1:] twice) and the 100-bin end_mtx
 * (np.histogram over np.arange(0, 1.01, 0.01); end_ratio != -1 replaces every ratio first).  The file is written under a temporary name
 * and renamed: a failure leaves nothing behind.  TKSMSEQ_EINVAL: fewer than two grid indices, an end ratio outside [0, 1] that is not
 * -1, a malformed PAF line, no primary alignment; TKSMSEQ_EIO: the PAF cannot be read or the output not written; TKSMSEQ_ELIMIT: more
 * than 4096 cells per axis. */
typedef struct tksmseq_kde_model_params {
    uint64_t seed;                   /* -s/--seed: the bandwidth search's draws */
    uint64_t cv_samples;             /* --cv-samples (100000) */
    double bandwidth;                /* -b/--bandwidth (100); <= 0: cross-validated search */
    int64_t grid_start, grid_end, grid_step;   /* --grid-start (0), --grid-end (10000), --grid-step (100) */
    int32_t model_lengths;           /* --model-lengths */
    int32_t reserved;
    double end_ratio;                /* --end-ratio (-1: from the PAF) */
} tksmseq_kde_model_params;
int tksmseq_kde_grid(tksmseq_ctx* ctx, const double* xy, uint64_t n, const double* px, uint32_t gx, const double* py, uint32_t gy,
                     double bandwidth, double* out);
int tksmseq_kde_cv_bandwidth(tksmseq_ctx* ctx, const double* xy, uint64_t n, uint64_t seed, uint64_t cv_samples, double* bandwidth,
                             double* scores /* [3][10] or NULL */);
int tksmseq_model_truncation(tksmseq_ctx* ctx, const tksmseq_kde_model_params* params, const char* paf_path, const char* out_path);
/* `tksm model-truncation` (src/model_truncation.cpp, py/truncate_kde.py:36-112): -i, -o, -b, --grid-start, --grid-end, --grid-step,
 * --model-lengths, --end-ratio, -t (accepted, ignored), --list; here also -s, --cv-samples, --devices (the first entry is used), --verbosity,
 * --log-file.  Exit codes as argparse: 2 for a missing -i / -o or an unknown option, 1 for everything that fails later. */
int tksmseq_model_truncation_main(int argc, char** argv);

/* ---- abundance: transcript expression from a PAF by EM on the device -----------------------------------------------------------------------
 * Replaces py/transcript_abundance.py (behind src/abundance.cpp): the table `tksm transcribe -a` reads.
 *
 * tksmseq_abundance is main() (:326-389).  The host reads the PAF (parse_paf :182-203: every line, columns 1, 2, 6, 8, 10, 11; reads and
 * transcripts numbered in order of first appearance, a read's records all lines with its name in file order) and, per options, the lr-br
 * table (parse_lr_bc_matches :166-179) or the whitelist.  On the device: get_compatibility (:210-256: the read length is the first record's;
 * the best record is replaced on more matches, or as many and target_start < 20; a read whose best block length / read length is below 0.5
 * is dropped; a record is a hit when matches / best matches > 0.95 in IEEE double and its full-length flag equals the best's; every hit
 * starts at 1 / hits), em_iterations rounds of calculate_abundance + update_compatibility (:260-289), and calculate_split_abundance
 * (:292-302) per (transcript, cell), rows in order of first appearance of the pair over the surviving reads and their hits.
 *
 * Ordered sums: no floating-point atomics anywhere.  The hits of a transcript (or pair), in read order, are cut into chunks of 1024; a chunk is
 * 64 running sums (sum l takes positions l, l + 64, ...) folded by the tree 32, 16, ..., 1; a transcript's chunks are added in chunk order;
 * the grand total is the transcripts' sums in transcript order through fixed trees of 256, their results in order the same way.  The result
 * is a function of the input alone: the same bits on every run, device, clone and launch shape.  It is NOT the left-to-right order of the
 * reference: abundances agree with it to rounding (tests: relative 1e-9), the printed %.3f values wherever no value sits on a rounding boundary.
 *
 * Cells: none of the options: every read is in cell ".".  lr_br_path: a read takes column 5 of the last line that names it with column 3
 * == "1"; other reads ".".  cb_count > 0 (the reference draws from numpy's legacy generator in dict order; here counter-based, Philox4x32-10
 * keyed by (seed, g, stream, n), words x, y, ...):
 *   stream 57  barcode b, position p of cb_pattern: letter = set[umulhi32(x, |set|)], set the IUPAC letter's bases in the reference's order; (g, n) = (b, p)
 *   stream 58  barcode b from the whitelist cb_txt_path (one per line): list[umulhi32(x, |list|)], with replacement; (g, n) = (b, 0)
 *   stream 59  weight of barcode b: exp(mu + sigma z), z = sqrt(-2 ln((x + 1) / 2^32)) cos(2 pi y / 2^32); (g, n) = (b, 0)
 *   stream 60  the cell of the k-th SURVIVING read: u = x / 2^32; the first barcode whose running weight sum (left to right; the last entry
 *              is the dropout cell "." with (sum of weights x dropout) / (1 - dropout)) exceeds u x the total; (g, n) = (k, 0)
 * Equal barcode strings are one cell.  dropout 1: every read is in ".".
 *
 * TKSMSEQ_EINVAL: the reference's argument checks (lr_br_path with cb_count; no pattern and no whitelist; a pattern letter outside IUPAC;
 * dropout outside [0, 1]; sigma <= 0; a whitelist shorter than cb_count); a PAF line with fewer than 11 columns or a used column that is
 * no integer in [0, 2^31) ("PAF line N: ..."); an lr-br line without exactly five columns; a read the reference ends on with a
 * ZeroDivisionError -- a first record of length 0, or a best record with 0 matches behind the 0.5 gate -- named in tksmseq_last_error.
 * TKSMSEQ_EIO: a file that cannot be read.  TKSMSEQ_ELIMIT: 2^31 reads, records, transcripts or barcodes, or more. */
typedef struct tksmseq_abundance_result tksmseq_abundance_result;
typedef struct tksmseq_abundance_params {
    uint64_t seed;                   /* --random-seed (42): the --cb-count draws */
    int32_t em_iterations;           /* -em/--em-iterations (10); 0 leaves the uniform split */
    int32_t keep_hits;               /* != 0: the final hits stay readable through tksmseq_abundance_hits */
    int64_t cb_count;                /* --cb-count (0) */
    double cb_dropout;               /* --cb-dropout (0.2) */
    double cb_mu, cb_sigma;          /* --cb-lognorm-params (10, 1) */
    const char* cb_pattern;          /* --cb-pattern ("NNNNNNNNNNNN"); NULL: "" */
    const char* cb_txt_path;         /* --cb-txt; NULL or "": none */
    const char* lr_br_path;          /* -m/--lr-br; NULL or "": none */
} tksmseq_abundance_params;
int tksmseq_abundance(tksmseq_ctx* ctx, const tksmseq_abundance_params* params, const char* paf_path, tksmseq_abundance_result** out);
/* rows: the rows the writer prints (tpm >= 0.001 and not "0.000"); surviving_reads: len(transcript_compatibility) (:371) */
int tksmseq_abundance_info(const tksmseq_abundance_result* r, uint64_t* rows, uint64_t* surviving_reads, uint64_t* reads, uint64_t* transcripts, uint64_t* hits);
/* row i: tpm = a x 1e6 as a double (the file has it as %.3f) */
int tksmseq_abundance_row(const tksmseq_abundance_result* r, uint64_t i, const char** transcript, const char** cell, double* tpm);
/* [transcripts], in order of first appearance in the PAF: the abundance of the last calculate_abundance of the EM loop, before the split
 * (em_iterations 0: of the uniform split) */
int tksmseq_abundance_vector(const tksmseq_abundance_result* r, const double** abundance);
int tksmseq_abundance_transcript(const tksmseq_abundance_result* r, uint64_t t, const char** name);
int tksmseq_abundance_cell(const tksmseq_abundance_result* r, uint64_t c, const char** name);
/* read i in order of first appearance: its name, and whether it survived the 0.5 gate */
int tksmseq_abundance_read(const tksmseq_abundance_result* r, uint64_t i, const char** name, int32_t* kept);
/* keep_hits: surviving[k] = the read, cell[k] its cell (tksmseq_abundance_cell), and its hits [hit_offsets[k], hit_offsets[k + 1]) in record
 * order: transcript and final weight.  TKSMSEQ_ESTATE without keep_hits. */
int tksmseq_abundance_hits(const tksmseq_abundance_result* r, const uint32_t** surviving, const uint32_t** cell, const uint32_t** hit_offsets,
                           const uint32_t** hit_transcript, const double** hit_weight);
/* device time by HIP events: compatibility, index, the EM rounds and the split (uploads and downloads excluded) */
int tksmseq_abundance_device_ms(const tksmseq_abundance_result* r, float* ms);
/* "target_id\ttpm\tcell" and the rows (:373-388); gzipped (host zlib) when the name ends in .gz; written under a temporary name and renamed.
 * TKSMSEQ_EIO when the file cannot be written; there is no context here, so tksmseq_last_error is NOT set: the caller names the path */
int tksmseq_abundance_write(const tksmseq_abundance_result* r, const char* out_path);
void tksmseq_abundance_free(tksmseq_abundance_result* r);
/* `tksm abundance` (src/abundance.cpp, py/transcript_abundance.py:32-139): -p/--paf, -m/--lr-br, --cb-count, --cb-lognorm-params, --cb-pattern,
 * --cb-dropout, --cb-txt, -o/--output, -em/--em-iterations, --random-seed, -v/--verbose, --list; here also --devices (the first entry is
 * used), --verbosity, --log-file.  Exit codes as argparse: 2 for a missing -p / -o, an unknown option or a failed argument check
 * ("abundance: error: ..."), 1 for everything that fails later.  Stdout: the reference's progress lines and "Parsed alignments for N reads". */
int tksmseq_abundance_main(int argc, char** argv);

/* ---- model-sequence: Badread error and q-score models built on the device --------------------------------------------------------------------
 * Replaces `badread error_model` + `badread qscore_model` (the model_sequence rule, Snakefile:507-546): the two files that
 * tksmseq_load_error_model / tksmseq_load_qscore_model read.  Badread's source is not part of the reference tree: the FILE FORMATS are the
 * reference's (the loaders py/tksm_badread.py:91-117 and :546-582, the window use :584-655, the shipped files), the COUNTING RULES below
 * are this build's own ("model-sequence").
 *
 * Inputs.  The context's reference (upper-cased).  reads_paths: a comma list of FASTQ files, plain or .gz; four lines per record, the name is
 * the header up to the first white space, bases upper-cased, quality = char - 33 in [0, 93].  paf_path: a PAF with cg:Z: tags; columns
 * 1, 2, 3, 4, 5, 6, 8, 9 (1-based) and the tags tp:A: and cg:Z: are read.
 *
 * Lines, in file order.  SKIPPED (one counter each): no cg:Z: tag; tp:A:S; a read name that is in no FASTQ file; a target that is not in
 * the reference; a CIGAR with an op outside M = X I D.  TKSMSEQ_EINVAL ("PAF line N: ..."): fewer than 12 columns; a used column that is
 * no integer in [0, 2^31); start > end or end > length (the target's length is the reference contig's); column 2 differs from the FASTQ
 * read's length; a CIGAR that does not consume exactly qend - qstart read bases and tend - tstart reference bases.  max_alignments N > 0
 * stops after N USED lines.  Strand '-': the read is reverse-complemented and its qualities reversed; the aligned part is then
 * [qlen - qend, qlen - qstart) of that.
 *
 * Columns.  The CIGAR expands to alignment columns: an M, = or X column is '=' if both bytes are equal and in ACGT, else 'X'; 'I' a read
 * base without a reference base, 'D' a reference base without a read base.
 *
 * Error model (error_k K in [3, 8], max_alt in [0, 31]).  Every reference offset t, tstart <= t, t + K <= tend, with c0 / c1 the columns of
 * reference bases t / t + K - 1, COUNTS when all K reference bases are in ACGT, columns c0 and c1 are '=' and every read base in columns
 * c0..c1 is in ACGT.  Its alternative is the read's bases in c0..c1.  total[kmer] += 1; an alternative of at most K + 4 bases also does
 * count[kmer][alt] += 1 (longer ones stay in the total: the residual).  The file: one line per k-mer, all 4^K in ACGT order,
 * "KMER,p;ALT,p;...;\n": the k-mer itself first (also with count 0), then the up to max_alt other alternatives by count descending, length
 * ascending, bytes ascending; p = count / total as a double, "%.6f"; a k-mer with total 0: "KMER,1.000000;".
 *
 * Q-score model (qscore_k Kq odd in [1, 29]).  Every read position i of the aligned part (n = qend - qstart) and every half-width
 * h = 0 .. (Kq - 1) / 2 with i - h >= 0 and i + h <= n - 1: the key is the column letters from the column of read position i - h to that of
 * i + h.  A key with a run of more than max_del 'D's is not counted (windows_max_del); otherwise one longer than 29 letters is not counted
 * (keys_too_long); otherwise count[key][q_i] += 1.  overall[q_i] += 1 once per read position.  The file: "overall;N;q:p,...,\n", then
 * the keys with N >= min_occur by N descending, length ascending, bytes ascending, at most max_output of them; '=', 'X' and 'I' are always
 * among the written keys (each takes the place of the last key of the cut that is not one of the three, or is added when max_output is
 * below 3); any of the three with count 0: TKSMSEQ_EINVAL naming it.  A line: "KEY;N;q:p,q:p,...,\n", every q with count > 0
 * ascending, p = count / N as "%.6f" with the trailing zeros removed ("0.0185", "0.").
 *
 * On the device: the columns of every alignment (one wave each), one event per reference offset and (Kq + 1) / 2 + 1 per read position,
 * radix sort + run lengths, per chunk of at most chunk_events events (0: sized from free device memory); the chunks' tables are merged by
 * concatenate, sort and reduce, so the files are the same bytes for every chunk size and on every run.  All counts are integers; there is
 * no floating point on the device.  error_out / qscore_out: either may be NULL; gzipped (host zlib) when the name ends in .gz; written
 * under <path>.tmp and renamed.
 *
 * TKSMSEQ_EINVAL also: both outputs NULL, a parameter out of range, a malformed FASTQ record, no used alignment.  TKSMSEQ_EIO: a file
 * that cannot be read or written.  TKSMSEQ_ELIMIT: 2^31 alignments, 2^31 events or more in one chunk (one alignment), 2^31 distinct keys, an alternative counted 2^32 times. */
typedef struct tksmseq_model_sequence_params {
    int32_t error_k;                 /* --error-k (7) */
    int32_t qscore_k;                /* --qscore-k (9) */
    int64_t max_alignments;          /* --max_alignments (0: all) */
    int32_t max_alt;                 /* --max_alt (25) */
    int32_t max_del;                 /* --max_del (6) */
    int64_t min_occur;               /* --min_occur (100) */
    int64_t max_output;              /* --max_output (10000) */
    uint64_t chunk_events;           /* events per chunk; 0: from free device memory */
} tksmseq_model_sequence_params;
typedef struct tksmseq_model_sequence_info {
    uint64_t lines;                  /* PAF lines read (up to the stop of max_alignments) */
    uint64_t used;                   /* alignments used */
    uint64_t skipped_no_cigar, skipped_supplementary, skipped_unknown_read, skipped_unknown_target, skipped_cigar_op;
    uint64_t counting_positions;     /* error model: the sum of the totals */
    uint64_t alternatives_too_long;  /* ... of them with an alternative above K + 4 */
    uint64_t windows_max_del;        /* q-score windows not counted for a 'D' run above max_del */
    uint64_t keys_too_long;          /* ... for more than 29 letters */
    uint64_t read_positions;         /* the N of the overall line */
    uint64_t error_keys, qscore_keys;   /* distinct (k-mer, alternative) / q-score keys counted */
    uint64_t chunks, events;
    float device_ms;                 /* by HIP events, all chunks: */
    float stage_ms[4];               /* columns, events, sort + reduce + merge, select */
    float reserved;
    double read_ms, upload_ms, write_ms;   /* host wall time: reading and parsing, uploads, formatting and writing */
} tksmseq_model_sequence_info;
int tksmseq_model_sequence(tksmseq_ctx* ctx, const tksmseq_model_sequence_params* params, const char* reads_paths /* comma list */, const char* paf_path,
                           const char* error_out /* or NULL */, const char* qscore_out /* or NULL */, tksmseq_model_sequence_info* info /* or NULL */);
/* `tksm model-sequence`: --reference R[,R] --reads F[,F] --alignment PAF [--error-model OUT] [--qscore-model OUT] [--error-k 7] [--qscore-k 9]
 * [--max_alignments 0] [--max_alt 25] [--max_del 6] [--min_occur 100] [--max_output 10000] [--devices D] [--verbosity V] [--log-file L]; at least
 * one output.  Exit codes as the other model modules: 2 for a missing required option, an unknown option or a value out of range
 * ("model-sequence: error: ..."), 1 for everything that fails later. */
int tksmseq_model_sequence_main(int argc, char** argv);

/* ---- barcode-match: long reads to cell barcodes on the device ---------------------------------------------------------------------------------
 * Replaces the three scTagger rules of the reference's single-cell route (scTagger_lr_seg, scTagger_extract_bc, scTagger_match: Snakefile,
 * "Preprocessing rules"): FASTQ reads and a barcode whitelist in, the lr_matches.tsv file that `abundance --lr-br` reads out.  scTagger's
 * source is not part of the reference tree: the FILE FORMAT is the consumer's (parse_lr_bc_matches, py/transcript_abundance.py:166-180: five
 * columns, columns 1, 3 and 5 used, a read kept only when column 3 is "1"), the RULES below are this build's own, and so are the defaults
 * (choices, not measurements of anything).  These are not scTagger's rules ("barcode-match").
 *
 * Inputs.  reads_paths: a comma list of FASTQ files, plain or .gz, read like model-sequence's (the name is the header up to the first white
 * space, bases upper-cased; a name may occur once over all files).  whitelist_path: one barcode per line, plain or .gz, empty lines skipped;
 * every barcode has the same length L in [4, 32] and letters in ACGT only; two lines with the same spelling: TKSMSEQ_EINVAL naming both.
 * adapter: 4 to 32 letters of ACGT.  window >= the adapter's length, pad in [0, 16], max_adapter_errors < the adapter's length,
 * max_errors < L, min_exact >= 0.  A byte of a read outside ACGT matches nothing and its complement is itself.  With revcomp_barcodes the
 * spelling that is MATCHED is the reverse complement of the file's; the spelling that is PRINTED is always the file's.
 *
 * Infix distance.  d(P, T) = the minimum Levenshtein distance of P to any substring of T, the empty one included; its end e(P, T) = the
 * smallest number of consumed letters of T at which that minimum is reached: the (|P| + 1) x (|T| + 1) table with row 0 all zeros and
 * column 0 = i, d = the minimum of the last row, e = its first column.
 *
 * Adapter.  For orientation o = 0 (the read) and 1 (its reverse complement), T_o the oriented read: (da_o, ja_o) = (d, e) of the adapter in
 * the first min(window, length) letters of T_o.  The smaller da wins, o = 0 wins a tie.  Winning da > max_adapter_errors: the read counts as
 * no_adapter and appears in no output.
 *
 * Segment.  seg = T_o[max(0, ja - pad) : min(length, ja + L + pad)], bounds in the whole oriented read: at most L + 2 pad <= 64 letters.
 *
 * Selection.  Every window of L letters of every segment that is all ACGT and spells a whitelist barcode (matched spelling) adds 1 to
 * exact[b]; every window counts, also twice in one segment.  The candidates: the barcodes with exact[b] >= min_exact, in whitelist order
 * (min_exact 0: the whole whitelist).
 *
 * Match.  For every segment and every candidate b: d(matched spelling of b, seg); dmin = the minimum over the candidates.  No candidate, or
 * dmin > max_errors: the read counts as no_barcode and gets no line.  Otherwise one line of matches_out, the reads in input order:
 *     RID <TAB> dmin <TAB> COUNT <TAB> da <TAB> BC[,BC...] <NL>
 * COUNT = the number of candidates at dmin; the list holds the first min(COUNT, 8) of them in whitelist order.
 * segments_out (or NULL): RID <TAB> da <TAB> +|- <TAB> start <TAB> SEGMENT for every read with an adapter (start: the segment's first letter
 * in the oriented read).  selected_out (or NULL): BARCODE <TAB> exact, one line per candidate.  Files are written under <path>.tmp and renamed,
 * gzipped (host zlib) when the name ends in .gz.
 *
 * On the device: at most window + L + pad letters of each end of a read are uploaded, 2 bits a letter and a validity bit; the adapter is
 * aligned by the bit-parallel column step of Myers (1999) in one 32-bit word, one lane per read and orientation; the whitelist's 64-bit keys
 * are sorted once and every segment window is looked up by binary search, counted with integer atomics; every segment is aligned to every
 * candidate, the barcode as the pattern in one 32-bit word.  Reads go in chunks of chunk_reads (0: sized from free device memory); selection
 * sees all chunks before any match starts; the outputs are the same bytes for every chunk size and on every run.  No floating point.
 *
 * TKSMSEQ_EINVAL: a parameter out of range, a malformed FASTQ or whitelist, no reads.  TKSMSEQ_EIO: a file that cannot be read or written.
 * TKSMSEQ_ELIMIT: 2^31 reads or 2^27 whitelist lines, or more. */
typedef struct tksmseq_barcode_match_params {
    const char* adapter;             /* --adapter (NULL: CTACACGACGCTCTTCCGATCT) */
    int32_t window;                  /* --window (200) */
    int32_t max_adapter_errors;      /* --max-adapter-errors (5) */
    int32_t pad;                     /* --pad (4) */
    int32_t max_errors;              /* --max-errors (2) */
    int64_t min_exact;               /* --min-exact (2) */
    int32_t revcomp_barcodes;        /* --revcomp-barcodes */
    int32_t reserved;
    uint64_t chunk_reads;            /* reads per chunk; 0: from free device memory */
    const char* segments_out;        /* --segments-out, or NULL */
    const char* selected_out;        /* --selected-out, or NULL */
} tksmseq_barcode_match_params;
typedef struct tksmseq_barcode_match_info {
    uint64_t reads;
    uint64_t no_adapter, forward, reverse;     /* reads = no_adapter + forward + reverse (the winning orientation) */
    uint64_t whitelist, candidates;
    uint64_t no_barcode, unique, ambiguous;    /* forward + reverse = no_barcode + unique (COUNT = 1) + ambiguous */
    uint64_t pairs;                  /* (segment, candidate) pairs compared */
    uint64_t chunks;
    float device_ms;                 /* by HIP events, all chunks: */
    float stage_ms[4];               /* adapter, selection, match, gather */
    float reserved;
    double read_ms, upload_ms, write_ms;   /* host wall time: reading and parsing, packing and uploads, formatting and writing */
} tksmseq_barcode_match_info;
int tksmseq_barcode_match(tksmseq_ctx* ctx, const tksmseq_barcode_match_params* params, const char* reads_paths /* comma list */, const char* whitelist_path,
                          const char* matches_out, tksmseq_barcode_match_info* info /* or NULL */);
/* `tksm barcode-match`: --reads F[,F] --whitelist W -o LR_MATCHES.tsv[.gz] [--adapter A] [--window 200] [--max-adapter-errors 5] [--pad 4] [--max-errors 2]
 * [--min-exact 2] [--revcomp-barcodes] [--segments-out F] [--selected-out F] [--chunk-reads N] [--devices D] [--verbosity V] [--log-file L].  Exit codes
 * as the other model modules: 2 for a missing required option, an unknown option or a value out of range ("barcode-match: error: ..."), checked
 * before any device is opened; 1 for everything that fails later. */
int tksmseq_barcode_match_main(int argc, char** argv);

/* ---- map: long reads to transcripts by minimizer chains on the device --------------------------------------------------------------------------
 * Replaces the two minimap2 rules of the reference's workflow (minimap_cdna, minimap_cdna_for_badread_models: Snakefile): FASTQ reads and the
 * context's reference (a cDNA FASTA) in, the PAF that `abundance -p` (columns 1, 2, 6, 8, 10, 11) and `model-truncation -i` (columns 7, 8, 9)
 * read out.  tksmseq_map seeds and chains only, the PAF minimap2 writes without -c; tksmseq_map_align ("map, alignment" below) adds the
 * base-level alignment of the written chains and the cg:Z: tag model-sequence reads.  minimap2's source is not part of the reference tree: the FILE FORMAT is the consumers', the RULES below are this build's own, and so
 * are the defaults (choices, not measurements of anything).  These are not minimap2's rules ("map").  Everything is integer: the
 * output is the same bytes on every run and for every chunk size.
 *
 * Inputs.  The targets are the contigs of the context's reference, in contig order.  reads_paths: a comma list of FASTQ files, plain or .gz,
 * read like model-sequence's (the name is the header up to the first white space, bases upper-cased, a name at most once).  A byte outside
 * ACGT is invalid and belongs to no k-mer.
 *
 * k-mer.  k in [4, 28] (15), w in [1, 64] (10).  Position p covers [p, p + k).  fwd holds 2 bits per letter (A C G T = 0..3), the first
 * letter highest; rev is the code of the reverse complement.  The k-mer is valid when all k letters are ACGT and fwd != rev; its strand is
 * s = rev < fwd; its hash h is the splitmix64 finaliser of min(fwd, rev), all 64 bits kept:
 *     x ^= x >> 30; x *= 0xbf58476d1ce4e5b9; x ^= x >> 27; x *= 0x94d049bb133111eb; x ^= x >> 31.
 *
 * Minimizers.  A sequence with n = len - k + 1 <= 0 positions has none.  Otherwise its windows are [j, min(j + w, n)) for
 * j = 0 .. max(0, n - w).  Each window selects its valid position with the smallest (h, p); a window without a valid position selects
 * nothing.  The minimizers are the distinct selected positions.
 *
 * Index.  Every target minimizer (h, target, p, s), ordered by (h, target, p).  A hash that occurs more than max_occ times (500) seeds nothing.
 *
 * Anchors.  For a read minimizer (h, q, sr) and an index entry (h, t, p, st): rel = sr ^ st; qa = q when rel = 0, else qlen - k - q (the
 * k-mer's start in the reverse-complemented read); the anchor is (t, rel, p, qa).  The anchors of one (read, t, rel) form a group, ordered by
 * (p, qa).
 *
 * Chain.  For anchor i of a group, f[i] = k with no predecessor to begin with.  Every j in [max(0, i - 64), i) with dt = p_i - p_j and
 * dq = qa_i - qa_j is a candidate predecessor when dt > 0 and dq > 0, dt <= max_gap and dq <= max_gap (5000), and g = |dt - dq| <= bandwidth
 * (500).  Its score is f[j] + min(k, dt, dq) - cost(g), cost(0) = 0 and cost(g) = g k / 100 + floor(log2 g) / 2 in integer division.  The
 * largest candidate wins, among equal candidates the largest j; it becomes the predecessor, and f[i] its score, only when it exceeds k.
 * The group's chain ends at the i with the largest f (the smallest such i on a tie) and is followed back through the predecessors: a group
 * gives one chain, with cnt = its anchors, score = f[i], nmatch = k + the sum of min(k, dt, dq) over its links, tstart = p_first,
 * tend = p_last + k, qs = qa_first, qe = qa_last + k, blen = max(tend - tstart, qe - qs).  It is kept when cnt >= min_count (3) and
 * score >= min_score (40).
 *
 * Per read.  The kept chains ordered by (score descending, target ascending, rel ascending).  The first is the primary (tp:A:P), its
 * mapq = min(60, 60 (s1 - s2) / s1) with s2 the second chain's score, or 0 when there is none.  The others are written as tp:A:S with mapq 0
 * while score 1000 >= P s1, at most max_secondary of them (5); P = 1000 secondary_ratio rounded half up, computed on the host (0.8; the
 * reference's workflow passes -p 0.0).  Reads appear in input order; a read without a kept chain gets no line and counts as unmapped.
 *
 * Line.  QNAME qlen qstart qend +|- TNAME tlen tstart tend nmatch blen mapq tp:A:P|S cm:i:cnt s1:i:score, tab-separated.  For rel = 1 the
 * query interval is given in the original read: qstart = qlen - qe, qend = qlen - qs.  The file is written under <path>.tmp and renamed,
 * gzipped (host zlib) when the name ends in .gz.
 *
 * On the device: the k-mer codes are cut from whole words of the packed sequences (the reads are packed like the reference), the window
 * minimum is taken over an LDS tile; the index is radix-sorted by hash once per call and kept over the chunks; every read minimizer finds its
 * hash by binary search; the anchors are sorted by (read, target, rel, p, qa) in two stable passes; groups below min_count anchors are dropped
 * before chaining; a wave chains one group, lane l holding one of the 64 predecessors in registers.  Reads go in chunks of chunk_reads
 * (0: sized from free device memory); a chunk with more anchors than the budget is split, never truncated.  No floating point.
 *
 * TKSMSEQ_EINVAL: a parameter out of range (also max_occ < 1, min_count < 1, a negative max_gap, bandwidth or min_score, secondary_ratio
 * outside [0, 1], max_secondary outside [0, 1000]), a malformed FASTQ, no reads, or no reference.  TKSMSEQ_EIO: a file that cannot be read or
 * written.  TKSMSEQ_ELIMIT: 2^31 reads, or a read or target of 2^31 bases, or more; one read with more anchors than a chunk may hold (2^24). */
typedef struct tksmseq_map_params {
    int32_t k;                       /* -k (15) */
    int32_t w;                       /* -w (10) */
    int32_t max_occ;                 /* --max-occ (500) */
    int32_t max_gap;                 /* --max-gap (5000) */
    int32_t bandwidth;               /* --bandwidth (500) */
    int32_t min_count;               /* --min-count (3) */
    int32_t min_score;               /* --min-score (40) */
    int32_t reserved;
    double secondary_ratio;          /* -p (0.8) */
    int32_t max_secondary;           /* -N (5) */
    int32_t reserved2;
    uint64_t chunk_reads;            /* reads per chunk; 0: from free device memory */
} tksmseq_map_params;
typedef struct tksmseq_map_info {
    uint64_t reads, mapped, unmapped, lines, secondary;        /* reads = mapped + unmapped; lines = mapped + secondary */
    uint64_t target_minimizers, distinct_hashes, dropped_hashes;
    uint64_t read_minimizers, anchors, groups, chained_groups, chunks;   /* chained_groups: the groups of at least min_count anchors */
    float device_ms, stage_ms[5];    /* by HIP events, all chunks: sketch, index, seed, chain, select */
    double read_ms, upload_ms, write_ms;   /* host wall time: reading and parsing, packing and uploads, formatting and writing */
} tksmseq_map_info;
/* params NULL: the defaults above */
int tksmseq_map(tksmseq_ctx* ctx, const tksmseq_map_params* params, const char* reads_paths /* comma list */, const char* paf_out, tksmseq_map_info* info /* or NULL */);

/* ---- map, alignment: base-level alignment of the written chains on the device (map -c: cg:Z:, NM:i:) ------------------------------------------
 * Applies to every line map writes, primary and secondary, after the selection: a chain that is not written is never aligned.  These are
 * this build's rules, not minimap2's: unit cost, a static band, no end extension unless --extend ("map, end extension" below), a waypoint
 * at every anchor ("map").
 *
 * Waypoints.  A written chain has anchors a_0 .. a_{n-1}, a_i = (p_i, qa_i): the target position and the position in the read in the strand
 * of rel.  Along a chain dt = p_{i+1} - p_i > 0 and dq = qa_{i+1} - qa_i > 0 (the chain rule).  The alignment passes through every
 * (p_i, qa_i) and through (p_{n-1} + k, qa_{n-1} + k): n segments, n - 1 between consecutive anchors and the last anchor's k-mer
 * (dt = dq = k).  It covers exactly [tstart, tend) x [qs, qe) of the chain (unless --extend).  Columns 1-9 and 12 and the tp, cm and s1 tags of a line are
 * the same with and without alignment.
 *
 * Letters.  T[i] is the target letter at p + i.  Q[j] is the read letter at qa + j for rel = 0, and the complement of the read letter at
 * qlen - 1 - (qa + j) for rel = 1.  Two letters match when both are ACGT and equal: a letter outside ACGT matches nothing, itself included.
 *
 * Segment.  A global, unit-cost alignment of T[0, dt) against Q[0, dq) inside a static band around the straight line between the two
 * corners: cell (i, j), 0 <= i <= dt, 0 <= j <= dq, is allowed iff 2 |i dq - j dt| <= W (dt + dq) in 64-bit integers, W the band in
 * [1, 63] (63).  D[0][0] = 0; otherwise D[i][j] is the minimum over the allowed predecessors of D[i-1][j-1] + (T[i-1] matches Q[j-1] ? 0 : 1),
 * D[i-1][j] + 1 and D[i][j-1] + 1.  (dt, dq) is reachable for every W >= 1; an anti-diagonal i + j = s holds at most W + 1 allowed cells,
 * with consecutive i; when 2 dt dq <= W (dt + dq) every cell is allowed and D is the Levenshtein distance.
 *
 * Traceback.  From (dt, dq), at each cell the first of these moves that reproduces D[i][j] from an allowed predecessor: the diagonal (a
 * column = or X), then (i-1, j) (a column D, which consumes the target), then (i, j-1) (a column I, which consumes the read).
 *
 * Line.  The columns of the segments in chain order, run-length encoded: = X I D with eqx, else = and X merged into M.  Column 10 becomes
 * the number of = columns and column 11 the number of all columns; after s1:i: come NM:i: (the sum of the segments' D[dt][dq], which is the
 * number of X, I and D columns) and cg:Z: (the CIGAR).  The CIGAR consumes tend - tstart target letters and qend - qstart read letters;
 * for rel = 1 it is in target order, like minimap2's.  Everything is integer: the same bytes on every run and for every chunk size.
 *
 * On the device: the anchors of a written chain are walked back from its end anchor, found by binary search in the sorted group, through
 * the predecessors the chain kernel left; one wave aligns the segments of one line, lane i % 64 owning cell (i, s - i) of anti-diagonal s
 * with its neighbours' values one lane below; two traceback bits per cell go to a store of the wave, which the same wave walks back; the
 * columns are run-length encoded on the device.  A chunk whose alignment does not fit its budget of device bytes is split like one with
 * too many anchors.
 *
 * TKSMSEQ_EINVAL: band outside [1, 63]; max_gap above 65536 with alignment (a segment's traceback store is sized by dt + dq).
 * TKSMSEQ_ELIMIT: one read whose alignment does not fit a chunk's budget. */
typedef struct tksmseq_align_params {
    int32_t band;                    /* --align-band (63) */
    int32_t eqx;                     /* --eqx: = and X in place of M */
} tksmseq_align_params;
typedef struct tksmseq_align_info {
    uint64_t lines, segments, longest_segment /* dt + dq */, cells /* allowed cells computed */;
    uint64_t columns, matches, mismatches, inserted, deleted;   /* columns = the sum of the other four */
    float align_ms, reserved;        /* by HIP events, all chunks */
} tksmseq_align_info;
/* align NULL: exactly tksmseq_map.  align_info may be NULL. */
int tksmseq_map_align(tksmseq_ctx* ctx, const tksmseq_map_params* params, const tksmseq_align_params* align, const char* reads_paths, const char* paf_out,
                      tksmseq_map_info* info, tksmseq_align_info* align_info);

/* ---- map, end extension: X-drop extension of both ends of the written chains on the device (map --extend) -------------------------------------
 * Without it a line covers exactly its chain: tstart is the first anchor, tend the last anchor plus k, and the first and last surviving
 * minimizers of an erroneous read lie well inside it.  With it both corners of every line map writes, primary and secondary, after the
 * selection, move outward as far as a banded alignment with an X-drop stop carries them, with and without alignment.  It never changes
 * which lines are written, their order, mapq, tp, cm or s1.  These are this build's rules, not minimap2's ("map").
 *
 * Ends.  Coordinates are the chain's: the target runs forward, the read is in the strand of rel; T[i] and Q[j] and what matches are those
 * of "Letters" above.  Right end: the corner is (tend, qe), T' = T[tend ...], Q' = Q[qe ...].  Left end: the corner is (tstart, qs), T' and
 * Q' are the letters before the corner, read backwards.  Both are cut to at most max_ext letters, Lt and Lq; when Lt = 0 or Lq = 0 the end
 * is not extended.
 *
 * Cells.  Match +1, mismatch -2, a gap column -2 (linear; fixed, not options).  Cell (i, j), 0 <= i <= Lt, 0 <= j <= Lq, is allowed iff
 * |i - j| <= B: an anti-diagonal s = i + j holds at most B + 1 allowed cells.  H[0][0] = 0 with m[0][0] = 0 matches; otherwise H[i][j] is
 * the largest, over the allowed predecessors, of H[i-1][j-1] + (T'[i-1] matches Q'[j-1] ? 1 : -2), H[i-1][j] - 2 (a column D) and
 * H[i][j-1] - 2 (a column I); on equal values the first in this order wins, m is carried from the chosen predecessor, plus 1 on a
 * matching diagonal, and the traceback follows the same choice.
 *
 * Best cell and stop.  The anti-diagonals are computed for s = 1, 2, ...; mx_s is the largest H of anti-diagonal s (mx_0 = 0).  The best
 * cell is the one with the largest H: among equal positive values the later anti-diagonal wins, within one anti-diagonal the smallest i;
 * when no cell is above 0 it is (0, 0).  After anti-diagonal s (its cells counted in) the extension stops when
 * max(mx_s, mx_{s-1}) < best - Z, when s = Lt + Lq, or before an anti-diagonal without an allowed cell.  Single cells are never pruned.
 *
 * Line.  The best cell (ei, ej) moves the corner: tend += ei, qe += ej, or tstart -= ei, qs -= ej.  Columns 3, 4, 8 and 9 are those of
 * the moved corners (for rel = 1 the read interval is converted as before).  Without alignment column 10 = the chain's nmatch + the m of
 * both ends and column 11 = max(tend - tstart, qe - qs) of the moved corners.  With alignment the columns are the left end's traceback in
 * target order, the chain's segments, the right end's traceback; columns 10 and 11, NM:i: and cg:Z: are computed over all of them by the
 * rules above (eqx as there), and the CIGAR consumes exactly tend - tstart target letters and qend - qstart read letters.  No tag is
 * added.  band B in [1, 63] (31), drop Z in [1, 1000] (40), max_ext in [1, 32768] (2000): choices, not measurements.  Everything is
 * integer: the same bytes on every run and for every chunk size.
 *
 * On the device: one wave per (line, end); on anti-diagonal s lane (i - j + B) >> 1 owns cell (i, j), its own value of step s - 2 is the
 * diagonal and its two neighbours of step s - 1, one of them its own and which one alternating with the parity of s + B, are the D and I
 * predecessors; a wave-wide maximum per step serves the stop and the best cell; the letters are cut from the packed words, the left end
 * walking them backwards.  A first pass keeps no store and gives (ei, ej, m).  With alignment a second pass over the ends that moved
 * computes anti-diagonals 1 .. ei + ej again with two traceback bits per cell in a store of the wave, which the same wave walks back from
 * (ei, ej): stores and columns are sized by what the first pass found, not by max_ext.  A chunk whose extension does not fit its budget
 * of device bytes is split like one with too many anchors.
 *
 * TKSMSEQ_EINVAL: band, drop or max_ext out of range.  TKSMSEQ_ELIMIT: one read whose extension does not fit a chunk's budget. */
typedef struct tksmseq_extend_params {
    int32_t band;                    /* --ext-band (31) */
    int32_t drop;                    /* --ext-drop (40) */
    int32_t max_ext;                 /* --ext-max (2000) */
    int32_t reserved;
} tksmseq_extend_params;
typedef struct tksmseq_extend_info {
    uint64_t lines, ends_moved /* of 2 lines */, target_gained, read_gained /* letters, both ends */, matches /* the sum of m */;
    uint64_t antidiagonals, cells /* computed by the first pass */, longest /* the largest ei + ej */;
    float extend_ms, reserved;       /* by HIP events, all chunks, both passes */
} tksmseq_extend_info;
/* extend NULL: exactly tksmseq_map_align; align NULL: no alignment, as there.  align_info and extend_info may be NULL. */
int tksmseq_map_extend(tksmseq_ctx* ctx, const tksmseq_map_params* params, const tksmseq_align_params* align, const tksmseq_extend_params* extend, const char* reads_paths,
                       const char* paf_out, tksmseq_map_info* info, tksmseq_align_info* align_info, tksmseq_extend_info* extend_info);

/* ---- map, split reads: supplementary lines for chimeric and hairpin reads on the device (map --split) ----------------------------------------
 * Without it a (read, target, strand) group gives one chain and a read one primary line with its alternatives: of a read glued from several
 * molecules (`unsegment`) or folded back onto itself (`tail-noise --palindromic`) one piece is reported.  With it every further piece gets a
 * tp:A:P line of its own, the way minimap2 writes supplementary alignments in a PAF.  A read whose lines all overlap gets exactly the lines
 * it gets without it.  These are this build's rules, not minimap2's ("map").
 *
 * Rounds.  Round 1 of a group is the chain of "Chain" above over all its anchors, unchanged.  When the chain of round r is kept, its read
 * interval in the strand of rel is [qs, qe): every anchor of the group whose k-mer meets it (qa < qe and qa + k > qs) leaves the group, the
 * chain's own anchors among them.  When at least min_count anchors remain, round r + 1 applies the same chain rule to the remaining anchors
 * in their (p, qa) order: the 64 predecessors of a step are the 64 REMAINING anchors before it.  The rounds of a group end with the first
 * chain that is not kept, with fewer than min_count remaining anchors, or after `chains` rounds, chains in [1, 16] (4).  A chain of a later
 * round has the fields of a round-1 chain and is kept by the same min_count / min_score test.
 *
 * Step A.  The primary, its mapq and the secondaries are chosen exactly as in "Per read" above, from the round-1 chains alone.
 *
 * Step B.  The candidates are the read's kept chains of all rounds that step A did not write, ordered by (score descending, target
 * ascending, rel ascending, round ascending) and walked in that order.  Read intervals are in original read coordinates, [qstart, qend) of
 * "Line" above, of the chain's own corners (before any --extend).  A candidate is accepted when its read interval shares at most `overlap`
 * letters, overlap in [0, 2^31) (30), with the primary's and with that of every candidate accepted before it; otherwise it is rejected, and
 * the walk goes on.  The walk ends after segments - 1 acceptances, segments in [2, 64] (8); candidates it does not reach are neither
 * accepted nor rejected.  Secondaries take no part in the overlap test.  The three defaults are choices, not measurements of anything.
 *
 * mapq of a supplementary line: min(60, 60 (s - s2) / s), and 0 when s2 >= s.  s is the line's score; s2 is the largest score among the
 * read's kept chains of any round that are not written as tp:A:P and share more than `overlap` letters with this line's read interval, or 0
 * when there is none.
 *
 * Lines of a read: the primary, its secondaries, then the supplementary lines in order of acceptance.  A supplementary line is formatted
 * like a primary: tp:A:P, its own cm:i: and s1:i:.  When a read has n >= 2 tp:A:P lines, each of them carries sn:i:n and si:i:i directly
 * after s1:i: (before NM:i: with alignment): i is the line's 0-based rank among the read's tp:A:P lines by (qstart, qend, order of
 * acceptance, the primary first), of the chain's own corners.  Secondary lines, and all lines of a read with one tp:A:P line, are byte for
 * byte those without --split.  -c and --extend apply to a supplementary line as to any written line, by their rules above: the selection
 * precedes both, so neither changes which lines are written.  `abundance` and `model-truncation` read these lines as they read any other
 * (INTEGRATION.md).
 *
 * Counters.  split_reads: reads with a supplementary line.  supplementary: those lines.  later_chains: kept chains of rounds >= 2.  rounds:
 * all rounds run, all groups (a group that is chained runs at least one).  rejected_overlap: candidates the walk of step B rejected.  With
 * split tksmseq_map_info.lines = mapped + secondary + supplementary.  split_ms: by HIP events, the chain stage and the select
 * stage whole, that is stage_ms[3] + stage_ms[4] of the same call: the chain kernel with all its rounds, and the selection with its key
 * kernel, the sort of the chain keys and the copies of the lines to the host.  One kernel runs all rounds of a group, so the first
 * round is not timed apart, and the two stages are not bracketed more tightly than without split.
 *
 * Estimate.  Every segment of a molecule but the first was glued with probability p, so with J supplementary lines in M mapped reads the
 * module logs "split: J junctions in M mapped reads: unsegment -p estimate J / (M + J - 1)".
 *
 * On the device: one wave chains all rounds of a group.  It gathers the anchors through a list of the remaining original indices (one
 * scratch word per anchor; round 1 is the identity) and keeps the register scheme of the chain kernel, a lane holding one of the last 64
 * anchors of the LIST.  After a kept round it compacts the list in place, tile by tile (a ballot of the survivors, ranks by popcount).
 * The predecessor table keeps original group-relative indices and a round writes only the entries of anchors still in the list, so -c
 * walks a written chain of any round back from its end anchor exactly as before ((p, qa) is unique in a group: the binary search for the
 * end anchor stays unique).  Chains go to chain[c * chains + r], kept = 0 for a round not run: the stable sort by (read, score) keeps
 * (target, rel, round) on ties.  One lane per read does steps A and B, the accepted chains in LDS.  The list and the further chains
 * count in the chunk budget; a chunk that does not fit is split, never truncated.
 *
 * TKSMSEQ_EINVAL: chains, overlap or segments out of range. */
typedef struct tksmseq_split_params {
    int32_t chains;                  /* --split-chains (4) */
    int32_t overlap;                 /* --split-overlap (30) */
    int32_t segments;                /* --split-segments (8) */
    int32_t reserved;
} tksmseq_split_params;
typedef struct tksmseq_split_info {
    uint64_t split_reads, supplementary, later_chains, rounds, rejected_overlap;
    float split_ms, reserved;        /* by HIP events, all chunks */
} tksmseq_split_info;
/* split NULL: exactly tksmseq_map_extend; align NULL, extend NULL: as there.  align_info, extend_info and split_info may be NULL. */
int tksmseq_map_split(tksmseq_ctx* ctx, const tksmseq_map_params* params, const tksmseq_align_params* align, const tksmseq_extend_params* extend,
                      const tksmseq_split_params* split, const char* reads_paths, const char* paf_out, tksmseq_map_info* info, tksmseq_align_info* align_info,
                      tksmseq_extend_info* extend_info, tksmseq_split_info* split_info);

/* ---- map, annotated targets: map to transcripts spliced from genome + GTF on the device (map -g, --genome-coords, --targets-out) ------------------
 * The mapper above wants a cDNA FASTA as its reference.  A target set is that reference made from what the simulator starts from: the
 * context's reference (the genome) and its transcript table (tksmseq_transcripts_add_gtf).  Target t is by definition the molecule
 * `transcribe` emits for its transcript.  These are this build's rules; no tool of the reference does this.
 *
 * Which transcripts become targets.  The walk goes over the transcript table in table order.  A transcript is skipped and counted when it
 * has no exon or all its exons are empty, start = end (skipped_empty); else when any exon names a contig the context's reference lacks, or
 * one that is declared only (skipped_unknown_contig); else when any exon has end < start or end > its contig's length (skipped_bad_exon).
 * The kept ones are the targets 0 .. n - 1 in table order; the name of a target is the table's id.  transcripts = targets + the three.
 *
 * Letters.  Target t is the concatenation of its exons in FILE order (src/gtf.h:295-301: exons stay in file order, each with its own
 * strand).  A `+` exon gives the contig's letters [start, end), upper-cased; a `-` exon their reverse complement, exon by exon.  This is
 * the sequence `tksm sequence --perfect` writes for the molecule `tksm transcribe` emits for that transcript.  A letter is valid iff the
 * genome letter is one of ACGT; an invalid letter has code 0 and validity bit 0.
 *
 * Image.  The layout is the one the mapper reads: target t starts at validity word voff[t], its code words at 2 voff[t]; 16 letters a code
 * word, letter g in bits 2 (g & 15); 32 letters a validity word, letter g in bit g & 31.  voff[0] = 0, voff[t + 1] = voff[t] +
 * ceil(len[t] / 32), image_vwords = voff[n].  Every bit at or behind len[t] in a target's last words is 0 in both images: no result depends
 * on what recycled device memory held.
 *
 * FASTA.  ">name\n", then the letters decoded from the downloaded image, N for an invalid letter, wrapped at line_width letters (0: one
 * line), every record ends with '\n'.  A path that ends in .gz is compressed by the host's zlib.  The file goes to <path>.tmp and is renamed.
 *
 * Projectable.  A target is projectable when its non-empty exons all lie on one contig with one strand and do not turn back: in file
 * order start[i + 1] >= end[i] for `+`, end[i + 1] <= start[i] for `-`.  Empty exons are ignored.
 *
 * Staleness.  A target set belongs to the context that made it and records that context's reference version (it changes with every contig
 * added or declared) and the serial of the transcript table.  Using it after either has changed is TKSMSEQ_EINVAL.
 *
 * Limits.  2^31 targets, a target of 2^31 letters, or 2^36 letters in all: TKSMSEQ_ELIMIT.  No transcript table, no reference, or no
 * target kept: TKSMSEQ_EINVAL.
 *
 * On the device: the validity of the genome is built as for the mapper (one bit a letter, from the exception blocks); one kernel then
 * builds both images in one pass from the genome's packed image, that validity and the kept exons as tuples (first letter in the genome,
 * letters of the target before it, length and strand): one lane per validity word finds its target and its first exon by binary search
 * and walks the exons until its 32 letters are filled, a `+` exon by a funnel shift of adjacent genome words, a `-` exon from the mirrored
 * words.  The transcripts are not uploaded as text and the host does not splice.  splice_ms: by HIP events, the validity and the splice.
 *
 * Mapping.  tksmseq_map_targets with targets == NULL is exactly tksmseq_map_split.  With a target set, its image, names and lengths take
 * the place of the context's reference in the index, the alignment, the extension and the lines; sketch, seed, chain, select, -c,
 * --extend and --split keep their rules.  Defining property: with genome_coords = 0 the PAF is byte for byte the PAF of tksmseq_map_split
 * on a context whose reference is the FASTA of tksmseq_targets_write_fasta, for every combination of the modes and every chunk_reads.
 *
 * Projection (genome_coords = 1; needs targets, else TKSMSEQ_EINVAL), on the host as the lines are written.
 * Mapping a position: let m be the transcript's strand; transcript position x lies in (non-empty) exon e at offset o; G(x) = start_e + o
 * for `+`, G(x) = end_e - 1 - o for `-`.
 * Which lines: a line with target interval [a, b) on a projectable target is projected; a line on any other target is written unchanged
 * and counted (unprojected); after such a call tksmseq_last_error names the first such transcript, and the module logs that line once.
 * Columns of a projected line: column 5 is `+` iff rel ^ m == 0; column 6 is the contig's name, column 7 its length; columns 8 and 9 are
 * G(a), G(b - 1) + 1 for `+` and G(b - 1), G(a) + 1 for `-`; columns 1 to 4, 10, 11, 12 and the tp cm s1 sn si NM tags are unchanged;
 * tx:Z:<transcript id> is appended as the last tag.
 * CIGAR of a projected line (with -c): the runs are walked in transcript order.  A run that consumes the target (M = X D) is cut at exon
 * ends; immediately before the first target-consuming column of the next exon a run <gap>N is inserted, gap = start_next - end_prev for
 * `+` and start_prev - end_next for `-`; a gap of 0 inserts nothing.  I runs stay where they are: an I at a junction stays with the exon
 * before it in transcript order.  Equal neighbours are then merged, and for a `-` transcript the list is reversed.  The CIGAR then consumes
 * column 9 - column 8 genome letters, N included, and qend - qstart read letters.
 * Counters: lines = projected + unprojected; junctions: the N runs written, or without -c the exon boundaries the projected intervals cross. */
typedef struct tksmseq_targets tksmseq_targets;               /* opaque; belongs to the context that made it */
typedef struct tksmseq_targets_info {
    uint64_t transcripts, targets, letters, exons;            /* table size; targets kept; their letters; their (non-empty) exons */
    uint64_t skipped_empty, skipped_unknown_contig, skipped_bad_exon;
    uint64_t projectable;                                     /* targets that genome_coords can project */
    uint64_t image_vwords;                                    /* validity words of the image (32 letters each) */
    float splice_ms, reserved;                                /* by HIP events */
} tksmseq_targets_info;
int tksmseq_targets_from_transcripts(tksmseq_ctx* ctx, tksmseq_targets** out, tksmseq_targets_info* info /* or NULL */);
/* target t: its name (valid until the set is freed), length, first validity word, and whether it is projectable; any may be NULL */
int tksmseq_targets_get(const tksmseq_targets* targets, uint64_t t, const char** name, uint32_t* len, uint64_t* voff, int32_t* projectable);
int tksmseq_targets_download(tksmseq_ctx* ctx, const tksmseq_targets* targets, uint32_t* codes /* 2 * image_vwords */, uint32_t* valid /* image_vwords */);
int tksmseq_targets_write_fasta(tksmseq_ctx* ctx, const tksmseq_targets* targets, const char* path, int32_t line_width /* 0: one line; the CLI writes 60 */);
void tksmseq_targets_free(tksmseq_ctx* ctx, tksmseq_targets* targets);
typedef struct tksmseq_map_targets_params {
    int32_t genome_coords;           /* --genome-coords */
    int32_t reserved;
} tksmseq_map_targets_params;
typedef struct tksmseq_project_info {
    uint64_t lines, projected, unprojected, junctions;
} tksmseq_project_info;
/* targets NULL: exactly tksmseq_map_split (tp NULL or genome_coords 0).  tp NULL: genome_coords 0.  The info pointers may be NULL. */
int tksmseq_map_targets(tksmseq_ctx* ctx, const tksmseq_targets* targets, const tksmseq_map_targets_params* tp, const tksmseq_map_params* params,
                        const tksmseq_align_params* align, const tksmseq_extend_params* extend, const tksmseq_split_params* split, const char* reads_paths,
                        const char* paf_out, tksmseq_map_info* info, tksmseq_align_info* align_info, tksmseq_extend_info* extend_info, tksmseq_split_info* split_info,
                        tksmseq_project_info* project_info);
/* `tksm map`: -r REF.fa[.gz][,REF2.fa] [-g GTF[,GTF...] [--genome-coords] [--targets-out CDNA.fa[.gz]]] --reads F.fq[.gz][,MORE] -o OUT.paf[.gz] [-k 15] [-w 10] [--max-occ 500] [--max-gap 5000] [--bandwidth 500]
 * [--min-count 3] [--min-score 40] [-p 0.8] [-N 5] [-c [--eqx] [--align-band 63]] [--extend [--ext-band 31] [--ext-drop 40] [--ext-max 2000]]
 * [--split [--split-chains 4] [--split-overlap 30] [--split-segments 8]] [--chunk-reads N] [--devices D] [--verbosity V] [--log-file L].
 * Exit codes as the other model modules: 2 for a missing required option, an unknown option or a value out of range ("map: error: ..."; also
 * --eqx or --align-band without -c, an --ext-* option without --extend, a --split-* option without --split, and --max-gap above 65536 with
 * -c), checked before any device is opened; 1 for everything that fails later.
 * With -g the reference is the genome and the targets are the transcripts of the GTFs (read with skip_non_coding = 0), "map, annotated
 * targets" above; --targets-out writes their FASTA (60 letters a line).  --genome-coords or --targets-out without -g is exit 2.  With -g
 * --targets-out, --reads and -o may both be absent: the FASTA is then the only output; one of the two without the other is exit 2. */
int tksmseq_map_main(int argc, char** argv);

/* The batch as MDF text, the way molecule_descriptor::operator<< writes it (src/interval.h:898-905): "+id<TAB>depth<TAB>comment",
 * then "chr<TAB>start<TAB>end<TAB>strand<TAB>pos<base>,..." per segment; depth 1 per molecule; comments re-serialised key-sorted
 * like dump_comment (:880-890).  *text is malloc'ed: release with tksmseq_text_free. */
int tksmseq_batch_to_mdf_text(tksmseq_ctx* ctx, const tksmseq_batch* b, char** text, uint64_t* len);
void tksmseq_text_free(char* text);

/* The `tksm pcr` and `tksm truncate` modules (PCR_module / Truncate_module: src/pcr.cpp:91-260, src/truncate.cpp:236-451) on
 * top of the functions above: same flags, MDF file in, MDF file out; argv[0] is the module name. */
int tksmseq_pcr_main(int argc, char** argv);
int tksmseq_truncate_main(int argc, char** argv);
/* `tksm polyA`, `tksm tag`, `tksm scb`, `tksm flip` (PolyA_module src/polyA.cpp:17-237, TAG_module src/tag.cpp:16-129, SingleCellBarcoder_module
 * src/scb.cpp:14-92, StrandMan_module src/strand_man.cpp:20-124): the reference's flags and validation messages, MDF file in, MDF file out,
 * streamed in batches of --batch-bytes over --devices like `tksm truncate`. */
int tksmseq_polya_main(int argc, char** argv);
int tksmseq_tag_main(int argc, char** argv);
int tksmseq_scb_main(int argc, char** argv);
int tksmseq_flip_main(int argc, char** argv);
/* `tksm random-wgs` (RWGS_module src/random_wgs.cpp:24-229): -r/--reference, --frag-len-dist "NAME A [B]", -o/--output, --base-count |
 * --depth, the reference's messages and exit codes; the contig table from <reference>.fai (from the FASTA itself when that is missing);
 * MDF text out, streamed in batches of --batch-molecules candidates over --devices. */
int tksmseq_random_wgs_main(int argc, char** argv);
/* `tksm tail-noise` (AppendNoise_module src/append_noise.cpp:131-229): -i, -o, --length-dist NAME,MU,SIGMA, --alphabet, --palindromic,
 * --error-rate with the reference's messages and exit codes; streamed in batches of --batch-bytes over --devices like `tksm polyA`. */
int tksmseq_tail_noise_main(int argc, char** argv);
int tksmseq_sequence_main(int argc, char** argv);

#ifdef __cplusplus
}
#endif
#endif
