// tool_modules.cpp -- the modules that read files and write files, no MDF on either side, one context on the first entry of --devices:
//   model-truncation        py/truncate_kde.py:36-112, :323-352 (behind src/model_truncation.cpp) PAF in, KDE model JSON out
//   abundance               py/transcript_abundance.py:32-139, :326-389 (behind src/abundance.cpp) PAF in, expression TSV out
//   model-sequence          the model_sequence rule (Snakefile:507-546: badread error_model + qscore_model) reference, FASTQ and PAF in, two model files out
//   barcode-match           the three scTagger rules (Snakefile, "Preprocessing rules") FASTQ and whitelist in, lr_matches.tsv out
//   map                     the two minimap2 rules (Snakefile: minimap_cdna, minimap_cdna_for_badread_models) reference and FASTQ in, PAF out
// The argument loop, the common flags and the log are those of the MDF modules (module_cli.h, defined in mdf_modules.cpp).  Exit codes: 2 for a
// missing required option, an unknown option or a value out of range, all before any device is opened; 1 for everything that fails later.
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../include/tksmseq.h"
#include "abund_host.h"
#include "kde_host.h"
#include "module_cli.h"

using namespace tkmod;

namespace {

using Clock = std::chrono::steady_clock;
double seconds_since(Clock::time_point t0) { return std::chrono::duration<double>(Clock::now() - t0).count(); }

bool integer(const char* v, long long& out) { char* e = nullptr; out = strtoll(v, &e, 10); return e != v && !*e; }
bool real(const char* v, double& out) { char* e = nullptr; out = strtod(v, &e); return e != v && !*e; }

// An integer option with a stated range.  check(): false when v is no integer; a value outside [lo, hi] is remembered (the first one only: it is
// reported once the required arguments are known to be there).  iv comes back within [-1, clamp] so that it fits its field: that changes a value only when it is out of range, and then the tool exits with 2
struct Ranges {
    std::string error;
    bool check(const std::string& o, const char* v, long long lo, long long hi, const char* what, long long& iv, long long clamp = 0x7FFFFFFFll) {
        if (!integer(v, iv)) return false;
        if ((iv < lo || iv > hi) && error.empty()) error = o + " " + what;
        iv = std::max(-1ll, std::min(iv, clamp));
        return true;
    }
};

// the common flags a tool does not have: without MDF batches, and without -i and -s
const std::vector<std::string> NO_BATCHES{"--batch-bytes", "--slice-molecules"}, NO_INPUT_SEED{"-i", "--input", "-s", "--seed", "--batch-bytes", "--slice-molecules"};
bool among(const std::string& o, const std::vector<std::string>& set) { return std::find(set.begin(), set.end(), o) != set.end(); }

struct Need { const std::string& value; const char* flag; };
// false, with argparse's line, when a value is empty
bool have_required(const char* tool, std::initializer_list<Need> needs) {
    std::string missing;
    for (const Need& n : needs) if (n.value.empty()) missing += (missing.empty() ? "" : ", ") + std::string(n.flag);
    if (!missing.empty()) fprintf(stderr, "%s: error: the following arguments are required: %s\n", tool, missing.c_str());
    return missing.empty();
}

// every FASTA of a comma-separated list into the context's reference
int load_references(tksmseq_ctx* ctx, const std::string& list, Logger& log) {
    int rc = 0;
    for (size_t a = 0; a <= list.size() && !rc;) {
        size_t b = list.find(',', a);
        if (b == std::string::npos) b = list.size();
        if (b > a) {
            log.log(Logger::INFO, "Reading %s", list.substr(a, b - a).c_str());
            rc = tksmseq_reference_add_fasta(ctx, list.substr(a, b - a).c_str());
        }
        a = b + 1;
    }
    return rc;
}

// one context on the first device around call(ctx); then the context's error on stderr, or report(t0): the tool's log lines (non-zero: it failed itself and has said why)
template <class Call, class Report>
int with_context(const Common& c, Call call, Report report) {
    tksmseq_ctx* ctx = nullptr;
    if (tksmseq_create(c.devices[0], &ctx)) { fprintf(stderr, "Error: %s\n", tksmseq_last_error(nullptr)); return 1; }
    const auto t0 = Clock::now();
    int rc = call(ctx);
    if (rc) fprintf(stderr, "Error: %s\n", tksmseq_last_error(ctx));
    else rc = report(t0);
    fflush(stdout);
    tksmseq_destroy(ctx);
    return rc ? 1 : 0;
}

}  // namespace

// `tksm model-truncation`: the reference runs py/truncate_kde.py (argparse: a missing -i / -o and an unknown option exit with 2; --list
// prints the option names and exits before anything is required).
extern "C" int tksmseq_model_truncation_main(int argc, char** argv) {
    Common c;
    tksmseq_kde_model_params p{};
    p.bandwidth = 100.0; p.grid_start = 0; p.grid_end = 10000; p.grid_step = 100; p.end_ratio = -1.0; p.cv_samples = 100000;
    bool list = false;
    if (!parse_args(argc, argv, c, [&](const std::string& o, const char* v) -> int {
            if (among(o, NO_BATCHES)) return NO_SUCH;
            if (o == "--list") { list = true; return TOOK_FLAG; }
            if (o == "--model-lengths") { p.model_lengths = 1; return TOOK_FLAG; }
            long long iv = 0;
            if ((o == "-b" || o == "--bandwidth") && v) { if (!real(v, p.bandwidth)) return MALFORMED; }
            else if (o == "--end-ratio" && v) { if (!real(v, p.end_ratio)) return MALFORMED; }
            else if (o == "--grid-start" && v) { if (!integer(v, iv)) return MALFORMED; p.grid_start = iv; }
            else if (o == "--grid-end" && v) { if (!integer(v, iv)) return MALFORMED; p.grid_end = iv; }
            else if (o == "--grid-step" && v) { if (!integer(v, iv)) return MALFORMED; p.grid_step = iv; }
            else if (o == "--cv-samples" && v) { if (!integer(v, iv) || iv < 3) return MALFORMED; p.cv_samples = (uint64_t)iv; }
            else if ((o == "-t" || o == "--threads") && v) { if (!integer(v, iv)) return MALFORMED; }      // accepted, ignored: the device does the work
            else return NOT_MINE;
            return TOOK_VALUE;
        })) return 2;
    if (list) { printf("help\ninput\noutput\nbandwidth\ngrid_start\ngrid_end\ngrid_step\nthreads\nmodel_lengths\nlist\nend_ratio\nseed\ncv_samples\ndevices\nverbosity\nlog_file\n"); return 0; }
    if (c.help) { printf("KDE computation module of truncation of transcriptomic long-reads using their cDNA mapping.\n"
                         "usage: model-truncation -i INPUT.paf -o OUTPUT.json [-b BANDWIDTH] [--grid-start 0] [--grid-end 10000] [--grid-step 100] [--model-lengths]\n"
                         "                        [--end-ratio R] [-t THREADS] [--list] [-s SEED] [--cv-samples 100000] [--devices D] [--verbosity L] [--log-file F]\n"
                         "BANDWIDTH <= 0: chosen by 3-fold cross-validation over 50, 150, ..., 950 on --cv-samples draws (seeded by -s)\n"); return 0; }
    if (!have_required("model-truncation", {{c.input, "-i/--input"}, {c.output, "-o/--output"}})) return 2;
    if (p.end_ratio != -1.0 && !(p.end_ratio >= 0.0 && p.end_ratio <= 1.0)) { fprintf(stderr, "Error: --end-ratio must be -1 or between 0 and 1\n"); return 1; }
    Logger log;
    if (!open_log(c, "model-truncation", log)) return 1;
    p.seed = (uint64_t)c.seed;
    log.log(Logger::INFO, "Reading %s", c.input.c_str());
    log.log(Logger::INFO, p.model_lengths ? "Modelling read lengths" : "Modelling truncation lengths");
    tkh::KdeBuildInfo info;
    return with_context(c, [&](tksmseq_ctx* ctx) { return tkh::kde_build_model(ctx, &p, c.input.c_str(), c.output.c_str(), &info); }, [&](Clock::time_point t0) {
        if (info.searched) {
            log.log(Logger::INFO, "Non-positive bandwidth selected: recomputed by 3-fold cross-validation on %llu draws (seed %lld)", (unsigned long long)p.cv_samples, c.seed);
            for (int r = 0; r < 3; r++) {
                int arg = 0;
                for (int k = 1; k < 10; k++) if (info.scores[10 * r + k] > info.scores[10 * r + arg]) arg = k;
                log.log(Logger::DEBUG, "repeat %d: bandwidth %d (mean score %.17g)", r, 50 + 100 * arg, info.scores[10 * r + arg]);
            }
        }
        log.log(Logger::INFO, "bandwidth: %.17g", info.bandwidth);
        log.log(Logger::INFO, "model-truncation: %llu primary alignments, %llu end ratios, model written to %s in %.2f s", (unsigned long long)info.n_pairs,
                (unsigned long long)info.n_ratios, c.output.c_str(), seconds_since(t0));
        return 0;
    });
}

// `tksm abundance`: the reference runs py/transcript_abundance.py (argparse: a missing -p / -o, an unknown option and a failed check of
// parse_args :121-138 exit with 2 and "abundance: error: ..."; --list prints the option names and exits before anything is required).
// Stdout carries the script's progress lines (no progress bars).
extern "C" int tksmseq_abundance_main(int argc, char** argv) {
    Common c;
    tksmseq_abundance_params p{};
    p.seed = 42; p.em_iterations = 10; p.cb_dropout = 0.2; p.cb_mu = 10.0; p.cb_sigma = 1.0;
    std::string paf, lr_br, pattern = "NNNNNNNNNNNN", txt, lognorm = "10,1";
    long long verbose = 0;
    bool list = false;
    if (!parse_args(argc, argv, c, [&](const std::string& o, const char* v) -> int {
            if (among(o, NO_INPUT_SEED)) return NO_SUCH;
            if (o == "--list") { list = true; return TOOK_FLAG; }
            long long iv = 0;
            if ((o == "-p" || o == "--paf") && v) paf = v;
            else if ((o == "-m" || o == "--lr-br") && v) lr_br = v;
            else if (o == "--cb-count" && v) { if (!integer(v, iv)) return MALFORMED; p.cb_count = iv; }
            else if (o == "--cb-lognorm-params" && v) lognorm = v;
            else if (o == "--cb-pattern" && v) pattern = v;
            else if (o == "--cb-dropout" && v) { if (!real(v, p.cb_dropout)) return MALFORMED; }
            else if (o == "--cb-txt" && v) txt = v;
            else if ((o == "-em" || o == "--em-iterations") && v) { if (!integer(v, iv) || iv < -2147483648ll || iv > 2147483647ll) return MALFORMED; p.em_iterations = (int32_t)iv; }
            else if (o == "--random-seed" && v) { if (!integer(v, iv)) return MALFORMED; p.seed = (uint64_t)iv; }
            else if ((o == "-v" || o == "--verbose") && v) { if (!integer(v, verbose)) return MALFORMED; }
            else return NOT_MINE;
            return TOOK_VALUE;
        })) return 2;
    if (list) { printf("help\npaf\nlr_br\ncb_count\ncb_lognorm_params\ncb_pattern\ncb_dropout\ncb_txt\noutput\nem_iterations\nrandom_seed\nverbose\nlist\ndevices\nverbosity\nlog_file\n"); return 0; }
    if (c.help) { printf("Output a TSV file of the long-read trasncript expresion.\n"
                         "usage: abundance -p PAF -o OUTPUT[.gz] [-m LR_BR] [--cb-count N] [--cb-lognorm-params MEAN,SD] [--cb-pattern NNNNNNNNNNNN] [--cb-dropout 0.2]\n"
                         "                 [--cb-txt WHITELIST] [-em 10] [--random-seed 42] [-v 0] [--list] [--devices D] [--verbosity L] [--log-file F]\n"
                         "--cb-count N > 0 splits the abundance over N simulated cell barcodes (seeded draws: include/tksmseq.h); not with --lr-br\n"); return 0; }
    if (!have_required("abundance", {{paf, "-p/--paf"}, {c.output, "-o/--output"}})) return 2;
    if (p.cb_count > 0) {
        const size_t comma = lognorm.find(',');
        const bool two = comma != std::string::npos && lognorm.find(',', comma + 1) == std::string::npos;
        if (!two || !real(lognorm.substr(0, comma).c_str(), p.cb_mu) || !real(lognorm.substr(comma + 1).c_str(), p.cb_sigma)) {
            fprintf(stderr, "abundance: error: --cb-lognorm-params takes two comma-separated values: mean and standard deviation\n");
            return 2;
        }
        std::string why;
        if (!tkh::abund_check_args(p.cb_count, lr_br.c_str(), pattern.c_str(), txt.c_str(), p.cb_dropout, p.cb_mu, p.cb_sigma, why)) {
            fprintf(stderr, "abundance: error: %s\n", why.c_str());
            return 2;
        }
    }
    Logger log;
    if (!open_log(c, "abundance", log)) return 1;
    p.cb_pattern = pattern.c_str(); p.cb_txt_path = txt.c_str(); p.lr_br_path = lr_br.c_str();
    tksmseq_abundance_result* res = nullptr;
    return with_context(c, [&](tksmseq_ctx* ctx) {
        if (!lr_br.empty() && p.cb_count <= 0) printf("Parsing LR barcode matches TSV...\n");
        printf("Parsing PAF file...\n");
        fflush(stdout);
        return tksmseq_abundance(ctx, &p, paf.c_str(), &res);
    }, [&](Clock::time_point t0) {
        uint64_t rows = 0, surviving = 0, reads = 0, transcripts = 0, hits = 0;
        float ms = 0.f;
        tksmseq_abundance_info(res, &rows, &surviving, &reads, &transcripts, &hits);
        tksmseq_abundance_device_ms(res, &ms);
        // (one library call does the three steps: their lines follow it, so a PAF that does not parse shows none of them)
        printf("Computing compatibility of different alignments for each read...\nRunning EM...\nParsed alignments for %llu reads\n", (unsigned long long)surviving);
        const int rc = tksmseq_abundance_write(res, c.output.c_str());
        if (rc) fprintf(stderr, "Error: cannot write %s\n", c.output.c_str());
        else
            log.log(Logger::INFO, "abundance: %llu reads (%llu kept, %llu hits) on %llu transcripts, %llu rows written to %s in %.2f s (device %.2f ms)",
                    (unsigned long long)reads, (unsigned long long)surviving, (unsigned long long)hits, (unsigned long long)transcripts, (unsigned long long)rows,
                    c.output.c_str(), seconds_since(t0), ms);
        tksmseq_abundance_free(res);
        return rc;
    });
}

// `tksm model-sequence`: the model_sequence rule of the reference's workflow (Snakefile:507-546) runs `badread error_model` and `badread
// qscore_model`; this module builds both files in one pass (include/tksmseq.h).
extern "C" int tksmseq_model_sequence_main(int argc, char** argv) {
    Common c;
    tksmseq_model_sequence_params p{};
    p.error_k = 7; p.qscore_k = 9; p.max_alt = 25; p.max_del = 6; p.min_occur = 100; p.max_output = 10000;
    std::string reference, reads, paf, error_out, qscore_out;
    Ranges ranges;
    if (!parse_args(argc, argv, c, [&](const std::string& o, const char* v) -> int {
            if (among(o, NO_INPUT_SEED) || o == "-o" || o == "--output") return NO_SUCH;
            long long iv = 0;
            constexpr long long MAX64 = 0x7FFFFFFFFFFFFFFFll;
            if ((o == "-r" || o == "--reference") && v) reference = v;
            else if (o == "--reads" && v) reads = v;
            else if (o == "--alignment" && v) paf = v;
            else if (o == "--error-model" && v) error_out = v;
            else if (o == "--qscore-model" && v) qscore_out = v;
            else if (o == "--error-k" && v) { if (!ranges.check(o, v, 3, 8, "must be between 3 and 8", iv, 99)) return MALFORMED; p.error_k = (int32_t)iv; }
            else if (o == "--qscore-k" && v) {
                if (!ranges.check(o, v, 1, 29, "must be odd and between 1 and 29", iv, 99)) return MALFORMED;
                if (iv % 2 == 0 && ranges.error.empty()) ranges.error = o + " must be odd and between 1 and 29";
                p.qscore_k = (int32_t)iv;
            }
            else if (o == "--max_alignments" && v) { if (!ranges.check(o, v, 0, MAX64, "must not be negative", iv, MAX64)) return MALFORMED; p.max_alignments = iv; }
            else if (o == "--max_alt" && v) { if (!ranges.check(o, v, 0, 31, "must be between 0 and 31", iv, 99)) return MALFORMED; p.max_alt = (int32_t)iv; }
            else if (o == "--max_del" && v) { if (!ranges.check(o, v, 0, 1 << 20, "must be between 0 and 1048576", iv, 1ll << 20)) return MALFORMED; p.max_del = (int32_t)iv; }
            else if (o == "--min_occur" && v) { if (!ranges.check(o, v, 0, MAX64, "must not be negative", iv, MAX64)) return MALFORMED; p.min_occur = iv; }
            else if (o == "--max_output" && v) { if (!ranges.check(o, v, 0, 0x7FFFFFFEll, "must be between 0 and 2147483646", iv, MAX64)) return MALFORMED; p.max_output = iv; }
            else return NOT_MINE;
            return TOOK_VALUE;
        })) return 2;
    if (c.help) { printf("Builds the Badread error model and q-score model of `tksm sequence` from reads aligned to a reference.\n"
                         "usage: model-sequence --reference R[,R] --reads F[,F] --alignment PAF [--error-model OUT] [--qscore-model OUT] [--error-k 7] [--qscore-k 9]\n"
                         "                      [--max_alignments 0] [--max_alt 25] [--max_del 6] [--min_occur 100] [--max_output 10000] [--devices D] [--verbosity V]\n"
                         "                      [--log-file L]\n"
                         "PAF: `tksm map -c` or minimap2 -c output (cg:Z: tags); FASTQ and model files may be .gz; at least one of --error-model, --qscore-model\n"); return 0; }
    if (!have_required("model-sequence", {{reference, "--reference"}, {reads, "--reads"}, {paf, "--alignment"}})) return 2;
    if (error_out.empty() && qscore_out.empty()) { fprintf(stderr, "model-sequence: error: at least one of --error-model and --qscore-model is required\n"); return 2; }
    if (!ranges.error.empty()) { fprintf(stderr, "model-sequence: error: %s\n", ranges.error.c_str()); return 2; }
    Logger log;
    if (!open_log(c, "model-sequence", log)) return 1;
    tksmseq_model_sequence_info info{};
    return with_context(c, [&](tksmseq_ctx* ctx) {
        if (int rc = load_references(ctx, reference, log)) return rc;
        return tksmseq_model_sequence(ctx, &p, reads.c_str(), paf.c_str(), error_out.empty() ? nullptr : error_out.c_str(), qscore_out.empty() ? nullptr : qscore_out.c_str(), &info);
    }, [&](Clock::time_point t0) {
        log.log(Logger::INFO, "model-sequence: %llu PAF lines, %llu used (skipped: %llu without cg:Z:, %llu tp:A:S, %llu unknown reads, %llu unknown targets, %llu other CIGAR ops)",
                (unsigned long long)info.lines, (unsigned long long)info.used, (unsigned long long)info.skipped_no_cigar, (unsigned long long)info.skipped_supplementary,
                (unsigned long long)info.skipped_unknown_read, (unsigned long long)info.skipped_unknown_target, (unsigned long long)info.skipped_cigar_op);
        log.log(Logger::INFO, "model-sequence: %llu counting positions (%llu alternatives too long), %llu read positions (%llu windows over --max_del, %llu keys too long), "
                "%llu + %llu distinct keys", (unsigned long long)info.counting_positions, (unsigned long long)info.alternatives_too_long, (unsigned long long)info.read_positions,
                (unsigned long long)info.windows_max_del, (unsigned long long)info.keys_too_long, (unsigned long long)info.error_keys, (unsigned long long)info.qscore_keys);
        log.log(Logger::INFO, "model-sequence: %llu events in %llu chunks, written in %.2f s (device %.2f ms)", (unsigned long long)info.events,
                (unsigned long long)info.chunks, seconds_since(t0), info.device_ms);
        return 0;
    });
}

// `tksm barcode-match`: the three scTagger rules of the reference's single-cell route (Snakefile, "Preprocessing rules") in one call: FASTQ
// reads and a barcode whitelist in, the lr_matches.tsv of `tksm abundance --lr-br` out (include/tksmseq.h).
extern "C" int tksmseq_barcode_match_main(int argc, char** argv) {
    Common c;
    tksmseq_barcode_match_params p{};
    p.window = 200; p.max_adapter_errors = 5; p.pad = 4; p.max_errors = 2; p.min_exact = 2;
    std::string reads, whitelist, adapter = "CTACACGACGCTCTTCCGATCT", segments_out, selected_out;
    Ranges ranges;
    if (!parse_args(argc, argv, c, [&](const std::string& o, const char* v) -> int {
            if (among(o, NO_INPUT_SEED)) return NO_SUCH;
            long long iv = 0;
            if (o == "--revcomp-barcodes") { p.revcomp_barcodes = 1; return TOOK_FLAG; }
            if (o == "--reads" && v) reads = v;
            else if (o == "--whitelist" && v) whitelist = v;
            else if (o == "--adapter" && v) adapter = v;
            else if (o == "--segments-out" && v) segments_out = v;
            else if (o == "--selected-out" && v) selected_out = v;
            else if (o == "--window" && v) { if (!ranges.check(o, v, 4, 0x7FFFFFFF, "must be between the adapter's length and 2147483647", iv)) return MALFORMED; p.window = (int32_t)iv; }
            else if (o == "--max-adapter-errors" && v) { if (!ranges.check(o, v, 0, 31, "must be between 0 and the adapter's length - 1", iv)) return MALFORMED; p.max_adapter_errors = (int32_t)iv; }
            else if (o == "--pad" && v) { if (!ranges.check(o, v, 0, 16, "must be between 0 and 16", iv)) return MALFORMED; p.pad = (int32_t)iv; }
            else if (o == "--max-errors" && v) { if (!ranges.check(o, v, 0, 31, "must be between 0 and the barcodes' length - 1", iv)) return MALFORMED; p.max_errors = (int32_t)iv; }
            else if (o == "--min-exact" && v) { if (!ranges.check(o, v, 0, 0x7FFFFFFF, "must be between 0 and 2147483647", iv)) return MALFORMED; p.min_exact = iv; }
            else if (o == "--chunk-reads" && v) { if (!ranges.check(o, v, 0, 0x7FFFFFFF, "must be between 0 and 2147483647", iv)) return MALFORMED; p.chunk_reads = (uint64_t)std::max(0ll, iv); }
            else return NOT_MINE;
            return TOOK_VALUE;
        })) return 2;
    if (c.help) { printf("Assigns long reads to cell barcodes: finds the adapter at either end of a read and matches the bases behind it to a whitelist.\n"
                         "usage: barcode-match --reads F[,F...] --whitelist W -o LR_MATCHES.tsv[.gz] [--adapter CTACACGACGCTCTTCCGATCT] [--window 200]\n"
                         "                     [--max-adapter-errors 5] [--pad 4] [--max-errors 2] [--min-exact 2] [--revcomp-barcodes] [--segments-out F]\n"
                         "                     [--selected-out F] [--chunk-reads N] [--devices D] [--verbosity V] [--log-file L]\n"
                         "FASTQ, whitelist and outputs may be .gz; the output is the file `tksm abundance --lr-br` reads\n"); return 0; }
    if (!have_required("barcode-match", {{reads, "--reads"}, {whitelist, "--whitelist"}, {c.output, "-o/--output"}})) return 2;
    if (ranges.error.empty()) {
        bool acgt = adapter.size() >= 4 && adapter.size() <= 32;
        for (char ch : adapter) acgt = acgt && (ch == 'A' || ch == 'C' || ch == 'G' || ch == 'T');
        if (!acgt) ranges.error = "--adapter must have 4 to 32 letters of ACGT";
        else if (p.window < (int32_t)adapter.size()) ranges.error = "--window must be between the adapter's length and 2147483647";
        else if (p.max_adapter_errors >= (int32_t)adapter.size()) ranges.error = "--max-adapter-errors must be between 0 and the adapter's length - 1";
    }
    if (!ranges.error.empty()) { fprintf(stderr, "barcode-match: error: %s\n", ranges.error.c_str()); return 2; }
    Logger log;
    if (!open_log(c, "barcode-match", log)) return 1;
    tksmseq_barcode_match_info info{};
    return with_context(c, [&](tksmseq_ctx* ctx) {
        p.adapter = adapter.c_str();
        p.segments_out = segments_out.empty() ? nullptr : segments_out.c_str();
        p.selected_out = selected_out.empty() ? nullptr : selected_out.c_str();
        return tksmseq_barcode_match(ctx, &p, reads.c_str(), whitelist.c_str(), c.output.c_str(), &info);
    }, [&](Clock::time_point t0) {
        log.log(Logger::INFO, "barcode-match: %llu reads: %llu without adapter, %llu forward, %llu reverse", (unsigned long long)info.reads, (unsigned long long)info.no_adapter,
                (unsigned long long)info.forward, (unsigned long long)info.reverse);
        log.log(Logger::INFO, "barcode-match: %llu of %llu barcodes are candidates; %llu reads with one barcode, %llu with several, %llu with none",
                (unsigned long long)info.candidates, (unsigned long long)info.whitelist, (unsigned long long)info.unique, (unsigned long long)info.ambiguous,
                (unsigned long long)info.no_barcode);
        log.log(Logger::INFO, "barcode-match: %llu pairs in %llu chunks, written to %s in %.2f s (device %.2f ms)", (unsigned long long)info.pairs,
                (unsigned long long)info.chunks, c.output.c_str(), seconds_since(t0), info.device_ms);
        return 0;
    });
}

// `tksm map`: the two minimap2 rules of the reference's workflow (Snakefile: minimap_cdna, minimap_cdna_for_badread_models), -c included: FASTQ
// reads and a cDNA FASTA in, the PAF of `tksm abundance -p` and `tksm model-truncation -i` out (include/tksmseq.h).
extern "C" int tksmseq_map_main(int argc, char** argv) {
    Common c;
    tksmseq_map_params p{};
    p.k = 15; p.w = 10; p.max_occ = 500; p.max_gap = 5000; p.bandwidth = 500; p.min_count = 3; p.min_score = 40; p.secondary_ratio = 0.8; p.max_secondary = 5;
    tksmseq_align_params ap{63, 0};
    tksmseq_extend_params xp{31, 40, 2000, 0};
    tksmseq_split_params sp{4, 30, 8, 0};
    bool align = false, band_given = false, extend = false, split = false;
    std::string ext_given, split_given;                         // the first --ext-* and the first --split-* option seen
    std::string reference, reads, gtfs, targets_out;
    bool genome_coords = false;
    Ranges ranges;
    if (!parse_args(argc, argv, c, [&](const std::string& o, const char* v) -> int {
            if (among(o, NO_INPUT_SEED)) return NO_SUCH;
            if (o == "-c") { align = true; return TOOK_FLAG; }
            if (o == "--genome-coords") { genome_coords = true; return TOOK_FLAG; }
            if (o == "--eqx") { ap.eqx = 1; return TOOK_FLAG; }
            if (o == "--extend") { extend = true; return TOOK_FLAG; }
            if (o == "--split") { split = true; return TOOK_FLAG; }
            long long iv = 0;
            if ((o == "-r" || o == "--reference") && v) reference = v;
            else if (o == "--reads" && v) reads = v;
            else if ((o == "-g" || o == "--gtf") && v) gtfs = v;
            else if (o == "--targets-out" && v) targets_out = v;
            else if (o == "--align-band" && v) { if (!ranges.check(o, v, 1, 63, "must be between 1 and 63", iv)) return MALFORMED; ap.band = (int32_t)iv; band_given = true; }
            else if (o == "--ext-band" && v) { if (!ranges.check(o, v, 1, 63, "must be between 1 and 63", iv)) return MALFORMED; xp.band = (int32_t)iv; if (ext_given.empty()) ext_given = o; }
            else if (o == "--ext-drop" && v) { if (!ranges.check(o, v, 1, 1000, "must be between 1 and 1000", iv)) return MALFORMED; xp.drop = (int32_t)iv; if (ext_given.empty()) ext_given = o; }
            else if (o == "--ext-max" && v) { if (!ranges.check(o, v, 1, 32768, "must be between 1 and 32768", iv)) return MALFORMED; xp.max_ext = (int32_t)iv; if (ext_given.empty()) ext_given = o; }
            else if (o == "--split-chains" && v) { if (!ranges.check(o, v, 1, 16, "must be between 1 and 16", iv)) return MALFORMED; sp.chains = (int32_t)iv; if (split_given.empty()) split_given = o; }
            else if (o == "--split-overlap" && v) { if (!ranges.check(o, v, 0, 0x7FFFFFFF, "must be between 0 and 2147483647", iv)) return MALFORMED; sp.overlap = (int32_t)iv; if (split_given.empty()) split_given = o; }
            else if (o == "--split-segments" && v) { if (!ranges.check(o, v, 2, 64, "must be between 2 and 64", iv)) return MALFORMED; sp.segments = (int32_t)iv; if (split_given.empty()) split_given = o; }
            else if (o == "-k" && v) { if (!ranges.check(o, v, 4, 28, "must be between 4 and 28", iv)) return MALFORMED; p.k = (int32_t)iv; }
            else if (o == "-w" && v) { if (!ranges.check(o, v, 1, 64, "must be between 1 and 64", iv)) return MALFORMED; p.w = (int32_t)iv; }
            else if (o == "--max-occ" && v) { if (!ranges.check(o, v, 1, 0x7FFFFFFF, "must be between 1 and 2147483647", iv)) return MALFORMED; p.max_occ = (int32_t)iv; }
            else if (o == "--max-gap" && v) { if (!ranges.check(o, v, 0, 0x7FFFFFFF, "must be between 0 and 2147483647", iv)) return MALFORMED; p.max_gap = (int32_t)iv; }
            else if (o == "--bandwidth" && v) { if (!ranges.check(o, v, 0, 0x7FFFFFFF, "must be between 0 and 2147483647", iv)) return MALFORMED; p.bandwidth = (int32_t)iv; }
            else if (o == "--min-count" && v) { if (!ranges.check(o, v, 1, 0x7FFFFFFF, "must be between 1 and 2147483647", iv)) return MALFORMED; p.min_count = (int32_t)iv; }
            else if (o == "--min-score" && v) { if (!ranges.check(o, v, 0, 0x7FFFFFFF, "must be between 0 and 2147483647", iv)) return MALFORMED; p.min_score = (int32_t)iv; }
            else if (o == "-N" && v) { if (!ranges.check(o, v, 0, 1000, "must be between 0 and 1000", iv)) return MALFORMED; p.max_secondary = (int32_t)iv; }
            else if (o == "--chunk-reads" && v) { if (!ranges.check(o, v, 0, 0x7FFFFFFF, "must be between 0 and 2147483647", iv)) return MALFORMED; p.chunk_reads = (uint64_t)std::max(0ll, iv); }
            else if (o == "-p" && v) {
                if (!real(v, p.secondary_ratio)) return MALFORMED;
                if (!(p.secondary_ratio >= 0.0 && p.secondary_ratio <= 1.0) && ranges.error.empty()) ranges.error = o + " must be between 0 and 1";
            }
            else return NOT_MINE;
            return TOOK_VALUE;
        })) return 2;
    if (c.help) { printf("Maps long reads to transcripts by chains of minimizers; with -c the written chains are aligned base by base (cg:Z: and NM:i: tags);\n"
                         "with --extend both ends of every line are extended to where an X-drop alignment carries them; with --split every further piece of a\n"
                         "chimeric or hairpin read gets a supplementary tp:A:P line (sn:i: and si:i: tags).  With -g the reference is the genome and the reads\n"
                         "are mapped to the transcripts of the GTFs, spliced on the device; --targets-out writes them as a FASTA, --genome-coords writes the\n"
                         "lines in genome coordinates (N runs in cg:Z:, tx:Z: tag).\n"
                         "usage: map -r REF.fa[.gz][,REF2.fa] [-g GTF[,GTF...] [--genome-coords] [--targets-out CDNA.fa[.gz]]] --reads F.fq[.gz][,MORE] -o OUT.paf[.gz] [-k 15] [-w 10] [--max-occ 500] [--max-gap 5000] [--bandwidth 500]\n"
                         "           [--min-count 3] [--min-score 40] [-p 0.8] [-N 5] [-c [--eqx] [--align-band 63]] [--extend [--ext-band 31] [--ext-drop 40] [--ext-max 2000]]\n"
                         "           [--split [--split-chains 4] [--split-overlap 30] [--split-segments 8]] [--chunk-reads N] [--devices D] [--verbosity V] [--log-file L]\n"
                         "the output is the file `tksm abundance -p` and `tksm model-truncation -i` read; with -c also the one `tksm model-sequence --alignment` reads\n"); return 0; }
    // with -g --targets-out the FASTA may be the only output
    const bool fasta_only = !gtfs.empty() && !targets_out.empty() && reads.empty() && c.output.empty();
    if (fasta_only ? !have_required("map", {{reference, "-r/--reference"}}) : !have_required("map", {{reference, "-r/--reference"}, {reads, "--reads"}, {c.output, "-o/--output"}}))
        return 2;
    if (gtfs.empty() && (genome_coords || !targets_out.empty())) { fprintf(stderr, "map: error: %s needs -g\n", genome_coords ? "--genome-coords" : "--targets-out"); return 2; }
    if (fasta_only && genome_coords) { fprintf(stderr, "map: error: --genome-coords needs --reads and -o\n"); return 2; }
    if (!ranges.error.empty()) { fprintf(stderr, "map: error: %s\n", ranges.error.c_str()); return 2; }
    if (!align && (ap.eqx || band_given)) { fprintf(stderr, "map: error: %s needs -c\n", ap.eqx ? "--eqx" : "--align-band"); return 2; }
    if (!extend && !ext_given.empty()) { fprintf(stderr, "map: error: %s needs --extend\n", ext_given.c_str()); return 2; }
    if (!split && !split_given.empty()) { fprintf(stderr, "map: error: %s needs --split\n", split_given.c_str()); return 2; }
    if (align && p.max_gap > 65536) { fprintf(stderr, "map: error: --max-gap must be at most 65536 with -c\n"); return 2; }
    Logger log;
    if (!open_log(c, "map", log)) return 1;
    tksmseq_map_info info{};
    tksmseq_align_info ainfo{};
    tksmseq_extend_info xinfo{};
    tksmseq_split_info sinfo{};
    tksmseq_targets_info tinfo{};
    tksmseq_project_info pinfo{};
    std::string unprojected_note;
    return with_context(c, [&](tksmseq_ctx* ctx) {
        if (int rc = load_references(ctx, reference, log)) return rc;
        if (gtfs.empty())
            return tksmseq_map_split(ctx, &p, align ? &ap : nullptr, extend ? &xp : nullptr, split ? &sp : nullptr, reads.c_str(), c.output.c_str(), &info, &ainfo, &xinfo, &sinfo);
        for (size_t a = 0; a <= gtfs.size();) {
            size_t b = gtfs.find(',', a);
            if (b == std::string::npos) b = gtfs.size();
            if (b > a) {
                log.log(Logger::INFO, "Reading %s", gtfs.substr(a, b - a).c_str());
                if (int rc = tksmseq_transcripts_add_gtf(ctx, gtfs.substr(a, b - a).c_str(), 0)) return rc;
            }
            a = b + 1;
        }
        tksmseq_targets* targets = nullptr;
        int rc = tksmseq_targets_from_transcripts(ctx, &targets, &tinfo);
        if (!rc && !targets_out.empty()) rc = tksmseq_targets_write_fasta(ctx, targets, targets_out.c_str(), 60);
        if (!rc && !fasta_only) {
            const tksmseq_map_targets_params tp{genome_coords ? 1 : 0, 0};
            rc = tksmseq_map_targets(ctx, targets, &tp, &p, align ? &ap : nullptr, extend ? &xp : nullptr, split ? &sp : nullptr, reads.c_str(), c.output.c_str(), &info, &ainfo,
                                     &xinfo, &sinfo, &pinfo);
            if (!rc && pinfo.unprojected) unprojected_note = tksmseq_last_error(ctx);
        }
        tksmseq_targets_free(ctx, targets);
        return rc;
    }, [&](Clock::time_point t0) {
        if (!gtfs.empty()) {
            log.log(Logger::INFO, "map: %llu transcripts: %llu targets of %llu letters in %llu exons (%llu projectable); skipped: %llu empty, %llu on unknown contigs, %llu with a bad exon; "
                    "spliced in %.3f ms on the device%s%s",
                    (unsigned long long)tinfo.transcripts, (unsigned long long)tinfo.targets, (unsigned long long)tinfo.letters, (unsigned long long)tinfo.exons,
                    (unsigned long long)tinfo.projectable, (unsigned long long)tinfo.skipped_empty, (unsigned long long)tinfo.skipped_unknown_contig,
                    (unsigned long long)tinfo.skipped_bad_exon, tinfo.splice_ms, targets_out.empty() ? "" : ", written to ", targets_out.c_str());
            if (fasta_only) return 0;
        }
        if (genome_coords) {
            log.log(Logger::INFO, "map: %llu lines: %llu projected to the genome over %llu junctions, %llu left in transcript coordinates", (unsigned long long)pinfo.lines,
                    (unsigned long long)pinfo.projected, (unsigned long long)pinfo.junctions, (unsigned long long)pinfo.unprojected);
            if (!unprojected_note.empty()) log.log(Logger::INFO, "%s", unprojected_note.c_str());
        }
        log.log(Logger::INFO, "map: %llu target minimizers under %llu hashes (%llu over --max-occ); %llu read minimizers, %llu anchors, %llu groups, %llu chained",
                (unsigned long long)info.target_minimizers, (unsigned long long)info.distinct_hashes, (unsigned long long)info.dropped_hashes,
                (unsigned long long)info.read_minimizers, (unsigned long long)info.anchors, (unsigned long long)info.groups, (unsigned long long)info.chained_groups);
        log.log(Logger::INFO, "map: %llu reads: %llu mapped, %llu unmapped; %llu lines (%llu secondary) in %llu chunks, written to %s in %.2f s (device %.2f ms)",
                (unsigned long long)info.reads, (unsigned long long)info.mapped, (unsigned long long)info.unmapped, (unsigned long long)info.lines,
                (unsigned long long)info.secondary, (unsigned long long)info.chunks, c.output.c_str(), seconds_since(t0), info.device_ms);
        if (align)
            log.log(Logger::INFO, "map: %llu lines aligned in %llu segments (the longest spans %llu anti-diagonals), %llu cells: %llu columns, %llu =, %llu X, %llu I, %llu D (device %.2f ms)",
                    (unsigned long long)ainfo.lines, (unsigned long long)ainfo.segments, (unsigned long long)ainfo.longest_segment, (unsigned long long)ainfo.cells,
                    (unsigned long long)ainfo.columns, (unsigned long long)ainfo.matches, (unsigned long long)ainfo.mismatches, (unsigned long long)ainfo.inserted,
                    (unsigned long long)ainfo.deleted, ainfo.align_ms);
        if (extend)
            log.log(Logger::INFO, "map: %llu lines extended, %llu ends moved (the longest by %llu anti-diagonals): %llu target and %llu read letters gained, %llu matches; %llu anti-diagonals, %llu cells (device %.2f ms)",
                    (unsigned long long)xinfo.lines, (unsigned long long)xinfo.ends_moved, (unsigned long long)xinfo.longest, (unsigned long long)xinfo.target_gained,
                    (unsigned long long)xinfo.read_gained, (unsigned long long)xinfo.matches, (unsigned long long)xinfo.antidiagonals, (unsigned long long)xinfo.cells, xinfo.extend_ms);
        if (split) {
            log.log(Logger::INFO, "map: %llu reads split, %llu supplementary lines; %llu rounds, %llu kept chains of later rounds, %llu candidates refused for overlap (device %.2f ms)",
                    (unsigned long long)sinfo.split_reads, (unsigned long long)sinfo.supplementary, (unsigned long long)sinfo.rounds, (unsigned long long)sinfo.later_chains,
                    (unsigned long long)sinfo.rejected_overlap, sinfo.split_ms);
            // every segment of a molecule but the first was glued with probability p
            const unsigned long long J = sinfo.supplementary, M = info.mapped;
            log.log(Logger::INFO, "split: %llu junctions in %llu mapped reads: unsegment -p estimate %.6f", J, M, M + J > 1 ? (double)J / (double)(M + J - 1) : 0.0);
        }
        return 0;
    });
}
