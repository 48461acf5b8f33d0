// sequencer_module.cpp -- the `tksm sequence` module on top of the C-ABI.
//
// Mirrors (file:line into vpc-ccg/tksm):
//   Sequencer_module::impl::run     src/sequence.cpp:30-54   ($TKSM_MODELS handling, then the sequencer)
//   parse_args                      py/sequence.py:34-165    (flags, defaults, validation texts, exit codes)
//   main block                      py/sequence.py:323-376   (load reference + models, stream the MDF, write)
//   get_output_file                 py/sequence.py:291-300   (extension decides FASTQ/FASTA; .gz ok)
//   utility flags                   src/module.h:75-104      (-s/--seed default 42, --verbosity, --log-file)
//   worker pool                     py/sequence.py:354-366   (multiprocessing.Pool + imap_unordered over molecules)
// Streaming: the reader cuts the MDF text into batches of whole molecules and numbers their reads; two parser threads per
// device group (contexts of their own) turn the text into device batches ahead of time; --in-flight worker threads (one
// context each, sharing the packed reference and the model tables) run and download a batch each, so that parsing, the
// device work of consecutive batches, the copies and the writes overlap.  Regular output files are written at their final
// offsets (pwrite, MDF order) by a writer thread per worker, from a device-side copy of the batch's records, while the worker's
// context runs its next batch; pipes and devices by the same writer threads, each in its batch's turn.  A host-compressed .gz
// (--gzip host) is made in the worker's host buffers: a regular file gets its members at their place from the worker itself, and
// when such a .gz is no regular file, every output of the run goes through one writer that takes the batches in MDF order (Route).
// Exit codes: 0 ok; 1 for `sys.exit("msg")`-style validation and runtime errors; 2 for argparse
// usage errors (missing -i, neither -o nor --perfect) -- what the embedded interpreter returns.
#include "sequencer_module.h"

#include <fcntl.h>
#include <poll.h>
#include <sys/stat.h>
#include <unistd.h>
#include <zlib.h>

#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cerrno>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <map>
#include <mutex>
#include <memory>
#include <string>
#include <thread>
#include <vector>

#include "../../include/tksmseq.h"
#include "module_log.h"
#include "module_stream.h"

namespace {

using Clock = std::chrono::steady_clock;
double seconds(Clock::time_point from, Clock::time_point to = Clock::now()) { return std::chrono::duration<double>(to - from).count(); }

struct Args {
    std::string input, badread, perfect, output_format, identity = "84.0,99.0,5.5";
    double mean = 0, maxi = 0, sd = 0;                                   // ... parsed (validate)
    std::string error_model, qscore_model, tail_model = "no_noise";      // "": nanopore2020 if discoverable, else random
    std::vector<std::string> references;
    bool skip_qual = false, list = false, help = false;
    int threads = 1, in_flight = 3;
    std::string gzip = "host";                           // --gzip host|device: where a .gz output is compressed
    std::vector<int> devices{0};
    long long seed = 42;
    uint64_t batch_bytes = 64ull << 20;
    std::string verbosity = "INFO", log_file = "stderr";
    // chained stages (BASELINE config 5): `tksm pcr` and / or `tksm truncate` in front of the sequencer, molecule tables staying on
    // the device -- same results as the three-module route over MDF files with the same -s (src/pcr.cpp:91-260, src/truncate.cpp:236-451)
    bool pcr_on = false, pcr_have_cycles = false, pcr_have_count = false, pcr_have_er = false, pcr_have_ef = false;
    tksmseq_pcr_params pcr{};
    std::string pcr_preset;
    uint64_t pcr_slice = 2000000;
    int trc_n = 0;
    tksmseq_trc_params trc{};
    std::string trc_kde;
    // chained random-wgs (src/random_wgs.cpp:24-229) in place of -i: the molecules are made on the device of the context that sequences them
    bool wgs_on = false, wgs_have_dist = false, wgs_have_bc = false, wgs_have_depth = false;
    std::string wgs_dist;
    long long wgs_base_count = 0; double wgs_depth = 0.0;
    uint64_t wgs_batch = 524288;                           // candidates per batch
    tksmseq_wgs_params wgs{};
    // chained transcribe (src/transcribe.cpp:19-218) in place of -i: the molecules of the abundance tables' rows, made on the device of the
    // context that sequences them.  tsb_texts: the tables themselves, read before any device is opened; tsb_w: every table's weight
    bool tsb_on = false, tsb_have_count = false, tsb_use_whole_id = false;
    std::vector<std::string> tsb_gtfs, tsb_abundances, tsb_texts;
    std::vector<double> tsb_weights, tsb_w;
    long long tsb_count = 0, tsb_default_depth = 0;
    std::string tsb_prefix = "M";
    uint64_t tsb_batch = 524288;                           // molecules per batch
};

void usage(FILE* f) {
    fprintf(f,
            "usage: sequence [-h] -i INPUT [-r REFERENCES [REFERENCES ...]] [-o BADREAD] [--perfect PERFECT]\n"
            "                [--skip-qual-compute] [-O {fastq,fasta}] [-t THREADS] [--badread-identity BADREAD_IDENTITY]\n"
            "                [--badread-error-model M] [--badread-qscore-model M] [--badread-tail-model M] [--list]\n"
            "                [-s SEED] [--devices D[,D...]] [--batch-bytes B] [--in-flight N] [--gzip {host,device}] [--verbosity L]\n"
            "                [--log-file F]\n"
            "                [--pcr-cycles C --pcr-molecule-count N (--pcr-preset X | --pcr-error-rate E --pcr-efficiency F)]\n"
            "                [--truncate-normal MU,SIGMA | --truncate-lognormal MU,SIGMA | --truncate-kde-model M.json\n"
            "                 [--truncate-always-end] [--truncate-kde-models-length]]\n"
            "       sequence -r REFERENCES --wgs-frag-len-dist \"NAME A [B]\" (--wgs-base-count N | --wgs-depth D) [--wgs-batch-molecules M]\n"
            "                (no -i: whole-genome fragments made on the device; the other options as above)\n"
            "       sequence -r REFERENCES --transcribe-gtf G[,G...] --transcribe-abundance A[,A...] --transcribe-molecule-count N\n"
            "                [--transcribe-use-whole-id] [--transcribe-default-depth D] [--transcribe-molecule-prefix P]\n"
            "                [--transcribe-weights W[,W...]] [--transcribe-batch-molecules M]\n"
            "                (no -i: the molecules of `tksm transcribe` made on the device; not with --wgs-*, --pcr-* or --truncate-*)\n");
}

// argparse's parser.error(): the usage, the message, exit code 2
int usage_error(const char* fmt, ...) __attribute__((format(printf, 1, 2)));
int usage_error(const char* fmt, ...) {
    usage(stderr);
    fputs("sequence: error: ", stderr);
    va_list ap; va_start(ap, fmt); vfprintf(stderr, fmt, ap); va_end(ap);
    fputc('\n', stderr);
    return 2;
}
int die(const std::string& msg) { fprintf(stderr, "%s\n", msg.c_str()); return 1; }     // sys.exit("msg")

// The option table: everything the command line accepts.  `dest` is argparse's name in the --list output (the options the reference
// does not have are not listed); `set` stores the value (nullptr for a flag) and returns what argparse would say about it ("": fine).
// --references has nargs="+" and is read by the argument loop itself.
struct Option { const char* name; char letter; bool takes_value; const char* dest; std::string (*set)(Args& a, const char* v); };

bool whole_number(const char* v, uint64_t& out) { char* e = nullptr; out = strtoull(v, &e, 10); return e != v && !*e; }
std::string truncate_mu_sigma(Args& a, const char* v, int mode) {
    char* e = nullptr;
    a.trc.mu = strtod(v, &e);
    if (!e || *e != ',') return "expected MU,SIGMA";
    a.trc.sigma = strtod(e + 1, &e);
    if (!e || *e) return "expected MU,SIGMA";
    a.trc.mode = mode; a.trc_n++;
    return {};
}

void split_commas(const char* v, std::vector<std::string>& out) {       // cxxopts' vector<string>: every occurrence, split at ','
    for (const char* q = v;;) {
        const char* e = strchr(q, ',');
        out.emplace_back(q, e ? (size_t)(e - q) : strlen(q));
        if (!e) return;
        q = e + 1;
    }
}

#define SET(...) [](Args& a, const char* v) -> std::string { (void)v; __VA_ARGS__; return {}; }
const Option OPTIONS[] = {
    {"--help", 'h', false, "help", SET(a.help = true)},
    {"--input", 'i', true, "input", SET(a.input = v)},
    {"--references", 'r', true, "references", nullptr},
    {"--badread", 'o', true, "badread", SET(a.badread = v)},
    {"--perfect", 0, true, "perfect", SET(a.perfect = v)},
    {"--skip-qual-compute", 0, false, "skip_qual_compute", SET(a.skip_qual = true)},
    {"--output-format", 'O', true, "output_format", SET(        // parsed and, like the reference, not used (py/sequence.py:65-72)
        a.output_format = v;
        if (a.output_format != "fastq" && a.output_format != "fasta") return "invalid choice: '" + a.output_format + "' (choose from 'fastq', 'fasta')")},
    {"--threads", 't', true, "threads", SET(a.threads = atoi(v))},
    {"--badread-identity", 0, true, "badread_identity", SET(a.identity = v)},
    {"--badread-error-model", 0, true, "badread_error_model", SET(a.error_model = v)},
    {"--badread-qscore-model", 0, true, "badread_qscore_model", SET(a.qscore_model = v)},
    {"--badread-tail-model", 0, true, "badread_tail_model", SET(a.tail_model = v)},
    {"--list", 0, false, "list", SET(a.list = true)},
    {"--seed", 's', true, "seed", SET(a.seed = atoll(v))},
    {"--devices", 0, true, "devices", SET(                      // one group of --in-flight contexts per entry (an entry may repeat)
        if (!tkmod::parse_device_list(v, a.devices)) return "invalid device list: '" + std::string(v) + "'")},
    {"--batch-bytes", 0, true, nullptr, SET(
        if (!whole_number(v, a.batch_bytes) || a.batch_bytes < 1) return "expected a positive integer, got '" + std::string(v) + "'")},
    {"--in-flight", 0, true, nullptr, SET(
        a.in_flight = atoi(v);
        if (a.in_flight < 1) return "expected a positive integer, got '" + std::string(v) + "'")},
    {"--gzip", 0, true, nullptr, SET(a.gzip = v)},
    {"--pcr-cycles", 0, true, nullptr, SET(a.pcr.cycles = atoi(v); a.pcr_have_cycles = true)},
    {"--pcr-molecule-count", 0, true, nullptr, SET(a.pcr.target_count = strtoull(v, nullptr, 10); a.pcr_have_count = true)},
    {"--pcr-error-rate", 0, true, nullptr, SET(a.pcr.error_rate = atof(v); a.pcr_have_er = true)},
    {"--pcr-efficiency", 0, true, nullptr, SET(a.pcr.efficiency = atof(v); a.pcr_have_ef = true)},
    {"--pcr-preset", 0, true, nullptr, SET(a.pcr_preset = v)},
    {"--pcr-slice-molecules", 0, true, nullptr, SET(a.pcr_slice = std::max<uint64_t>(1, strtoull(v, nullptr, 10)))},
    {"--truncate-normal", 0, true, nullptr, SET(return truncate_mu_sigma(a, v, TKSMSEQ_TRC_NORMAL))},
    {"--truncate-lognormal", 0, true, nullptr, SET(return truncate_mu_sigma(a, v, TKSMSEQ_TRC_LOGNORMAL))},
    {"--truncate-kde-model", 0, true, nullptr, SET(a.trc_kde = v; a.trc.mode = TKSMSEQ_TRC_KDE; a.trc_n++)},
    {"--truncate-always-end", 0, false, nullptr, SET(a.trc.always_end = 1)},
    {"--truncate-kde-models-length", 0, false, nullptr, SET(a.trc.kde_models_length = 1)},
    {"--wgs-frag-len-dist", 0, true, nullptr, SET(a.wgs_dist = v; a.wgs_have_dist = true)},
    {"--wgs-base-count", 0, true, nullptr, SET(a.wgs_base_count = atoll(v); a.wgs_have_bc = true)},
    {"--wgs-depth", 0, true, nullptr, SET(a.wgs_depth = atof(v); a.wgs_have_depth = true)},
    {"--wgs-batch-molecules", 0, true, nullptr, SET(
        if (!whole_number(v, a.wgs_batch) || a.wgs_batch < 1 || a.wgs_batch > (1ull << 28)) return "expected an integer between 1 and 268435456, got '" + std::string(v) + "'";
        a.wgs_on = true)},
    {"--transcribe-gtf", 0, true, nullptr, SET(split_commas(v, a.tsb_gtfs); a.tsb_on = true)},
    {"--transcribe-abundance", 0, true, nullptr, SET(split_commas(v, a.tsb_abundances); a.tsb_on = true)},
    {"--transcribe-molecule-count", 0, true, nullptr, SET(
        char* e = nullptr; a.tsb_count = strtoll(v, &e, 10);
        if (e == v || *e || a.tsb_count < -2147483648ll || a.tsb_count > 2147483647ll) return "expected an integer, got '" + std::string(v) + "'";
        a.tsb_have_count = true; a.tsb_on = true)},
    {"--transcribe-use-whole-id", 0, false, nullptr, SET(a.tsb_use_whole_id = true; a.tsb_on = true)},
    {"--transcribe-default-depth", 0, true, nullptr, SET(a.tsb_default_depth = atoll(v); a.tsb_on = true)},
    {"--transcribe-molecule-prefix", 0, true, nullptr, SET(a.tsb_prefix = v; a.tsb_on = true)},
    {"--transcribe-weights", 0, true, nullptr, SET(
        std::vector<std::string> t; split_commas(v, t);
        for (auto& x : t) { char* e = nullptr; const double w = strtod(x.c_str(), &e); if (e == x.c_str() || *e) return "expected numbers, got '" + std::string(v) + "'"; a.tsb_weights.push_back(w); }
        a.tsb_on = true)},
    {"--transcribe-batch-molecules", 0, true, nullptr, SET(
        if (!whole_number(v, a.tsb_batch) || a.tsb_batch < 1 || a.tsb_batch > (1ull << 28)) return "expected an integer between 1 and 268435456, got '" + std::string(v) + "'";
        a.tsb_on = true)},
    {"--verbosity", 0, true, "verbosity", SET(a.verbosity = v)},
    {"--log-file", 0, true, "log_file", SET(a.log_file = v)}};
#undef SET

const Option* short_option(char letter) { for (const Option& o : OPTIONS) if (o.letter && o.letter == letter) return &o; return nullptr; }
const Option* find_option(const std::string& t) {                        // a normalised token: `-x` or the full `--name`
    if (t.size() == 2 && t[0] == '-' && t[1] != '-') return short_option(t[1]);
    for (const Option& o : OPTIONS) if (t == o.name) return &o;
    return nullptr;
}
std::string display_name(const Option& o) { return o.letter ? std::string("-") + o.letter + "/" + o.name : std::string(o.name); }

}  // namespace

// The reference's parser is argparse with its defaults (py/sequence.py:35-40, :124): a long option may be abbreviated to any
// unambiguous prefix, `--opt=value` and a value glued to a short option (`-t8`) are accepted.  The command line is rewritten into
// the plain `--opt value` form the argument loop reads; `glued` marks values that came with their option (for -r/--references,
// nargs="+": an explicit value is the option's only one).
int normalise_args(int argc, char** argv, std::vector<std::string>& out, std::vector<char>& glued) {
    out.clear(); glued.clear();
    auto put = [&](const std::string& t, bool g) { out.push_back(t); glued.push_back(g ? 1 : 0); };
    if (argc > 0) put(argv[0], false);
    for (int i = 1; i < argc; i++) {
        const std::string t = argv[i];
        if (t.size() > 2 && t[0] == '-' && t[1] == '-') {
            const size_t eq = t.find('=');
            const std::string name = t.substr(0, eq);
            const Option* hit = nullptr; std::string could;
            int n_hit = 0;
            for (const Option& o : OPTIONS) if (name == o.name) { hit = &o; n_hit = 1; break; }
            if (!hit)
                for (const Option& o : OPTIONS)
                    if (strncmp(o.name, name.c_str(), name.size()) == 0) { hit = &o; n_hit++; could += (could.empty() ? "" : ", ") + std::string(o.name); }
            if (n_hit > 1) return usage_error("ambiguous option: %s could match %s", name.c_str(), could.c_str());
            if (n_hit == 0) { put(t, false); continue; }                       // the loop reports it as unrecognized
            put(hit->name, false);
            if (eq != std::string::npos) {
                if (!hit->takes_value) return usage_error("argument %s: ignored explicit argument '%s'", hit->name, t.substr(eq + 1).c_str());
                put(t.substr(eq + 1), true);
            }
        } else if (t.size() > 2 && t[0] == '-' && t[1] != '-' && short_option(t[1]) && short_option(t[1])->takes_value) {
            put(t.substr(0, 2), false);
            put(t.substr(t[2] == '=' ? 3 : 2), true);
        } else put(t, false);
    }
    return 0;
}

namespace {

using tkmod::Logger;        // --verbosity / --log-file: module_log.h.  What the reference's Python prints unconditionally (model loading
                            // progress, "Loading reference") stays unconditional; the module's own diagnostics go through the logger.

// one gzip member (RFC 1952) holding d[0..n): members simply follow each other in a .gz file, so batches -- and pieces of
// a batch -- are compressed independently, on the worker threads, and the writer appends bytes
bool gzip_member(const uint8_t* d, size_t n, std::vector<uint8_t>& out) {
    z_stream z{};
    if (deflateInit2(&z, 1, Z_DEFLATED, 15 + 16, 8, Z_DEFAULT_STRATEGY) != Z_OK) return false;
    out.resize(deflateBound(&z, (uLong)n) + 64);
    z.next_in = const_cast<Bytef*>(d); z.avail_in = (uInt)n;
    z.next_out = out.data(); z.avail_out = (uInt)out.size();
    const int rc = deflate(&z, Z_FINISH);
    out.resize(rc == Z_STREAM_END ? z.total_out : 0);
    deflateEnd(&z);
    return rc == Z_STREAM_END;
}

struct Writer {
    int fd = -1; bool gz = false, fastq = false, wrote = false;
    bool bgzf = false;                                   // --gzip device: the bytes are BGZF members made on the device; close() ends the file
    bool positional = false;                             // a regular file: the workers write their batches at their offsets (pwrite)
    void classify(const std::string& path) {             // get_output_file, py/sequence.py:291-300: the NAME decides format and compression
        std::string p = path;
        gz = false;
        if (p.size() >= 3 && p.compare(p.size() - 3, 3, ".gz") == 0) { gz = true; p.resize(p.size() - 3); }
        auto ends = [&](const char* s) { size_t n = strlen(s); return p.size() >= n && p.compare(p.size() - n, n, s) == 0; };
        fastq = ends(".fastq") || ends(".fq");
    }
    bool open(const std::string& path) {                 // creates / truncates: only once devices, references, models and the input are usable
        classify(path);
        fd = ::open(path.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0666);
        if (fd < 0) return false;
        struct stat st;
        positional = fstat(fd, &st) == 0 && S_ISREG(st.st_mode);
        return true;
    }
    bool write(const uint8_t* d, size_t n) {             // appends; for .gz outputs the bytes are finished gzip members
        wrote = wrote || n;
        while (n) {
            const ssize_t w = ::write(fd, d, std::min<size_t>(n, (size_t)1 << 30));
            if (w < 0) { if (errno == EINTR) continue; return false; }
            d += w; n -= (size_t)w;
        }
        return true;
    }
    bool write_at(const uint8_t* d, size_t n, uint64_t off) const {
        while (n) {
            const ssize_t w = ::pwrite(fd, d, std::min<size_t>(n, (size_t)1 << 30), (off_t)off);
            if (w < 0) { if (errno == EINTR) continue; return false; }
            d += w; n -= (size_t)w; off += (uint64_t)w;
        }
        return true;
    }
    bool close() {                                       // false: the last bytes could not be written
        if (fd < 0) return true;
        bool ok = true;
        if (gz && bgzf) {                                // the EOF member, behind everything the run has written (an empty run: it alone)
            uint8_t e[28];
            tksmseq_gzip_eof(e);
            ok = (!positional || lseek(fd, 0, SEEK_END) >= 0) && write(e, sizeof e);
        } else if (gz && !wrote) { std::vector<uint8_t> e; if (gzip_member(nullptr, 0, e)) ok = write(e.data(), e.size()); }   // a valid empty .gz
        ok = ::close(fd) == 0 && ok;
        fd = -1;
        return ok;
    }
};

struct Chunk { uint64_t seq = 0, first_read = 0, n_reads = 0; std::vector<char> text; uint64_t t_begin = 0, t_end = 0; size_t table = 0; };   // text, or (chained PCR) a slice of the templates, or (chained transcribe) of an abundance table's molecules
// a parsed batch on its way from a parser thread to a worker of the same device group
struct Parsed { uint64_t seq = 0, first_read = 0, n_reads = 0; tksmseq_batch* b = nullptr; };
struct GroupQueue {                                       // per device group: its parsers hand over in the order in which they took the chunks
    GroupQueue(size_t cap, bool one_maker) : q(cap), turn(one_maker) {}
    tkmod::BoundedQueue<Parsed> q; tkmod::Handover turn;
};

struct Worker {                                           // one batch in flight: context + page-locked record buffers
    tksmseq_ctx* ctx = nullptr;
    uint8_t* host[2] = {nullptr, nullptr}; uint64_t host_cap[2] = {0, 0};
    std::vector<uint8_t> packed[2];                     // .gz outputs: the batch as gzip members
    // regular uncompressed files: the records pass through two page-locked pieces (one being written while the next arrives)
    uint64_t piece = 64ull << 20;                       // (TKSMSEQ_PIECE_BYTES: small pieces for the tests)
    uint8_t* ring[2] = {nullptr, nullptr};
    // ... behind the worker's back: the batch's records are copied into one of two device buffers of the writer's (a device copy
    // takes a millisecond), and the worker's context runs the next batch while a thread of its own streams the buffer out
    struct Job { int stage = 0, k = 0; uint64_t bytes = 0, off = 0, seq = 0; };
    tksmseq_ctx* wctx = nullptr;                        // the writer thread's context (its stream carries the copies)
    void* stage[2] = {nullptr, nullptr}; uint64_t stage_cap[2] = {0, 0};
    std::mutex m; std::condition_variable cv;
    bool stage_busy[2] = {false, false};                // guarded by m
    std::deque<Job> jobs; bool jobs_closed = false;     // guarded by m
    int cur_stage = 0;
    bool stage_reserve(int q, uint64_t bytes) {
        if (bytes <= stage_cap[q]) return true;
        tksmseq_device_free(wctx, stage[q]); stage[q] = nullptr; stage_cap[q] = 0;
        const uint64_t want = bytes + bytes / 8 + 4096;
        if (tksmseq_device_alloc(wctx, want, &stage[q])) return false;
        stage_cap[q] = want;
        return true;
    }
    bool ring_ready() {
        for (int q = 0; q < 2; q++)
            if (!ring[q]) { void* p = nullptr; if (tksmseq_host_alloc(piece, &p)) return false; ring[q] = (uint8_t*)p; }
        return true;
    }
    bool reserve(int k, uint64_t bytes) {
        if (bytes <= host_cap[k]) return true;
        tksmseq_host_free(host[k]); host[k] = nullptr; host_cap[k] = 0;
        const uint64_t want = bytes + bytes / 4 + 4096;
        void* p = nullptr;
        if (tksmseq_host_alloc(want, &p)) return false;
        host[k] = (uint8_t*)p; host_cap[k] = want;
        return true;
    }
    ~Worker() {                                           // the writer's context (a clone of ctx) before ctx
        for (int q = 0; q < 2; q++) { tksmseq_host_free(host[q]); tksmseq_host_free(ring[q]); }
        if (wctx) { tksmseq_device_free(wctx, stage[0]); tksmseq_device_free(wctx, stage[1]); tksmseq_destroy(wctx); }
        if (ctx) tksmseq_destroy(ctx);
    }
};

// One group of --in-flight contexts per entry of --devices: the first context of a group loads the reference and the models onto its
// device, the others share them (tksmseq_clone).  Reads are numbered by the reader, batches go to whichever context is free, the
// writer restores MDF order: the output does not depend on the device list.  MDF text is parsed (and its tables uploaded) ahead of the
// workers, by two parser threads per device group with contexts of their own, so that a worker's cycle is run + copy + write only.
struct Devices {
    static constexpr int parsers_per_group = 2;
    const Args& a; const bool compute_q;
    const int n_groups, per_group, n_workers;
    std::vector<std::unique_ptr<Worker>> workers;
    std::vector<tksmseq_ctx*> pctx;                                      // the parser threads' contexts (clones)
    std::vector<tksmseq_batch*> templates;                               // chained PCR: the whole input, one batch per device group
    // chained transcribe: every parser context's plan of every abundance table ([parser][table]; a group's tables are parsed once, its
    // second parser shares the rows), and the tables' molecule counts
    std::vector<std::vector<tksmseq_tsb_plan*>> tsb_plans;
    std::vector<uint64_t> tsb_molecules;
    std::vector<std::string> tsb_missing;                                // ids the GTFs lack, in row order
    std::string error;                                                   // why the set-up failed ("": it did not)

    Worker& first(int g) { return *workers[(size_t)g * per_group]; }
    tksmseq_ctx* parser(int g, int j = 0) { return pctx[(size_t)g * parsers_per_group + j]; }

    Devices(const Args& a, bool compute_q) : a(a), compute_q(compute_q), n_groups((int)a.devices.size()), per_group(std::max(1, std::min(a.in_flight, 8))),
                                              n_workers(n_groups * per_group), templates((size_t)n_groups, nullptr) {
        for (int w = 0; w < n_workers; w++) workers.emplace_back(new Worker());
        if (const char* pb = getenv("TKSMSEQ_PIECE_BYTES")) for (auto& W : workers) W->piece = std::max<uint64_t>(4096, strtoull(pb, nullptr, 10));
        // the models are parsed (and the identity quantile table computed) on threads of their own while the devices are set up and
        // the reference is read and packed: the loaders find them parsed (models.cpp keeps parsed models)
        std::vector<std::thread> prefetch;
        if (!a.badread.empty()) {
            prefetch.emplace_back([&]() { (void)tksmseq_prefetch_identity(a.mean, a.maxi, a.sd); });
            prefetch.emplace_back([&]() { (void)tksmseq_prefetch_model(a.error_model.c_str(), "error"); });
            if (compute_q) prefetch.emplace_back([&]() { (void)tksmseq_prefetch_model(a.qscore_model.c_str(), "qscore"); });
        }
        std::once_flag joined;
        auto join_prefetch = [&]() { std::call_once(joined, [&]() { for (auto& t : prefetch) t.join(); }); };
        std::vector<std::string> gerr((size_t)n_groups);
        std::vector<std::thread> gt;
        for (int g = 0; g < n_groups; g++) gt.emplace_back([&, g]() { gerr[(size_t)g] = load_group(g, join_prefetch); });
        for (auto& t : gt) t.join();
        join_prefetch();
        for (auto& e : gerr) if (error.empty()) error = e;
        if (error.empty()) clone_parsers();
        if (error.empty() && a.tsb_on) plan_transcribe();
    }
    void plan_transcribe() {
        tsb_plans.assign(pctx.size(), std::vector<tksmseq_tsb_plan*>());
        tsb_molecules.assign(a.tsb_texts.size(), 0);
        uint64_t first_row = 0;
        for (size_t f = 0; f < a.tsb_texts.size() && error.empty(); f++) {
            tksmseq_tsb_params p{};
            p.seed = (uint64_t)a.seed; p.molecule_count = a.tsb_count; p.weight = a.tsb_w[f]; p.first_row_index = first_row;
            p.use_whole_id = a.tsb_use_whole_id ? 1 : 0; p.prefix = a.tsb_prefix.c_str();
            uint64_t rows = 0;
            for (size_t pi = 0; pi < pctx.size() && error.empty(); pi++) {
                tksmseq_tsb_plan* plan = nullptr;
                const bool first = pi % parsers_per_group == 0;
                const int rc = first ? tksmseq_transcribe_plan_create(pctx[pi], nullptr, a.tsb_texts[f].data(), a.tsb_texts[f].size(), &p, &plan)
                                     : tksmseq_transcribe_plan_clone(pctx[pi], tsb_plans[pi - pi % parsers_per_group][f], &plan);
                if (rc) { error = std::string("Error: transcribe: ") + tksmseq_last_error(pctx[pi]); break; }
                tsb_plans[pi].push_back(plan);
                if (pi == 0) {
                    uint64_t n_missing = 0;
                    tksmseq_transcribe_plan_info(plan, &rows, nullptr, &tsb_molecules[f], &n_missing);
                    for (uint64_t i = 0; i < n_missing; i++) {
                        const char* id = nullptr; uint64_t len = 0;
                        tksmseq_transcribe_plan_missing(plan, i, &id, &len);
                        tsb_missing.emplace_back(id, (size_t)len);
                    }
                }
            }
            first_row += rows;
        }
    }
    // the group's first context, with the reference and the models, and its clones; "": fine
    template <class Join> std::string load_group(int g, Join& join_prefetch) {
        tksmseq_ctx*& ctx = first(g).ctx;
        if (tksmseq_create(a.devices[(size_t)g], &ctx)) return std::string("Error: ") + tksmseq_last_error(nullptr);
        auto fail = [&](const std::string& what) { return "Error: " + what + ": " + tksmseq_last_error(ctx); };
        tksmseq_set_host_threads(ctx, a.threads);
        for (auto& r : a.references) {
            if (g == 0) { printf("Loading reference %s...\n", r.c_str()); fflush(stdout); }
            if (tksmseq_reference_add_fasta(ctx, r.c_str())) return fail("loading reference");
        }
        for (auto& gtf : a.tsb_gtfs)                                      // (before the clones are made: they share the table)
            if (tksmseq_transcripts_add_gtf(ctx, gtf.c_str(), a.tsb_default_depth != 0)) return fail("reading GTF");
        if (!a.badread.empty()) {
            join_prefetch();
            if (tksmseq_set_identity(ctx, a.mean, a.maxi, a.sd)) return fail("identity distribution");
            if (g == 0) fprintf(stderr, "\nLoading error model from %s\n", a.error_model.c_str());
            if (tksmseq_load_error_model(ctx, a.error_model.c_str())) return fail("error model");
            if (compute_q) {
                if (g == 0) fprintf(stderr, "\nLoading qscore model from %s\n", a.qscore_model.c_str());
                if (tksmseq_load_qscore_model(ctx, a.qscore_model.c_str())) return fail("qscore model");
            }
            if (tksmseq_load_tail_model(ctx, a.tail_model.c_str())) return fail("tail model");     // py/sequence.py:343-345
        }
        for (int j = 1; j < per_group; j++)
            if (tksmseq_clone(ctx, &workers[(size_t)g * per_group + j]->ctx)) return fail("second context");
        return {};
    }
    void clone_parsers() {
        pctx.assign((size_t)n_groups * parsers_per_group, nullptr);
        for (size_t p = 0; p < pctx.size() && error.empty(); p++) {
            tksmseq_ctx* from = first((int)p / parsers_per_group).ctx;
            if (tksmseq_clone(from, &pctx[p])) error = std::string("Error: parser context: ") + tksmseq_last_error(from);
            else tksmseq_set_host_threads(pctx[p], a.threads);
        }
    }
    // clones before the contexts they borrow from: the templates and the parser contexts first, then every group's workers from the
    // last back to the first (which holds the reference and the models)
    ~Devices() {
        for (int g = 0; g < n_groups; g++) if (templates[(size_t)g]) tksmseq_batch_free(parser(g), templates[(size_t)g]);
        for (auto& plans : tsb_plans) for (auto* p : plans) tksmseq_transcribe_plan_free(p);
        for (auto& c : pctx) if (c) tksmseq_destroy(c);
        while (!workers.empty()) workers.pop_back();
    }
};

// How a batch's records reach an output; decided once per output when the files are open (Sinks::open):
//   StagedBehind  uncompressed outputs, and .gz with --gzip device (the compressed stream is just bytes of known size): the records
//                 move into a staging buffer on the device, and a writer thread per worker streams them out -- at their place in a
//                 regular file, in batch order into anything else -- while the worker's context runs its next batch
//   HostGzipAt    a regular .gz file compressed on the host: the worker downloads the batch, compresses its members side by side and
//                 writes them at their place
//   HostOrdered   some output is a host-compressed .gz that is no regular file: every output of the run gets whole-batch host
//                 buffers, and one writer thread puts them out in batch order
enum class Route { None, StagedBehind, HostGzipAt, HostOrdered };

struct Sinks {
    Writer w[2];                                          // 0: -o/--badread, 1: --perfect
    Route route[2] = {Route::None, Route::None};
    bool behind = false, positional = false;             // (the stats file names them)
    bool ordered() const { return route[0] == Route::HostOrdered || route[1] == Route::HostOrdered; }
    int first() const { return route[0] == Route::None ? 1 : 0; }
    // creates the files; false: `failed` could not be opened
    bool open(const Args& a, std::string& failed) {
        const std::string* path[2] = {&a.badread, &a.perfect};
        for (int k = 0; k < 2; k++)
            if (!path[k]->empty() && !w[k].open(*path[k])) { if (k) w[0].close(); failed = *path[k]; return false; }
        auto all = [&](auto&& pred) { return (path[0]->empty() || pred(w[0])) && (path[1]->empty() || pred(w[1])); };
        for (Writer& x : w) x.bgzf = x.gz && a.gzip == "device";
        positional = all([](const Writer& x) { return x.positional; });
        behind = all([](const Writer& x) { return !x.gz || x.bgzf; });
        for (int k = 0; k < 2; k++)
            if (!path[k]->empty()) route[k] = behind ? Route::StagedBehind : !positional ? Route::HostOrdered : w[k].gz ? Route::HostGzipAt : Route::StagedBehind;
        return true;
    }
};

// stage clocks (TKSMSEQ_VERBOSE, TKSMSEQ_STATS_FILE): seconds summed over the threads of a stage, in the order of the stats file's keys
enum Stage { PARSE, RUN, DEVICE_COPY, D2H_WAIT, WRITE, WAIT_FOR_WRITER, READ_COUNT, N_STAGES };
const char* const STAGE_KEY[N_STAGES] = {"parse_s", "run_s", "device_copy_s", "d2h_wait_s", "write_s", "wait_for_writer_s", "read_count_s"};
struct StageClocks {
    std::mutex m; double s[N_STAGES] = {};
    void add(Stage k, Clock::time_point t0) { const double dt = seconds(t0); std::lock_guard<std::mutex> l(m); s[k] += dt; }
};

struct Ending { bool verbose = false; Clock::time_point t_close, t_closed; };      // for the run's last verbose line, printed once the devices are released

struct Input {                                            // -i, read through its descriptor (Stream::read_full)
    FILE* f = nullptr; int fd = -1; bool regular = false;
    bool open(const std::string& path) {
        f = fopen(path.c_str(), "rb");
        if (!f) return false;
        fd = fileno(f);
        struct stat st; regular = fstat(fd, &st) == 0 && S_ISREG(st.st_mode);
        return true;
    }
    ~Input() { if (f) fclose(f); }
};

// The run once devices, input and outputs are there: the main thread feeds, two parser threads per group make device batches, a worker
// per context runs them and sends the records down their output's route.
struct Stream {
    const Args& a; Logger& log; Devices& dev; Sinks& out; Input& in;
    const bool compute_q, verbose, verbose2;
    const Clock::time_point t_start = Clock::now();
    tkmod::BoundedQueue<Chunk> chunks;
    std::vector<std::unique_ptr<GroupQueue>> groups;
    tkmod::BatchOrder order;
    StageClocks clk;
    std::atomic<uint64_t> bytes_in{0}, bytes_d2h{0};
    std::mutex err_m; std::string first_error;
    uint64_t seq = 0, read_index = 0;                    // the next batch number and the first read of that batch: the feeder's (chained wgs: under wgs_m)
    // chained random-wgs: the only state that is serial across batches (guarded by wgs_m): next candidate, molecules and bases so far.
    // A maker thread takes it, makes its batch on its own context (milliseconds next to the sequencing of a batch) and hands it back;
    // the batch numbers keep the writers' order, and a read's global index is its molecule's index.
    std::mutex wgs_m; tksmseq_wgs_progress wgs_st{}; bool wgs_done;

    Stream(const Args& a, Logger& log, Devices& dev, Sinks& out, Input& in, bool compute_q)
        : a(a), log(log), dev(dev), out(out), in(in), compute_q(compute_q), verbose(getenv("TKSMSEQ_VERBOSE") != nullptr || log.level <= Logger::DEBUG),
          verbose2(getenv("TKSMSEQ_VERBOSE") && atoi(getenv("TKSMSEQ_VERBOSE")) >= 2), chunks((size_t)dev.n_workers),
          order((size_t)dev.n_workers, out.first()), wgs_done(a.wgs_on && a.wgs.base_count <= 0) {
        for (int g = 0; g < dev.n_groups; g++) groups.emplace_back(new GroupQueue((size_t)dev.per_group, a.wgs_on));
    }
    bool failed() const { return order.failed(); }
    void set_error(const std::string& msg) {
        std::lock_guard<std::mutex> l(err_m);
        if (!failed()) first_error = msg;
        order.fail();
        chunks.close();
        for (auto& g : groups) g->q.close();
        for (auto& W : dev.workers) { { std::lock_guard<std::mutex> lw(W->m); } W->cv.notify_all(); }      // (a worker waiting for a staging buffer)
    }
    bool ctx_error(tksmseq_ctx* c) { set_error(tksmseq_last_error(c)); return false; }
    double since_start() const { return seconds(t_start); }

    // ---- sources: what the main thread feeds (feed_*), and what a parser thread makes of it (next_*) -------------------------------
    enum class Made { End, Nothing, Batch };             // End: the source is exhausted (or the run has failed)
    typedef void (Stream::*Feed)();
    typedef Made (Stream::*Next)(int pi, Parsed& pr, uint64_t& ticket);
    Feed feed() const { return a.wgs_on ? &Stream::feed_wgs : a.tsb_on ? &Stream::feed_transcribe : a.pcr_on ? &Stream::feed_pcr_slices : &Stream::feed_text; }
    Next next() const { return a.wgs_on ? &Stream::next_wgs : a.tsb_on ? &Stream::next_transcribe : a.pcr_on ? &Stream::next_pcr_slice : &Stream::next_text; }
    GroupQueue& group_of_parser(int pi) { return *groups[(size_t)(pi / Devices::parsers_per_group)]; }

    // like fread(dst, 1, n, in): n bytes unless the input ends -- or the run has failed.  A pipe (Snakemake's `tksm ... | tksm sequence
    // -i /dev/stdin`, Snakefile:283-305) may stay open with nothing to read while a worker has already failed: the reader polls it and
    // gives up then, instead of sleeping in a read() until the producer closes
    size_t read_full(char* dst, size_t n) {
        size_t got = 0;
        while (got < n && !failed()) {
            if (!in.regular) {
                struct pollfd pf; pf.fd = in.fd; pf.events = POLLIN; pf.revents = 0;
                const int pr = poll(&pf, 1, 200);
                if (pr == 0) continue;
                if (pr < 0) { if (errno == EINTR) continue; break; }
            }
            const ssize_t r = ::read(in.fd, dst + got, std::min<size_t>(n - got, (size_t)1 << 30));
            if (r < 0) { if (errno == EINTR) continue; break; }
            if (r == 0) break;
            got += (size_t)r;
        }
        return got;
    }
    void push_chunk(Chunk&& c, uint64_t n_reads) {
        c.seq = seq++; c.first_read = read_index; c.n_reads = n_reads;
        read_index += n_reads;
        chunks.push(std::move(c));
    }
    // MDF text: batches of whole molecules, numbered; the first read index of a batch is known before it is parsed
    void feed_text() {
        tkmod::ChunkReader rd;
        rd.bytes = a.batch_bytes;
        rd.read = [this](char* dst, size_t n) { return read_full(dst, n); };
        for (;;) {
            const auto t_read = Clock::now();
            Chunk c;
            if (failed() || !rd.next(c.text) || failed()) break;
            const uint64_t n_reads = tkmod::count_reads(c.text.data(), c.text.size());
            bytes_in += c.text.size();
            clk.add(READ_COUNT, t_read);
            push_chunk(std::move(c), n_reads);
        }
    }
    // chained PCR (src/pcr.cpp:215: the module holds its whole input): the templates go to every device group once; the copies per
    // template (tksmseq_pcr_template_counts) cut them into slices of about --pcr-slice-molecules copies, which the parser threads
    // amplify (and truncate) in place of parsing text
    void feed_pcr_slices() {
        std::vector<char> all;
        { std::vector<char> tmp(1 << 20); size_t n; while ((n = read_full(tmp.data(), tmp.size())) > 0) all.insert(all.end(), tmp.begin(), tmp.begin() + (ptrdiff_t)n); }
        for (int g = 0; g < dev.n_groups && !failed(); g++)
            if (tksmseq_molecules_from_mdf_text(dev.parser(g), all.data(), all.size(), &dev.templates[(size_t)g])) ctx_error(dev.parser(g));
        uint64_t nt = 0;
        std::vector<uint64_t> counts;
        if (!failed()) {
            tksmseq_batch_info(dev.templates[0], &nt, nullptr, nullptr);
            counts.resize(nt);
            if (tksmseq_pcr_template_counts(dev.parser(0), dev.templates[0], &a.pcr, counts.data())) ctx_error(dev.parser(0));
        }
        uint64_t u0 = 0, acc = 0;
        auto push_slice = [&](uint64_t b0, uint64_t e0, uint64_t n_out) { Chunk c; c.t_begin = b0; c.t_end = e0; push_chunk(std::move(c), n_out); };
        for (uint64_t u = 0; u < nt && !failed(); u++) {
            acc += counts[u];
            if (acc >= a.pcr_slice && u + 1 < nt) { push_slice(u0, u + 1, acc); u0 = u + 1; acc = 0; }
        }
        if (!failed()) push_slice(u0, nt, acc);                  // the last slice (the only, empty one of an input without molecules)
    }
    void feed_wgs() {}                                           // nothing to read: the parser threads make the batches
    // chained transcribe: consecutive slices of every table's unrolled molecules, tables in order; a read's global index is its
    // molecule's position in that order, which is the order of the file `tksm transcribe` writes
    void feed_transcribe() {
        for (size_t f = 0; f < dev.tsb_molecules.size(); f++)
            for (uint64_t m = 0; m < dev.tsb_molecules[f] && !failed(); m += a.tsb_batch) {
                Chunk c;
                c.table = f; c.t_begin = m; c.t_end = std::min(dev.tsb_molecules[f], m + a.tsb_batch);
                const uint64_t n = c.t_end - c.t_begin;
                push_chunk(std::move(c), n);
            }
    }

    bool take_chunk(int pi, Chunk& c, uint64_t& ticket) { return group_of_parser(pi).turn.take(ticket, [&] { return chunks.pop(c); }); }
    // --truncate-* behind the parse / the amplification; pr.b becomes the truncated batch
    bool truncate(tksmseq_ctx* pc, Parsed& pr) {
        if (!a.trc_n) return true;
        tksmseq_trc_params q = a.trc;
        q.flags = TKSMSEQ_MOL_NO_COMMENTS;
        q.first_molecule_index = pr.first_read;
        tksmseq_batch* cut = nullptr;
        const bool ok = !tksmseq_truncate(pc, pr.b, &q, &cut) || ctx_error(pc);
        tksmseq_batch_free(pc, pr.b);
        pr.b = cut;
        return ok;
    }
    Made parsed(int pi, const Parsed& pr, bool ok, Clock::time_point t_parse) {
        clk.add(PARSE, t_parse);
        if (verbose2) fprintf(stderr, "[sequence] batch %llu parser %d: parsed / made in %.3f s at %.3f s\n", (unsigned long long)pr.seq, pi, seconds(t_parse), since_start());
        return ok ? Made::Batch : Made::Nothing;
    }
    Made next_text(int pi, Parsed& pr, uint64_t& ticket) {
        Chunk c;
        if (!take_chunk(pi, c, ticket)) return Made::End;
        if (failed()) return Made::Nothing;
        pr.seq = c.seq; pr.first_read = c.first_read; pr.n_reads = c.n_reads;
        tksmseq_ctx* pc = dev.pctx[(size_t)pi];
        const auto t_parse = Clock::now();
        bool ok = !(a.trc_n ? tksmseq_molecules_from_mdf_text : tksmseq_batch_from_mdf_text)(pc, c.text.data(), c.text.size(), &pr.b) || ctx_error(pc);
        ok = ok && truncate(pc, pr);
        return parsed(pi, pr, ok, t_parse);
    }
    // a slice of the templates amplified on the device: its copies are numbered from c.first_read on
    Made next_pcr_slice(int pi, Parsed& pr, uint64_t& ticket) {
        Chunk c;
        if (!take_chunk(pi, c, ticket)) return Made::End;
        if (failed()) return Made::Nothing;
        pr.seq = c.seq; pr.first_read = c.first_read; pr.n_reads = c.n_reads;
        tksmseq_ctx* pc = dev.pctx[(size_t)pi];
        const auto t_parse = Clock::now();
        tksmseq_pcr_params q = a.pcr;
        q.flags = TKSMSEQ_MOL_NO_COMMENTS;             // (Seq never reads header comments: no per-molecule text on the host)
        q.template_begin = c.t_begin; q.template_end = c.t_end;
        if (c.t_begin == c.t_end) { q.template_begin = q.template_end = 0; q.cycles = 0; }
        bool ok = !tksmseq_pcr(pc, dev.templates[(size_t)(pi / Devices::parsers_per_group)], &q, &pr.b) || ctx_error(pc);
        if (verbose2) fprintf(stderr, "[sequence] slice %llu parser %d: pcr %.3f s at %.3f s\n", (unsigned long long)c.seq, pi, seconds(t_parse), since_start());
        ok = ok && truncate(pc, pr);
        return parsed(pi, pr, ok, t_parse);
    }
    Made next_transcribe(int pi, Parsed& pr, uint64_t& ticket) {
        Chunk c;
        if (!take_chunk(pi, c, ticket)) return Made::End;
        if (failed()) return Made::Nothing;
        pr.seq = c.seq; pr.first_read = c.first_read; pr.n_reads = c.n_reads;
        tksmseq_ctx* pc = dev.pctx[(size_t)pi];
        const auto t_parse = Clock::now();
        // (Seq never reads header comments: no per-molecule text on the host)
        const bool ok = !tksmseq_transcribe(pc, dev.tsb_plans[(size_t)pi][c.table], c.t_begin, c.t_end - c.t_begin, TKSMSEQ_MOL_NO_COMMENTS, &pr.b) || ctx_error(pc);
        return parsed(pi, pr, ok, t_parse);
    }
    // the next whole-genome batch, made under the lock of the serial state (the group's hand-over ticket is taken together with the
    // batch number: tickets and numbers rise together; the group's other maker starts only once this batch is handed over)
    Made next_wgs(int pi, Parsed& pr, uint64_t& ticket) {
        tksmseq_ctx* pc = dev.pctx[(size_t)pi];
        Clock::time_point t_make;
        const bool made = group_of_parser(pi).turn.take(ticket, [&] {
            std::lock_guard<std::mutex> l(wgs_m);
            if (wgs_done || failed()) return false;
            t_make = Clock::now();
            tksmseq_wgs_params q = a.wgs;
            q.first_candidate = wgs_st.next_candidate; q.n_candidates = a.wgs_batch; q.molecules_before = wgs_st.molecules; q.bases_before = wgs_st.bases;
            tksmseq_wgs_progress np{};
            if (tksmseq_wgs(pc, &q, &pr.b, &np)) return ctx_error(pc);
            tksmseq_batch_info(pr.b, &pr.n_reads, nullptr, nullptr);
            if (!pr.n_reads && !np.reached) {
                tksmseq_batch_free(pc, pr.b);
                set_error("none of " + std::to_string(a.wgs_batch) + " candidate fragments has a base (fragment length distribution '" + a.wgs_dist + "'): giving up");
                return false;
            }
            pr.seq = seq++; pr.first_read = wgs_st.molecules;
            wgs_st = np;
            if (np.reached) wgs_done = true;
            return true;
        });                                              // (the other groups make their batches while this one waits for room)
        if (!made) return Made::End;
        clk.add(PARSE, t_make);
        if (verbose2) fprintf(stderr, "[sequence] batch %llu maker %d: %llu molecules made in %.3f s at %.3f s\n", (unsigned long long)pr.seq, pi, (unsigned long long)pr.n_reads, seconds(t_make), since_start());
        return Made::Batch;
    }
    void parse_ahead(int pi) {
        GroupQueue& g = group_of_parser(pi);
        const Next next_batch = next();
        for (;;) {
            Parsed pr; uint64_t ticket = 0;
            const Made made = (this->*next_batch)(pi, pr, ticket);
            if (made == Made::End) return;
            g.turn.hand(ticket, [&] { if (made == Made::Batch && !g.q.push(std::move(pr))) tksmseq_batch_free(dev.pctx[(size_t)pi], pr.b); });   // (closed after an error)
        }
    }

    // ---- sinks: a worker runs its batch once per output and sends the records down that output's route --------------------------------
    struct Batch { Worker& W; int wi; const Parsed& c; uint64_t n = 0; tkmod::Finished fin; bool waited = false; };

    bool emit(Batch& bt, int k, int mode, int quirk) {
        Worker& W = bt.W;
        tksmseq_run_params p{};
        p.seed = (uint64_t)a.seed; p.first_read_index = bt.c.first_read; p.read_index_stride = 1;
        p.mode = mode; p.fastq = out.w[k].fastq; p.compute_qual = compute_q; p.perfect_of_badread = quirk;
        tksmseq_result r{};
        const auto t_run = Clock::now();
        if (tksmseq_run(W.ctx, bt.c.b, &p, &r)) return ctx_error(W.ctx);
        clk.add(RUN, t_run);
        if (verbose2) fprintf(stderr, "[sequence] batch %llu worker %d: run %.3f s (%llu reads) at %.3f s\n", (unsigned long long)bt.c.seq, bt.wi, seconds(t_run), (unsigned long long)bt.n, since_start());
        switch (out.route[k]) {
            case Route::StagedBehind: return emit_staged(bt, k, r.records_bytes);
            case Route::HostGzipAt: return emit_host_gzip_at(bt, k, r.records_bytes);
            case Route::HostOrdered: return emit_host_ordered(bt, k, r.records_bytes);
            case Route::None: break;
        }
        return true;
    }
    // an empty batch still takes its (empty) place, and its turn in a non-seekable output
    bool emit_empty(Batch& bt, int k) {
        uint64_t off = 0;
        if (out.route[k] == Route::None || out.route[k] == Route::HostOrdered) return true;      // (the ordered writer is handed its zero bytes)
        if (!order.take_place(k, bt.c.seq, 0, 0, off)) return false;
        if (out.route[k] == Route::StagedBehind && !out.w[k].positional) { order.wait_turn(k, bt.c.seq); order.turn_done(k, true); }
        return true;
    }
    // The records, or (--gzip device) their BGZF members, move into a staging buffer of the writer thread's (device to device), which
    // streams them out while this context runs its next batch.  A regular file: the batch's place in it is known as soon as every
    // earlier batch has announced its size (writes into ONE file are serialised by the file system: 11 - 13.5 GB/s on the test box
    // whatever the number of threads, tools/fs_write_probe.py -- the bound of the end-to-end rate)
    bool emit_staged(Batch& bt, int k, uint64_t out_bytes) {
        Worker& W = bt.W; Writer& wr = out.w[k];
        if (wr.bgzf) {
            tksmseq_gzip_result g{};
            const auto t_gz = Clock::now();
            if (tksmseq_result_gzip(W.ctx, &g)) return ctx_error(W.ctx);
            clk.add(RUN, t_gz);
            out_bytes = g.bytes;
        }
        uint64_t off = 0;
        if (!order.take_place(k, bt.c.seq, out_bytes, bt.n, off)) return false;
        // (blocks allocated ahead of the writes: the writes into one file are serialised by the file system, and
        // the allocation would happen inside them -- 12 -> 13.5 GB/s on the test box, tools/fs_write_probe.py)
        if (out_bytes && wr.positional) (void)posix_fallocate(wr.fd, (off_t)off, (off_t)out_bytes);
        const auto t_copy = Clock::now();
        int q;
        {
            std::unique_lock<std::mutex> l(W.m);
            q = W.cur_stage;
            W.cv.wait(l, [&] { return !W.stage_busy[q] || failed(); });
            if (failed()) return false;
            W.stage_busy[q] = true;
            W.cur_stage ^= 1;
        }
        if (!W.stage_reserve(q, out_bytes)) { set_error("out of device memory for the output staging buffers"); return false; }
        if (out_bytes && ((wr.bgzf ? tksmseq_gzip_copy_device(W.ctx, W.stage[q]) : tksmseq_result_copy_device(W.ctx, W.stage[q], nullptr)) || tksmseq_synchronize(W.ctx))) return ctx_error(W.ctx);
        clk.add(DEVICE_COPY, t_copy);
        { std::lock_guard<std::mutex> l(W.m); Worker::Job j; j.stage = q; j.k = k; j.bytes = out_bytes; j.off = off; j.seq = bt.c.seq; W.jobs.push_back(j); }
        W.cv.notify_all();
        bt.fin.bytes[k] = out_bytes;
        return true;
    }
    // the batch's records in the worker's page-locked buffer k
    bool download(Batch& bt, int k, uint64_t bytes) {
        Worker& W = bt.W;
        if (failed()) return false;
        const auto t_copy = Clock::now();
        if (!W.reserve(k, bytes)) { set_error("out of page-locked host memory"); return false; }
        const auto t_copy2 = Clock::now();
        if (tksmseq_result_download(W.ctx, W.host[k], nullptr)) return ctx_error(W.ctx);
        clk.add(DEVICE_COPY, t_copy);
        if (verbose2) fprintf(stderr, "[sequence] batch %llu worker %d: host buffer %.3f s, copy %.3f s\n", (unsigned long long)bt.c.seq, bt.wi, seconds(t_copy, t_copy2), seconds(t_copy2));
        bt.fin.bytes[k] = bytes;
        return true;
    }
    // ... as gzip members in W.packed[k]: 16 MB pieces, compressed side by side (level 1), concatenated in order
    bool compress(Batch& bt, int k, uint64_t bytes) {
        Worker& W = bt.W;
        const size_t piece = 16u << 20, np = (size_t)((bytes + piece - 1) / piece);
        std::vector<std::vector<uint8_t>> parts(np);
        std::vector<char> okp(np, 0);
        std::vector<std::thread> zt;
        std::atomic<size_t> nextp{0};
        auto zwork = [&]() { for (size_t q; (q = nextp++) < np;) okp[q] = gzip_member(W.host[k] + q * piece, (size_t)std::min<uint64_t>(piece, bytes - q * piece), parts[q]); };
        for (size_t q = 0; q < std::min<size_t>(np, 6); q++) zt.emplace_back(zwork);
        for (auto& t : zt) t.join();
        size_t total = 0;
        for (size_t q = 0; q < np; q++) { if (!okp[q]) { set_error("gzip compression failed"); return false; } total += parts[q].size(); }
        W.packed[k].resize(total);
        size_t at = 0;
        for (size_t q = 0; q < np; q++) { memcpy(W.packed[k].data() + at, parts[q].data(), parts[q].size()); at += parts[q].size(); }
        bt.fin.bytes[k] = total;
        return true;
    }
    // a regular .gz file: the worker writes its members at their place
    bool emit_host_gzip_at(Batch& bt, int k, uint64_t bytes) {
        if (!download(bt, k, bytes) || !compress(bt, k, bytes)) return false;
        uint64_t off = 0;
        if (!order.take_place(k, bt.c.seq, bt.fin.bytes[k], bt.n, off)) return false;
        const auto t_write = Clock::now();
        const bool wok = out.w[k].write_at(bt.W.packed[k].data(), bt.fin.bytes[k], off);
        clk.add(WRITE, t_write);
        if (!wok) set_error("write failed");
        return wok;
    }
    // whole-batch host buffers for the ordered writer, once it has written this worker's previous batch
    bool emit_host_ordered(Batch& bt, int k, uint64_t bytes) {
        const auto t_wait = Clock::now();
        if (!bt.waited) { order.wait_host_free(bt.wi); bt.waited = true; }
        clk.add(WAIT_FOR_WRITER, t_wait);
        return download(bt, k, bytes) && (!out.w[k].gz || compress(bt, k, bytes));
    }
    void work(int wi) {
        Worker& W = *dev.workers[(size_t)wi];
        GroupQueue& g = *groups[(size_t)(wi / dev.per_group)];
        Parsed c;
        while (g.q.pop(c)) {
            if (failed()) { tksmseq_batch_free(W.ctx, c.b); continue; }
            Batch bt{W, wi, c};
            tksmseq_batch_info(c.b, &bt.n, nullptr, nullptr);
            bt.fin.worker = wi; bt.fin.n_reads = bt.n;
            bool ok = bt.n == c.n_reads;
            if (!ok) set_error("internal: the reader and the parser disagree on the number of reads of a batch");
            const bool both = out.route[0] != Route::None && out.route[1] != Route::None;
            if (ok && bt.n) {
                if (out.route[0] != Route::None) ok = emit(bt, 0, TKSMSEQ_MODE_BADREAD, 0);
                if (ok && out.route[1] != Route::None) ok = both ? emit(bt, 1, TKSMSEQ_MODE_BADREAD, 1) : emit(bt, 1, TKSMSEQ_MODE_PERFECT, 0);
            } else if (ok) ok = emit_empty(bt, 0) && emit_empty(bt, 1);
            tksmseq_batch_free(W.ctx, c.b);
            if (ok && out.ordered()) order.finished(c.seq, bt.fin);
        }
    }
    // the one ordered writer: the finished batches' host buffers, in batch order
    void write_ordered() {
        tkmod::Finished fin;
        for (uint64_t next = 0; order.next_finished(next, fin); next++) {
            Worker& W = *dev.workers[(size_t)fin.worker];
            bool ok = true;
            const auto t_write = Clock::now();
            for (int k = 0; k < 2 && ok; k++)
                if (fin.bytes[k]) ok = out.w[k].write(out.w[k].gz ? W.packed[k].data() : W.host[k], fin.bytes[k]);
            clk.add(WRITE, t_write);
            order.written(fin, ok);
            if (!ok) { set_error("write failed"); return; }
        }
    }
    // a writer thread per worker takes the staged batches in order, copies them to the host in pieces (two page-locked pieces: the
    // copy of one under the write of the other) and writes them: at their place in a regular file, in its turn into anything else
    void write_behind(int wi) {
        Worker& W = *dev.workers[(size_t)wi];
        for (;;) {
            Worker::Job j;
            {
                std::unique_lock<std::mutex> l(W.m);
                W.cv.wait(l, [&] { return !W.jobs.empty() || W.jobs_closed; });
                if (W.jobs.empty()) return;
                j = W.jobs.front(); W.jobs.pop_front();
            }
            Writer& wr = out.w[j.k];
            bool ok = !failed() && W.ring_ready();
            if (!ok && !failed()) set_error("out of page-locked host memory");
            const uint64_t np = (j.bytes + W.piece - 1) / W.piece;
            auto piece_bytes = [&](uint64_t q) { return std::min<uint64_t>(W.piece, j.bytes - q * W.piece); };
            const uint8_t* src = (const uint8_t*)W.stage[j.stage];
            if (ok && np && tksmseq_copy_to_host(W.wctx, W.ring[0], src, piece_bytes(0), 1)) ok = ctx_error(W.wctx);
            if (ok && !wr.positional) ok = order.wait_turn(j.k, j.seq);
            for (uint64_t q = 0; q < np && ok; q++) {
                const auto t_d2h = Clock::now();
                const bool sync_failed = tksmseq_synchronize(W.wctx) != 0;
                clk.add(D2H_WAIT, t_d2h);
                bytes_d2h += piece_bytes(q);
                if (sync_failed) { ok = ctx_error(W.wctx); break; }
                if (q + 1 < np && tksmseq_copy_to_host(W.wctx, W.ring[(q + 1) & 1], src + (q + 1) * W.piece, piece_bytes(q + 1), 1)) { ok = ctx_error(W.wctx); break; }
                const auto t_write = Clock::now();
                const bool wok = wr.positional ? wr.write_at(W.ring[q & 1], piece_bytes(q), j.off + q * W.piece) : wr.write(W.ring[q & 1], piece_bytes(q));
                clk.add(WRITE, t_write);
                if (!wok) { (void)tksmseq_synchronize(W.wctx); set_error("write failed"); ok = false; }
            }
            if (!wr.positional) order.turn_done(j.k, ok);
            { std::lock_guard<std::mutex> l(W.m); W.stage_busy[j.stage] = false; }
            W.cv.notify_all();
        }
    }

    // ---- the run ------------------------------------------------------------------------------------------------------------------
    // start threads -> feed -> join; the batch count of the run
    uint64_t run() {
        std::vector<std::thread> workers, parsers, writers;
        if (!out.ordered())
            for (int w = 0; w < dev.n_workers; w++) {
                Worker& W = *dev.workers[(size_t)w];
                if (tksmseq_clone(W.ctx, &W.wctx)) { set_error(std::string("writer context: ") + tksmseq_last_error(W.ctx)); break; }
                writers.emplace_back(&Stream::write_behind, this, w);
            }
        for (int w = 0; w < dev.n_workers; w++) workers.emplace_back(&Stream::work, this, w);
        for (int pi = 0; pi < dev.n_groups * Devices::parsers_per_group; pi++) parsers.emplace_back(&Stream::parse_ahead, this, pi);
        std::thread writer;
        if (out.ordered()) writer = std::thread(&Stream::write_ordered, this);

        (this->*feed())();
        chunks.close();
        for (auto& t : parsers) t.join();
        order.end(seq);
        for (auto& g : groups) g->q.close();                                                       // (the workers take what is still queued)
        for (auto& t : workers) t.join();
        for (auto& W : dev.workers) { { std::lock_guard<std::mutex> l(W->m); W->jobs_closed = true; } W->cv.notify_all(); }
        for (auto& t : writers) t.join();
        if (writer.joinable()) writer.join();
        return seq;
    }
    // the stats file, the verbose summary, the outputs' last bytes; the exit code
    int report(uint64_t n_batches, Clock::time_point t_begin, Ending& end) {
        if (!out.ordered() && !failed()) for (int k = 0; k < 2; k++) out.w[k].wrote = out.w[k].wrote || order.bytes(k) != 0;
        int status = failed() ? 1 : 0;
        if (status) fprintf(stderr, "Error: %s\n", first_error.c_str());
        const double t_stream = since_start();                   // first chunk read -> last record byte written
        const uint64_t total_reads = order.reads(), out_bytes = order.bytes(0) + order.bytes(1);
        const int n_parsers = dev.n_groups * Devices::parsers_per_group;
        if (const char* sf = getenv("TKSMSEQ_STATS_FILE")) {
            // machine-readable stage clocks of this run (bench.py's end-to-end leg): seconds are summed over the threads of a stage
            if (FILE* f = fopen(sf, "w")) {
                fprintf(f, "{\"reads\": %llu, \"batches\": %llu, \"workers\": %d, \"parsers\": %d, \"parse_threads\": %d, \"mdf_bytes\": %llu, "
                           "\"record_bytes\": %llu, \"d2h_bytes\": %llu, \"setup_s\": %.4f, \"stream_s\": %.4f, ",
                        (unsigned long long)total_reads, (unsigned long long)n_batches, dev.n_workers, n_parsers, a.threads, (unsigned long long)bytes_in.load(),
                        (unsigned long long)out_bytes, (unsigned long long)bytes_d2h.load(), seconds(t_begin, t_start), t_stream);
                for (int k = 0; k < N_STAGES; k++) fprintf(f, "\"%s\": %.4f, ", STAGE_KEY[k], clk.s[k]);
                fprintf(f, "\"written_behind\": %s, \"positional\": %s, \"status\": %d}\n", out.behind ? "true" : "false", out.positional ? "true" : "false", status);
                fclose(f);
            }
        }
        if (verbose)
            fprintf(stderr, "[sequence] %d batches, %d in flight, %.2f s streaming: parse %.2f, run %.2f, copy %.2f, wait for writer %.2f "
                            "(summed over workers); waiting for device-to-host pieces %.2f, write %.2f (summed over writers); read + count %.2f\n", (int)n_batches, dev.n_workers,
                    t_stream, clk.s[PARSE], clk.s[RUN], clk.s[DEVICE_COPY], clk.s[WAIT_FOR_WRITER], clk.s[D2H_WAIT], clk.s[WRITE], clk.s[READ_COUNT]);
        end.verbose = verbose; end.t_close = Clock::now();
        if ((!out.w[0].close() || !out.w[1].close()) && !status) { status = 1; fprintf(stderr, "Error: write failed\n"); }
        end.t_closed = Clock::now();
        if (!status) log.log(Logger::INFO, "Sequencing: %llu reads, %llu record bytes, %.2f s streaming (%.2f M reads/s)", (unsigned long long)total_reads,
                             (unsigned long long)out_bytes, t_stream, t_stream > 0 ? total_reads / t_stream / 1e6 : 0.0);
        return status;
    }
};

}  // namespace

class Sequencer_module::impl {
    int argc; char** argv;
    Args a;
    Logger log;
    enum { GO_ON = -1 };

    int parse() {
        std::vector<std::string> t; std::vector<char> glued;
        if (int rc = normalise_args(argc, argv, t, glued)) return rc;
        for (size_t i = 1; i < t.size(); i++) {
            const Option* o = find_option(t[i]);
            if (!o) return usage_error("unrecognized arguments: %s", t[i].c_str());
            if (!o->set) {                                                // -r/--references, nargs="+"
                if (i + 1 < t.size() && glued[i + 1]) a.references.push_back(t[++i]);
                else while (i + 1 < t.size() && t[i + 1][0] != '-') a.references.push_back(t[++i]);
                if (a.references.empty()) return usage_error("argument -r/--references: expected at least one argument");
                continue;
            }
            if (o->takes_value && i + 1 >= t.size()) return usage_error("argument %s: expected one argument", t[i].c_str());
            const std::string bad = o->set(a, o->takes_value ? t[++i].c_str() : nullptr);
            if (!bad.empty()) return usage_error("argument %s: %s", display_name(*o).c_str(), bad.c_str());
        }
        return 0;
    }

    // --badread-identity MEAN,MAX,STDEV (py/sequence.py:134-164)
    int validate_identity() {
        double idv[3] = {0, 0, 0}; int nid = 0; bool bad = false;
        for (size_t p = 0; p <= a.identity.size(); nid++) {
            size_t q = a.identity.find(',', p);
            if (q == std::string::npos) q = a.identity.size();
            const std::string t = a.identity.substr(p, q - p);
            char* e = nullptr;
            const double v = strtod(t.c_str(), &e);
            if (t.empty() || *e) bad = true;
            if (nid < 3) idv[nid] = v;
            p = q + 1;
        }
        if (bad) return die("Error: could not parse --identity values");
        if (nid != 3) return die("AssertionError: Must specify 3 values for --badread-identity");
        a.mean = idv[0]; a.maxi = idv[1]; a.sd = idv[2];
        if (a.mean > 100.0) return die("Error: mean read identity cannot be more than 100");
        if (a.maxi > 100.0) return die("Error: max read identity cannot be more than 100");
        if (a.mean <= 50) return die("Error: mean read identity must be at least 50");
        if (a.maxi <= 50) return die("Error: max read identity must be at least 50");
        if (a.mean > a.maxi) { char b[200]; snprintf(b, sizeof b, "Error: mean identity (%g) cannot be larger than max identity (%g)", a.mean, a.maxi); return die(b); }
        if (a.sd < 0.0) return die("Error: read identity stdev cannot be negative");
        return GO_ON;
    }
    // the chained stages' own argument checks (src/pcr.cpp:148-185, src/truncate.cpp:278-300; validate_arguments, src/random_wgs.cpp:95-127)
    int validate_chained() {
        int missing = 0;
        auto require = [&](bool have, const char* text) { if (!have) { fprintf(stderr, "%s\n", text); missing++; } };
        if (a.pcr_on) {
            require(a.pcr_have_count, "molecule-count is required!");
            require(a.pcr_have_cycles, "cycles is required!");
            if (!a.pcr_preset.empty()) {
                double er = 0, ef = 0;
                if (tksmseq_pcr_preset(a.pcr_preset.c_str(), &er, &ef)) { fprintf(stderr, "Preset %s not found\n", a.pcr_preset.c_str()); missing++; }
                else { if (!a.pcr_have_er) a.pcr.error_rate = er; if (!a.pcr_have_ef) a.pcr.efficiency = ef; }
            } else {
                require(a.pcr_have_er, "Error rate is required!");
                require(a.pcr_have_ef, "Efficiency is required!");
            }
            if (missing) return 1;
            a.pcr.seed = (uint64_t)a.seed;
        }
        if (a.wgs_on) {
            require(!a.references.empty(), "reference is required!");
            require(a.wgs_have_dist, "frag-len-dist is required!");
            if (missing) return 1;
            if (!a.wgs_have_bc && !a.wgs_have_depth) return die("Either base-count or depth is required!");
            int dist = 0;
            const int bad_dist = tkmod::parse_frag_len_dist(a.wgs_dist, dist, a.wgs.a, a.wgs.b);
            if (bad_dist) return die(bad_dist == 1 ? "Invalid fragment length distribution" : "Invalid fragment length distribution parameters");
            a.wgs.dist = dist; a.wgs.seed = (uint64_t)a.seed;
        }
        if (a.tsb_on) {
            // validate_arguments (src/transcribe.cpp:90-108), process_file_weights (:65-77); the tables are read here, before any device
            require(!a.tsb_gtfs.empty(), "Missing mandatory parameter gtf");
            require(!a.tsb_abundances.empty(), "Missing mandatory parameter abundance");
            require(a.tsb_have_count, "Missing mandatory parameter molecule-count");
            if (missing) return 1;
            if (a.tsb_weights.empty()) a.tsb_weights.push_back(1.0);
            const size_t nf = a.tsb_abundances.size();
            if (a.tsb_weights.size() != 1 && a.tsb_weights.size() != nf) return die("Error: --transcribe-weights takes one weight, or one per abundance file");
            a.tsb_w.assign(nf, a.tsb_weights[0] / (double)nf);
            if (a.tsb_weights.size() > 1) { double sum = 0.0; for (double w : a.tsb_weights) sum += w; for (size_t i = 0; i < nf; i++) a.tsb_w[i] = a.tsb_weights[i] / sum; }
            for (auto& g : a.tsb_gtfs) { FILE* f = fopen(g.c_str(), "rb"); if (!f) return die("Could not open GTF file " + g + "!"); fclose(f); }
            for (auto& t : a.tsb_abundances) {
                FILE* f = fopen(t.c_str(), "rb");
                if (!f) return die("Could not open abundance file " + t + "!");
                a.tsb_texts.emplace_back();
                char buf[1 << 16];
                for (size_t n; (n = fread(buf, 1, sizeof buf, f)) > 0;) a.tsb_texts.back().append(buf, n);
                fclose(f);
            }
        }
        if (a.gzip != "host" && a.gzip != "device") return die("Error: --gzip must be 'host' or 'device', got '" + a.gzip + "'");
        if (a.trc_n > 1) return die("Only one of kde-model, normal or lognormal is allowed!");
        if (a.trc_n == 1) { a.trc.seed = (uint64_t)a.seed; if (a.trc.mode == TKSMSEQ_TRC_KDE) a.trc.kde_model_path = a.trc_kde.c_str(); }
        return GO_ON;
    }
    // everything between the command line and the first device call: the exit code, or GO_ON
    int validate() {
        if (a.help) { usage(stdout); return 0; }
        if (a.list) { for (const Option& o : OPTIONS) if (o.dest) printf("%s\n", o.dest); return 0; }
        a.pcr_on = a.pcr_have_cycles || a.pcr_have_count || a.pcr_have_er || a.pcr_have_ef || !a.pcr_preset.empty();
        a.wgs_on = a.wgs_on || a.wgs_have_dist || a.wgs_have_bc || a.wgs_have_depth;
        if (a.wgs_on && !a.input.empty()) return usage_error("argument -i/--input: not allowed with the --wgs-* options (the molecules are made on the device)");
        if (a.wgs_on && (a.pcr_on || a.trc_n)) return usage_error("the --wgs-* options cannot be combined with --pcr-* / --truncate-*");
        if (a.tsb_on && !a.input.empty()) return usage_error("argument -i/--input: not allowed with the --transcribe-* options (the molecules are made on the device)");
        if (a.tsb_on && a.wgs_on) return usage_error("the --transcribe-* options cannot be combined with --wgs-*");
        if (a.tsb_on && (a.pcr_on || a.trc_n)) return usage_error("the --transcribe-* options cannot be combined with --pcr-* / --truncate-*");
        if (a.input.empty() && !a.wgs_on && !a.tsb_on) return usage_error("the following arguments are required: -i/--input");
        if (int rc = validate_identity(); rc != GO_ON) return rc;
        if (a.badread.empty() && a.perfect.empty()) return usage_error("Must specify either --output or --perfect.");
        if (int rc = validate_chained(); rc != GO_ON) return rc;
        // utility flags (src/module.h:106-125)
        const int lv = Logger::parse(a.verbosity);
        if (lv < 0) return die("Error: unknown verbosity level '" + a.verbosity + "' (choose from DEBUG, INFO, WARN, ERROR, OFF)");
        log.level = lv;
        if (!log.open(a.log_file)) return die("Error: cannot open log file " + a.log_file);
        // $TKSM_MODELS handling of the shim (src/sequence.cpp:38-52) happens in the library's model lookup: the built-in model
        // directory comes first, then the entries of $TKSM_MODELS in order.  Default models: nanopore2020 if it can be found,
        // else `random` (py/sequence.py:86-107).
        if (const char* env = getenv("TKSM_MODELS")) log.log(Logger::DEBUG, "TKSM_MODELS was set to %s; the built-in model directory is searched first", env);
        else log.log(Logger::DEBUG, "TKSM_MODELS not set: built-in model directory only");
        if (a.error_model.empty()) a.error_model = tksmseq_model_available("nanopore2020", "error") ? "nanopore2020" : "random";
        if (a.qscore_model.empty()) a.qscore_model = tksmseq_model_available("nanopore2020", "qscore") ? "nanopore2020" : "random";
        if (a.threads < 1) a.threads = 1;
        return GO_ON;
    }

    // set up devices -> open input and outputs -> stream -> report; returns with the devices released
    int sequence(Clock::time_point t_begin, Ending& end) {
        // the output NAMES decide what is computed (py/sequence.py:349-353); the files are created once the devices, references, models
        // and the input have turned out usable (a run that fails before that leaves no empty output behind)
        Sinks out;
        if (!a.badread.empty()) out.w[0].classify(a.badread);
        const bool compute_q = !a.badread.empty() && !a.skip_qual && out.w[0].fastq;
        if (!a.badread.empty() && !a.perfect.empty())
            log.log(Logger::WARN, "with both -o and --perfect the reference writes the badread sequence (quals 'K') to the "
                                  "--perfect file (py/sequence.py:317-319); reproduced here");
        // a hardware queue per stream in flight: with the runtime's default of 4 the main streams of several contexts share queues,
        // and kernels of different batches that could run side by side run one after the other (tools/calib/hwq_check.hip).  Read
        // when the runtime starts, i.e. at the first device call below; a value set by the user wins.
        setenv("GPU_MAX_HW_QUEUES", "16", 0);
        Devices dev(a, compute_q);
        if (!dev.error.empty()) return die(dev.error);
        log.log(Logger::INFO, "%d device group(s) x %d contexts in flight, %d parser(s) per group with %d host thread(s) each", dev.n_groups, dev.per_group,
                Devices::parsers_per_group, a.threads);
        if (a.wgs_on) {
            uint64_t ref_length = 0;
            tksmseq_reference_info(dev.first(0).ctx, nullptr, &ref_length, nullptr);
            a.wgs.base_count = a.wgs_have_bc ? (int64_t)a.wgs_base_count : (int64_t)(a.wgs_depth * (double)ref_length);      // src/random_wgs.cpp:169-176
            log.log(Logger::INFO, "Reference length: %llu; whole-genome fragments for %lld bases", (unsigned long long)ref_length, (long long)a.wgs.base_count);
        }
        Input in;
        for (auto& id : dev.tsb_missing) log.log(Logger::WARN, "Isoform %s is not found in the input GTFs!", id.c_str());
        if (!a.wgs_on && !a.tsb_on && !in.open(a.input)) return die("Error: cannot open " + a.input);
        std::string unopened;
        if (!out.open(a, unopened)) return die("Error: cannot open " + unopened);
        Stream s(a, log, dev, out, in, compute_q);
        if (s.verbose) fprintf(stderr, "[sequence] device, reference and models ready after %.2f s\n", seconds(t_begin, s.t_start));
        const uint64_t n_batches = s.run();
        return s.report(n_batches, t_begin, end);
    }

public:
    impl(int argc, char** argv) : argc(argc), argv(argv) {}

    int run() {
        if (int rc = parse()) return rc;
        if (int rc = validate(); rc != GO_ON) return rc;
        const auto t_begin = Clock::now();
        Ending end;
        const int status = sequence(t_begin, end);
        if (end.verbose) fprintf(stderr, "[sequence] closing the outputs %.2f s, releasing the device %.2f s\n", seconds(end.t_close, end.t_closed), seconds(end.t_closed));
        return status;
    }
};

Sequencer_module::Sequencer_module(int argc, char** argv) : pimpl{std::make_unique<impl>(argc, argv)} {}
Sequencer_module::~Sequencer_module() = default;
int Sequencer_module::run() { return pimpl->run(); }

extern "C" int tksmseq_sequence_main(int argc, char** argv) { return Sequencer_module{argc, argv}.run(); }
