// mdf_modules.cpp -- the `tksm pcr`, `truncate`, `polyA`, `tag`, `scb`, `flip`, `tail-noise`, `filter` (two outputs), `unsegment` and `shuffle` modules on top of the
// C-ABI (MDF file in, MDF file out), and `random-wgs` (no input: MDF file out).
//
// Mirrors (file:line into vpc-ccg/tksm):
//   PCR_module::impl        src/pcr.cpp:91-260       flags -i -o --molecule-count --cycles --error-rate --efficiency -x/--preset,
//                                                    mandatory-argument and preset checks; the whole input is held (:215: the drop
//                                                    ratio needs the number of templates), the output is streamed
//   Truncate_module::impl   src/truncate.cpp:236-451 flags -i -o --kde-model --always-end --kde-models-length --normal --lognormal,
//                                                    "exactly one of kde-model, normal or lognormal"; a stream transform (:322-351)
//   PolyA_module            src/polyA.cpp:17-237     --gamma / --poisson / --weibull / --normal, --min-length, --max-length
//   TAG_module              src/tag.cpp:16-129       -5/--format5, -3/--format3 (a leading digit: that many N's)
//   SingleCellBarcoder      src/scb.cpp:14-92        --keep-meta-barcodes
//   StrandMan_module        src/strand_man.cpp:20-124 -p/--flip-probability (outside [0, 1]: logged, not refused)
//   RWGS_module             src/random_wgs.cpp:24-229 -r/--reference, --frag-len-dist "NAME A [B]", -o, --base-count | --depth
//   AppendNoise_module      src/append_noise.cpp:131-229 --length-dist NAME,MU,SIGMA, --alphabet, --palindromic, --error-rate
//   Filter_module           src/filter.cpp:119-231   -i, -t/--true-output, -f/--false-output, -c/--condition (comma-separated, repeatable), --negate
//   Unsegment_module        src/unsegment.cpp:22-116 -i, -o, -p/--probability ("<name> is required!", the help, exit 1)
//   Shuffle_module          src/shuffle.cpp:22-125   -i, -o, --buffer-size (long only); the whole input is one batch
//   Mutate_module           src/mutate.cpp:182-233   -i, -o, -t/--tsv ("<name> is required!", the help, exit 1); the table is checked before any context
//   Splicer_module          src/transcribe.cpp:19-218 -g/--gtf, -a/--abundance, --molecule-count, -w/--weights, ... (no fusion submodule): GTF + TSV in, MDF out
//   utility flags           src/module.h:75-104      -s/--seed (default 42), --verbosity, --log-file, -h (module_cli.h: shared with the tools of tool_modules.cpp)
// All stream: `truncate` and the four segment edits read the input in batches of whole molecules (--batch-bytes), `pcr` amplifies its templates in slices
// of about --slice-molecules output molecules (tksmseq_pcr_params::template_begin / _end); the pieces go round the entries of
// --devices D[,D...] (two contexts per entry: one formats its text while the other computes) and are written in input order, so the
// output does not depend on the device list or the piece size.
// Exit codes as the reference's run(): 0 ok (also for --help), 1 for missing / inconsistent arguments and runtime errors.
#include <deque>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <algorithm>
#include <cctype>
#include <cmath>
#include <vector>

#include "../../include/tksmseq.h"
#include "abund_host.h"
#include "filter_host.h"
#include "glue_cut.h"
#include "host.h"
#include "module_cli.h"
#include "module_log.h"
#include "sequencer_module.h"

using namespace tkmod;

namespace {

bool read_file(const std::string& path, std::string& out) {
    FILE* f = fopen(path.c_str(), "rb");
    if (!f) return false;
    char buf[1 << 16];
    size_t n;
    while ((n = fread(buf, 1, sizeof buf, f)) > 0) out.append(buf, n);
    fclose(f);
    return true;
}

// returns 1 if the flag was one of the common ones (i advanced), 0 if not, -1 on a missing / malformed value
int common_flag(int argc, char** argv, int& i, Common& c) {
    const std::string o = argv[i];
    auto val = [&]() -> const char* { return i + 1 < argc ? argv[++i] : nullptr; };
    const char* v = nullptr;
    if (o == "-h" || o == "--help") { c.help = true; return 1; }
    if (o == "-i" || o == "--input") { if (!(v = val())) return -1; c.input = v; return 1; }
    if (o == "-o" || o == "--output") { if (!(v = val())) return -1; c.output = v; return 1; }
    if (o == "-s" || o == "--seed") { if (!(v = val())) return -1; c.seed = atoll(v); return 1; }
    if (o == "--devices") { if (!(v = val()) || !tkmod::parse_device_list(v, c.devices)) return -1; return 1; }
    if (o == "--verbosity") { if (!(v = val())) return -1; c.verbosity = v; return 1; }
    if (o == "--log-file") { if (!(v = val())) return -1; c.log_file = v; return 1; }
    if (o == "--batch-bytes") { if (!(v = val()) || strtoull(v, nullptr, 10) < 1) return -1; c.batch_bytes = strtoull(v, nullptr, 10); return 1; }
    if (o == "--slice-molecules") { if (!(v = val()) || strtoull(v, nullptr, 10) < 1) return -1; c.slice_molecules = strtoull(v, nullptr, 10); return 1; }
    return 0;
}

}  // namespace

// (module_cli.h)
bool tkmod::parse_args(int argc0, char** argv0, Common& c, const std::function<int(const std::string&, const char*)>& own) {
    std::vector<std::string> arg_store; std::vector<char*> arg_ptrs;
    tkmod::split_equals(argc0, argv0, arg_store, arg_ptrs);
    const int argc = (int)arg_ptrs.size(); char** const argv = arg_ptrs.data();
    for (int i = 1; i < argc; i++) {
        int k = own(std::string(argv[i]), i + 1 < argc ? argv[i + 1] : nullptr);
        if (k == TOOK_VALUE) i++;
        if (k == NOT_MINE) { const int f = common_flag(argc, argv, i, c); k = f > 0 ? TOOK_FLAG : f < 0 ? MALFORMED : NO_SUCH; }   // (advances i itself)
        if (k == MALFORMED) fprintf(stderr, "Option '%s' is missing an argument or has a malformed one\n", argv[i]);
        if (k == NO_SUCH) fprintf(stderr, "Option '%s' does not exist or is missing an argument\n", argv[i]);
        if (k < 0) return false;
    }
    return true;
}

bool tkmod::open_log(const Common& c, const char* module, Logger& log) {
    log.module = module;
    const int lv = Logger::parse(c.verbosity);
    if (lv < 0) { fprintf(stderr, "Error: unknown verbosity level '%s' (choose from DEBUG, INFO, WARN, ERROR, OFF)\n", c.verbosity.c_str()); return false; }
    log.level = lv;
    if (!log.open(c.log_file)) { fprintf(stderr, "Error: cannot open log file %s\n", c.log_file.c_str()); return false; }
    return true;
}

namespace {

// pieces of output text, written in the order of their numbers whatever the order in which they are finished
struct OrderedOut {
    FILE* f = nullptr; std::mutex m; std::condition_variable cv; uint64_t next = 0; bool failed = false;
    bool put(uint64_t k, const char* text, uint64_t len) {
        std::unique_lock<std::mutex> l(m);
        cv.wait(l, [&] { return next == k || failed; });
        if (failed) return false;
        if (len && fwrite(text, 1, len, f) != len) failed = true;
        next++;
        cv.notify_all();
        return !failed;
    }
    void fail() { std::lock_guard<std::mutex> l(m); failed = true; cv.notify_all(); }
};

// truncate: text + first molecule index; pcr: template slice; error: set by a work() that fails for a reason of its own (not the library's)
// second: filter's false side, written to the second output (null: nothing for it)
struct Piece { uint64_t seq = 0, first = 0, begin = 0, end = 0; std::vector<char> text; std::string error; tksmseq_batch* second = nullptr; };

// The common engine: `n_ctx` worker threads (two per entry of --devices), each with a context of its own; prepare() runs once per
// context (pcr: parse the templates), pieces come from next_piece() (serialised), work() turns one into a batch, whose MDF text is
// written in piece order.  serial_work: work() runs under next_piece()'s lock as well (random-wgs: a batch starts where the one before it
// ended; only the text is made in parallel).  summary(): what the closing log line says between the molecule count and the time.
template <class Prepare, class Next, class Work>
int run_pieces(const Common& c, Logger& log, const char* what, Prepare prepare, Next next_piece, Work work, bool serial_work = false,
               std::function<std::string()> summary = nullptr, const std::string* second_output = nullptr) {
    OrderedOut out, out2;                                       // out2: the second ordered sink (filter's false side), same piece numbers
    out.f = fopen(c.output.c_str(), "wb");
    if (!out.f) { fprintf(stderr, "Error: cannot write %s\n", c.output.c_str()); return 1; }
    if (second_output && !(out2.f = fopen(second_output->c_str(), "wb"))) { fprintf(stderr, "Error: cannot write %s\n", second_output->c_str()); fclose(out.f); return 1; }
    const int per_device = 2, n_ctx = (int)c.devices.size() * per_device;
    std::mutex err_m, next_m; std::string first_error; std::atomic<bool> failed{false};
    auto set_error = [&](const std::string& e) { std::lock_guard<std::mutex> l(err_m); if (!failed.exchange(true)) first_error = e; out.fail(); out2.fail(); };
    std::atomic<uint64_t> molecules{0};
    const auto t0 = std::chrono::steady_clock::now();
    auto worker = [&](int wi) {
        tksmseq_ctx* ctx = nullptr;
        if (tksmseq_create(c.devices[(size_t)(wi / per_device)], &ctx)) { set_error(tksmseq_last_error(nullptr)); return; }
        // host threads for the MDF parser and writer (the reference's modules are single-threaded; results do not depend on it)
        tksmseq_set_host_threads(ctx, (int)std::max(1u, std::min(8u, std::thread::hardware_concurrency() / (unsigned)std::max(1, n_ctx / 2))));
        void* state = nullptr;
        if (!prepare(ctx, &state)) set_error(tksmseq_last_error(ctx));
        while (!failed) {
            Piece p;
            tksmseq_batch* b = nullptr;
            char* text = nullptr; uint64_t len = 0;
            int rc;
            {
                std::unique_lock<std::mutex> l(next_m);
                if (failed || !next_piece(p)) break;
                if (!serial_work) l.unlock();
                rc = work(ctx, state, p, &b);
            }
            if (!rc) rc = tksmseq_batch_to_mdf_text(ctx, b, &text, &len);
            if (rc) set_error(std::string(what) + ": " + (p.error.empty() ? tksmseq_last_error(ctx) : p.error.c_str()));
            else {
                uint64_t n = 0;
                tksmseq_batch_info(b, &n, nullptr, nullptr);
                molecules += n;
                log.log(Logger::DEBUG, "piece %llu: %llu molecules, %.1f MB of text (context %d)", (unsigned long long)p.seq, (unsigned long long)n, len / 1e6, wi);
                if (!out.put(p.seq, text, len) && !failed) set_error("cannot write " + c.output);
                if (out2.f && !failed) {
                    char* text2 = nullptr; uint64_t len2 = 0;
                    if (p.second && tksmseq_batch_to_mdf_text(ctx, p.second, &text2, &len2)) set_error(std::string(what) + ": " + tksmseq_last_error(ctx));
                    else if (!out2.put(p.seq, text2, len2) && !failed) set_error("cannot write " + *second_output);
                    tksmseq_text_free(text2);
                }
            }
            tksmseq_text_free(text);
            if (b) tksmseq_batch_free(ctx, b);
            if (p.second) tksmseq_batch_free(ctx, p.second);
        }
        if (state) prepare(ctx, &state);                        // (second call: releases what the first one made)
        tksmseq_destroy(ctx);
    };
    std::vector<std::thread> th;
    for (int w = 0; w < n_ctx; w++) th.emplace_back(worker, w);
    for (auto& t : th) t.join();
    bool close_ok = fclose(out.f) == 0;
    if (out2.f && fclose(out2.f) != 0) close_ok = false;
    if (failed) { fprintf(stderr, "Error: %s\n", first_error.c_str()); return 1; }
    if (!close_ok || out.failed || out2.failed) { fprintf(stderr, "Error: cannot write %s\n", c.output.c_str()); return 1; }
    log.log(Logger::INFO, "%s: %llu molecules%s written in %.2f s (%d device group(s))", what, (unsigned long long)molecules.load(), summary ? summary().c_str() : "",
            std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(), (int)c.devices.size());
    return 0;
}

// The input in pieces of whole molecules, on_batch(ctx, batch, piece, out) on each (piece.first: the index of its first molecule in the whole
// input; piece.second: a second output batch for second_output), and the outputs written in input order.
// joins (unsegment): a piece ends only in front of a record whose first molecule g has joins(g) == 0 (glue_cut.h) -- the reader holds the text
// behind the last such record back and puts it in front of the next chunk, and reads on while a chunk has none.
template <class OnBatch>
int stream_batches(const Common& c, Logger& log, const char* what, OnBatch on_batch, const std::string* second_output = nullptr,
                   std::function<bool(uint64_t)> joins = nullptr) {
    // a reader thread of its own cuts the input into pieces of whole molecules and numbers them (input order), a few pieces ahead of the
    // workers: what the engine serialises is a pop from this queue, not the read + scan of a piece.  Its state lives on the heap and is
    // shared with the thread: after an error the module returns without waiting for a reader that may sit in a read() on a pipe nobody
    // closes (the thread is detached and ends with the process).
    struct ReaderState {
        tkmod::ChunkReader rd;
        std::mutex m; std::condition_variable put, get; std::deque<Piece> pieces; bool done = false, stop = false; size_t cap = 3;
    };
    auto rs = std::make_shared<ReaderState>();
    rs->rd.in = fopen(c.input.c_str(), "rb");
    if (!rs->rd.in) { fprintf(stderr, "Could not open file %s\n", c.input.c_str()); return 1; }
    rs->rd.bytes = c.batch_bytes;
    rs->cap = c.devices.size() * 2 + 1;
    std::thread reader([rs, joins]() {
        uint64_t seq = 0, first = 0;
        tkmod::GlueHold hold;                                     // (joins) the text behind the last cut
        std::vector<char> chunk;
        for (;;) {
            Piece pc;
            uint64_t molecules = 0;
            if (joins) {
                if (rs->rd.next(chunk)) { if (!hold.push(chunk, first, joins, pc.text, molecules)) continue; }
                else if (seq && hold.held.empty()) break;
                else hold.flush(pc.text, molecules);              // (an empty input still makes an (empty) output)
            } else {
                if (!rs->rd.next(pc.text)) {
                    if (seq) break;
                    pc.text.clear();                              // an empty input still makes an (empty) output
                }
                molecules = tkmod::count_reads(pc.text.data(), pc.text.size());
            }
            pc.seq = seq++; pc.first = first;
            first += molecules;
            std::unique_lock<std::mutex> l(rs->m);
            rs->put.wait(l, [&] { return rs->pieces.size() < rs->cap || rs->stop; });
            if (rs->stop) break;
            rs->pieces.push_back(std::move(pc));
            rs->get.notify_one();
        }
        { std::lock_guard<std::mutex> l(rs->m); rs->done = true; }
        rs->get.notify_all();
    });
    auto prepare = [&](tksmseq_ctx*, void**) -> bool { return true; };
    auto next_piece = [&](Piece& pc) -> bool {
        std::unique_lock<std::mutex> l(rs->m);
        rs->get.wait(l, [&] { return !rs->pieces.empty() || rs->done; });
        if (rs->pieces.empty()) return false;
        pc = std::move(rs->pieces.front()); rs->pieces.pop_front();
        rs->put.notify_one();
        return true;
    };
    auto work = [&](tksmseq_ctx* ctx, void*, Piece& pc, tksmseq_batch** out) -> int {
        tksmseq_batch* in = nullptr;
        int rc = tksmseq_molecules_from_mdf_text(ctx, pc.text.data(), pc.text.size(), &in);
        if (rc) return rc;
        rc = on_batch(ctx, in, pc, out);
        tksmseq_batch_free(ctx, in);
        return rc;
    };
    const int rc = run_pieces(c, log, what, prepare, next_piece, work, false, nullptr, second_output);
    bool finished;
    { std::lock_guard<std::mutex> l(rs->m); rs->stop = true; finished = rs->done; }      // (an error: the reader may be waiting for room, or for input)
    rs->put.notify_all();
    if (rc == 0 || finished) { reader.join(); fclose(rs->rd.in); }
    else reader.detach();
    return rc;
}

// A stream transform (truncate, polyA, tag, scb, flip, tail-noise): fn(ctx, batch, parameters, out) on each piece -- the parameters are p
// with the index of the piece's first molecule in p.*first_index (null: fn numbers nothing).
template <class P>
int stream_transform(const Common& c, Logger& log, const char* what, const P& p, int (*fn)(tksmseq_ctx*, const tksmseq_batch*, const P*, tksmseq_batch**),
                     uint64_t P::*first_index = &P::first_molecule_index) {
    return stream_batches(c, log, what, [&](tksmseq_ctx* ctx, const tksmseq_batch* in, Piece& pc, tksmseq_batch** out) -> int {
        P q = p;
        if (first_index) q.*first_index = pc.first;
        return fn(ctx, in, &q, out);
    });
}

}  // namespace

extern "C" int tksmseq_pcr_main(int argc, char** argv) {
    Common c;
    bool have_count = false, have_cycles = false, have_er = false, have_ef = false;
    std::string preset;
    tksmseq_pcr_params p{};
    if (!parse_args(argc, argv, c, [&](const std::string& o, const char* v) -> int {
            if (o == "--molecule-count" && v) { p.target_count = strtoull(v, nullptr, 10); have_count = true; }
            else if (o == "--cycles" && v) { p.cycles = atoi(v); have_cycles = true; }
            else if (o == "--error-rate" && v) { p.error_rate = atof(v); have_er = true; }
            else if (o == "--efficiency" && v) { p.efficiency = atof(v); have_ef = true; }
            else if ((o == "-x" || o == "--preset") && v) preset = v;
            else return NOT_MINE;
            return TOOK_VALUE;
        })) return 1;
    if (c.help) { printf("PCR amplification module\nusage: pcr -i INPUT -o OUTPUT --molecule-count N --cycles C [-x PRESET | --error-rate E --efficiency F] [-s SEED]\n"
                         "           [--devices D[,D...]] [--slice-molecules N] [--verbosity L] [--log-file F]\n"); return 0; }
    int missing = 0;
    if (c.input.empty()) { fprintf(stderr, "input is required!\n"); missing++; }
    if (c.output.empty()) { fprintf(stderr, "output is required!\n"); missing++; }
    if (!have_count) { fprintf(stderr, "molecule-count is required!\n"); missing++; }
    if (!have_cycles) { fprintf(stderr, "cycles is required!\n"); missing++; }
    if (!preset.empty()) {
        double er = 0, ef = 0;
        if (tksmseq_pcr_preset(preset.c_str(), &er, &ef)) { fprintf(stderr, "Preset %s not found\n", preset.c_str()); missing++; }
        else { if (!have_er) p.error_rate = er; if (!have_ef) p.efficiency = ef; }       // explicit values override the preset (src/pcr.cpp:205-210)
    } else {
        if (!have_er) { fprintf(stderr, "Error rate is required!\n"); missing++; }
        if (!have_ef) { fprintf(stderr, "Efficiency is required!\n"); missing++; }
    }
    if (missing) return 1;
    Logger log;
    if (!open_log(c, "pcr", log)) return 1;
    p.seed = (uint64_t)c.seed;
    std::string text;
    if (!read_file(c.input, text)) { fprintf(stderr, "Could not open file %s\n", c.input.c_str()); return 1; }
    // the slices of templates: consecutive runs that write about slice_molecules copies each, from the per-template counts
    std::vector<uint64_t> cuts;                                  // template index where slice k begins; cuts.back() = number of templates
    std::mutex cuts_m; bool cuts_done = false, cuts_failed = false; std::condition_variable cuts_cv;
    uint64_t next_slice = 0;
    auto prepare = [&](tksmseq_ctx* ctx, void** state) -> bool {
        if (*state) { tksmseq_batch_free(ctx, (tksmseq_batch*)*state); *state = nullptr; return true; }
        tksmseq_batch* T = nullptr;
        if (tksmseq_molecules_from_mdf_text(ctx, text.data(), text.size(), &T)) return false;
        *state = T;
        bool mine = false;
        { std::lock_guard<std::mutex> l(cuts_m); if (cuts.empty()) { cuts.push_back(0); mine = true; } }
        if (mine) {
            uint64_t n = 0;
            tksmseq_batch_info(T, &n, nullptr, nullptr);
            std::vector<uint64_t> counts(n);
            const bool ok = tksmseq_pcr_template_counts(ctx, T, &p, counts.data()) == 0;
            std::lock_guard<std::mutex> l(cuts_m);
            uint64_t acc = 0, total = 0;
            for (uint64_t u = 0; u < n && ok; u++) { acc += counts[u]; total += counts[u]; if (acc >= c.slice_molecules && u + 1 < n) { cuts.push_back(u + 1); acc = 0; } }
            cuts.push_back(n);
            cuts_done = true; cuts_failed = !ok;
            cuts_cv.notify_all();
            if (ok) log.log(Logger::INFO, "%llu templates -> %llu molecules in %zu slice(s)", (unsigned long long)n, (unsigned long long)total, cuts.size() - 1);
            return ok;
        }
        std::unique_lock<std::mutex> l(cuts_m);
        cuts_cv.wait(l, [&] { return cuts_done; });
        return !cuts_failed;
    };
    auto next_piece = [&](Piece& pc) -> bool {
        std::lock_guard<std::mutex> l(cuts_m);
        if (next_slice + 1 >= cuts.size()) return false;
        pc.seq = next_slice; pc.begin = cuts[next_slice]; pc.end = cuts[next_slice + 1];
        next_slice++;
        return true;
    };
    auto work = [&](tksmseq_ctx* ctx, void* state, const Piece& pc, tksmseq_batch** out) -> int {
        tksmseq_pcr_params q = p;
        q.template_begin = pc.begin; q.template_end = pc.end;
        if (pc.begin == pc.end) { q.template_begin = 0; q.template_end = 0; q.cycles = 0; }     // (an input without molecules: one empty piece)
        return tksmseq_pcr(ctx, (const tksmseq_batch*)state, &q, out);
    };
    return run_pieces(c, log, "PCR", prepare, next_piece, work);
}

extern "C" int tksmseq_truncate_main(int argc, char** argv) {
    Common c;
    tksmseq_trc_params p{};
    std::string kde;
    int n_dist = 0;
    auto two = [](const char* v, double& a, double& b) { char* e = nullptr; a = strtod(v, &e); if (!e || *e != ',') return false; b = strtod(e + 1, &e); return e && !*e; };
    if (!parse_args(argc, argv, c, [&](const std::string& o, const char* v) -> int {
            if (o == "--always-end") { p.always_end = 1; return TOOK_FLAG; }
            if (o == "--kde-models-length") { p.kde_models_length = 1; return TOOK_FLAG; }
            if (o == "--kde-model" && v) kde = v;
            else if ((o == "--normal" || o == "--lognormal") && v) {
                if (!two(v, p.mu, p.sigma)) { fprintf(stderr, "%s needs mu,sigma\n", o.c_str()); return REFUSED; }
                p.mode = o == "--normal" ? TKSMSEQ_TRC_NORMAL : TKSMSEQ_TRC_LOGNORMAL;
            } else return NOT_MINE;
            n_dist++;
            return TOOK_VALUE;
        })) return 1;
    if (c.help) { printf("Truncate module\nusage: truncate -i INPUT -o OUTPUT (--kde-model M.json [--always-end] [--kde-models-length] | --normal MU,SIGMA | --lognormal MU,SIGMA) [-s SEED]\n"
                         "                [--devices D[,D...]] [--batch-bytes B] [--verbosity L] [--log-file F]\n"); return 0; }
    int missing = 0;
    if (c.input.empty()) { fprintf(stderr, "input is required!\n"); missing++; }
    if (c.output.empty()) { fprintf(stderr, "output is required!\n"); missing++; }
    if (n_dist == 0) { fprintf(stderr, "One of kde-model, normal or lognormal is required!\n"); missing++; }
    if (n_dist > 1) { fprintf(stderr, "Only one of kde-model, normal or lognormal is allowed!\n"); missing++; }
    if (missing) return 1;
    Logger log;
    if (!open_log(c, "truncate", log)) return 1;
    if (!kde.empty()) { p.mode = TKSMSEQ_TRC_KDE; p.kde_model_path = kde.c_str(); }
    p.seed = (uint64_t)c.seed;
    return stream_transform(c, log, "truncate", p, tksmseq_truncate);
}

// comma-separated doubles (cxxopts' vector<double>); false on a malformed list
static bool parse_doubles(const char* v, std::vector<double>& out) {
    out.clear();
    const char* q = v;
    for (;;) {
        char* e = nullptr;
        const double d = strtod(q, &e);
        if (e == q || (*e && *e != ',')) return false;
        out.push_back(d);
        if (!*e) return true;
        q = e + 1;
    }
}

extern "C" int tksmseq_polya_main(int argc, char** argv) {
    Common c;
    tksmseq_polya_params p{};
    p.min_length = 0; p.max_length = 5000;
    static const char* names[4] = {"gamma", "poisson", "weibull", "normal"};
    static const char* titles[4] = {"Gamma", "Poisson", "Weibull", "Normal"};
    std::vector<double> vals[4];
    int count[4] = {0, 0, 0, 0};
    if (!parse_args(argc, argv, c, [&](const std::string& o, const char* v) -> int {
            int d = -1;
            for (int q = 0; q < 4; q++) if (o == std::string("--") + names[q]) d = q;
            if (d >= 0 && v) { if (!parse_doubles(v, vals[d])) { fprintf(stderr, "Option '%s' needs a comma-separated list of numbers\n", o.c_str()); return REFUSED; } count[d]++; }
            else if (o == "--min-length" && v) p.min_length = atoi(v);
            else if (o == "--max-length" && v) p.max_length = atoi(v);
            else return NOT_MINE;
            return TOOK_VALUE;
        })) return 1;
    if (c.help) { printf("polyA module: adds polyA tails to molecules with given size distribution\n"
                         "usage: polyA -i INPUT -o OUTPUT (--gamma A,B | --poisson L | --weibull A,B | --normal MU,SIGMA) [--min-length N] [--max-length N]\n"
                         "             [-s SEED] [--devices D[,D...]] [--batch-bytes B] [--verbosity L] [--log-file F]\n"); return 0; }
    // validate_arguments (src/polyA.cpp:61-118)
    int missing = 0;
    if (c.input.empty()) { fprintf(stderr, "Missing parameter: input\n"); missing++; }
    if (c.output.empty()) { fprintf(stderr, "Missing parameter: output\n"); missing++; }
    const int n_dist = (count[0] > 0) + (count[1] > 0) + (count[2] > 0) + (count[3] > 0);
    if (n_dist == 0) { fprintf(stderr, "No distribution specified\n"); missing++; }
    if (n_dist > 1) { fprintf(stderr, "Multiple distributions specified\n"); missing++; }
    for (int q = 0; q < 4; q++) {
        const size_t want = q == 1 ? 1 : 2;
        if (count[q] && vals[q].size() != want) { fprintf(stderr, "%s distribution requires %s\n", titles[q], want == 1 ? "one parameter" : "two parameters"); missing++; }
    }
    if (p.min_length < 0) { fprintf(stderr, "Minimum length of polyA cannot be negative\n"); missing++; }
    if (p.max_length < 0) { fprintf(stderr, "Maximum length of polyA cannot be negative\n"); missing++; }
    if (p.min_length > p.max_length) { fprintf(stderr, "Minimum length of polyA cannot be greater than maximum length of polyA\n"); missing++; }
    if (missing) return 1;
    for (int q = 0; q < 4; q++)
        if (count[q]) { p.dist = q == 0 ? TKSMSEQ_PLA_GAMMA : q == 1 ? TKSMSEQ_PLA_POISSON : q == 2 ? TKSMSEQ_PLA_WEIBULL : TKSMSEQ_PLA_NORMAL; p.a = vals[q][0]; p.b = vals[q].size() > 1 ? vals[q][1] : 0.0; }
    // (parameters the std:: distributions leave undefined: rejected before any work, with the library's message)
    {
        const bool two = p.dist != TKSMSEQ_PLA_POISSON;
        if (!std::isfinite(p.a) || (two && !std::isfinite(p.b)) || (p.dist != TKSMSEQ_PLA_NORMAL && !(p.a > 0.0)) || (two && !(p.b > 0.0))) {
            fprintf(stderr, "Error: %s distribution parameters must be finite and positive (the mean of a normal distribution may be any finite number)\n", titles[p.dist == TKSMSEQ_PLA_GAMMA ? 0 : p.dist == TKSMSEQ_PLA_POISSON ? 1 : p.dist == TKSMSEQ_PLA_WEIBULL ? 2 : 3]);
            return 1;
        }
    }
    Logger log;
    if (!open_log(c, "polyA", log)) return 1;
    p.seed = (uint64_t)c.seed;
    return stream_transform(c, log, "polyA", p, tksmseq_polya);
}

extern "C" int tksmseq_tag_main(int argc, char** argv) {
    Common c;
    std::string fmt[2];
    if (!parse_args(argc, argv, c, [&](const std::string& o, const char* v) -> int {
            if ((o == "-5" || o == "--format5") && v) fmt[0] = v;
            else if ((o == "-3" || o == "--format3") && v) fmt[1] = v;
            else return NOT_MINE;
            return TOOK_VALUE;
        })) return 1;
    if (c.help) { printf("TAGging module\nusage: tag -i INPUT -o OUTPUT [-5 FORMAT5] [-3 FORMAT3] [-s SEED]\n"
                         "           [--devices D[,D...]] [--batch-bytes B] [--verbosity L] [--log-file F]\n"
                         "FORMAT: IUPAC letters (ACGTU RYKMSW BDHV N), or a number of N's\n"); return 0; }
    // validate_arguments (src/tag.cpp:41-63)
    int missing = 0;
    if (c.input.empty()) { fprintf(stderr, "input is required!\n"); missing++; }
    if (c.output.empty()) { fprintf(stderr, "output is required!\n"); missing++; }
    if (fmt[0].empty() && fmt[1].empty()) { fprintf(stderr, "At least one of the TAG formats must be provided\n"); missing++; }
    if (missing) return 1;
    // a format that starts with a digit is that many N's (std::stoi, src/tag.cpp:84-91)
    for (auto& f : fmt)
        if (!f.empty() && isdigit((unsigned char)f[0])) {
            const long long len = strtoll(f.c_str(), nullptr, 10);
            if (len > (1 << 20)) { fprintf(stderr, "Error: tag length %s is not supported (at most 1048576)\n", f.c_str()); return 1; }
            f.assign((size_t)len, 'N');
        }
    Logger log;
    if (!open_log(c, "tag", log)) return 1;
    tksmseq_tag_params p{};
    p.seed = (uint64_t)c.seed; p.format5 = fmt[0].c_str(); p.format3 = fmt[1].c_str();
    return stream_transform(c, log, "tag", p, tksmseq_tag);
}

// cxxopts' boolean: --flag, or --flag=true|false
static int bool_flag(const char* v, int32_t& value) {
    const bool given = v && (!strcmp(v, "true") || !strcmp(v, "false"));
    value = given ? !strcmp(v, "true") : 1;
    return given ? TOOK_VALUE : TOOK_FLAG;
}

extern "C" int tksmseq_scb_main(int argc, char** argv) {
    Common c;
    tksmseq_scb_params p{};
    if (!parse_args(argc, argv, c, [&](const std::string& o, const char* v) -> int { return o == "--keep-meta-barcodes" ? bool_flag(v, p.keep_meta_barcodes) : NOT_MINE; })) return 1;
    if (c.help) { printf("Single cell barcode module\nusage: scb -i INPUT -o OUTPUT [--keep-meta-barcodes]\n"
                         "           [--devices D[,D...]] [--batch-bytes B] [--verbosity L] [--log-file F]\n"); return 0; }
    int missing = 0;
    if (c.input.empty()) { fprintf(stderr, "Missing parameter: input\n"); missing++; }
    if (c.output.empty()) { fprintf(stderr, "Missing parameter: output\n"); missing++; }
    if (missing) return 1;
    Logger log;
    if (!open_log(c, "scb", log)) return 1;
    return stream_transform<tksmseq_scb_params>(c, log, "scb", p, tksmseq_scb, nullptr);      // (the barcodes come from the comments: nothing is numbered)
}

extern "C" int tksmseq_flip_main(int argc, char** argv) {
    Common c;
    tksmseq_flip_params p{};
    bool have_p = false;
    if (!parse_args(argc, argv, c, [&](const std::string& o, const char* v) -> int {
            if ((o != "-p" && o != "--flip-probability") || !v) return NOT_MINE;
            p.flip_probability = atof(v); have_p = true;
            return TOOK_VALUE;
        })) return 1;
    if (c.help) { printf("Flip module\nusage: flip -i INPUT -o OUTPUT -p PROBABILITY [-s SEED]\n"
                         "            [--devices D[,D...]] [--batch-bytes B] [--verbosity L] [--log-file F]\n"); return 0; }
    int missing = 0;
    if (c.input.empty()) { fprintf(stderr, "Missing parameter: input\n"); missing++; }
    if (c.output.empty()) { fprintf(stderr, "Missing parameter: output\n"); missing++; }
    if (!have_p) { fprintf(stderr, "Missing parameter: flip-probability\n"); missing++; }
    if (missing) return 1;
    // the reference logs this and runs anyway (validate_arguments returns 0: src/strand_man.cpp:80-85)
    if (p.flip_probability < 0.0 || p.flip_probability > 1.0) fprintf(stderr, "Flip probability must be between 0 and 1\n");
    Logger log;
    if (!open_log(c, "flip", log)) return 1;
    p.seed = (uint64_t)c.seed;
    return stream_transform(c, log, "flip", p, tksmseq_flip);
}

extern "C" int tksmseq_tail_noise_main(int argc, char** argv) {
    Common c;
    tksmseq_noise_params p{};
    p.error_rate = 0.5;
    std::string alphabet = "AGTC", dist_text;
    bool have_dist = false;
    if (!parse_args(argc, argv, c, [&](const std::string& o, const char* v) -> int {
            if (o == "--palindromic") return bool_flag(v, p.palindromic);
            if (o == "--length-dist" && v) { dist_text = v; have_dist = true; }
            else if (o == "--alphabet" && v) alphabet = v;
            else if (o == "--error-rate" && v) p.error_rate = atof(v);
            else return NOT_MINE;
            return TOOK_VALUE;
        })) return 1;
    static const char* help =
        "Append Noise module\nusage: tail-noise -i INPUT -o OUTPUT --length-dist NAME,MU,SIGMA [--alphabet AGTC] [--palindromic] [--error-rate 0.5] [-s SEED]\n"
        "                  [--devices D[,D...]] [--batch-bytes B] [--verbosity L] [--log-file F]\n"
        "NAME: normal | lognormal.  Random noise: a literal of that many letters of the alphabet (a repeated letter is more likely) behind every\n"
        "molecule; --palindromic: the molecule's last bases again as a hairpin, each substituted with probability --error-rate\n";
    if (c.help) { printf("%s", help); return 0; }
    // validate_arguments (src/append_noise.cpp:174-190)
    int missing = 0;
    if (c.input.empty()) { fprintf(stderr, "input is required!\n"); missing++; }
    if (c.output.empty()) { fprintf(stderr, "output is required!\n"); missing++; }
    if (!have_dist) { fprintf(stderr, "length-dist is required!\n"); missing++; }
    if (missing) { fprintf(stderr, "%s\n", help); return 1; }
    // DistVisitor::get_dist (:26-45): the name first; the reference throws on a list without three fields or a field that is no number
    {
        std::vector<std::string> f;
        size_t a = 0;
        for (;;) { const size_t e = dist_text.find(',', a); f.push_back(dist_text.substr(a, e == std::string::npos ? e : e - a)); if (e == std::string::npos) break; a = e + 1; }
        if (f[0] == "normal") p.dist = TKSMSEQ_NOISE_NORMAL;
        else if (f[0] == "lognormal") p.dist = TKSMSEQ_NOISE_LOGNORMAL;
        else { fprintf(stderr, "Distribution not implemented!\n"); return 1; }
        std::vector<double> d;
        if (f.size() != 3 || !parse_doubles((f[1] + "," + f[2]).c_str(), d) || d.size() != 2) { fprintf(stderr, "length-dist needs NAME,MU,SIGMA (got '%s')\n", dist_text.c_str()); return 1; }
        p.mu = d[0]; p.sigma = d[1];
    }
    // (what the std:: distributions leave undefined: refused before any work, with the library's messages)
    if (!std::isfinite(p.mu) || !std::isfinite(p.sigma) || !(p.sigma > 0.0)) { fprintf(stderr, "Error: tail-noise: mu must be finite, sigma finite and positive\n"); return 1; }
    if (alphabet.empty()) { fprintf(stderr, "Error: tail-noise: the alphabet is empty\n"); return 1; }
    if (std::isnan(p.error_rate)) { fprintf(stderr, "Error: tail-noise: the error rate is not a number\n"); return 1; }
    Logger log;
    if (!open_log(c, "tail-noise", log)) return 1;
    p.seed = (uint64_t)c.seed; p.alphabet = alphabet.c_str();
    return stream_transform(c, log, "tail-noise", p, tksmseq_append_noise);
}

// The contig table of random-wgs: names and lengths from <reference>.fai (src/random_wgs.cpp:139-161: the first two columns), or, when
// there is no such file, from the FASTA itself (the reference reads nothing then, and writes nothing).
static bool wgs_contig_table(const std::string& reference, std::vector<std::pair<std::string, uint64_t>>& table, std::string& err) {
    table.clear();
    const std::string fai = reference + ".fai";
    std::string text;
    if (read_file(fai, text)) {
        size_t a = 0;
        while (a < text.size()) {
            size_t e = text.find('\n', a);
            if (e == std::string::npos) e = text.size();
            size_t i = a;
            while (i < e && isspace((unsigned char)text[i])) i++;
            size_t j = i;
            while (j < e && !isspace((unsigned char)text[j])) j++;
            if (j > i) {
                size_t k = j;
                while (k < e && isspace((unsigned char)text[k])) k++;
                char* end = nullptr;
                const std::string num = text.substr(k, e - k);
                const unsigned long long len = strtoull(num.c_str(), &end, 10);
                if (num.empty() || end == num.c_str() || num[0] == '-') { err = "malformed line in " + fai + ": " + text.substr(a, e - a); return false; }
                table.emplace_back(text.substr(i, j - i), (uint64_t)len);
            }
            a = e + 1;
        }
        return true;
    }
    std::vector<tkh::FastaRecord> recs;
    if (!tkh::read_fasta(reference, recs, err)) return false;
    for (auto& r : recs) table.emplace_back(r.name, (uint64_t)r.seq.size());
    return true;
}

extern "C" int tksmseq_random_wgs_main(int argc, char** argv) {
    Common c;
    std::string reference, dist_text;
    bool have_bc = false, have_depth = false, have_dist = false;
    long long base_count = 0; double depth = 0.0;
    uint64_t batch_molecules = 2000000;
    if (!parse_args(argc, argv, c, [&](const std::string& o, const char* v) -> int {
            // (the common flags know -i, --batch-bytes and --slice-molecules, which this module does not have)
            if (o == "-i" || o == "--input" || o == "--batch-bytes" || o == "--slice-molecules") return NO_SUCH;
            if ((o == "-r" || o == "--reference") && v) reference = v;
            else if (o == "--frag-len-dist" && v) { dist_text = v; have_dist = true; }
            else if (o == "--base-count" && v) { base_count = atoll(v); have_bc = true; }
            else if (o == "--depth" && v) { depth = atof(v); have_depth = true; }
            else if (o == "--batch-molecules" && v) { batch_molecules = strtoull(v, nullptr, 10); if (batch_molecules < 1 || batch_molecules > (1ull << 28)) return MALFORMED; }
            else return NOT_MINE;
            return TOOK_VALUE;
        })) return 1;
    static const char* help =
        "Random whole-genome fragments module\nusage: random-wgs -r REFERENCE --frag-len-dist \"NAME A [B]\" -o OUTPUT (--base-count N | --depth D) [-s SEED]\n"
        "                  [--devices D[,D...]] [--batch-molecules M] [--verbosity L] [--log-file F]\n"
        "NAME: normal MEAN SIGMA | uniform LOW HIGH | lognormal M S | exponential RATE; the contig table comes from REFERENCE.fai\n"
        "(from REFERENCE itself when there is no such file)\n";
    if (c.help) { printf("%s", help); return 0; }
    // validate_arguments (src/random_wgs.cpp:95-127)
    int missing = 0;
    if (reference.empty()) { fprintf(stderr, "reference is required!\n"); missing++; }
    if (c.output.empty()) { fprintf(stderr, "output is required!\n"); missing++; }
    if (!have_dist) { fprintf(stderr, "frag-len-dist is required!\n"); missing++; }
    if (missing) { fprintf(stderr, "%s\n", help); return 1; }
    if (!have_bc && !have_depth) { fprintf(stderr, "Either base-count or depth is required!\n"); return 1; }
    tksmseq_wgs_params p{};
    {
        int dist = 0;
        const int bad = tkmod::parse_frag_len_dist(dist_text, dist, p.a, p.b);
        if (bad) { fprintf(stderr, bad == 1 ? "Invalid fragment length distribution\n" : "Invalid fragment length distribution parameters\n"); return 1; }
        p.dist = dist;
    }
    Logger log;
    if (!open_log(c, "random-wgs", log)) return 1;
    std::vector<std::pair<std::string, uint64_t>> table;
    {
        std::string err;
        if (!wgs_contig_table(reference, table, err)) { fprintf(stderr, "Error: %s\n", err.c_str()); return 1; }
        std::vector<std::string> names;
        for (auto& t : table) names.push_back(t.first);
        std::sort(names.begin(), names.end());
        for (size_t i = 1; i < names.size(); i++)
            if (names[i] == names[i - 1]) { fprintf(stderr, "Error: contig name %s appears more than once in the reference\n", names[i].c_str()); return 1; }
    }
    uint64_t ref_length = 0;
    for (auto& t : table) ref_length += t.second;
    log.log(Logger::INFO, "Reference length: %llu", (unsigned long long)ref_length);
    if (!ref_length) { fprintf(stderr, "Error: the reference has no contigs (or none with a base)\n"); return 1; }
    p.seed = (uint64_t)c.seed;
    p.base_count = have_bc ? (int64_t)base_count : (int64_t)(depth * (double)ref_length);      // (:169-176)
    // the only state that is serial across batches: next candidate, molecules and bases so far, next piece number.  A batch is made under
    // the engine's lock (serial_work): what it carries over is known once the batch before it has been made (milliseconds)
    tksmseq_wgs_progress st{}; uint64_t next_seq = 0; bool done = p.base_count <= 0;
    auto prepare = [&](tksmseq_ctx* ctx, void**) -> bool {
        for (auto& t : table)
            if (tksmseq_reference_declare_contig(ctx, t.first.c_str(), t.second)) return false;
        return true;
    };
    auto next_piece = [&](Piece& pc) -> bool { pc.seq = next_seq; return !done; };
    auto work = [&](tksmseq_ctx* ctx, void*, Piece& pc, tksmseq_batch** out) -> int {
        tksmseq_wgs_params q = p;
        q.first_candidate = st.next_candidate; q.n_candidates = batch_molecules; q.molecules_before = st.molecules; q.bases_before = st.bases;
        tksmseq_wgs_progress pr{};
        const int rc = tksmseq_wgs(ctx, &q, out, &pr);
        if (rc) return rc;
        uint64_t n = 0;
        tksmseq_batch_info(*out, &n, nullptr, nullptr);
        if (!n && !pr.reached) {
            pc.error = "none of " + std::to_string(batch_molecules) + " candidate fragments has a base (fragment length distribution '" + dist_text + "'): giving up";
            return 1;
        }
        st = pr; next_seq++;
        if (pr.reached) done = true;
        return 0;
    };
    return run_pieces(c, log, "random-wgs", prepare, next_piece, work, true, [&] {
        return ", " + std::to_string(st.bases) + " bases from " + std::to_string(st.next_candidate) + " candidates";
    });
}

// `tksm transcribe` (Splicer_module, src/transcribe.cpp:19-218) without the fusion submodule: GTFs and abundance tables in, the reference's
// compact MDF out (one record per emitted row, depth = its count).  One context on the first entry of --devices: the counts are made on the
// device (tksmseq_transcribe_plan_create), the text from them on the host (tksmseq_transcribe_text), --batch-molecules records at a time.
static void split_commas(const char* v, std::vector<std::string>& out) {      // cxxopts' vector<string>: every occurrence, split at ','
    const char* q = v;
    for (;;) {
        const char* e = strchr(q, ',');
        out.emplace_back(q, e ? (size_t)(e - q) : strlen(q));
        if (!e) return;
        q = e + 1;
    }
}

extern "C" int tksmseq_transcribe_main(int argc, char** argv) {
    Common c;
    std::vector<std::string> gtfs, abundances;
    std::vector<double> weights;
    bool have_count = false;
    long long molecule_count = 0, default_depth = 0;
    int32_t use_whole_id = 0, non_coding = 0;
    std::string prefix = "M";
    uint64_t batch_molecules = 1 << 20;
    auto integer = [](const char* v, long long& out) { char* e = nullptr; out = strtoll(v, &e, 10); return e != v && !*e; };
    if (!parse_args(argc, argv, c, [&](const std::string& o, const char* v) -> int {
            // (the common flags know -i, --batch-bytes and --slice-molecules, which this module does not have)
            if (o == "-i" || o == "--input" || o == "--batch-bytes" || o == "--slice-molecules") return NO_SUCH;
            if (o == "--use-whole-id") return bool_flag(v, use_whole_id);
            if (o == "--non-coding") return bool_flag(v, non_coding);
            if ((o == "-g" || o == "--gtf") && v) split_commas(v, gtfs);
            else if ((o == "-a" || o == "--abundance") && v) split_commas(v, abundances);
            else if (o == "--molecule-count" && v) { if (!integer(v, molecule_count) || molecule_count < -2147483648ll || molecule_count > 2147483647ll) return MALFORMED; have_count = true; }
            else if (o == "--default-depth" && v) { if (!integer(v, default_depth)) return MALFORMED; }
            else if (o == "--molecule-prefix" && v) prefix = v;
            else if ((o == "-w" || o == "--weights") && v) { std::vector<double> w; if (!parse_doubles(v, w)) return MALFORMED; weights.insert(weights.end(), w.begin(), w.end()); }
            else if (o == "--batch-molecules" && v) { batch_molecules = strtoull(v, nullptr, 10); if (batch_molecules < 1 || batch_molecules > (1ull << 28)) return MALFORMED; }
            else return NOT_MINE;
            return TOOK_VALUE;
        })) return 1;
    static const char* help =
        "RNA Splicing module\nusage: transcribe -g GTF[,GTF...] -a ABUNDANCE[,ABUNDANCE...] --molecule-count N -o OUTPUT [--use-whole-id] [--non-coding]\n"
        "                  [--default-depth D] [--molecule-prefix M] [-w W[,W...]] [-s SEED] [--devices D] [--batch-molecules M] [--verbosity L] [--log-file F]\n"
        "ABUNDANCE: a header line, then rows `transcript_id tpm cell-barcode`; -w: one weight, or one per abundance table\n"
        "--default-depth D: a non-zero D keeps only the lines whose gene_biotype is protein_coding; --non-coding has no effect (both as the reference)\n"
        "The gene-fusion options of the reference (--fusion-gtf, --fusion-file, --fusion-output, --fusion-count, --disable-deletions,\n"
        "--translocation-ratio, --expression-fallback) are not built: they are refused like any unknown option\n";
    if (c.help) { printf("%s", help); return 0; }
    // validate_arguments (src/transcribe.cpp:90-108)
    int missing = 0;
    if (gtfs.empty()) { fprintf(stderr, "Missing mandatory parameter gtf\n"); missing++; }
    if (abundances.empty()) { fprintf(stderr, "Missing mandatory parameter abundance\n"); missing++; }
    if (c.output.empty()) { fprintf(stderr, "Missing mandatory parameter output\n"); missing++; }
    if (!have_count) { fprintf(stderr, "Missing mandatory parameter molecule-count\n"); missing++; }
    if (missing) { printf("%s\n", help); return 1; }
    // process_file_weights (:65-77): one weight for all tables, or one each
    if (weights.empty()) weights.push_back(1.0);
    if (weights.size() != 1 && weights.size() != abundances.size()) {
        fprintf(stderr, "Error: -w/--weights takes one weight, or one per abundance file (%zu weights for %zu files)\n", weights.size(), abundances.size());
        return 1;
    }
    std::vector<double> file_w(abundances.size());
    if (weights.size() == 1) for (auto& w : file_w) w = weights[0] / (double)abundances.size();
    else { double sum = 0.0; for (double w : weights) sum += w; for (size_t i = 0; i < file_w.size(); i++) file_w[i] = weights[i] / sum; }
    Logger log;
    if (!open_log(c, "transcribe", log)) return 1;
    for (auto& g : gtfs) { FILE* f = fopen(g.c_str(), "rb"); if (!f) { fprintf(stderr, "Could not open GTF file %s!\n", g.c_str()); return 1; } fclose(f); }
    for (auto& a : abundances) { FILE* f = fopen(a.c_str(), "rb"); if (!f) { fprintf(stderr, "Could not open abundance file %s!\n", a.c_str()); return 1; } fclose(f); }
    tksmseq_ctx* ctx = nullptr;
    if (tksmseq_create(c.devices[0], &ctx)) { fprintf(stderr, "Error: %s\n", tksmseq_last_error(nullptr)); return 1; }
    const auto t0 = std::chrono::steady_clock::now();
    int rc = 0;
    FILE* out = nullptr;
    uint64_t n_records = 0, n_molecules = 0, first_row = 0;
    for (auto& g : gtfs) {
        log.log(Logger::INFO, "Reading GTF file %s", g.c_str());
        if (tksmseq_transcripts_add_gtf(ctx, g.c_str(), default_depth != 0)) { fprintf(stderr, "Error: %s\n", tksmseq_last_error(ctx)); rc = 1; break; }
    }
    if (!rc && !(out = fopen(c.output.c_str(), "wb"))) { fprintf(stderr, "Error: cannot write %s\n", c.output.c_str()); rc = 1; }
    for (size_t k = 0; k < abundances.size() && !rc; k++) {
        log.log(Logger::INFO, "Reading abundance file %s and printing simulated molecules to %s!", abundances[k].c_str(), c.output.c_str());
        tksmseq_tsb_params p{};
        p.seed = (uint64_t)c.seed; p.molecule_count = molecule_count; p.weight = file_w[k]; p.first_row_index = first_row; p.use_whole_id = use_whole_id;
        p.prefix = prefix.c_str();
        tksmseq_tsb_plan* plan = nullptr;
        if (tksmseq_transcribe_plan_create(ctx, abundances[k].c_str(), nullptr, 0, &p, &plan)) { fprintf(stderr, "%s\n", tksmseq_last_error(ctx)); rc = 1; break; }
        uint64_t rows = 0, records = 0, molecules = 0, n_missing = 0;
        tksmseq_transcribe_plan_info(plan, &rows, &records, &molecules, &n_missing);
        for (uint64_t i = 0; i < n_missing; i++) {
            const char* id = nullptr; uint64_t len = 0;
            tksmseq_transcribe_plan_missing(plan, i, &id, &len);
            log.log(Logger::WARN, "Isoform %.*s is not found in the input GTFs!", (int)len, id);
        }
        for (uint64_t r = 0; r < records && !rc; r += batch_molecules) {
            char* text = nullptr; uint64_t len = 0;
            if (tksmseq_transcribe_text(plan, r, batch_molecules, &text, &len)) { fprintf(stderr, "Error: out of memory\n"); rc = 1; }
            else if (len && fwrite(text, 1, len, out) != len) { fprintf(stderr, "Error: cannot write %s\n", c.output.c_str()); rc = 1; }
            tksmseq_text_free(text);
        }
        tksmseq_transcribe_plan_free(plan);
        first_row += rows; n_records += records; n_molecules += molecules;
    }
    if (out && fclose(out) != 0 && !rc) { fprintf(stderr, "Error: cannot write %s\n", c.output.c_str()); rc = 1; }
    tksmseq_destroy(ctx);
    if (!rc)
        log.log(Logger::INFO, "transcribe: %llu records (%llu molecules) written in %.2f s", (unsigned long long)n_records, (unsigned long long)n_molecules,
                std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
    return rc;
}

// `tksm filter` (Filter_module, src/filter.cpp:119-231): the conditions are checked before anything is opened; the two sides are written
// through two ordered sinks, piece for piece.  Without -f the false side is not made.
extern "C" int tksmseq_filter_main(int argc, char** argv) {
    Common c;
    std::string false_output;
    std::vector<std::string> conditions;
    int32_t negate = 0;
    if (!parse_args(argc, argv, c, [&](const std::string& o, const char* v) -> int {
            // (the common flags know -o and --slice-molecules, which this module does not have)
            if (o == "-o" || o == "--output" || o == "--slice-molecules") return NO_SUCH;
            if (o == "--negate") return bool_flag(v, negate);
            if ((o == "-t" || o == "--true-output") && v) c.output = v;
            else if ((o == "-f" || o == "--false-output") && v) false_output = v;
            else if ((o == "-c" || o == "--condition") && v) split_commas(v, conditions);
            else return NOT_MINE;
            return TOOK_VALUE;
        })) return 1;
    static const char* help =
        "Filter module: Splits the input to 2 files w.r.t. condition\nusage: filter -i INPUT -t TRUE_OUTPUT [-f FALSE_OUTPUT] -c CONDITION[,CONDITION...] [--negate]\n"
        "              [--devices D[,D...]] [--batch-bytes B] [--verbosity L] [--log-file F]\n"
        "CONDITION (all must hold; -c may be repeated): \"info KEY\" | \"size OP N\" with OP one of < <= > >= == != (no space before N) |\n"
        "\"locus CHR\" | \"locus CHR:START-END\" | \"locus CHR:POSITION\"\n";
    if (c.help) { printf("%s", help); return 0; }
    // validate_arguments (src/filter.cpp:157-173)
    int missing = 0;
    if (c.input.empty()) { fprintf(stderr, "Missing parameter: input\n"); missing++; }
    if (c.output.empty()) { fprintf(stderr, "Missing parameter: true-output\n"); missing++; }
    if (conditions.empty()) { fprintf(stderr, "Missing parameter: condition\n"); missing++; }
    if (missing) { fprintf(stderr, "%s\n", help); return 1; }
    for (auto& t : conditions) {
        tkh::FilterCond parsed;
        if (!tkh::parse_filter_condition(t, parsed)) { fprintf(stderr, "Invalid condition: %s\n", t.c_str()); return 1; }
    }
    Logger log;
    if (!open_log(c, "filter", log)) return 1;
    std::vector<tksmseq_filter_cond> conds(conditions.size());
    for (size_t k = 0; k < conds.size(); k++) { conds[k] = tksmseq_filter_cond{}; conds[k].kind = TKSMSEQ_FLT_TEXT; conds[k].text = conditions[k].c_str(); }
    tksmseq_filter_params p{};
    p.conditions = conds.data(); p.n_conditions = conds.size(); p.negate = negate;
    const bool both = !false_output.empty();
    return stream_batches(c, log, "filter", [&](tksmseq_ctx* ctx, const tksmseq_batch* in, Piece& pc, tksmseq_batch** out) -> int {
        return tksmseq_filter(ctx, in, &p, out, both ? &pc.second : nullptr);
    }, both ? &false_output : nullptr);
}

// `tksm unsegment` (Unsegment_module, src/unsegment.cpp:22-116).  Pieces end only where no chain crosses (glue_cut.h), so the output is
// that of one call on the whole input whatever --batch-bytes and --devices are; with a probability of 1 or more the whole input is one piece.
extern "C" int tksmseq_unsegment_main(int argc, char** argv) {
    Common c;
    tksmseq_glue_params p{};
    bool have_p = false;
    if (!parse_args(argc, argv, c, [&](const std::string& o, const char* v) -> int {
            if ((o != "-p" && o != "--probability") || !v) return NOT_MINE;
            p.probability = atof(v); have_p = true;
            return TOOK_VALUE;
        })) return 1;
    static const char* help =
        "Unsegment module: Concatenate adjacent molecules with a probability\nusage: unsegment -i INPUT -o OUTPUT -p PROBABILITY [-s SEED]\n"
        "                 [--devices D[,D...]] [--batch-bytes B] [--verbosity L] [--log-file F]\n"
        "Every molecule but the first is glued behind its predecessor with probability PROBABILITY; the glued ids are listed under Cat.\n";
    if (c.help) { printf("%s", help); return 0; }
    // validate_arguments (src/unsegment.cpp:52-68)
    int missing = 0;
    if (c.input.empty()) { fprintf(stderr, "input is required!\n"); missing++; }
    if (c.output.empty()) { fprintf(stderr, "output is required!\n"); missing++; }
    if (!have_p) { fprintf(stderr, "probability is required!\n"); missing++; }
    if (missing) { fprintf(stderr, "%s\n", help); return 1; }
    Logger log;
    if (!open_log(c, "unsegment", log)) return 1;
    p.seed = (uint64_t)c.seed;
    return stream_batches(c, log, "unsegment", [&](tksmseq_ctx* ctx, const tksmseq_batch* in, Piece& pc, tksmseq_batch** out) -> int {
        tksmseq_glue_params q = p;
        q.first_molecule_index = pc.first;
        return tksmseq_glue(ctx, in, &q, out);
    }, nullptr, [p](uint64_t g) { return tksmseq_glue_joins(p.seed, p.probability, g) != 0; });
}

// `tksm mutate` (Mutate_module, src/mutate.cpp:141-250: -i, -o, -t/--tsv; "<name> is required!" per missing one, the help, exit 1).  The table is
// read and checked here, before any context exists: a bad table ends the run with its line named and without a device.
extern "C" int tksmseq_mutate_main(int argc, char** argv) {
    Common c;
    std::string tsv;
    if (!parse_args(argc, argv, c, [&](const std::string& o, const char* v) -> int {
            if (o == "--slice-molecules") return NO_SUCH;            // (a common flag this module does not have; -s/--seed is taken and draws nothing)
            if ((o != "-t" && o != "--tsv") || !v) return NOT_MINE;
            tsv = v;
            return TOOK_VALUE;
        })) return 1;
    static const char* help =
        "Mutate module: apply the SNVs, insertions and deletions of a table to every molecule\nusage: mutate -i INPUT -o OUTPUT -t TSV\n"
        "              [--devices D[,D...]] [--batch-bytes B] [--verbosity L] [--log-file F]\n"
        "TSV: one variant per line, 'chr pos modification' (pos 0-based, plus strand): all digits = deletion of [pos, modification),\n"
        "one letter = SNV, '.SEQ' or 'XSEQ' = SEQ inserted behind pos (X replaces the base at pos).\n";
    if (c.help) { printf("%s", help); return 0; }
    int missing = 0;
    if (c.input.empty()) { fprintf(stderr, "input is required!\n"); missing++; }
    if (c.output.empty()) { fprintf(stderr, "output is required!\n"); missing++; }
    if (tsv.empty()) { fprintf(stderr, "tsv is required!\n"); missing++; }
    if (missing) { fprintf(stderr, "%s\n", help); return 1; }
    Logger log;
    if (!open_log(c, "mutate", log)) return 1;
    tksmseq_variants* table = nullptr;
    if (tksmseq_variants_load(nullptr, tsv.c_str(), nullptr, 0, &table)) { fprintf(stderr, "Error: %s\n", tksmseq_last_error(nullptr)); return 1; }
    uint64_t rows = 0, snvs = 0, ins = 0, dels = 0, ranges = 0, dropped = 0;
    tksmseq_variants_info(table, &rows, &snvs, &ins, &dels, &ranges, &dropped);
    log.log(Logger::INFO, "%s: %llu variants (%llu SNVs, %llu insertions, %llu deletions in %llu ranges; %llu SNVs / insertions inside a deletion dropped)", tsv.c_str(),
            (unsigned long long)rows, (unsigned long long)snvs, (unsigned long long)ins, (unsigned long long)dels, (unsigned long long)ranges, (unsigned long long)dropped);
    const tksmseq_mutate_params p{};
    const int rc = stream_batches(c, log, "mutate", [&](tksmseq_ctx* ctx, const tksmseq_batch* in, Piece&, tksmseq_batch** out) -> int {
        return tksmseq_mutate(ctx, in, table, &p, out);
    });
    tksmseq_variants_free(table);
    return rc;
}

// `tksm shuffle` (Shuffle_module, src/shuffle.cpp:22-125): the whole input is one batch on the first entry of --devices, as the reference
// without --buffer-size (and `tksm pcr` here) holds it; --buffer-size chooses the order the reference's buffer would give, not the memory.
extern "C" int tksmseq_shuffle_main(int argc, char** argv) {
    Common c;
    tksmseq_shuffle_params p{};
    bool have_b = false;
    if (!parse_args(argc, argv, c, [&](const std::string& o, const char* v) -> int {
            if (o == "--batch-bytes" || o == "--slice-molecules") return NO_SUCH;      // (common flags this module does not have)
            if (o != "--buffer-size" || !v) return NOT_MINE;
            char* e = nullptr;
            p.buffer_size = strtoull(v, &e, 10);
            if (e == v || *e || v[0] == '-') return MALFORMED;
            have_b = true;
            return TOOK_VALUE;
        })) return 1;
    static const char* help =
        "Shuffle module: shuffles mdfs\nusage: shuffle -i INPUT -o OUTPUT [--buffer-size B] [-s SEED]\n"
        "               [--devices D[,D...]] [--verbosity L] [--log-file F]\n"
        "Without --buffer-size the molecules come out in a uniformly random order.  --buffer-size B gives the order of the reference's buffer of\n"
        "B molecules (a molecule moves at most about B places forward); it does NOT bound memory: the whole input is one batch on the first device.\n";
    if (c.help) { printf("%s", help); return 0; }
    // validate_arguments (src/shuffle.cpp:74-90)
    int missing = 0;
    if (c.input.empty()) { fprintf(stderr, "input is required!\n"); missing++; }
    if (c.output.empty()) { fprintf(stderr, "output is required!\n"); missing++; }
    if (missing) { fprintf(stderr, "%s\n", help); return 1; }
    // (the reference builds uniform_int_distribution(0, buffer_size - 1) there: undefined)
    if (have_b && p.buffer_size == 0) { fprintf(stderr, "buffer-size must be at least 1 (leave it out to shuffle the whole input)\n"); return 1; }
    Logger log;
    if (!open_log(c, "shuffle", log)) return 1;
    p.seed = (uint64_t)c.seed;
    std::string text;
    if (!read_file(c.input, text)) { fprintf(stderr, "Could not open file %s\n", c.input.c_str()); return 1; }
    FILE* out = fopen(c.output.c_str(), "wb");
    if (!out) { fprintf(stderr, "Error: cannot write %s\n", c.output.c_str()); return 1; }
    tksmseq_ctx* ctx = nullptr;
    if (tksmseq_create(c.devices[0], &ctx)) { fprintf(stderr, "Error: %s\n", tksmseq_last_error(nullptr)); fclose(out); return 1; }
    tksmseq_set_host_threads(ctx, (int)std::max(1u, std::min(8u, std::thread::hardware_concurrency())));
    const auto t0 = std::chrono::steady_clock::now();
    tksmseq_batch *in = nullptr, *b = nullptr;
    char* mdf = nullptr; uint64_t len = 0, n = 0;
    int rc = tksmseq_molecules_from_mdf_text(ctx, text.data(), text.size(), &in);
    if (!rc) rc = tksmseq_shuffle(ctx, in, &p, &b);
    if (!rc) rc = tksmseq_batch_to_mdf_text(ctx, b, &mdf, &len);
    if (rc) fprintf(stderr, "Error: shuffle: %s\n", tksmseq_last_error(ctx));
    else if (len && fwrite(mdf, 1, len, out) != len) { fprintf(stderr, "Error: cannot write %s\n", c.output.c_str()); rc = 1; }
    if (b) tksmseq_batch_info(b, &n, nullptr, nullptr);
    tksmseq_text_free(mdf);
    if (b) tksmseq_batch_free(ctx, b);
    if (in) tksmseq_batch_free(ctx, in);
    tksmseq_destroy(ctx);
    if (fclose(out) != 0 && !rc) { fprintf(stderr, "Error: cannot write %s\n", c.output.c_str()); rc = 1; }
    if (rc) return 1;
    log.log(Logger::INFO, "shuffle: %llu molecules written in %.2f s", (unsigned long long)n, std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
    return 0;
}
