// tool_run.h -- internal: the device plumbing shared by the tools that read files and write files (abund_api.cpp, ms_api.cpp, bm_api.cpp,
// map_api.cpp; kde_api.cpp for the copies): host timing, copies to and from a TmpBuf, the scan over ctx->w_scan, one RAII set of events and
// the run starts of sorted keys.  Everything works on the context's stream.  NOT for the batch family: mdf_batch.h's scan_async and upload
// work on DevBuf and add slack bytes the batch kernels rely on -- the two sets stay apart on purpose.
// A TmpBuf goes back to the cache when it dies (DevBuf::release drains the stream first): a helper here owns a temporary only where
// it has drained the stream itself before it returns, so that no block goes back earlier than the work queued on it ends.
#pragma once
#include <chrono>
#include <vector>

#include "ctx.h"
#include "ms_kernels.h"

inline double ms_since(std::chrono::steady_clock::time_point t0) { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); }

// d = v[0 .. n), queued; d holds at least one element
template <class T>
hipError_t upload(TmpBuf& d, const T* v, size_t n, hipStream_t s) {
    hipError_t e = d.ensure(std::max<size_t>(n, 1) * sizeof(T));
    if (e != hipSuccess || !n) return e;
    return hipMemcpyAsync(d.p, v, n * sizeof(T), hipMemcpyHostToDevice, s);
}
template <class T>
hipError_t upload(TmpBuf& d, const std::vector<T>& v, hipStream_t s) { return upload(d, v.data(), v.size(), s); }
// v[0 .. n) = d, queued
template <class T>
hipError_t download(T* v, const TmpBuf& d, size_t n, hipStream_t s) { return n ? hipMemcpyAsync(v, d.p, n * sizeof(T), hipMemcpyDeviceToHost, s) : hipSuccess; }
template <class T>
hipError_t download(std::vector<T>& v, const TmpBuf& d, size_t n, hipStream_t s) { v.resize(n); return download(v.data(), d, n, s); }

// out[0 .. n] = the exclusive scan of in[0 .. n), queued
inline int scan_u64(tksmseq_ctx* ctx, const uint64_t* in, uint64_t* out, uint64_t n) {
    HIPCHK(ctx, ctx->w_scan.ensure(tk::scan_temp_bytes(n) + 64));
    HIPCHK(ctx, tk::launch_scan(in, out, n, ctx->w_scan.p, ctx->w_scan.cap, ctx->stream));
    return TKSMSEQ_OK;
}
// v = *d, waited for
inline int fetch_u64(tksmseq_ctx* ctx, const uint64_t* d, uint64_t& v) {
    HIPCHK(ctx, hipMemcpyAsync(&v, d, 8, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return TKSMSEQ_OK;
}

// N events that go with their owner.  mark(i) records event i; add(i, sum) adds the time from mark i to mark i + 1 (both reached: the
// caller has synchronized).  Marks 0 .. k back to back with one synchronization and k add()s (model-sequence, barcode-match), or
// mark 0, mark 1 and a synchronization per stage (MapRun::begin / end): both are spelled with these two.
template <int N>
struct Events {
    hipEvent_t e[N] = {};
    ~Events() { for (hipEvent_t x : e) if (x) (void)hipEventDestroy(x); }
    int create(tksmseq_ctx* ctx) { for (auto& x : e) HIPCHK(ctx, hipEventCreate(&x)); return TKSMSEQ_OK; }
    int mark(tksmseq_ctx* ctx, int i) { HIPCHK(ctx, hipEventRecord(e[i], ctx->stream)); return TKSMSEQ_OK; }
    int add(tksmseq_ctx* ctx, int i, float& sum) {
        float ms = 0.f;
        HIPCHK(ctx, hipEventElapsedTime(&ms, e[i], e[i + 1]));
        sum += ms;
        return TKSMSEQ_OK;
    }
};

// sorted[0 .. n) in ascending (key, sub) order, subs or null: d_start[run] = the first item of every run of equal (key, sub), d_start[runs] = n;
// info[0] = the runs, info[1] != 0: the last run is the one of MS_NO_EVENT (ms_kernels.h).  Waited for: the three temporaries go back drained.
inline int run_starts(tksmseq_ctx* ctx, const uint64_t* sorted, const uint32_t* subs, uint32_t n, TmpBuf& d_start, uint64_t info[2]) {
    hipStream_t s = ctx->stream;
    TmpBuf d_flag(s), d_scan(s), d_info(s);
    HIPCHK(ctx, d_flag.ensure(((size_t)n + 1) * 8));
    HIPCHK(ctx, d_scan.ensure(((size_t)n + 1) * 8));
    HIPCHK(ctx, d_info.ensure(16));
    HIPCHK(ctx, d_start.ensure(((size_t)n + 2) * 4));
    HIPCHK(ctx, tk::launch_ms_run_flags(sorted, subs, n, d_flag.as<uint64_t>(), s));
    if (int rc = scan_u64(ctx, d_flag.as<uint64_t>(), d_scan.as<uint64_t>(), n)) return rc;
    HIPCHK(ctx, tk::launch_ms_run_starts(sorted, n, d_flag.as<uint64_t>(), d_scan.as<uint64_t>(), d_start.as<uint32_t>(), d_info.as<uint64_t>(), s));
    HIPCHK(ctx, hipMemcpyAsync(info, d_info.p, 16, hipMemcpyDeviceToHost, s));
    HIPCHK(ctx, hipStreamSynchronize(s));
    return TKSMSEQ_OK;
}
