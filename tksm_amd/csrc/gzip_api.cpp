// gzip_api.cpp -- the C-ABI of the device-side BGZF encoder (include/tksmseq.h, "BGZF on the device"): host orchestration of
// gzip_kernels.hip.  No CPU fallback: every byte of a member is written by the kernels.
#include <cstring>

#include "ctx.h"
#include "gzip_kernels.h"

static int gzip_run(tksmseq_ctx* ctx, const void* src, uint64_t bytes, int fmt, tksmseq_gzip_result* out) {
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    ctx->have_gzip = false;
    const uint64_t nc = tkgz::n_chunks(bytes);
    if (nc >= (1ull << 31)) { ctx->err = "gzip: input too large for one call"; return TKSMSEQ_ELIMIT; }
    HIPCHK(ctx, ctx->g_offs.ensure((nc + 1) * 8));
    tksmseq_gzip_result r{};
    r.member_offsets = ctx->g_offs.p;
    r.n_members = nc;
    if (!nc) {
        HIPCHK(ctx, hipMemsetAsync(ctx->g_offs.p, 0, 8, s));
        HIPCHK(ctx, hipStreamSynchronize(s));
    } else {
        HIPCHK(ctx, ctx->g_counts.ensure((nc + 1) * 8));
        HIPCHK(ctx, ctx->g_nlscan.ensure((nc + 1) * 8));
        HIPCHK(ctx, ctx->g_sizes.ensure((nc + 1) * 8));
        HIPCHK(ctx, ctx->g_plans.ensure(nc * sizeof(tkgz::ChunkPlan)));
        HIPCHK(ctx, ctx->w_scan.ensure(tk::scan_temp_bytes(nc) + 64));
        const bool T = ctx->timing;
        if (T) HIPCHK(ctx, hipEventRecord(ctx->ev[0], s));
        const uint8_t* in = (const uint8_t*)src;
        if (fmt != tkgz::FMT_RAW) {
            // line phase: the line of a record that a chunk's first byte is in, from the newlines before it
            HIPCHK(ctx, tkgz::launch_count(in, bytes, ctx->g_counts.as<uint64_t>(), s));
            HIPCHK(ctx, tk::launch_scan(ctx->g_counts.as<uint64_t>(), ctx->g_nlscan.as<uint64_t>(), nc, ctx->w_scan.p, ctx->w_scan.cap, s));
        }
        tkgz::CrcOps ops;
        tkgz::make_crc_ops(ops, (uint32_t)(bytes - (nc - 1) * tkgz::CHUNK));
        HIPCHK(ctx, tkgz::launch_plan(in, bytes, fmt, ctx->g_nlscan.as<uint64_t>(), ops, ctx->g_plans.as<tkgz::ChunkPlan>(), ctx->g_sizes.as<uint64_t>(), s));
        HIPCHK(ctx, tk::launch_scan(ctx->g_sizes.as<uint64_t>(), ctx->g_offs.as<uint64_t>(), nc, ctx->w_scan.p, ctx->w_scan.cap, s));
        // the sizes are exact: the members are written at their final offsets into a buffer of the stream's size
        uint64_t total = 0;
        HIPCHK(ctx, hipMemcpyAsync(&total, ctx->g_offs.as<uint64_t>() + nc, 8, hipMemcpyDeviceToHost, s));
        HIPCHK(ctx, hipStreamSynchronize(s));
        const uint64_t words = (total + 3) / 4 + 1;
        ctx->g_out.pooled = true;
        ctx->g_out.pool_stream = s;
        HIPCHK(ctx, ctx->g_out.ensure(words * 4));
        HIPCHK(ctx, hipMemsetAsync(ctx->g_out.p, 0, words * 4, s));
        HIPCHK(ctx, tkgz::launch_encode(in, bytes, fmt, ctx->g_nlscan.as<uint64_t>(), ctx->g_plans.as<tkgz::ChunkPlan>(), ctx->g_offs.as<uint64_t>(),
                                        ctx->g_out.as<uint32_t>(), words, s));
        if (T) {
            HIPCHK(ctx, hipEventRecord(ctx->ev[1], s));
            HIPCHK(ctx, hipEventSynchronize(ctx->ev[1]));
            HIPCHK(ctx, hipEventElapsedTime(&r.device_ms, ctx->ev[0], ctx->ev[1]));
        }
        r.bytes = total;
    }
    r.data = ctx->g_out.p;
    ctx->last_gzip = r;
    ctx->have_gzip = true;
    if (out) *out = r;
    return TKSMSEQ_OK;
}

extern "C" {

int tksmseq_result_gzip(tksmseq_ctx* ctx, tksmseq_gzip_result* out) {
    if (!ctx) return TKSMSEQ_EINVAL;
    if (!ctx->have_last) { ctx->err = "gzip: no result on this context"; return TKSMSEQ_ESTATE; }
    return gzip_run(ctx, ctx->last.records, ctx->last.records_bytes, ctx->last_fastq ? tkgz::FMT_FASTQ : tkgz::FMT_FASTA, out);
}

int tksmseq_gzip_device(tksmseq_ctx* ctx, const void* src_device, uint64_t bytes, int format, tksmseq_gzip_result* out) {
    if (!ctx) return TKSMSEQ_EINVAL;
    if ((!src_device && bytes) || format < TKSMSEQ_GZIP_RAW || format > TKSMSEQ_GZIP_FASTQ) { ctx->err = "gzip: bad source or format"; return TKSMSEQ_EINVAL; }
    return gzip_run(ctx, src_device, bytes, format, out);
}

int tksmseq_gzip_download_range(tksmseq_ctx* ctx, uint8_t* dst, uint64_t offset, uint64_t bytes, int async) {
    if (!ctx || !ctx->have_gzip || (!dst && bytes)) return TKSMSEQ_ESTATE;
    if (offset > ctx->last_gzip.bytes || bytes > ctx->last_gzip.bytes - offset) { ctx->err = "range outside the last compressed stream"; return TKSMSEQ_EINVAL; }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (bytes) HIPCHK(ctx, hipMemcpyAsync(dst, (const uint8_t*)ctx->last_gzip.data + offset, bytes, hipMemcpyDeviceToHost, ctx->stream));
    if (!async) HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return TKSMSEQ_OK;
}

int tksmseq_gzip_download_offsets(tksmseq_ctx* ctx, uint64_t* offsets) {
    if (!ctx || !ctx->have_gzip || !offsets) return TKSMSEQ_ESTATE;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, hipMemcpyAsync(offsets, ctx->last_gzip.member_offsets, (ctx->last_gzip.n_members + 1) * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return TKSMSEQ_OK;
}

int tksmseq_gzip_copy_device(tksmseq_ctx* ctx, void* dst) {
    if (!ctx || !ctx->have_gzip || (!dst && ctx->last_gzip.bytes)) return TKSMSEQ_ESTATE;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (ctx->last_gzip.bytes) HIPCHK(ctx, hipMemcpyAsync(dst, ctx->last_gzip.data, ctx->last_gzip.bytes, hipMemcpyDeviceToDevice, ctx->stream));
    return TKSMSEQ_OK;
}

int tksmseq_gzip_eof(uint8_t out[28]) {
    static const uint8_t eof[28] = {0x1f, 0x8b, 0x08, 0x04, 0, 0, 0, 0, 0, 0xff, 0x06, 0, 0x42, 0x43, 0x02, 0, 0x1b, 0, 0x03, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    if (!out) return TKSMSEQ_EINVAL;
    memcpy(out, eof, 28);
    return TKSMSEQ_OK;
}

}  // extern "C"
