// map_targets_api.cpp -- C-ABI of the target sets of map -g (include/tksmseq.h, "map, annotated targets"): the host walks the transcript table
// and lays the image out (map_host.cpp), the device builds the genome's validity and splices both images in one pass
// (map_targets_kernels.hip); the FASTA is decoded from the downloaded image.  tksmseq_map_targets itself is in map_api.cpp.
#include <memory>
#include <string>
#include <vector>

#include "abund_host.h"
#include "map_targets.h"
#include "map_targets_kernels.h"
#include "tool_run.h"

int map_targets_check(tksmseq_ctx* ctx, const tksmseq_targets* t) {
    if (t->ctx != ctx) { ctx->err = "map: the target set belongs to another context"; return TKSMSEQ_EINVAL; }
    if (t->ref_version != ctx->ref_version) { ctx->err = "map: the reference has changed since the target set was made"; return TKSMSEQ_EINVAL; }
    if (!ctx->tsb || ctx->tsb->serial != t->tsb_serial) { ctx->err = "map: the transcript table has changed since the target set was made"; return TKSMSEQ_EINVAL; }
    return TKSMSEQ_OK;
}

extern "C" {

int tksmseq_targets_from_transcripts(tksmseq_ctx* ctx, tksmseq_targets** out, tksmseq_targets_info* info_out) {
    if (!ctx) return TKSMSEQ_EINVAL;
    if (!out) { ctx->err = "map: null argument"; return TKSMSEQ_EINVAL; }
    *out = nullptr;
    if (!ctx->tsb) { ctx->err = "map: no GTF has been added (tksmseq_transcripts_add_gtf)"; return TKSMSEQ_EINVAL; }
    if (ctx->contigs.empty()) { ctx->err = "map: the context has no reference"; return TKSMSEQ_EINVAL; }
    const tsb::Transcripts& T = *ctx->tsb;
    std::vector<int32_t> contig_of(T.contig_names.size());
    for (size_t i = 0; i < contig_of.size(); i++) {
        const int ci = ctx->find(T.contig_names[i]);
        contig_of[i] = ci >= 0 && !ctx->contig_declared[(size_t)ci] ? ci : -1;
    }
    std::unique_ptr<tksmseq_targets> t(new tksmseq_targets);
    t->ctx = ctx; t->ref_version = ctx->ref_version; t->tsb_serial = T.serial;
    if (int rc = tkh::map_targets_select(T, contig_of, ctx->contigs, t->h, ctx->err)) return rc;
    const tkh::MapTargets& H = t->h;
    const size_t n = H.n();
    t->names.resize(n);
    std::vector<tkh::MapSeq> seqs(n);
    for (size_t i = 0; i < n; i++) {
        t->names[i].assign(T.id_pool.data() + T.id_off[H.tx[i]], T.id_len[H.tx[i]]);
        seqs[i] = {H.voff[i], H.len[i], 0u};
    }
    t->contig_names = ctx->contig_names;
    for (size_t c = 0; c < ctx->contig_names.size(); c++) t->contig_lens.push_back(ctx->contigs[2 * c + 1]);

    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const uint64_t vwords = H.info.image_vwords, g_vwords = ctx->total_alloc / 32;
    TmpBuf d_gvalid(s), d_efirst(s), d_exons(s);
    Events<2> ev;
    if (int rc = ev.create(ctx)) return rc;
    HIPCHK(ctx, t->d_seqs.ensure(n * sizeof(tkh::MapSeq)));
    HIPCHK(ctx, t->d_codes.ensure(vwords * 8));
    HIPCHK(ctx, t->d_valid.ensure(vwords * 4));
    HIPCHK(ctx, hipMemcpyAsync(t->d_seqs.p, seqs.data(), n * sizeof(tkh::MapSeq), hipMemcpyHostToDevice, s));
    HIPCHK(ctx, upload(d_efirst, H.efirst, s));
    HIPCHK(ctx, upload(d_exons, H.exons, s));
    HIPCHK(ctx, d_gvalid.ensure(std::max<uint64_t>(g_vwords, 1) * 4));
    const tk::RefView R{ctx->d_packed.as<uint32_t>(), ctx->d_blocktab.as<uint32_t>(), ctx->d_pool.as<uint8_t>(), ctx->d_contigs.as<uint64_t>(), (uint32_t)(ctx->contigs.size() / 2)};
    const tk::MapSplice S{R.packed, d_gvalid.as<uint32_t>(), t->d_seqs.as<tk::MapSeq>(), d_efirst.as<uint64_t>(), d_exons.as<tk::MapTargetExon>(), (uint32_t)n, vwords};
    if (int rc = ev.mark(ctx, 0)) return rc;
    HIPCHK(ctx, tk::launch_map_ref_valid(R, g_vwords, d_gvalid.as<uint32_t>(), s));
    HIPCHK(ctx, tk::launch_map_splice_targets(S, t->d_codes.as<uint32_t>(), t->d_valid.as<uint32_t>(), s));
    if (int rc = ev.mark(ctx, 1)) return rc;
    HIPCHK(ctx, hipStreamSynchronize(s));
    if (int rc = ev.add(ctx, 0, t->h.info.splice_ms)) return rc;
    if (info_out) *info_out = t->h.info;
    *out = t.release();
    return TKSMSEQ_OK;
}

int tksmseq_targets_get(const tksmseq_targets* t, uint64_t i, const char** name, uint32_t* len, uint64_t* voff, int32_t* projectable) {
    if (!t || i >= t->h.n()) return TKSMSEQ_EINVAL;
    if (name) *name = t->names[i].c_str();
    if (len) *len = t->h.len[i];
    if (voff) *voff = t->h.voff[i];
    if (projectable) *projectable = t->h.projectable[i];
    return TKSMSEQ_OK;
}

int tksmseq_targets_download(tksmseq_ctx* ctx, const tksmseq_targets* t, uint32_t* codes, uint32_t* valid) {
    if (!ctx) return TKSMSEQ_EINVAL;
    if (!t || !codes || !valid) { ctx->err = "map: null argument"; return TKSMSEQ_EINVAL; }
    if (int rc = map_targets_check(ctx, t)) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const uint64_t vwords = t->h.info.image_vwords;
    HIPCHK(ctx, hipMemcpyAsync(codes, t->d_codes.p, vwords * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(valid, t->d_valid.p, vwords * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return TKSMSEQ_OK;
}

int tksmseq_targets_write_fasta(tksmseq_ctx* ctx, const tksmseq_targets* t, const char* path, int32_t line_width) {
    if (!ctx) return TKSMSEQ_EINVAL;
    if (!t || !path || !*path) { ctx->err = "map: null argument"; return TKSMSEQ_EINVAL; }
    if (line_width < 0) { ctx->err = "map: line_width must not be negative"; return TKSMSEQ_EINVAL; }
    const uint64_t vwords = t->h.info.image_vwords;
    std::vector<uint32_t> codes(2 * vwords), valid(vwords);
    if (int rc = tksmseq_targets_download(ctx, t, codes.data(), valid.data())) return rc;
    std::string text;
    text.reserve(t->h.info.letters + t->h.info.letters / (line_width > 0 ? (uint64_t)line_width : ~0ull) + 64 * t->h.n());
    tkh::map_targets_fasta(t->h, t->names, codes.data(), valid.data(), line_width, text);
    std::string e;
    if (!tkh::write_abundance_file(path, text, e)) { ctx->err = "map: cannot write " + std::string(path); return TKSMSEQ_EIO; }
    return TKSMSEQ_OK;
}

void tksmseq_targets_free(tksmseq_ctx* ctx, tksmseq_targets* t) {
    if (!t) return;
    if (ctx && ctx->stream) (void)hipStreamSynchronize(ctx->stream);      // (nothing queued may still read the image that goes)
    delete t;
}

}  // extern "C"
