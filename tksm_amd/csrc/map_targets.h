// map_targets.h -- internal: the object behind tksmseq_targets (include/tksmseq.h, "map, annotated targets"), shared by map_targets_api.cpp,
// which builds it, and map_api.cpp, which maps against it.
#pragma once
#include <string>
#include <vector>

#include "ctx.h"
#include "map_host.h"

struct tksmseq_targets {
    tksmseq_ctx* ctx = nullptr;
    uint64_t ref_version = 0, tsb_serial = 0;       // what the set was made from: another value on the context makes it stale
    tkh::MapTargets h;                              // the kept transcripts, their layout and their exons
    std::vector<std::string> names;                 // [targets] the table's ids
    std::vector<std::string> contig_names;          // the reference's contigs as they were, for the projection
    std::vector<uint64_t> contig_lens;
    DevBuf d_codes, d_valid, d_seqs;                // the image and its { voff, len } table
};

// TKSMSEQ_OK when `t` may be used on `ctx` now; TKSMSEQ_EINVAL with ctx->err otherwise
int map_targets_check(tksmseq_ctx* ctx, const tksmseq_targets* t);
