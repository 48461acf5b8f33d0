// kde_host.h -- host side of model-truncation (py/truncate_kde.py): the PAF reader, the end-ratio histogram and the model writer.  No
// device code: tools/sanitize_kde_host.cpp runs these under ASan / UBSan.
#pragma once
#include <stdint.h>

#include <string>
#include <vector>

struct tksmseq_ctx;
struct tksmseq_kde_model_params;

namespace tkh {

// the pairs and end ratios of the lines that contain tp:A:P (get_truncation_lens_paired_with_transcript_lens :158-179; with
// model_lengths get_alignment_lens :182-206)
struct PafSample {
    std::vector<double> xy;            // [n][2]
    std::vector<double> ratios;
};
bool read_paf_sample(const std::string& path, bool model_lengths, PafSample& out, std::string& err);
bool parse_paf_sample(const char* text, size_t len, bool model_lengths, PafSample& out, std::string& err);

// np.histogram(ratios, bins=np.arange(0, 1.01, 0.01)) (:310): 100 bins, edge k = k * 0.01 as numpy's arange computes it, every bin closed
// on the left, the last one on the right as well; values outside [0, 1] (and NaN) are not counted.  labels = edges[1:]
void end_histogram(const std::vector<double>& ratios, std::vector<long long>& counts, std::vector<double>& labels);

// grid indices arange(start, end + 1, step) and the cell centres (idx[k] + idx[k + 1]) // 2 (:252-267); false: fewer than two indices
// or a non-positive step (and, as a guard for the loop, more than 2^20 indices: kde_build_model refuses above 4096 cells with ELIMIT before)
bool kde_grid_axes(long long start, long long end, long long step, std::vector<long long>& idx, std::vector<double>& centres);

// printModelJson (:298-320): P is row-major [g][g] for (centre i, centre j); "data" is P.T flattened.  Written to <path>.tmp first and
// renamed, so a failure leaves no partial file.
bool write_trc_model_json(const std::string& path, const std::vector<double>& P, const std::vector<long long>& idx,
                          const std::vector<long long>& counts, const std::vector<double>& labels, std::string& err);

// what tksmseq_model_truncation does, with what it found for the module's log
struct KdeBuildInfo {
    uint64_t n_pairs = 0, n_ratios = 0;
    bool searched = false;
    double bandwidth = 0.0;
    double scores[30] = {};
};
int kde_build_model(tksmseq_ctx* ctx, const tksmseq_kde_model_params* p, const char* paf_path, const char* out_path, KdeBuildInfo* info);

}  // namespace tkh
