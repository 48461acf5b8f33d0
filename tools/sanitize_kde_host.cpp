// AddressSanitizer + UBSan over the host-only code of model-truncation (csrc/kde_host.cpp): the PAF reader incl. malformed lines, the
// end-ratio histogram, the grid axes and the model writer.  CPU only, never loaded into Python:
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-omit-frame-pointer -I tksm_amd/csrc -o /tmp/sanitize_kde_host \
//       tools/sanitize_kde_host.cpp tksm_amd/csrc/kde_host.cpp
//   /tmp/sanitize_kde_host tests/golden/kde_build/reads.paf /tmp/kde_host_out
// Prints one "key value..." line per result (tests/test_kde_build.py compares them with numpy and the reference-written fixtures).
#include "kde_host.h"
#include <cstdio>
#include <cstring>
#include <limits>
using namespace tkh;
int main(int argc, char** argv) {
    if (argc < 3) { fprintf(stderr, "usage: %s reads.paf out_dir\n", argv[0]); return 2; }
    const std::string dir = argv[2];
    for (int ml = 0; ml < 2; ml++) {
        PafSample s; std::string e;
        if (!read_paf_sample(argv[1], ml != 0, s, e)) { printf("error %s\n", e.c_str()); return 1; }
        double sx = 0, sy = 0;
        for (size_t i = 0; i < s.xy.size(); i += 2) { sx += s.xy[i]; sy += s.xy[i + 1]; }
        printf("sample %d %zu %zu %.17g %.17g\n", ml, s.xy.size() / 2, s.ratios.size(), sx, sy);
        std::vector<long long> counts; std::vector<double> labels;
        end_histogram(s.ratios, counts, labels);
        printf("hist %d", ml); for (long long c : counts) printf(" %lld", c); printf("\n");
        std::vector<long long> idx; std::vector<double> cen;
        kde_grid_axes(0, 3000, 100, idx, cen);
        std::vector<double> P(cen.size() * cen.size());
        for (size_t i = 0; i < P.size(); i++) P[i] = 1.0 / (double)(i + 3);
        const std::string out = dir + "/model_" + std::to_string(ml) + ".json";
        printf("write %d %d\n", ml, (int)write_trc_model_json(out, P, idx, counts, labels, e));
    }
    { PafSample s; std::string e; std::vector<long long> c{1}; std::vector<double> l{1.0}, P{1.0}; std::vector<long long> idx{0, 100};
      printf("unwritable %d\n", (int)write_trc_model_json(dir + "/no/such/dir/m.json", P, idx, c, l, e));
      P[0] = std::numeric_limits<double>::infinity();
      printf("nonfinite %d\n", (int)write_trc_model_json(dir + "/inf.json", P, idx, c, l, e)); }
    const char* texts[] = {"", "\n", "tp:A:P", "tp:A:P\n", "a\tb\tc\td\t+\tf\t10\t2\t8\ttp:A:P", "a\tb\tc\td\t-\tf\t10\t2\t8\tx\ty\tz\ttp:A:P\n", "a\tb\tc\td\t+\tf\t10\t2\t\ttp:A:P\n",
                           "a\tb\tc\td\t+\tf\t10\t2\t8x\ttp:A:P\n", "a\tb\tc\td\t+\tf\t 10 \t+2\t-8\ttp:A:P\n", "a\tb\tc\td\t+\tf\t99999999999999999999\t2\t8\ttp:A:P\n",
                           "a\tb\tc\td\t+\tf\t10\t0\t10\ttp:A:P\n", "a\tb\tc\td\t+\tf\t10\t2\t8\ttp:A:S\n", "a\tb\tc\td\t+\tf\t10\t2\t8tp:A:P"};
    for (const char* t : texts)
        for (int ml = 0; ml < 2; ml++) { PafSample s; std::string e; const bool ok = parse_paf_sample(t, strlen(t), ml != 0, s, e); printf("parse %d %d %zu %zu %s\n", ml, (int)ok, s.xy.size() / 2, s.ratios.size(), e.c_str()); }
    {   // bin edges: numpy's own doubles, the last bin closed on the right
        std::vector<double> r{0.0, 0.01, 0.0099999999999999985, 0.29, 0.28999999999999998, 0.29000000000000004, 0.57, 0.58, 0.99, 1.0, 1.0000000000000002, -1e-300, -0.0,
                              std::numeric_limits<double>::quiet_NaN(), std::numeric_limits<double>::infinity(), 0.07, 0.07000000000000001, 0.14, 0.14000000000000001};
        std::vector<long long> counts; std::vector<double> labels;
        end_histogram(r, counts, labels);
        printf("edges"); for (long long c : counts) printf(" %lld", c); printf("\n");
        printf("labels"); for (double l : labels) printf(" %.17g", l); printf("\n");
    }
    const long long axes[][3] = {{0, 10000, 100}, {0, 1050, 100}, {0, 99, 100}, {0, 100, 100}, {-250, 250, 100}, {5, 4, 1}, {0, 10, 0}, {0, 10, -1}, {7, 1000, 333}};
    for (auto& a : axes) {
        std::vector<long long> idx; std::vector<double> cen;
        printf("axes %lld %lld %lld %d", a[0], a[1], a[2], (int)kde_grid_axes(a[0], a[1], a[2], idx, cen));
        for (long long v : idx) printf(" %lld", v);
        printf(" |"); for (double v : cen) printf(" %.17g", v);
        printf("\n");
    }
    return 0;
}
