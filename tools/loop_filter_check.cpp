// loop_filter_check.cpp -- the bounds table of k_loop's first thresholds (tksm_amd/csrc/loop_filter.h) run on the host: reads nk
// little-endian u32 thresholds from a file, writes the 2048 u16 entries of the table, and on request classifies a list of
// (kx, dw) u32 pairs against it (one byte per pair: 0 no-op, 1 changing, 2 undecided) with the function the kernel uses.
// tests/test_loop_filter.py compares both outputs with a numpy restatement, once from a plain build and once under
// -fsanitize=address,undefined.
//     g++ -O2 -std=c++17 -I tksm_amd/csrc tools/loop_filter_check.cpp -o loop_filter_check
//     ./loop_filter_check T0.bin TABLE.bin [PAIRS.bin CLASSES.bin]
#include <cstdio>
#include <vector>

#include "loop_filter.h"

using namespace tklf;

template <class T>
static bool read_all(const char* path, std::vector<T>& v) {
    FILE* fp = fopen(path, "rb");
    if (!fp) return false;
    T buf[4096];
    size_t g;
    while ((g = fread(buf, sizeof(T), 4096, fp)) > 0) v.insert(v.end(), buf, buf + g);
    fclose(fp);
    return true;
}

template <class T>
static bool write_all(const char* path, const std::vector<T>& v) {
    FILE* fp = fopen(path, "wb");
    if (!fp) return false;
    const bool ok = fwrite(v.data(), sizeof(T), v.size(), fp) == v.size();
    return fclose(fp) == 0 && ok;
}

int main(int argc, char** argv) {
    if (argc != 3 && argc != 5) { fprintf(stderr, "usage: loop_filter_check T0.bin TABLE.bin [PAIRS.bin CLASSES.bin]\n"); return 2; }
    std::vector<uint32_t> t0;
    if (!read_all(argv[1], t0)) return 2;
    std::vector<uint16_t> tab(LOOP_FILTER_KEYS);
    loop_filter_build(t0.data(), t0.size(), tab.data());
    if (!write_all(argv[2], tab)) return 2;
    if (argc == 5) {
        std::vector<uint32_t> pairs;
        if (!read_all(argv[3], pairs) || (pairs.size() & 1)) return 2;
        std::vector<uint8_t> cls(pairs.size() / 2);
        for (size_t i = 0; i < cls.size(); i++) {
            if (pairs[2 * i] >= t0.size()) { fprintf(stderr, "pair %zu: k-mer %u of %zu\n", i, pairs[2 * i], t0.size()); return 1; }
            cls[i] = (uint8_t)loop_filter_classify(tab[loop_filter_key(pairs[2 * i])], pairs[2 * i + 1]);
        }
        if (!write_all(argv[4], cls)) return 2;
    }
    return 0;
}
