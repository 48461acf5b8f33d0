// glue_cut_check.cpp -- stand-alone driver of tksm_amd/csrc/glue_cut.h (no HIP, no library), for tests/test_glue_shuffle.py, which builds it
// plain and with -fsanitize=address,undefined.
//   glue_cut_check cut FILE FIRST JOINS      one line "found offset molecules": glue_cut() on the file's text
//   glue_cut_check pieces FILE BYTES JOINS   one line "first molecules length" per piece, then the pieces' bytes on stderr: the file read in
//                                            chunks of BYTES by ChunkReader, cut by GlueHold -- the reader of `tksm unsegment`
// JOINS is a string of 0 / 1: character g says whether molecule g of the whole input joins its predecessor (beyond its end: 0).
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "glue_cut.h"
#include "module_log.h"

int main(int argc, char** argv) {
    if (argc != 5) { fprintf(stderr, "usage: glue_cut_check cut FILE FIRST JOINS | pieces FILE BYTES JOINS\n"); return 2; }
    const std::string mode = argv[1], flags = argv[4];
    auto joins = [&](uint64_t g) { return g < flags.size() && flags[(size_t)g] == '1'; };
    FILE* f = fopen(argv[2], "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[2]); return 2; }
    if (mode == "cut") {
        std::vector<char> text;
        char buf[4096];
        for (size_t n; (n = fread(buf, 1, sizeof buf, f)) > 0;) text.insert(text.end(), buf, buf + n);
        fclose(f);
        const tkmod::GlueCut k = tkmod::glue_cut(text.data(), text.size(), strtoull(argv[3], nullptr, 10), joins);
        printf("%d %zu %llu\n", k.found ? 1 : 0, k.offset, (unsigned long long)k.molecules);
        return 0;
    }
    if (mode != "pieces") return 2;
    tkmod::ChunkReader rd;
    rd.in = f;
    rd.bytes = strtoull(argv[3], nullptr, 10);
    tkmod::GlueHold hold;
    std::vector<char> chunk, piece;
    uint64_t first = 0, molecules = 0, seq = 0;
    for (;;) {
        piece.clear();
        if (rd.next(chunk)) { if (!hold.push(chunk, first, joins, piece, molecules)) continue; }
        else if (seq && hold.held.empty()) break;
        else hold.flush(piece, molecules);
        printf("%llu %llu %zu\n", (unsigned long long)first, (unsigned long long)molecules, piece.size());
        if (!piece.empty()) fwrite(piece.data(), 1, piece.size(), stderr);
        first += molecules; seq++;
    }
    fclose(f);
    return 0;
}
