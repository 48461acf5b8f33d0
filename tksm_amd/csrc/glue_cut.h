// glue_cut.h -- where `tksm unsegment` may end a piece of its input.  No HIP, no library: tools/glue_cut_check.cpp compiles it alone.
//
// A chain of glued molecules must not be split over two pieces, so a piece ends only in front of a record whose first unrolled molecule g
// does not join its predecessor (joins(g) == 0): that molecule is a head whichever piece holds it, and every decision behind it depends
// on indices alone.  ChunkReader (module_log.h) cuts the input at record boundaries; glue_cut() finds, inside such a chunk, the LAST
// record boundary of that kind.  The reader holds back the text behind it and puts it in front of the next chunk.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

namespace tkmod {

// found: the text has a record in front of which a piece may end; offset: where the last such record starts (0: the text's first record);
// molecules: the unrolled molecules of the records before it.  Without one: {false, 0, all molecules of the text}.
struct GlueCut { bool found; size_t offset; uint64_t molecules; };

// text[0, len): MDF text that starts at a record header (or is empty); a last line without a newline is a line.  first: the index of its
// first unrolled molecule in the whole input.  joins(g) != 0: molecule g is glued to molecule g - 1.  A record's molecules are counted as
// count_reads counts them: its depth column, a negative or unreadable one as 0.
template <class Joins>
GlueCut glue_cut(const char* text, size_t len, uint64_t first, Joins joins) {
    GlueCut cut{false, 0, 0};
    uint64_t n = 0;
    const char* p = text;
    const char* const end = text + len;
    while (p < end) {
        const char* nl = (const char*)memchr(p, '\n', (size_t)(end - p));
        const char* le = nl ? nl : end;
        if (*p == '+') {
            if (!joins(first + n)) cut = GlueCut{true, (size_t)(p - text), n};
            const char* t = (const char*)memchr(p, '\t', (size_t)(le - p));
            uint64_t d = 0;
            if (t) {
                const char* q = t + 1;
                const bool neg = q < le && *q == '-';
                if (neg) q++;
                while (q < le && *q >= '0' && *q <= '9') d = d * 10 + (uint64_t)(*q++ - '0');
                if (neg) d = 0;
            }
            n += d;
        }
        p = nl ? nl + 1 : end;
    }
    if (!cut.found) cut.molecules = n;
    return cut;
}

// The text a reader holds back between chunks.  It starts at a record that does not join (or at the start of the input) and has no other
// place to cut, so only each new chunk is searched.  push(): a chunk of whole records behind what is held; true when a piece is ready --
// `piece` then holds everything up to the chunk's last cut, `molecules` its molecule count, and the rest is held; false: read on.
// flush(): at the end of the input, what is held is the last piece (possibly empty).  `first` is the index of the first molecule of
// the next piece (the held text's first molecule).
struct GlueHold {
    std::vector<char> held;
    uint64_t held_molecules = 0;
    template <class Joins>
    bool push(std::vector<char>& chunk, uint64_t first, Joins joins, std::vector<char>& piece, uint64_t& molecules) {
        const GlueCut k = glue_cut(chunk.data(), chunk.size(), first + held_molecules, joins);
        if (!k.found || (k.offset == 0 && held.empty())) {       // (a cut at the very start of a piece would make an empty piece)
            held.insert(held.end(), chunk.begin(), chunk.end());
            held_molecules += k.found ? glue_cut(chunk.data(), chunk.size(), 0, [](uint64_t) { return true; }).molecules : k.molecules;
            return false;
        }
        held.insert(held.end(), chunk.begin(), chunk.begin() + (ptrdiff_t)k.offset);
        molecules = held_molecules + k.molecules;
        piece.swap(held);
        held.assign(chunk.begin() + (ptrdiff_t)k.offset, chunk.end());
        held_molecules = glue_cut(held.data(), held.size(), 0, [](uint64_t) { return true; }).molecules;
        return true;
    }
    void flush(std::vector<char>& piece, uint64_t& molecules) {
        piece.swap(held);
        held.clear();
        molecules = held_molecules; held_molecules = 0;
    }
};

}  // namespace tkmod
