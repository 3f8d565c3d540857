// lcb_file_host.h — the host's share of opening a junction file on the GPU (junctions.hip), free of any HIP call so that
// tests/emu/file_emu.cpp drives the emulated kernels with it and tests/emu/file_host_check.cpp runs it under a sanitizer: how the file
// is cut into tiles, the reader that fills one staging buffer per tile, the walk over the downloaded first raw indices of the runs and
// the comparison of the record counts - with the texts lcb_graph_load_impl (graph.cpp) has for the same files.
#ifndef LCB_FILE_HOST_H
#define LCB_FILE_HOST_H

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <string>

#include "lcb_host.h"

namespace lcb_file {

constexpr uint32_t FILE_T = 256;                   // = lcb_filek::F_T
constexpr uint32_t FILE_TILE = 1u << 22;           // records per upload tile when the options say 0
constexpr unsigned long long FILE_NONE = ~0ull;    // = lcb_graphk::G_NONE

// nRec records of 12 bytes (a remainder of 1 to 11 bytes is ignored, as the loader ignores it) in `tiles` tiles of `tile` records,
// a tile in `bpt` workgroups.
struct Tiling {
    uint64_t nRec = 0, tiles = 0;
    uint32_t tile = 1, bpt = 1;
    uint64_t first(uint64_t t) const { return t * tile; }
    uint64_t count(uint64_t t) const { return std::min<uint64_t>(tile, nRec - first(t)); }
    uint64_t blocks() const { return tiles * bpt; }
};
inline Tiling tiling(uint64_t fileBytes, uint32_t tileRecords)
{
    Tiling T;
    T.nRec = fileBytes / 12;
    T.tile = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(tileRecords ? tileRecords : FILE_TILE, T.nRec));
    T.bpt = (T.tile + FILE_T - 1) / FILE_T;
    T.tiles = (T.nRec + T.tile - 1) / T.tile;
    return T;
}

// The file, tile after tile into a buffer of the caller (a pinned staging buffer in junctions.hip). Closed when the reader dies.
struct Reader {
    FILE* f = nullptr;
    uint64_t bytes = 0;
    explicit Reader(const std::string& file)
    {
        f = fopen(file.c_str(), "rb");
        if (!f) throw LcbError("Can't read the input file");                            // junctionapi.h:46-49
        fseek(f, 0, SEEK_END);
        const long sz = ftell(f);
        fseek(f, 0, SEEK_SET);
        bytes = sz > 0 ? (uint64_t)sz : 0;
    }
    Reader(const Reader&) = delete;
    Reader& operator=(const Reader&) = delete;
    ~Reader() { if (f) fclose(f); }
    // Tile t of T -> dst (T.count(t) * 12 bytes). The tiles are asked for in order.
    void read(const Tiling& T, uint64_t t, void* dst)
    {
        const size_t want = (size_t)T.count(t) * 12;
        if (fread(dst, 1, want, f) != want) throw LcbError("Can't read the input file");
    }
};

// recFirst[s]: the first raw index of run s (the records between separators s - 1 and s), FILE_NONE for a run without a record.
// -> C, the chromosomes: the leading runs that have records. A run with records behind one without is what neither the reference nor
// the loader can represent; runs without records at the end are trailing separators.
inline size_t chromosomes(const unsigned long long* recFirst, size_t runs, uint64_t N)
{
    size_t C = 0;
    while (C < runs && recFirst[C] != FILE_NONE) C++;
    for (size_t r = C; r < runs; r++)
        if (recFirst[r] != FILE_NONE) throw LcbError("the junction file has a chromosome without junctions (unsupported)");
    for (size_t c = 0; c < C; c++)
        if (recFirst[c] >= N || (c ? recFirst[c] <= recFirst[c - 1] : recFirst[c] != 0)) throw LcbError("internal error: the first raw indices of the runs do not ascend");
    return C;
}

inline void sameRecords(size_t fastaRecords, size_t C)
{
    if (fastaRecords > C) throw LcbError("the FASTA input has more records than the junction file has chromosomes");
    if (fastaRecords < C) throw LcbError("the FASTA input has fewer records than the junction file has chromosomes");
}

}  // namespace lcb_file
#endif
