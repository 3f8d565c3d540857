// tests/emu/file_host_check.cpp — TEST-ONLY: the host's share of opening a junction file on the GPU (sibeliaz_amd/csrc/lcb_file_host.h: the
// tiling, the tile reader, the walk over the first raw indices of the runs, the record counts) as a stand-alone program, so that it can
// be compiled with -fsanitize=address,undefined and run on the CPU (tests/test_file_emu.py does). Every tile is read into a heap
// buffer of exactly its size; the first raw indices are made by a plain loop over the records, which stands for the kernels.
//   file_host_check <junctions> <tile> <fasta records>
// stdout: "records R separators S raw N chromosomes C tiles T blocks B", or "refused: <text>". Exit status 0 either way; 2 on usage.
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "lcb_file_host.h"

int main(int argc, char** argv)
{
    if (argc != 4) { fprintf(stderr, "usage: file_host_check <junctions> <tile> <fasta records>\n"); return 2; }
    try {
        lcb_file::Reader in(argv[1]);
        const lcb_file::Tiling T = lcb_file::tiling(in.bytes, (uint32_t)strtoul(argv[2], nullptr, 10));
        std::vector<unsigned long long> recFirst(1, lcb_file::FILE_NONE);
        uint64_t N = 0, seps = 0, seen = 0;
        bool open = true;                                  // the next record opens a run
        for (uint64_t t = 0; t < T.tiles; t++) {
            const size_t n = (size_t)T.count(t);
            std::unique_ptr<unsigned char[]> tile(new unsigned char[n * 12]);
            in.read(T, t, tile.get());
            if (T.first(t) != seen) throw LcbError("the tiles do not follow each other");
            for (size_t q = 0; q < n; q++, seen++) {
                uint32_t pos; int64_t id;
                memcpy(&pos, &tile[q * 12], 4); memcpy(&id, &tile[q * 12 + 4], 8);
                if (pos == 0xFFFFFFFFu || id == INT64_MAX) { seps++; recFirst.push_back(lcb_file::FILE_NONE); open = true; continue; }
                if (open) { recFirst.back() = N; open = false; }
                N++;
            }
        }
        if (seen != T.nRec || T.blocks() < (T.nRec + lcb_file::FILE_T - 1) / lcb_file::FILE_T) throw LcbError("the tiles do not cover the file");
        const size_t C = lcb_file::chromosomes(recFirst.data(), recFirst.size(), N);
        lcb_file::sameRecords((size_t)strtoull(argv[3], nullptr, 10), C);
        printf("records %llu separators %llu raw %llu chromosomes %zu tiles %llu blocks %llu\n", (unsigned long long)T.nRec, (unsigned long long)seps, (unsigned long long)N, C,
               (unsigned long long)T.tiles, (unsigned long long)T.blocks());
    } catch (LcbError& e) { printf("refused: %s\n", e.what()); }
    return 0;
}
