// tests/emu/junction_emu.cpp — TEST-ONLY: the kernels of the GPU junction finder (sibeliaz_amd/csrc/lcb_junction_kernels.h, unmodified) on the
// lockstep wavefront emulator, driven like csrc/junctions.hip drives them (table regrowth, tiles in file order), writing the junction
// file: junction_emu <k> <table_log2> <tile_windows> <out> <fasta...>. tests/test_junctions_emu.py compares it with lcb-mkgraph's.
// junction_emu scan <nb>: junctionScan alone on generated counts (junction_emu_common.h); tests/test_scan_pieces_emu.py runs it.
#include "junction_emu_common.h"
int main(int argc, char** argv) {
    if (argc == 3 && std::string(argv[1]) == "scan") return runJunctionScan((uint32_t)strtoul(argv[2], nullptr, 10));
    if (argc < 6) { fprintf(stderr, "usage: junction_emu <k> <table_log2> <tile_windows> <out> <fasta...> | junction_emu scan <nb>\n"); return 2; }
    int k = atoi(argv[1]); uint32_t capLog2 = atoi(argv[2]); uint32_t tileWindows = atoi(argv[3]); std::string out = argv[4];
    const Input in(argv + 5, argv + argc);
    const uint64_t len = in.len;
    std::vector<unsigned long long> key; std::vector<uint32_t> val; JState st; uint64_t mask; int rebuilds = 0;
    for (;; capLog2++) {
        uint64_t cap = 1ull << capLog2; mask = cap - 1; key.assign(cap, 0); val.assign(cap, 0); memset(&st, 0, sizeof(st));
        uint32_t grid = (len + J_WPB - 1) / J_WPB;
        launch(grid, JT, [&]() { junctionInsert(in.codes.data(), len, k, key.data(), val.data(), mask, &st); });
        if (!st.full && st.used * 10 <= cap * 9) break;
        rebuilds++;
    }
    FILE* f = fopen(out.c_str(), "wb"); uint64_t occ = 0; int tiles = 0;
    if (!runTiles(in, tileWindows, f, val.data(), st, occ, tiles, [&](uint64_t t0, uint32_t tileLen, unsigned long long* wslot) {
            junctionClassify(in.codes.data(), len, k, key.data(), val.data(), mask, t0, tileLen, wslot, &st);
        })) { fprintf(stderr, "LOST\n"); return 1; }
    fclose(f);
    fprintf(stderr, "emu: %zu records, %llu occ, %llu ids, slots 2^%u, rebuilds %d, tiles %d\n", in.recLen.size(), (unsigned long long)occ, st.idNext, capLog2, rebuilds, tiles);
}
