// tests/emu/junction_parts_emu.cpp — TEST-ONLY: the kernels of the PARTITIONED junction build (sibeliaz_amd/csrc/lcb_junction_kernels.h,
// unmodified) on the lockstep wavefront emulator, driven like csrc/junctions.hip drives them: partition after partition insert (with
// regrowth of that partition's table alone, or a split of the partition where the table may not grow) and mark, then the table of the
// junction k-mers and the tiles in file order. junction_parts_emu <k> <table_log2> <tile_windows> <partitions> <max_log2, 0 = none> <out>
// <fasta...>; tests/test_junction_partitions_emu.py compares the file with lcb-mkgraph's.
#include "junction_emu_common.h"
int main(int argc, char** argv) {
    if (argc < 8) { fprintf(stderr, "usage: junction_parts_emu k table_log2 tile_windows partitions max_log2 out fasta...\n"); return 2; }
    int k = atoi(argv[1]); uint32_t capLog2 = atoi(argv[2]); uint32_t tileWindows = atoi(argv[3]); uint32_t P = atoi(argv[4]); uint32_t maxLog2 = atoi(argv[5]);
    std::string out = argv[6];
    const Input in(argv + 7, argv + argc);
    const uint64_t len = in.len;
    const uint8_t* const codes = in.codes.data();
    std::vector<unsigned long long> key, bitmap((len + 63) / 64, 0); std::vector<uint32_t> val; JState st; uint64_t mask = 0; unsigned long long marked = 0;
    int rebuilds = 0, passes = 0; uint32_t maxSlotsLog2 = 0;
    const uint32_t gridAll = (len + J_WPB - 1) / J_WPB;
    auto fresh = [&](uint32_t log2) { uint64_t cap = 1ull << log2; mask = cap - 1; key.assign(cap, 0); val.assign(cap, 0); memset(&st, 0, sizeof(st)); };
    auto tooFull = [&]() { return st.full || st.used * 10 > (mask + 1) * 9; };

    // ---- phase A
    struct Part { uint32_t M, r, log2; };
    std::vector<Part> todo;
    for (uint32_t p = P; p-- > 0;) todo.push_back(Part{P, p, capLog2});
    while (!todo.empty()) {
        Part q = todo.back(); todo.pop_back();
        bool split = false;
        for (;;) {
            fresh(q.log2);
            launch(gridAll, JT, [&]() { junctionInsertPart(codes, len, k, key.data(), val.data(), mask, &st, q.M, q.r); });
            if (!tooFull()) break;
            rebuilds++;
            if (!maxLog2 || q.log2 < maxLog2) { q.log2++; continue; }
            if (2 * q.M > (uint32_t)J_MAX_PARTS) { fprintf(stderr, "a partition cannot be split any further\n"); return 1; }
            todo.push_back(Part{2 * q.M, q.r + q.M, q.log2}); todo.push_back(Part{2 * q.M, q.r, q.log2});
            split = true;
            break;
        }
        if (split) continue;
        maxSlotsLog2 = std::max(maxSlotsLog2, q.log2);
        launch(gridAll, JT, [&]() { junctionMarkPart(codes, len, k, key.data(), val.data(), mask, q.M, q.r, bitmap.data(), &marked, &st); });
        if (st.lost) { fprintf(stderr, "LOST (mark)\n"); return 1; }
        passes++;
    }
    unsigned long long bits = 0;
    for (unsigned long long w : bitmap) bits += __builtin_popcountll(w);
    if (bits != marked) { fprintf(stderr, "marked %llu windows, the bitmap holds %llu bits\n", marked, bits); return 1; }

    // ---- phase B: the table of junction k-mers (from the same small capacity: it has to grow too), then the tiles
    uint32_t jLog2 = capLog2;
    for (;; jLog2++) {
        fresh(jLog2);
        launch(gridAll, JT, [&]() { junctionFillMarked(codes, len, k, bitmap.data(), key.data(), val.data(), mask, &st); });
        if (!tooFull()) break;
        rebuilds++;
    }
    if (st.lost) { fprintf(stderr, "LOST (fill)\n"); return 1; }
    for (uint64_t h = 0; h <= mask; h++) if (key[h] && !(val[h] & 0x100)) { fprintf(stderr, "a key of the junction table is no junction\n"); return 1; }
    FILE* f = fopen(out.c_str(), "wb"); uint64_t occ = 0; int tiles = 0;
    if (!f) { fprintf(stderr, "cannot create %s\n", out.c_str()); return 1; }
    if (!runTiles(in, tileWindows, f, val.data(), st, occ, tiles, [&](uint64_t t0, uint32_t tileLen, unsigned long long* wslot) {
            junctionClassifyMarked(codes, len, k, bitmap.data(), key.data(), val.data(), mask, t0, tileLen, wslot, &st);
        })) { fprintf(stderr, "LOST (tiles)\n"); return 1; }
    fclose(f);
    if (occ != marked) { fprintf(stderr, "%llu records for %llu marked windows\n", (unsigned long long)occ, marked); return 1; }
    // (one line the test reads: what the run went through)
    fprintf(stderr, "emu: records=%zu occ=%llu ids=%llu partitions=%u passes=%d slots_log2=%u junction_slots_log2=%u rebuilds=%d tiles=%d\n", in.recLen.size(),
            (unsigned long long)occ, st.idNext, P, passes, maxSlotsLog2, jLog2, rebuilds, tiles);
}
