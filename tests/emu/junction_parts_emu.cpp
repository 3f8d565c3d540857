// tests/emu/junction_parts_emu.cpp — TEST-ONLY: the kernels of the PARTITIONED junction build (sibeliaz_amd/csrc/lcb_junction_kernels.h,
// unmodified) on the lockstep wavefront emulator, driven like csrc/junctions.hip drives them: partition after partition insert (with
// regrowth of that partition's table alone, or a split of the partition where the table may not grow) and mark, then the table of the
// junction k-mers and the tiles in file order. junction_parts_emu <k> <table_log2> <tile_windows> <partitions> <max_log2, 0 = none> <out>
// <fasta...>; tests/test_junction_partitions_emu.py compares the file with lcb-mkgraph's.
#include <hip/hip_runtime.h>     // the shadow header of this directory

// what these kernels use beyond the block finder's kernels
#include <algorithm>
using std::min;
static inline uint32_t emu_shfl_up(uint32_t v, int d, const char* f, int l) {
    int lane = emu_thread_idx().x & 63; int src = lane >= d ? lane - d : lane;
    return (uint32_t)emu_collective(EMU_SHFL, (uint64_t)v, src, f, l);
}
#define __shfl_up(v, d) emu_shfl_up((v), (d), __FILE__, __LINE__)
static inline int emu_sync_count(int p) {
    static thread_local int cnt;
    if (emu_thread_idx().x == 0) cnt = 0;
    __syncthreads(); if (p) cnt++; __syncthreads(); int r = cnt; __syncthreads(); return r;
}
#define __syncthreads_count(p) emu_sync_count((p) ? 1 : 0)
static inline unsigned long long atomicCAS(unsigned long long* a, unsigned long long cmp, unsigned long long val) { unsigned long long old = *a; if (old == cmp) *a = val; return old; }
static inline int __popc(uint32_t x) { return __builtin_popcount(x); }

#include <cstring>
#include <string>
#include <vector>

#include "emu_runtime.h"
#include "lcb_fasta.h"
#include "lcb_junction_kernels.h"
using namespace lcb_junction;
template <class F> void launch(uint32_t grid, int threads, F body) { for (uint32_t b = 0; b < grid; b++) emu_run_block(b, threads / 64, body); }
int main(int argc, char** argv) {
    if (argc < 8) { fprintf(stderr, "usage: junction_parts_emu k table_log2 tile_windows partitions max_log2 out fasta...\n"); return 2; }
    int k = atoi(argv[1]); uint32_t capLog2 = atoi(argv[2]); uint32_t tileWindows = atoi(argv[3]); uint32_t P = atoi(argv[4]); uint32_t maxLog2 = atoi(argv[5]);
    std::string out = argv[6];
    std::vector<lcb_fasta::Record> rec;
    for (int i = 7; i < argc; i++) lcb_fasta::readFasta(argv[i], rec);
    std::vector<uint64_t> base(rec.size() + 1), recLen(rec.size());
    uint64_t len = 1;
    for (size_t r = 0; r < rec.size(); r++) { base[r] = len; len += rec[r].seq.size() + 1; recLen[r] = rec[r].seq.size(); }
    std::vector<uint8_t> codes(len, 4);
    for (size_t r = 0; r < rec.size(); r++) for (size_t i = 0; i < rec[r].seq.size(); i++) { int c = lcb_fasta::code(rec[r].seq[i]); codes[base[r] + i] = c < 0 ? 4 : c; }
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
            launch(gridAll, JT, [&]() { junctionInsertPart(codes.data(), len, k, key.data(), val.data(), mask, &st, q.M, q.r); });
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
        launch(gridAll, JT, [&]() { junctionMarkPart(codes.data(), len, k, key.data(), val.data(), mask, q.M, q.r, bitmap.data(), &marked, &st); });
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
        launch(gridAll, JT, [&]() { junctionFillMarked(codes.data(), len, k, bitmap.data(), key.data(), val.data(), mask, &st); });
        if (!tooFull()) break;
        rebuilds++;
    }
    if (st.lost) { fprintf(stderr, "LOST (fill)\n"); return 1; }
    for (uint64_t h = 0; h <= mask; h++) if (key[h] && !(val[h] & 0x100)) { fprintf(stderr, "a key of the junction table is no junction\n"); return 1; }
    uint32_t tileBuf = std::min<uint64_t>(tileWindows, len);
    std::vector<unsigned long long> wslot(tileBuf); std::vector<JRecord> o(tileBuf); std::vector<uint32_t> cj((tileBuf + JT - 1) / JT), cf((tileBuf + JT - 1) / JT);
    FILE* f = fopen(out.c_str(), "wb"); size_t curRec = 0; uint64_t occ = 0; int tiles = 0;
    if (!f) { fprintf(stderr, "cannot create %s\n", out.c_str()); return 1; }
    auto put = [&](uint32_t pos, int64_t id) { fwrite(&pos, 4, 1, f); fwrite(&id, 8, 1, f); };
    for (uint64_t t0 = 0; t0 < len; t0 += tileWindows, tiles++) {
        uint32_t tileLen = std::min<uint64_t>(tileWindows, len - t0), nb = (tileLen + JT - 1) / JT;
        launch((tileLen + J_WPB - 1) / J_WPB, JT, [&]() { junctionClassifyMarked(codes.data(), len, k, bitmap.data(), key.data(), val.data(), mask, t0, tileLen, wslot.data(), &st); });
        launch(nb, JT, [&]() { junctionMarkFirst(wslot.data(), val.data(), tileLen, cj.data(), cf.data()); });
        launch(1, 1024, [&]() { junctionScan(cj.data(), cf.data(), nb, &st); });
        launch(nb, JT, [&]() { junctionAssignIds(wslot.data(), val.data(), tileLen, cf.data(), &st); });
        launch(nb, JT, [&]() { junctionEmit(wslot.data(), val.data(), tileLen, cj.data(), t0, o.data()); });
        if (st.lost) { fprintf(stderr, "LOST (tiles)\n"); return 1; }
        for (uint64_t q = 0; q < st.totJ; q++) {
            while (o[q].g >= base[curRec] + recLen[curRec]) { put(0xFFFFFFFFu, INT64_MAX); curRec++; }
            put((uint32_t)(o[q].g - base[curRec]), o[q].id);
        }
        occ += st.totJ;
    }
    for (; curRec < recLen.size(); curRec++) put(0xFFFFFFFFu, INT64_MAX);
    fclose(f);
    if (occ != marked) { fprintf(stderr, "%llu records for %llu marked windows\n", (unsigned long long)occ, marked); return 1; }
    // (one line the test reads: what the run went through)
    fprintf(stderr, "emu: records=%zu occ=%llu ids=%llu partitions=%u passes=%d slots_log2=%u junction_slots_log2=%u rebuilds=%d tiles=%d\n", rec.size(),
            (unsigned long long)occ, st.idNext, P, passes, maxSlotsLog2, jLog2, rebuilds, tiles);
}
