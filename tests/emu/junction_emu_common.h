// tests/emu/junction_emu_common.h — TEST-ONLY: what junction_emu.cpp and junction_parts_emu.cpp share: the shims the junction kernels
// need beyond hip/hip_runtime.h of this directory (emu_main.cpp compiles against that file with definitions of its own), FASTA ->
// code array as csrc/junctions.hip lays it out, launch, and the tile loop with the record writer.
#ifndef LCB_JUNCTION_EMU_COMMON_H
#define LCB_JUNCTION_EMU_COMMON_H
#include <hip/hip_runtime.h>     // the shadow header of this directory

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

struct Input {
    std::vector<uint64_t> base, recLen;     // of record r: its first position in codes[], its bases
    std::vector<uint8_t> codes;             // one breaker in front of the first record and one after every record
    uint64_t len = 1;
    Input(char** first, char** last) {
        std::vector<lcb_fasta::Record> rec;
        for (char** a = first; a != last; a++) lcb_fasta::readFasta(*a, rec);
        for (const lcb_fasta::Record& r : rec) { base.push_back(len); recLen.push_back(r.seq.size()); len += r.seq.size() + 1; }
        codes.assign(len, 4);
        for (size_t r = 0; r < rec.size(); r++) for (size_t i = 0; i < rec[r].seq.size(); i++) { int c = lcb_fasta::code(rec[r].seq[i]); codes[base[r] + i] = c < 0 ? 4 : c; }
    }
};

// The tiles in file order behind classify(t0, tileLen, wslot), and the junction file. false: a lookup missed.
template <class F> bool runTiles(const Input& in, uint32_t tileWindows, FILE* f, uint32_t* val, JState& st, uint64_t& occ, int& tiles, F classify) {
    uint32_t tileBuf = std::min<uint64_t>(tileWindows, in.len);
    std::vector<unsigned long long> wslot(tileBuf); std::vector<JRecord> o(tileBuf); std::vector<uint32_t> cj((tileBuf + JT - 1) / JT), cf((tileBuf + JT - 1) / JT);
    size_t curRec = 0;
    auto put = [&](uint32_t pos, int64_t id) { fwrite(&pos, 4, 1, f); fwrite(&id, 8, 1, f); };
    for (uint64_t t0 = 0; t0 < in.len; t0 += tileWindows, tiles++) {
        uint32_t tileLen = std::min<uint64_t>(tileWindows, in.len - t0), nb = (tileLen + JT - 1) / JT;
        launch((tileLen + J_WPB - 1) / J_WPB, JT, [&]() { classify(t0, tileLen, wslot.data()); });
        launch(nb, JT, [&]() { junctionMarkFirst(wslot.data(), val, tileLen, cj.data(), cf.data()); });
        launch(1, 1024, [&]() { junctionScan(cj.data(), cf.data(), nb, &st); });
        launch(nb, JT, [&]() { junctionAssignIds(wslot.data(), val, tileLen, cf.data(), &st); });
        launch(nb, JT, [&]() { junctionEmit(wslot.data(), val, tileLen, cj.data(), t0, o.data()); });
        if (st.lost) return false;
        for (uint64_t q = 0; q < st.totJ; q++) {
            while (o[q].g >= in.base[curRec] + in.recLen[curRec]) { put(0xFFFFFFFFu, INT64_MAX); curRec++; }
            put((uint32_t)(o[q].g - in.base[curRec]), o[q].id);
        }
        occ += st.totJ;
    }
    for (; curRec < in.recLen.size(); curRec++) put(0xFFFFFFFFu, INT64_MAX);
    return true;
}
#endif
