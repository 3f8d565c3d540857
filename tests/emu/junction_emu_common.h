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

// The `scan` mode: junctionScan alone on generated counts of nb workgroups (every content of scan_cases.h that 32-bit entries have), two
// tiles in a row through one JState, against serial 64-bit prefix sums: every offset, totJ, totF, tileIdBase and idNext after each tile,
// and the fields of JState that the kernel does not own. 0 = equal.
#include "scan_cases.h"
static int runJunctionScan(uint32_t nb) {
    const uint32_t per = (nb + 1023) / 1024;
    for (const char* content : SCAN_CONTENTS) {
        std::vector<uint32_t> probe;
        if (!scanFill(probe, nb, content, per, 0)) continue;
        JState st;
        memset(&st, 0, sizeof(st));
        st.used = 77; st.idNext = 5; st.tileIdBase = 0xEEEE; st.totJ = st.totF = 0xEEEE;      // (ids given before; stale values of an earlier tile)
        unsigned long long idNext = st.idNext;
        for (int tile = 0; tile < 2; tile++) {
            std::vector<uint32_t> cj, cf;
            scanFill(cj, nb, content, per, 10 + 2 * tile);
            scanFill(cf, nb, content, per, 11 + 2 * tile);
            for (uint32_t q = 0; q < nb; q++) cf[q] = std::min(cf[q], cj[q]);      // first occurrences are junctions
            std::vector<unsigned long long> wantJ, wantF;
            const unsigned long long totJ = scanSerial(cj, wantJ), totF = scanSerial(cf, wantF);
            cj.push_back(0xEEEEEEEEu); cf.push_back(0xEEEEEEEEu);
            launch(1, 1024, [&]() { junctionScan(cj.data(), cf.data(), nb, &st); });
            if (cj[nb] != 0xEEEEEEEEu || cf[nb] != 0xEEEEEEEEu) { fprintf(stderr, "junctionScan nb %u %s tile %d: the kernel wrote behind an array\n", nb, content, tile); return 1; }
            for (uint32_t q = 0; q < nb; q++)
                if (cj[q] != wantJ[q] || cf[q] != wantF[q]) {
                    fprintf(stderr, "junctionScan nb %u %s tile %d: entry %u is (%u, %u), the serial scan has (%llu, %llu)\n", nb, content, tile, q, cj[q], cf[q], wantJ[q], wantF[q]);
                    return 1;
                }
            if (st.totJ != totJ || st.totF != totF || st.tileIdBase != idNext || st.idNext != idNext + totF || st.used != 77 || st.full || st.lost) {
                fprintf(stderr, "junctionScan nb %u %s tile %d: totJ %llu totF %llu tileIdBase %llu idNext %llu used %llu full %u lost %u, expected %llu %llu %llu %llu 77 0 0\n", nb, content, tile,
                        st.totJ, st.totF, st.tileIdBase, st.idNext, st.used, st.full, st.lost, totJ, totF, idNext, idNext + totF);
                return 1;
            }
            idNext += totF;
            printf("scan junctionScan nb %u per %u %s tile %d totJ %llu totF %llu\n", nb, per, content, tile, totJ, totF);
        }
    }
    return 0;
}
#endif
