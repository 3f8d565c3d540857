// tests/emu/handover_emu.cpp — TEST-ONLY: the kernels of the hand-over route (sibeliaz_amd/csrc/lcb_handover_kernels.h, unmodified) on the
// lockstep wavefront emulator, behind the emulated table kernels (lcb_table_kernels.h), driven like csrc/tables.hip drives them on
// lcb_open_fasta's route: keys + counts, scan, radix sort, then handOccChr over the sorted payloads; and handPatch over a posCh that
// holds the graph build's sentinel wherever the code bytes have no letter. Fed the graph lcb_graph_load_impl makes of a junction file
// written by the CPU lcb-mkgraph, they must give back that graph's own host CSR and characters:
//   occChr                      = graph.cpp's occChr
//   the widened payload         = occG            (and the widened scan = occStart)
//   the compactSmall decision   = the host's      (the arithmetic of device.hip's createPools, from the downloaded lists)
//   posCh after handPatch       = the loader's posCh at the device indices of the plan, nothing written anywhere else
// once with Q = uint32_t on the dense plan and once with Q = unsigned long long on a plan with seg_cap 64 and seg_gap 64 (a larger cap
// where 64 would need more than 32 segments); the patch runs on both plans.
//   handover_emu <junctions> <k> <abundance> <fasta> [<fasta> ...]
// Exit status 0 = equal; otherwise the first difference on stderr. tests/test_handover_emu.py runs it.
#include <hip/hip_runtime.h>     // the shadow header of this directory

#include <algorithm>
#include <string>
#include <vector>
template <class V> static inline uint64_t emu_shfl_up(V v, int d, const char* f, int l)
{
    const int lane = emu_thread_idx().x & 63, src = lane >= d ? lane - d : lane;
    return emu_collective(EMU_SHFL, (uint64_t)v, src, f, l);
}
#define __shfl_up(v, d) emu_shfl_up((v), (d), __FILE__, __LINE__)

#include "emu_runtime.h"
#include "lcb_fasta.h"
#include "lcb_handover_kernels.h"
#include "lcb_host.h"
#include "lcb_segments.h"
#include "lcb_table_kernels.h"
using namespace lcb_tablek;
using namespace lcb_handk;

template <class F> void launch(uint64_t grid, int threads, F body) { for (uint64_t b = 0; b < grid; b++) emu_run_block((uint32_t)b, threads / 64, body); }
static uint64_t blocksOf(uint64_t n, uint64_t per) { return (n + per - 1) / per; }

#define FAIL(...) do { fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); return 1; } while (0)

// The 32-bit and the 64-bit instantiation of the kernels under one name each.
template <class Q> struct K;
template <> struct K<uint32_t> {
    static void keys(const TablePlan& pl, const int32_t* id, uint32_t* k, uint32_t* p, uint32_t* c, uint64_t P) { tableKeys32(pl, id, k, p, c, P); }
    static void scan(uint32_t* a, uint64_t n, unsigned long long* t) { tableScan32(a, n, t); }
    static void tileHist(const uint32_t* k, uint64_t n, int p, uint32_t* h, uint32_t nt) { tableTileHist32(k, n, p, h, nt); }
    static void scatter(const uint32_t* ki, const uint32_t* pi, uint32_t* ko, uint32_t* po, uint64_t n, int p, const uint32_t* o, uint32_t nt) { tableScatter32(ki, pi, ko, po, n, p, o, nt); }
    static void occChr(const TablePlan& pl, const uint32_t* p, uint32_t* c, uint64_t P) { handOccChr32(pl, p, c, P); }
};
template <> struct K<unsigned long long> {
    typedef unsigned long long Q;
    static void keys(const TablePlan& pl, const int32_t* id, uint32_t* k, Q* p, Q* c, uint64_t P) { tableKeys64(pl, id, k, p, c, P); }
    static void scan(Q* a, uint64_t n, unsigned long long* t) { tableScan64(a, n, t); }
    static void tileHist(const uint32_t* k, uint64_t n, int p, Q* h, uint32_t nt) { tableTileHist64(k, n, p, h, nt); }
    static void scatter(const uint32_t* ki, const Q* pi, uint32_t* ko, Q* po, uint64_t n, int p, const Q* o, uint32_t nt) { tableScatter64(ki, pi, ko, po, n, p, o, nt); }
    static void occChr(const TablePlan& pl, const Q* p, uint32_t* c, uint64_t P) { handOccChr64(pl, p, c, P); }
};

static const uint8_t GAP_BYTE = 0xEE;         // what the gaps of the device's posCh hold: a write inside a gap shows
static const uint8_t SENTINEL = 0xFF;         // G_PATCH of lcb_graph_kernels.h

// createPools of device.hip: small pools if the occurrence-weighted mean of the occurrences per vertex is at most 20
static bool compactSmall(const std::vector<uint64_t>& occStart, uint64_t P)
{
    long double occSq = 0;
    for (size_t v = 0; v + 1 < occStart.size(); v++) { const long double nv = (long double)(occStart[v + 1] - occStart[v]); occSq += nv * nv; }
    return P > 0 && occSq <= 20.0L * (long double)P;
}

// handPatch on `plan`: the device's posCh holds the loader's letters, the sentinel at every position of the patch list, GAP_BYTE elsewhere
static int patch(const lcb_graph& g, const LcbSegPlan& plan, const std::vector<unsigned long long>& patchQ, const std::vector<uint8_t>& patchLetter)
{
    const uint64_t P = g.nPos(), D = plan.devPositions;
    std::vector<uint8_t> posCh((size_t)D + 1, GAP_BYTE), inside((size_t)D + 1, 0);
    for (uint64_t q = 0; q < P; q++) { posCh[(size_t)plan.toDev(q)] = g.posCh[q]; inside[(size_t)plan.toDev(q)] = 1; }
    for (unsigned long long q : patchQ) posCh[(size_t)plan.toDev(q)] = SENTINEL;
    std::vector<unsigned long long> chrStart(g.chrStart.begin(), g.chrStart.end()), chrDev(plan.chrDev.begin(), plan.chrDev.end()), segBase(plan.segDev.begin(), plan.segDev.end());
    const TablePlan pl{chrStart.data(), chrDev.data(), plan.chrWord.data(), segBase.data(), g.nChr()};
    const uint64_t n = patchQ.size();
    if (n) launch(blocksOf(n, H_T), H_T, [&]() { handPatch(pl, patchQ.data(), patchLetter.data(), n, P, posCh.data()); });      // (no patches: no launch)
    for (uint64_t q = 0; q < P; q++)
        if (posCh[(size_t)plan.toDev(q)] != g.posCh[q]) FAIL("posCh of position %llu (device index %llu): emu 0x%02x, loader 0x%02x", (unsigned long long)q, (unsigned long long)plan.toDev(q), posCh[(size_t)plan.toDev(q)], g.posCh[q]);
    for (uint64_t at = 0; at <= D; at++)
        if (!inside[(size_t)at] && posCh[(size_t)at] != GAP_BYTE) FAIL("posCh was written at device index %llu, which holds no position", (unsigned long long)at);
    return 0;
}

// The CSR as tables.hip takes it from the build on lcb_open_fasta's route; compared with graph.cpp's. 0 = equal.
template <class Q>
static int csr(const lcb_graph& g, const LcbSegPlan& plan)
{
    const uint64_t P = g.nPos(), D = plan.devPositions, V1 = (uint64_t)g.nVertex + 1;
    std::vector<int32_t> posId((size_t)D + 1, (int32_t)0xEEEEEEEE);
    for (uint64_t q = 0; q < P; q++) posId[(size_t)plan.toDev(q)] = g.posId[q];
    std::vector<unsigned long long> chrStart(g.chrStart.begin(), g.chrStart.end()), chrDev(plan.chrDev.begin(), plan.chrDev.end()), segBase(plan.segDev.begin(), plan.segDev.end());
    const TablePlan pl{chrStart.data(), chrDev.data(), plan.chrWord.data(), segBase.data(), g.nChr()};
    std::vector<Q> occStart((size_t)V1, 0);
    std::vector<uint64_t> gotStart, gotG;
    std::vector<uint32_t> gotChr;
    if (P) {                                       // (no kept position: no kernel is launched)
        std::vector<uint32_t> keys((size_t)P), keys2((size_t)P);
        std::vector<Q> pay((size_t)P), pay2((size_t)P);
        launch(blocksOf(P, T_T), T_T, [&]() { K<Q>::keys(pl, posId.data(), keys.data(), pay.data(), occStart.data(), P); });
        unsigned long long total = 0;
        launch(1, T_SCAN_T, [&]() { K<Q>::scan(occStart.data(), V1, &total); });
        if (total != P) FAIL("the vertex counts sum to %llu, the graph has %llu positions", total, (unsigned long long)P);
        std::vector<unsigned long long> hist(T_DIGITS * 256, 0);
        launch(blocksOf(P, T_T * T_HIST_ITEMS), T_T, [&]() { tableDigitHist(keys.data(), P, hist.data()); });
        const uint32_t nTiles = (uint32_t)blocksOf(P, T_TILE);
        std::vector<Q> tileHist((size_t)nTiles * 256);
        uint32_t *kin = keys.data(), *kout = keys2.data();
        Q *pin = pay.data(), *pout = pay2.data();
        for (int p = 0; p < T_DIGITS; p++) {
            bool one = false;
            for (int x = 0; x < 256; x++) one = one || hist[p * 256 + x] == P;
            if (one) continue;
            launch(nTiles, 64, [&]() { K<Q>::tileHist(kin, P, p, tileHist.data(), nTiles); });
            launch(1, T_SCAN_T, [&]() { K<Q>::scan(tileHist.data(), (uint64_t)nTiles * 256, &total); });
            launch(nTiles, 64, [&]() { K<Q>::scatter(kin, pin, kout, pout, P, p, tileHist.data(), nTiles); });
            std::swap(kin, kout); std::swap(pin, pout);
        }
        // ---- the hook: handOccChr over the sorted payloads, then the three downloads (widened)
        std::vector<uint32_t> occChr((size_t)P + 1, 0xEEEEEEEEu);
        launch(blocksOf(P, H_T), H_T, [&]() { K<Q>::occChr(pl, pin, occChr.data(), P); });
        if (occChr[(size_t)P] != 0xEEEEEEEEu) FAIL("handOccChr wrote behind the last CSR slot");
        gotChr.assign(occChr.begin(), occChr.begin() + (ptrdiff_t)P);
        gotG.assign(pin, pin + P);
    }
    gotStart.assign(occStart.begin(), occStart.end());
    if (gotStart != g.occStart) {
        for (size_t v = 0; v < gotStart.size() && v < g.occStart.size(); v++)
            if (gotStart[v] != g.occStart[v]) FAIL("occStart[%zu]: emu %llu, host %llu", v, (unsigned long long)gotStart[v], (unsigned long long)g.occStart[v]);
        FAIL("occStart: %zu entries, the host has %zu", gotStart.size(), g.occStart.size());
    }
    if (gotG.size() != g.occG.size() || gotChr.size() != g.occChr.size()) FAIL("the CSR has %zu / %zu slots, the host's %zu", gotG.size(), gotChr.size(), g.occG.size());
    for (uint64_t j = 0; j < P; j++) {
        if (gotG[(size_t)j] != g.occG[(size_t)j]) FAIL("occG[%llu]: emu %llu, host %llu", (unsigned long long)j, (unsigned long long)gotG[(size_t)j], (unsigned long long)g.occG[(size_t)j]);
        if (gotChr[(size_t)j] != g.occChr[(size_t)j]) FAIL("occChr[%llu]: emu %u, host %u", (unsigned long long)j, gotChr[(size_t)j], g.occChr[(size_t)j]);
    }
    if (compactSmall(gotStart, P) != compactSmall(g.occStart, P)) FAIL("the compactSmall decision differs from the host's");
    return 0;
}

int main(int argc, char** argv)
{
    if (argc < 5) { fprintf(stderr, "usage: handover_emu <junctions> <k> <abundance> <fasta> [<fasta> ...]\n"); return 2; }
    try {
        const int k = atoi(argv[2]);
        const std::vector<std::string> fasta(argv + 4, argv + argc);
        lcb_graph* g = lcb_graph_load_impl(argv[1], fasta, k, atoi(argv[3]), 2);
        // the patch list as the host of lcb_open_fasta finds it: the positions whose next base the code bytes have no letter for
        std::vector<unsigned long long> patchQ;
        std::vector<uint8_t> patchLetter;
        uint64_t emptied = 0;
        for (size_t c = 0; c < g->nChr(); c++) {
            if (g->chrStart[c + 1] == g->chrStart[c]) emptied++;
            for (uint64_t q = g->chrStart[c]; q < g->chrStart[c + 1]; q++) {
                const size_t at = (size_t)g->posPos[q] + (size_t)k;
                if (at < g->seq[c].size() && lcb_fasta::code(g->seq[c][at]) < 0) { patchQ.push_back(q); patchLetter.push_back((uint8_t)g->seq[c][at]); }
            }
        }
        // seg_cap 64, seg_gap 64; an input whose small chromosomes fill more than 32 such segments has no such plan (a device would refuse
        // it too): the cap is doubled until there is one
        const LcbSegPlan dense = lcb_plan_segments(*g, 0, 0);
        uint64_t cap = 64;
        LcbSegPlan cut;
        for (;; cap *= 2) {
            try { cut = lcb_plan_segments(*g, cap, 64); break; } catch (LcbError&) { if (cap > g->nPos()) throw; }
        }
        int rc = csr<uint32_t>(*g, dense);
        rc = rc ? rc : csr<unsigned long long>(*g, cut);
        rc = rc ? rc : patch(*g, dense, patchQ, patchLetter);
        rc = rc ? rc : patch(*g, cut, patchQ, patchLetter);
        if (!rc)
            printf("positions %llu vertices %u chromosomes %u emptied %llu segments %u cap %llu patches %zu small %d\n", (unsigned long long)g->nPos(), g->nVertex, g->nChr(), (unsigned long long)emptied, cut.nSeg(), (unsigned long long)cap,
                   patchQ.size(), compactSmall(g->occStart, g->nPos()) ? 1 : 0);
        delete g;
        return rc;
    } catch (std::exception& e) { fprintf(stderr, "error: %s\n", e.what()); return 2; }
}
