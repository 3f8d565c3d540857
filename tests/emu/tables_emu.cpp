// tests/emu/tables_emu.cpp — TEST-ONLY: the kernels of the device table build (sibeliaz_amd/csrc/lcb_table_kernels.h, unmodified) on the
// lockstep wavefront emulator, driven like csrc/tables.hip drives them, against what the host route of csrc/device.hip uploads:
// lcb_window_table (lcb_segments.h), the graph's occStart and the occurrence records made from occG / occChr.
//   tables_emu graph <junctions> <fasta> <k> <abundance> <max_branch> [seg_cap seg_gap]   a loaded graph, tables laid out as device.hip lays them out
//   tables_emu edge <max_branch>                                                          a hand-made graph with positions at 0 and at 2^32 - 1
//   tables_emu scan <tableScan32|tableScan64> <n>                                         one scan kernel alone on generated arrays of n entries (every
//                                                                                         content of scan_cases.h), against a serial 64-bit prefix sum
// Exit status 0 = equal; otherwise the first difference on stderr. tests/test_tables_emu.py runs both.
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
#include "lcb_host.h"
#include "lcb_segments.h"
#include "lcb_table_kernels.h"
#include "scan_cases.h"
using namespace lcb_tablek;

template <class F> void launch(uint64_t grid, int threads, F body) { for (uint64_t b = 0; b < grid; b++) emu_run_block((uint32_t)b, threads / 64, body); }
static uint64_t blocksOf(uint64_t n, uint64_t per) { return (n + per - 1) / per; }

// The 32-bit and the 64-bit instantiation of the kernels under one name each.
template <class Q> struct K;
template <> struct K<uint32_t> {
    static void keys(const TablePlan& pl, const int32_t* id, uint32_t* k, uint32_t* p, uint32_t* c, uint64_t P) { tableKeys32(pl, id, k, p, c, P); }
    static void scan(uint32_t* a, uint64_t n, unsigned long long* t) { tableScan32(a, n, t); }
    static void tileHist(const uint32_t* k, uint64_t n, int p, uint32_t* h, uint32_t nt) { tableTileHist32(k, n, p, h, nt); }
    static void scatter(const uint32_t* ki, const uint32_t* pi, uint32_t* ko, uint32_t* po, uint64_t n, int p, const uint32_t* o, uint32_t nt) { tableScatter32(ki, pi, ko, po, n, p, o, nt); }
    static void gather(const TablePlan& pl, const uint32_t* p, const uint32_t* pos, const int32_t* id, uint4* r, uint64_t P) { tableGather32(pl, p, pos, id, r, P); }
};
template <> struct K<unsigned long long> {
    typedef unsigned long long Q;
    static void keys(const TablePlan& pl, const int32_t* id, uint32_t* k, Q* p, Q* c, uint64_t P) { tableKeys64(pl, id, k, p, c, P); }
    static void scan(Q* a, uint64_t n, unsigned long long* t) { tableScan64(a, n, t); }
    static void tileHist(const uint32_t* k, uint64_t n, int p, Q* h, uint32_t nt) { tableTileHist64(k, n, p, h, nt); }
    static void scatter(const uint32_t* ki, const Q* pi, uint32_t* ko, Q* po, uint64_t n, int p, const Q* o, uint32_t nt) { tableScatter64(ki, pi, ko, po, n, p, o, nt); }
    static void gather(const TablePlan& pl, const Q* p, const uint32_t* pos, const int32_t* id, uint4* r, uint64_t P) { tableGather64(pl, p, pos, id, r, P); }
};

static const uint32_t GAP_WORD = 0xEEEEEEEEu;      // what the gaps of the device tables hold: a read inside a gap shows, a write too

// The build as tables.hip runs it; compared with the host route. 0 = equal.
template <class Q>
static int build(const lcb_graph& g, const LcbSegPlan& plan, uint32_t maxBranch)
{
    const uint64_t P = g.nPos(), D = plan.devPositions;
    // the inputs on the "device"
    std::vector<int32_t> posId((size_t)D + 1, (int32_t)GAP_WORD);
    std::vector<uint32_t> posPos((size_t)D + 1, GAP_WORD), posWin((size_t)D + 1, GAP_WORD);
    for (uint32_t s = 0; s < plan.nSeg(); s++)
        for (uint64_t q = plan.segStart[s]; q < plan.segStart[s + 1]; q++) { posId[(size_t)(plan.segDev[s] + q - plan.segStart[s])] = g.posId[q]; posPos[(size_t)(plan.segDev[s] + q - plan.segStart[s])] = g.posPos[q]; }
    std::vector<unsigned long long> chrStart(g.chrStart.begin(), g.chrStart.end()), chrDev(plan.chrDev.begin(), plan.chrDev.end()), segBase(plan.segDev.begin(), plan.segDev.end());
    const TablePlan pl{chrStart.data(), chrDev.data(), plan.chrWord.data(), segBase.data(), g.nChr()};
    std::vector<Q> occStart((size_t)g.nVertex + 1, 0);
    std::vector<uint4> occRec((size_t)P);
    int passes = 0, skipped = 0;
    if (P) {                                       // (a launch of no workgroups never reaches the device)
        launch(blocksOf(P, T_T), T_T, [&]() { tableWindow(pl, posPos.data(), posWin.data(), P, maxBranch); });
        std::vector<uint32_t> keys((size_t)P), keys2((size_t)P);
        std::vector<Q> pay((size_t)P), pay2((size_t)P);
        launch(blocksOf(P, T_T), T_T, [&]() { K<Q>::keys(pl, posId.data(), keys.data(), pay.data(), occStart.data(), P); });
        unsigned long long total = 0;
        launch(1, T_SCAN_T, [&]() { K<Q>::scan(occStart.data(), (uint64_t)g.nVertex + 1, &total); });
        if (total != P) { fprintf(stderr, "the vertex counts sum to %llu, the graph has %llu positions\n", total, (unsigned long long)P); return 1; }
        std::vector<unsigned long long> hist(T_DIGITS * 256, 0);
        launch(blocksOf(P, T_T * T_HIST_ITEMS), T_T, [&]() { tableDigitHist(keys.data(), P, hist.data()); });
        const uint32_t nTiles = (uint32_t)blocksOf(P, T_TILE);
        std::vector<Q> tileHist((size_t)nTiles * 256);
        uint32_t *kin = keys.data(), *kout = keys2.data();
        Q *pin = pay.data(), *pout = pay2.data();
        for (int p = 0; p < T_DIGITS; p++) {
            bool one = false;
            unsigned long long sum = 0;
            for (int x = 0; x < 256; x++) { sum += hist[p * 256 + x]; one = one || hist[p * 256 + x] == P; }
            if (sum != P) { fprintf(stderr, "digit %d: the histogram counts %llu of %llu keys\n", p, sum, (unsigned long long)P); return 1; }
            if (one) { skipped++; continue; }
            launch(nTiles, 64, [&]() { K<Q>::tileHist(kin, P, p, tileHist.data(), nTiles); });
            launch(1, T_SCAN_T, [&]() { K<Q>::scan(tileHist.data(), (uint64_t)nTiles * 256, &total); });
            if (total != P) { fprintf(stderr, "digit %d: the tile histograms count %llu of %llu keys\n", p, total, (unsigned long long)P); return 1; }
            launch(nTiles, 64, [&]() { K<Q>::scatter(kin, pin, kout, pout, P, p, tileHist.data(), nTiles); });
            std::swap(kin, kout); std::swap(pin, pout);
            passes++;
        }
        launch(blocksOf(P, T_T), T_T, [&]() { K<Q>::gather(pl, pin, posPos.data(), posId.data(), occRec.data(), P); });
    } else skipped = T_DIGITS;
    printf("positions %llu vertices %u chromosomes %u segments %u tile %d passes %d skipped %d payload_bytes %d\n", (unsigned long long)P, g.nVertex, g.nChr(), plan.nSeg(), T_TILE, passes, skipped, (int)sizeof(Q));

    // ---- against the host route
    const std::vector<uint32_t> win = lcb_window_table(g, maxBranch);
    std::vector<uint8_t> inside((size_t)D + 1, 0);
    for (uint64_t q = 0; q < P; q++) {
        const uint64_t at = plan.toDev(q);
        inside[(size_t)at] = 1;
        if (posWin[(size_t)at] != win[(size_t)q]) { fprintf(stderr, "posWin of position %llu: emu 0x%08x, host 0x%08x\n", (unsigned long long)q, posWin[(size_t)at], win[(size_t)q]); return 1; }
    }
    for (uint64_t at = 0; at <= D; at++)
        if (!inside[(size_t)at] && posWin[(size_t)at] != GAP_WORD) { fprintf(stderr, "posWin was written at device index %llu, which holds no position\n", (unsigned long long)at); return 1; }
    for (size_t v = 0; v <= g.nVertex; v++)
        if ((uint64_t)occStart[v] != g.occStart[v]) { fprintf(stderr, "occStart[%zu]: emu %llu, host %llu\n", v, (unsigned long long)occStart[v], (unsigned long long)g.occStart[v]); return 1; }
    for (uint64_t j = 0; j < P; j++) {
        const uint64_t q = g.occG[j];
        const uint32_t cw = plan.chrWord[g.occChr[j]];
        const uint4 want{(uint32_t)(q - plan.segStart[cw >> LCB_SEG_SHIFT]), cw, g.posPos[q], (uint32_t)g.posId[q]}, got = occRec[(size_t)j];
        if (got.x != want.x || got.y != want.y || got.z != want.z || got.w != want.w) {
            fprintf(stderr, "occRec[%llu]: emu {%u, 0x%x, %u, %d}, host {%u, 0x%x, %u, %d}\n", (unsigned long long)j, got.x, got.y, got.z, (int32_t)got.w, want.x, want.y, want.z, (int32_t)want.w);
            return 1;
        }
    }
    return 0;
}

static int run(const lcb_graph& g, uint32_t maxBranch, uint64_t segCap, uint64_t segGap)
{
    const LcbSegPlan plan = lcb_plan_segments(g, segCap, segGap);
    const bool seg = plan.nSeg() > 1 || segCap != 0;           // d->seg of device.hip: the payload width follows it
    return seg ? build<unsigned long long>(g, plan, maxBranch) : build<uint32_t>(g, plan, maxBranch);
}

// Three chromosomes whose positions touch both ends of the 32-bit range: the saturation of pos + maxBranch and the floor of pos - maxBranch.
static lcb_graph edgeGraph()
{
    lcb_graph g;
    g.k = 15;
    const std::vector<std::vector<uint32_t>> pos = {{0, 1, 2, 5, 400, 401, 0xFFFFFFF0u, 0xFFFFFFFEu, 0xFFFFFFFFu}, {0xFFFFFFFFu}, {0, 0xFFFFFFFFu}, {3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20}};
    g.chrStart.push_back(0);
    int32_t next = 1;
    for (size_t c = 0; c < pos.size(); c++) {
        for (uint32_t p : pos[c]) { g.posPos.push_back(p); g.posId.push_back((next % 3 == 0 ? -1 : 1) * (1 + next % 5)); g.posCh.push_back('A'); g.posRevCh.push_back('T'); next++; }
        g.chrStart.push_back(g.posPos.size());
        g.chrName.push_back("c" + std::to_string(c));
    }
    g.seq.resize(pos.size());
    g.nVertex = 6;
    // the CSR as graph.cpp makes it: per vertex, ascending flat position
    g.occStart.assign((size_t)g.nVertex + 1, 0);
    for (int32_t id : g.posId) g.occStart[(size_t)std::abs(id) + 1]++;
    for (size_t v = 0; v < g.nVertex; v++) g.occStart[v + 1] += g.occStart[v];
    std::vector<uint64_t> cursor(g.occStart.begin(), g.occStart.end() - 1);
    g.occG.resize(g.nPos()); g.occChr.resize(g.nPos());
    for (uint64_t q = 0; q < g.nPos(); q++) g.occG[(size_t)cursor[(size_t)std::abs(g.posId[q])]++] = q;
    for (uint64_t j = 0; j < g.nPos(); j++) g.occChr[j] = (uint32_t)(std::upper_bound(g.chrStart.begin(), g.chrStart.end(), g.occG[j]) - g.chrStart.begin() - 1);
    return g;
}

template <class Q> static int runScan(const char* kernel, uint64_t n)
{
    return scanCheckAll<Q>(kernel, n, 4ull * T_SCAN_T, [](Q* a, uint64_t m, unsigned long long* t) { launch(1, T_SCAN_T, [&]() { K<Q>::scan(a, m, t); }); });
}

int main(int argc, char** argv)
{
    try {
        if (argc >= 4 && std::string(argv[1]) == "scan") {
            const uint64_t n = strtoull(argv[3], nullptr, 10);
            if (std::string(argv[2]) == "tableScan32") return runScan<uint32_t>("tableScan32", n);
            if (std::string(argv[2]) == "tableScan64") return runScan<unsigned long long>("tableScan64", n);
            fprintf(stderr, "unknown kernel %s\n", argv[2]);
            return 2;
        }
        if (argc >= 7 && std::string(argv[1]) == "graph") {
            lcb_graph* g = lcb_graph_load_impl(argv[2], {argv[3]}, atoi(argv[4]), atoi(argv[5]), 2);
            const int rc = run(*g, (uint32_t)strtoul(argv[6], nullptr, 10), argc > 7 ? strtoull(argv[7], nullptr, 10) : 0, argc > 8 ? strtoull(argv[8], nullptr, 10) : 0);
            delete g;
            return rc;
        }
        if (argc >= 3 && std::string(argv[1]) == "edge") {
            const lcb_graph g = edgeGraph();
            const uint32_t mb = (uint32_t)strtoul(argv[2], nullptr, 10);
            const int rc = run(g, mb, 0, 0);
            return rc ? rc : run(g, mb, 12, 100);              // ... and cut into segments with a gap: the 64-bit instantiation
        }
    } catch (std::exception& e) { fprintf(stderr, "error: %s\n", e.what()); return 2; }
    fprintf(stderr, "usage: tables_emu graph <junctions> <fasta> <k> <abundance> <max_branch> [seg_cap seg_gap] | tables_emu edge <max_branch> | tables_emu scan <kernel> <n>\n");
    return 2;
}
