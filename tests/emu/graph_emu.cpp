// tests/emu/graph_emu.cpp — TEST-ONLY: the kernels of the graph build on the GPU (sibeliaz_amd/csrc/lcb_graph_kernels.h, unmodified) on the
// lockstep wavefront emulator, driven like lcb_graph_build_impl of csrc/junctions.hip drives them behind the junction finder: the raw
// records of a junction file written by the CPU lcb-mkgraph stand for what the tiles emit ({g, id} in file order, cut into tiles of
// <tile> windows), the code bytes are made from the strings of graph.cpp's parser. Take, abundance (both instantiations), keep-count,
// scan, compaction, the host's patch and graph.cpp's CSR must give the graph lcb_graph_load_impl makes of the same file.
//   graph_emu <junctions> <k> <abundance> <tile> <fasta> [<fasta> ...]
//   graph_emu scan <n>          graphScan alone on generated arrays of n entries (every content of scan_cases.h), against a serial 64-bit prefix sum
// Exit status 0 = equal; otherwise the first difference on stderr. tests/test_graph_emu.py runs it.
#include <hip/hip_runtime.h>     // the shadow header of this directory

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>
using std::min;
template <class V> static inline uint64_t emu_shfl_up(V v, int d, const char* f, int l)
{
    const int lane = emu_thread_idx().x & 63, src = lane >= d ? lane - d : lane;
    return emu_collective(EMU_SHFL, (uint64_t)v, src, f, l);
}
#define __shfl_up(v, d) emu_shfl_up((v), (d), __FILE__, __LINE__)
static inline int emu_sync_count(int p)
{
    static thread_local int cnt;
    if (emu_thread_idx().x == 0) cnt = 0;
    __syncthreads(); if (p) cnt++; __syncthreads(); int r = cnt; __syncthreads(); return r;
}
#define __syncthreads_count(p) emu_sync_count((p) ? 1 : 0)
static inline unsigned long long atomicCAS(unsigned long long* a, unsigned long long cmp, unsigned long long val) { unsigned long long old = *a; if (old == cmp) *a = val; return old; }
static inline unsigned long long atomicMin(unsigned long long* a, unsigned long long v) { unsigned long long old = *a; if (v < old) *a = v; return old; }
static inline int __popc(uint32_t x) { return __builtin_popcount(x); }

#include "emu_runtime.h"
#include "lcb_fasta.h"
#include "lcb_graph_kernels.h"
#include "lcb_host.h"
#include "scan_cases.h"
using namespace lcb_graphk;

template <class F> void launch(uint64_t grid, int threads, F body) { for (uint64_t b = 0; b < grid; b++) emu_run_block((uint32_t)b, threads / 64, body); }
static uint64_t blocksOf(uint64_t n, uint64_t per) { return (n + per - 1) / per; }

#define FAIL(...) do { fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); return 1; } while (0)

template <class T> static int same(const char* what, const std::vector<T>& got, const std::vector<T>& want)
{
    if (got.size() != want.size()) FAIL("%s: %zu entries, the loader has %zu", what, got.size(), want.size());
    for (size_t i = 0; i < got.size(); i++)
        if (got[i] != want[i]) FAIL("%s[%zu]: emu %lld, loader %lld", what, i, (long long)got[i], (long long)want[i]);
    return 0;
}

static int run(const char* junctions, int k, int abundance, uint64_t tile, const std::vector<std::string>& fasta)
{
    lcb_graph* want = lcb_graph_load_impl(junctions, fasta, k, abundance, 2);
    lcb_graph g;
    g.k = k;
    const size_t nRec = lcb_graph_parse_fasta(g, fasta, 2);
    // the code array as junctions.hip lays it out: a breaker in front of the first record and behind every record
    std::vector<unsigned long long> base(nRec + 1);
    uint64_t len = 1;
    for (size_t r = 0; r < nRec; r++) { base[r] = len; len += g.seq[r].size() + 1; }
    base[nRec] = len;
    std::vector<uint8_t> codes((size_t)len, 4);
    for (size_t r = 0; r < nRec; r++)
        for (size_t i = 0; i < g.seq[r].size(); i++) { const int c = lcb_fasta::code(g.seq[r][i]); codes[(size_t)base[r] + i] = (uint8_t)(c < 0 ? 4 : c); }
    // the records the tiles would emit
    std::vector<JRecord> rec;
    long long maxId = 0;
    {
        FILE* f = fopen(junctions, "rb");
        if (!f) FAIL("cannot open %s", junctions);
        unsigned char b[12];
        size_t chr = 0;
        while (fread(b, 1, 12, f) == 12) {
            uint32_t pos; int64_t id;
            memcpy(&pos, b, 4); memcpy(&id, b + 4, 8);
            if (pos == 0xFFFFFFFFu || id == INT64_MAX) { chr++; continue; }
            if (chr >= nRec) FAIL("the junction file has more chromosomes than the FASTA has records");
            rec.push_back(JRecord{base[chr] + pos, id});
            maxId = std::max<long long>(maxId, id < 0 ? -id : id);
        }
        fclose(f);
    }
    const uint64_t N = rec.size();

    // ---- take, tile by tile
    std::vector<uint32_t> rawPos((size_t)N + 1, 0xEEEEEEEEu);
    std::vector<int32_t> rawId((size_t)N + 1, (int32_t)0xEEEEEEEE);
    std::vector<unsigned long long> recFirst(nRec + 1, G_NONE);
    uint64_t before = 0, tiles = 0;
    for (uint64_t t0 = 0; t0 < len; t0 += tile, tiles++) {
        uint64_t n = 0;
        while (before + n < N && rec[(size_t)(before + n)].g < t0 + tile) n++;
        if (n) launch(blocksOf(n, G_T), G_T, [&]() { graphTake(rec.data() + before, (uint32_t)n, before, base.data(), (uint32_t)nRec, rawPos.data(), rawId.data(), recFirst.data()); });
        before += n;
    }
    if (before != N) FAIL("the tiles hold %llu of %llu records", (unsigned long long)before, (unsigned long long)N);
    if (rawPos[(size_t)N] != 0xEEEEEEEEu || rawId[(size_t)N] != (int32_t)0xEEEEEEEE) FAIL("graphTake wrote behind the raw arrays");
    size_t C = 0;
    while (C < nRec && recFirst[C] != G_NONE) C++;
    for (size_t r = C; r < nRec; r++) if (recFirst[r] != G_NONE) FAIL("record %zu has junctions behind one that has none", r);
    if (C != nRec) FAIL("%zu of %zu records have junctions", C, nRec);
    for (size_t c = 0; c < C; c++) if (recFirst[c] >= N || (c ? recFirst[c] <= recFirst[c - 1] : recFirst[c] != 0)) FAIL("the first raw indices do not ascend at record %zu", c);

    // ---- abundance: both instantiations give the same counters
    g.nVertex = N ? (uint32_t)(maxId + 1) : 0u;
    std::vector<uint32_t> counter((size_t)g.nVertex + 1, 0), counterWave((size_t)g.nVertex + 1, 0);
    const uint64_t nb = blocksOf(N, G_T);
    if (N) {
        launch(nb, G_T, [&]() { graphAbundance(rawId.data(), N, counter.data()); });
        launch(nb, G_T, [&]() { graphAbundanceWave(rawId.data(), N, counterWave.data()); });
    }
    if (same("counter (wave against plain)", counterWave, counter)) return 1;

    // ---- keep-counts, scan, compaction
    std::vector<unsigned long long> blockKept((size_t)nb + 1, 0), totals(2, 0), chrStart(C + 1, 0xEEEEEEEEEEEEEEEEull);
    if (N) {
        launch(nb, G_T, [&]() { graphKeepCount(rawId.data(), N, counter.data(), (uint32_t)abundance, blockKept.data()); });
        launch(1, G_SCAN_T, [&]() { graphScan(blockKept.data(), nb, &totals[0]); });
    }
    const uint64_t K = totals[0];
    if (K > N) FAIL("%llu kept of %llu raw records", (unsigned long long)K, (unsigned long long)N);
    g.posId.assign((size_t)K + 1, (int32_t)0xEEEEEEEE); g.posPos.assign((size_t)K + 1, 0xEEEEEEEEu); g.posCh.assign((size_t)K + 1, 0xEE); g.posRevCh.assign((size_t)K + 1, 0xEE);
    if (N)
        launch(nb, G_T, [&]() {
            graphCompact(rawPos.data(), rawId.data(), N, counter.data(), (uint32_t)abundance, blockKept.data(), codes.data(), base.data(), recFirst.data(), (uint32_t)C, k, g.posId.data(),
                         g.posPos.data(), g.posCh.data(), g.posRevCh.data(), chrStart.data(), &totals[1]);
        });
    if (g.posId[(size_t)K] != (int32_t)0xEEEEEEEE || g.posPos[(size_t)K] != 0xEEEEEEEEu || g.posCh[(size_t)K] != 0xEE || g.posRevCh[(size_t)K] != 0xEE) FAIL("graphCompact wrote behind the kept arrays");
    g.posId.resize((size_t)K); g.posPos.resize((size_t)K); g.posCh.resize((size_t)K); g.posRevCh.resize((size_t)K);
    chrStart[C] = K;
    g.chrStart.assign(chrStart.begin(), chrStart.end());
    // ---- the host's patch
    uint64_t found = 0;
    for (size_t c = 0; c < C; c++)
        for (uint64_t i = g.chrStart[c]; i < g.chrStart[c + 1]; i++)
            if (g.posCh[(size_t)i] == G_PATCH) { g.posCh[(size_t)i] = (uint8_t)g.seq[c][(size_t)g.posPos[(size_t)i] + (size_t)k]; found++; }
    if (found != totals[1]) FAIL("the kernel counted %llu characters for the host, the arrays hold %llu", totals[1], (unsigned long long)found);
    lcb_graph_build_csr(&g, 2);
    printf("records %zu raw %llu kept %llu vertices %u patched %llu tiles %llu\n", nRec, (unsigned long long)N, (unsigned long long)K, g.nVertex, (unsigned long long)found, (unsigned long long)tiles);

    // ---- against the loader
    if (g.nVertex != want->nVertex) FAIL("nVertex: emu %u, loader %u", g.nVertex, want->nVertex);
    if (g.chrName != want->chrName) FAIL("the chromosome names differ");
    if (g.seq != want->seq) FAIL("the sequences differ");
    int rc = same("chrStart", g.chrStart, want->chrStart) || same("posId", g.posId, want->posId) || same("posPos", g.posPos, want->posPos) || same("posCh", g.posCh, want->posCh) ||
             same("posRevCh", g.posRevCh, want->posRevCh) || same("occStart", g.occStart, want->occStart) || same("occG", g.occG, want->occG) || same("occChr", g.occChr, want->occChr);
    delete want;
    return rc;
}

int main(int argc, char** argv)
{
    if (argc == 3 && std::string(argv[1]) == "scan")
        return scanCheckAll<unsigned long long>("graphScan", strtoull(argv[2], nullptr, 10), 4ull * G_SCAN_T,
                                                [](unsigned long long* a, uint64_t m, unsigned long long* t) { launch(1, G_SCAN_T, [&]() { graphScan(a, m, t); }); });
    if (argc < 6) { fprintf(stderr, "usage: graph_emu <junctions> <k> <abundance> <tile> <fasta> [<fasta> ...] | graph_emu scan <n>\n"); return 2; }
    try {
        return run(argv[1], atoi(argv[2]), atoi(argv[3]), strtoull(argv[4], nullptr, 10), std::vector<std::string>(argv + 5, argv + argc));
    } catch (std::exception& e) { fprintf(stderr, "error: %s\n", e.what()); return 2; }
}
