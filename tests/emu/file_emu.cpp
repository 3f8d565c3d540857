// tests/emu/file_emu.cpp — TEST-ONLY: the kernels that open a junction file on the GPU (sibeliaz_amd/csrc/lcb_file_kernels.h, unmodified) and
// the tail of the graph build (lcb_graph_kernels.h, unmodified) on the lockstep wavefront emulator, driven as graphFromFile and graphTail
// of csrc/junctions.hip drive them, with the host code they use (lcb_file_host.h): the file is read tile by tile into a staging buffer
// and copied to the resident words, fileCount per tile, the scan, fileTake, the walk over the runs, the FASTA by graph.cpp's parser,
// abundance, keep-count, scan, fileBounds, compaction, fileOrder, the host's patch and graph.cpp's CSR. The result must be the graph
// lcb_graph_load_impl makes of the same files - or the same refusal, word for word.
//   file_emu <junctions> <k> <abundance> <tile> <fasta> [<fasta> ...]
// Exit status 0 = equal graphs (a line of counts on stdout) or equal refusals ("refused: <text>" on stdout); otherwise the first
// difference on stderr. tests/test_file_emu.py runs it.
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
#include "lcb_file_host.h"
#include "lcb_file_kernels.h"
#include "lcb_graph_kernels.h"
#include "lcb_host.h"
using namespace lcb_graphk;
using namespace lcb_filek;

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

static const uint32_t PAD = 0xEEEEEEEEu;

// The device route; throws what the driver throws. 1: a guard word was overwritten or an internal count is off.
static int deviceRoute(const char* junctions, int k, int abundance, uint32_t tileRecords, const std::vector<std::string>& fasta, lcb_graph& g)
{
    // ---- the file: read, copy, count
    lcb_file::Reader in(junctions);
    const lcb_file::Tiling T = lcb_file::tiling(in.bytes, tileRecords);
    const uint64_t blocks = T.blocks();
    std::vector<uint32_t> words((size_t)T.nRec * 3 + 1, PAD);
    std::vector<unsigned char> stage((size_t)T.tile * 12);
    std::vector<unsigned long long> blockSep((size_t)blocks + 1, 0xEEEEEEEEEEEEEEEEull), flags(4, 0);
    for (uint64_t t = 0; t < T.tiles; t++) {
        in.read(T, t, stage.data());
        memcpy(words.data() + 3 * T.first(t), stage.data(), (size_t)T.count(t) * 12);
        launch(T.bpt, F_T, [&]() { fileCount(words.data(), T.nRec, T.tile, t, blockSep.data() + t * T.bpt, &flags[2]); });
    }
    if (words[(size_t)T.nRec * 3] != PAD) FAIL("the tiles wrote behind the file's words");
    if (blockSep[(size_t)blocks] != 0xEEEEEEEEEEEEEEEEull) FAIL("fileCount wrote behind the separator counts");
    if (flags[2] > T.nRec) FAIL("%llu separators in %llu records", flags[2], (unsigned long long)T.nRec);

    // ---- the raw records and the first raw index of every run
    const uint64_t N = T.nRec - flags[2];
    const size_t runs = (size_t)flags[2] + 1;
    std::vector<uint32_t> rawPos((size_t)N + 1, PAD);
    std::vector<int32_t> rawId((size_t)N + 1, (int32_t)PAD);
    std::vector<unsigned long long> recFirst(runs + 1, G_NONE);
    if (N) {
        launch(1, G_SCAN_T, [&]() { graphScan(blockSep.data(), blocks, &blockSep[(size_t)blocks]); });
        if (blockSep[(size_t)blocks] != flags[2]) FAIL("the scan of the separator counts ends at %llu, fileCount added %llu", blockSep[(size_t)blocks], flags[2]);
        launch(blocks, F_T, [&]() { fileTake(words.data(), T.nRec, T.tile, T.bpt, blockSep.data(), N, runs, rawPos.data(), rawId.data(), recFirst.data()); });
    }
    if (rawPos[(size_t)N] != PAD || rawId[(size_t)N] != (int32_t)PAD || recFirst[runs] != G_NONE) FAIL("fileTake wrote behind its arrays");
    for (uint64_t i = 0; i < N; i++) if (rawPos[(size_t)i] == PAD && rawId[(size_t)i] == (int32_t)PAD) FAIL("fileTake left raw record %llu unwritten", (unsigned long long)i);
    g.nVertex = N ? (uint32_t)flags[3] : 0u;

    // ---- the FASTA and its code bytes as junctions.hip lays them out: a breaker in front of the first record and behind every record
    g.k = k;
    const size_t nRec = lcb_graph_parse_fasta(g, fasta, 2);
    std::vector<unsigned long long> base(nRec + 1);
    uint64_t len = 1;
    for (size_t r = 0; r < nRec; r++) { base[r] = len; len += g.seq[r].size() + 1; }
    base[nRec] = len;
    std::vector<uint8_t> codes((size_t)len, 4);
    for (size_t r = 0; r < nRec; r++)
        for (size_t i = 0; i < g.seq[r].size(); i++) { const int c = lcb_fasta::code(g.seq[r][i]); codes[(size_t)base[r] + i] = (uint8_t)(c < 0 ? 4 : c); }

    // ---- the tail: what the loader refuses, abundance, keep-counts, scan, the bounds
    const size_t C = lcb_file::chromosomes(recFirst.data(), runs, N);
    lcb_file::sameRecords(nRec, C);
    std::vector<uint32_t> counter((size_t)g.nVertex + 1, 0);
    const uint64_t nb = blocksOf(N, G_T);
    std::vector<unsigned long long> blockKept((size_t)nb + 1, 0), totals(2, 0), chrStart(C + 1, 0xEEEEEEEEEEEEEEEEull);
    if (N) {
        launch(nb, G_T, [&]() { graphAbundance(rawId.data(), N, counter.data()); });
        launch(nb, G_T, [&]() { graphKeepCount(rawId.data(), N, counter.data(), (uint32_t)abundance, blockKept.data()); });
        launch(1, G_SCAN_T, [&]() { graphScan(blockKept.data(), nb, &totals[0]); });
        launch(nb, G_T, [&]() { fileBounds(rawPos.data(), rawId.data(), N, counter.data(), (uint32_t)abundance, base.data(), recFirst.data(), (uint32_t)C, k, flags.data()); });
        if (flags[0]) throw LcbError("a junction lies beyond the end of its sequence (junction file and FASTA do not match)");
    }
    const uint64_t K = totals[0];
    if (K > N) FAIL("%llu kept of %llu raw records", (unsigned long long)K, (unsigned long long)N);

    // ---- compaction, the order
    g.posId.assign((size_t)K + 1, (int32_t)PAD); g.posPos.assign((size_t)K + 1, PAD); g.posCh.assign((size_t)K + 1, 0xEE); g.posRevCh.assign((size_t)K + 1, 0xEE);
    if (N) {
        launch(nb, G_T, [&]() {
            graphCompact(rawPos.data(), rawId.data(), N, counter.data(), (uint32_t)abundance, blockKept.data(), codes.data(), base.data(), recFirst.data(), (uint32_t)C, k, g.posId.data(),
                         g.posPos.data(), g.posCh.data(), g.posRevCh.data(), chrStart.data(), &totals[1]);
        });
        if (K > 1) launch(blocksOf(K, G_T), G_T, [&]() { fileOrder(g.posPos.data(), K, chrStart.data(), (uint32_t)C, flags.data()); });
    }
    if (g.posId[(size_t)K] != (int32_t)PAD || g.posPos[(size_t)K] != PAD || g.posCh[(size_t)K] != 0xEE || g.posRevCh[(size_t)K] != 0xEE) FAIL("graphCompact wrote behind the kept arrays");
    if (flags[1]) throw LcbError("junction positions must strictly increase within a chromosome");
    g.posId.resize((size_t)K); g.posPos.resize((size_t)K); g.posCh.resize((size_t)K); g.posRevCh.resize((size_t)K);
    chrStart[C] = K;
    g.chrStart.assign(chrStart.begin(), chrStart.end());
    // ---- the host's patch and CSR
    uint64_t found = 0;
    for (size_t c = 0; c < C; c++)
        for (uint64_t i = g.chrStart[c]; i < g.chrStart[c + 1]; i++)
            if (g.posCh[(size_t)i] == G_PATCH) { g.posCh[(size_t)i] = (uint8_t)g.seq[c][(size_t)g.posPos[(size_t)i] + (size_t)k]; found++; }
    if (found != totals[1]) FAIL("the kernel counted %llu characters for the host, the arrays hold %llu", totals[1], (unsigned long long)found);
    lcb_graph_build_csr(&g, 2);
    printf("records %llu separators %llu chromosomes %zu raw %llu kept %llu vertices %u patched %llu tiles %llu\n", (unsigned long long)T.nRec, flags[2], C, (unsigned long long)N,
           (unsigned long long)K, g.nVertex, (unsigned long long)found, (unsigned long long)T.tiles);
    return 0;
}

static int run(const char* junctions, int k, int abundance, uint32_t tile, const std::vector<std::string>& fasta)
{
    lcb_graph* want = nullptr;
    std::string refusedL, refusedD;
    try { want = lcb_graph_load_impl(junctions, fasta, k, abundance, 2); } catch (LcbError& e) { refusedL = e.what(); }
    lcb_graph g;
    try {
        if (deviceRoute(junctions, k, abundance, tile, fasta, g)) return 1;
    } catch (LcbError& e) { refusedD = e.what(); }
    if (!refusedL.empty() || !refusedD.empty()) {
        delete want;
        if (refusedL != refusedD) FAIL("the loader says '%s', the device route '%s'", refusedL.c_str(), refusedD.c_str());
        printf("refused: %s\n", refusedD.c_str());
        return 0;
    }
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
    if (argc < 6) { fprintf(stderr, "usage: file_emu <junctions> <k> <abundance> <tile> <fasta> [<fasta> ...]\n"); return 2; }
    try {
        return run(argv[1], atoi(argv[2]), atoi(argv[3]), (uint32_t)strtoul(argv[4], nullptr, 10), std::vector<std::string>(argv + 5, argv + argc));
    } catch (std::exception& e) { fprintf(stderr, "error: %s\n", e.what()); return 2; }
}
