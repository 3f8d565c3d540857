// tests/emu/seeds_emu.cpp — TEST-ONLY: the kernels of the device seed enumeration (sibeliaz_amd/csrc/lcb_seed_kernels.h, unmodified) on the
// lockstep wavefront emulator, driven like csrc/seeds.hip drives them, against the host enumerator (csrc/bundles.cpp).
//   seeds_emu enum <junctions> <fasta> <k> <abundance> [seg_cap seg_gap]   tables laid out as device.hip lays them out (lcb_segments.h);
//                                                                          count, scan, fill, sort; compared field by field and in order
//   seeds_emu sort <N> <pattern>                                           the sort kernels alone on generated keys, against std::sort
//   seeds_emu scan <seedScan32|seedScan64> <n>                             one scan kernel alone on generated arrays of n entries (every content of
//                                                                          scan_cases.h), against a serial 64-bit prefix sum
// Exit status 0 = equal; otherwise the first difference on stderr. tests/test_seeds_emu.py runs both.
#include <hip/hip_runtime.h>     // the shadow header of this directory

#include <algorithm>
#include <random>
#include <string>
#include <vector>
using std::min;
static thread_local uint32_t emu_grid_x = 1;
struct EmuGrid { uint32_t x; };
#define gridDim (EmuGrid{emu_grid_x})
static inline uint32_t emu_shfl_up(uint32_t v, int d, const char* f, int l) {
    int lane = emu_thread_idx().x & 63; int src = lane >= d ? lane - d : lane;
    return (uint32_t)emu_collective(EMU_SHFL, (uint64_t)v, src, f, l);
}
#define __shfl_up(v, d) emu_shfl_up((v), (d), __FILE__, __LINE__)
static inline unsigned long long atomicMin(unsigned long long* a, unsigned long long v) { unsigned long long old = *a; if (v < old) *a = v; return old; }

#include "emu_runtime.h"
#include "lcb_host.h"
#include "lcb_seed_kernels.h"
#include "lcb_segments.h"
#include "scan_cases.h"
using namespace lcb_seedk;

template <class F> void launch(uint32_t grid, int threads, F body) { emu_grid_x = grid; for (uint32_t b = 0; b < grid; b++) emu_run_block(b, threads / 64, body); }

static bool seedLess(const lcb_seed& a, const lcb_seed& b)
{
    if (a.count != b.count) return a.count > b.count;
    if (a.rank != b.rank) return a.rank < b.rank;
    if (a.resolve_pos != b.resolve_pos) return a.resolve_pos < b.resolve_pos;
    return a.resolve_chr < b.resolve_chr;
}
static lcb_seed expand(const SeedRec& r) { return lcb_seed{r.vid, (int32_t)(signed char)(r.chrCh & 255u), r.count, r.rank, r.pos, r.chrCh >> 8}; }

// The sort as seeds.hip runs it: all digit histograms, then tile histogram + scan + stable scatter for every digit that tells two keys apart.
static void sortOnEmu(std::vector<SeedRec>& rec, int& passes, int& skipped)
{
    const unsigned long long n = rec.size();
    passes = skipped = 0;
    std::vector<unsigned long long> hist(S_DIGITS * 256, 0);
    if (n) launch((uint32_t)std::min<unsigned long long>((n + S_T - 1) / S_T, 3), S_T, [&]() { seedDigitHist(rec.data(), n, hist.data()); });
    const uint32_t nTiles = (uint32_t)((n + S_TILE - 1) / S_TILE);
    std::vector<SeedRec> other(rec.size());
    std::vector<uint32_t> tileHist((size_t)nTiles * 256);
    SeedRec *in = rec.data(), *out = other.data();
    for (int p = 0; p < S_DIGITS; p++) {
        bool one = n < 2;
        unsigned long long sum = 0;
        for (int x = 0; x < 256; x++) { sum += hist[p * 256 + x]; if (hist[p * 256 + x] == n) one = true; }
        if (sum != n) { fprintf(stderr, "digit %d: the histogram counts %llu of %llu records\n", p, sum, n); exit(1); }
        if (one) { skipped++; continue; }
        unsigned long long total = 0;
        launch(nTiles, 64, [&]() { seedTileHist(in, n, p, tileHist.data(), nTiles); });
        launch(1, S_SCAN_T, [&]() { seedScan32(tileHist.data(), (unsigned long long)nTiles * 256, &total); });
        if (total != n) { fprintf(stderr, "digit %d: the tile histograms count %llu of %llu records\n", p, total, n); exit(1); }
        launch(nTiles, 64, [&]() { seedScatter(in, out, n, p, tileHist.data(), nTiles); });
        std::swap(in, out);
        passes++;
    }
    if (in != rec.data()) rec.swap(other);
}

static int compare(const std::vector<SeedRec>& got, const std::vector<lcb_seed>& want, bool withPayload)
{
    if (got.size() != want.size()) { fprintf(stderr, "%zu seeds, the host has %zu\n", got.size(), want.size()); return 1; }
    for (size_t i = 0; i < got.size(); i++) {
        const lcb_seed a = expand(got[i]), b = want[i];
        const bool same = a.count == b.count && a.rank == b.rank && a.resolve_pos == b.resolve_pos && a.resolve_chr == b.resolve_chr && (!withPayload || (a.vid == b.vid && a.ch == b.ch));
        if (!same) {
            fprintf(stderr, "seed %zu differs: emu vid %d ch %d count %llu rank %llu resolve (%llu, %llu), host vid %d ch %d count %llu rank %llu resolve (%llu, %llu)\n", i, a.vid, a.ch,
                    (unsigned long long)a.count, (unsigned long long)a.rank, (unsigned long long)a.resolve_pos, (unsigned long long)a.resolve_chr, b.vid, b.ch, (unsigned long long)b.count,
                    (unsigned long long)b.rank, (unsigned long long)b.resolve_pos, (unsigned long long)b.resolve_chr);
            return 1;
        }
    }
    return 0;
}

static int runSort(unsigned long long n, const std::string& pattern)
{
    std::mt19937_64 rng(12345 + n);
    std::vector<SeedRec> rec((size_t)n);
    for (unsigned long long i = 0; i < n; i++) {
        SeedRec r{1000, 7, 100, (int32_t)i, (5u << 8) | 'A'};      // vid = the index: a key that ties shows an unstable pass
        if (pattern == "random") r = SeedRec{rng(), (uint32_t)rng(), (uint32_t)rng(), (int32_t)i, ((uint32_t)rng() & 0xFFFFFF00u) | 'C'};
        else if (pattern == "count_top") r.count = (uint32_t)(rng() & 255u) << 24;
        else if (pattern == "chr_only") r.chrCh = (((uint32_t)rng() & 0xFFFFFFu) << 8) | 'G';
        else if (pattern == "rank_low") r.rank = 0x1234567800ull | (rng() & 255u);
        else if (pattern == "rank_wrap") r.rank = (1ull << 63) + (unsigned long long)((long long)(rng() % 2001) - 1000);
        else if (pattern == "count_equal") { r.rank = rng(); r.pos = (uint32_t)rng(); r.count = 42; }
        else { fprintf(stderr, "unknown pattern %s\n", pattern.c_str()); return 2; }
        rec[(size_t)i] = r;
    }
    std::vector<lcb_seed> want;
    for (const SeedRec& r : rec) want.push_back(expand(r));
    std::stable_sort(want.begin(), want.end(), seedLess);
    int passes = 0, skipped = 0;
    sortOnEmu(rec, passes, skipped);
    printf("n %llu tile %d passes %d skipped %d\n", n, S_TILE, passes, skipped);
    if (passes + skipped != S_DIGITS) { fprintf(stderr, "%d + %d passes, the key has %d digits\n", passes, skipped, S_DIGITS); return 1; }
    return compare(rec, want, true);
}

static int runEnum(int argc, char** argv)
{
    const std::string junctions = argv[2], fasta = argv[3];
    const int k = atoi(argv[4]), abundance = atoi(argv[5]);
    const uint64_t segCap = argc > 6 ? strtoull(argv[6], nullptr, 10) : 0, segGap = argc > 7 ? strtoull(argv[7], nullptr, 10) : 0;
    lcb_graph* g = lcb_graph_load_impl(junctions.c_str(), {fasta}, k, abundance, 2);
    std::vector<lcb_seed> want;
    lcb_enumerate_seeds_impl(*g, 2, want);

    // the tables of device.hip
    const LcbSegPlan plan = lcb_plan_segments(*g, segCap, segGap);
    const bool seg = plan.nSeg() > 1 || segCap != 0;
    std::vector<uint8_t> posCh((size_t)plan.devPositions + 1, 0xEE), posRevCh((size_t)plan.devPositions + 1, 0xEE);     // (a read inside a gap shows)
    for (uint32_t s = 0; s < plan.nSeg(); s++)
        for (uint64_t q = plan.segStart[s]; q < plan.segStart[s + 1]; q++) { posCh[(size_t)(plan.segDev[s] + q - plan.segStart[s])] = g->posCh[q]; posRevCh[(size_t)(plan.segDev[s] + q - plan.segStart[s])] = g->posRevCh[q]; }
    std::vector<uint32_t> os32(g->occStart.begin(), g->occStart.end());
    std::vector<uint4> occRec((size_t)g->nPos());
    for (uint64_t j = 0; j < g->nPos(); j++) {
        const uint64_t q = g->occG[j];
        const uint32_t cw = plan.chrWord[g->occChr[j]];
        occRec[(size_t)j] = uint4{(uint32_t)(q - plan.segStart[cw >> LCB_SEG_SHIFT]), cw, g->posPos[q], (uint32_t)g->posId[q]};
    }
    SeedTables T{seg ? nullptr : os32.data(), seg ? g->occStart.data() : nullptr, occRec.data(), posCh.data(), posRevCh.data(), plan.segDev.data(), g->nVertex};

    const unsigned long long nWaves = ((unsigned long long)g->nVertex + S_VPW - 1) / S_VPW;
    const uint32_t grid = (uint32_t)((nWaves + S_WAVES - 1) / S_WAVES);
    std::vector<unsigned long long> waveCnt((size_t)grid * S_WAVES + 1, 0);
    unsigned long long total = 0;
    uint32_t err = 0;
    launch(grid, S_T, [&]() { seedCount(T, waveCnt.data()); });
    launch(1, S_SCAN_T, [&]() { seedScan64(waveCnt.data(), nWaves, &total); });
    std::vector<SeedRec> rec((size_t)total);
    launch(grid, S_T, [&]() { seedFill(T, waveCnt.data(), rec.data(), total, &err); });
    if (err) { fprintf(stderr, "the fill pass found more seeds than the count pass\n"); return 1; }
    int passes = 0, skipped = 0;
    sortOnEmu(rec, passes, skipped);
    unsigned long long maxCount = 0;
    for (const lcb_seed& s : want) maxCount = std::max<unsigned long long>(maxCount, s.count);
    printf("seeds %llu vertices %u segments %u max_count %llu passes %d skipped %d\n", total, g->nVertex, plan.nSeg(), maxCount, passes, skipped);
    const int rc = compare(rec, want, true);
    delete g;
    return rc;
}

static int runScan(const std::string& kernel, unsigned long long n)
{
    if (kernel == "seedScan32") return scanCheckAll<uint32_t>("seedScan32", n, 4ull * S_SCAN_T, [](uint32_t* a, unsigned long long m, unsigned long long* t) { launch(1, S_SCAN_T, [&]() { seedScan32(a, m, t); }); });
    // (a run of `per` consecutive entries per lane: the second lane's first entry stands for the second piece)
    if (kernel == "seedScan64") return scanCheckAll<unsigned long long>("seedScan64", n, (n + S_SCAN_T - 1) / S_SCAN_T, [](unsigned long long* a, unsigned long long m, unsigned long long* t) { launch(1, S_SCAN_T, [&]() { seedScan64(a, m, t); }); });
    fprintf(stderr, "unknown kernel %s\n", kernel.c_str());
    return 2;
}

int main(int argc, char** argv)
{
    try {
        if (argc >= 4 && std::string(argv[1]) == "scan") return runScan(argv[2], strtoull(argv[3], nullptr, 10));
        if (argc >= 4 && std::string(argv[1]) == "sort") return runSort(strtoull(argv[2], nullptr, 10), argv[3]);
        if (argc >= 6 && std::string(argv[1]) == "enum") return runEnum(argc, argv);
    } catch (std::exception& e) { fprintf(stderr, "error: %s\n", e.what()); return 2; }
    fprintf(stderr, "usage: seeds_emu enum <junctions> <fasta> <k> <abundance> [seg_cap seg_gap] | seeds_emu sort <N> <pattern> | seeds_emu scan <kernel> <n>\n");
    return 2;
}
