// seeds.hip — seed (bundle) enumeration and ordering on one MI355X: what bundles.cpp computes on the host (BlocksFinder::FindBlocks,
// blocksfinder.h:461-503, and the std::sort at :517), from the tables lcb_device_create has already put into HBM. The kernels are in
// lcb_seed_kernels.h; DESIGN.md §11 has the data read, the key layout and the memory formula.
//
//   enumerate   seedCount -> seedScan64 -> (S is known: everything else is sized by it) -> seedFill -> sort -> D2H of 24 B per seed ->
//               expansion to lcb_seed on the host
//   sort        seedDigitHist (all 19 digits) -> per digit that tells two keys apart: seedTileHist -> seedScan32 -> seedScatter
//
// Device memory is taken after the tables, accounted for, checked against hipMemGetInfo before it is taken, and released before the
// call returns, whatever way it ends.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "lcb_device.h"
#include "lcb_host.h"
#include "lcb_seed_kernels.h"

#define HIP_CHECK(x)                                                                              \
    do {                                                                                          \
        hipError_t e_ = (x);                                                                      \
        if (e_ != hipSuccess) throw LcbError(std::string(#x) + " failed: " + hipGetErrorString(e_)); \
    } while (0)

using namespace lcb_seedk;

namespace {

double nowMs() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

static_assert(sizeof(SeedRec) == 24, "a seed on the device is 24 bytes");

// Everything a call owns on the device; nothing stays behind.
struct Run {
    const char* fn;
    hipStream_t stream;
    hipEvent_t evA = nullptr, evB = nullptr;
    std::vector<std::pair<void*, uint64_t>> owned;
    uint64_t live = 0, peak = 0;
    Run(const char* name, hipStream_t s) : fn(name), stream(s)
    {
        HIP_CHECK(hipEventCreate(&evA));
        HIP_CHECK(hipEventCreate(&evB));
    }
    ~Run()
    {
        (void)hipStreamSynchronize(stream);
        for (auto& p : owned) if (p.first) (void)hipFree(p.first);
        if (evA) (void)hipEventDestroy(evA);
        if (evB) (void)hipEventDestroy(evB);
    }
    // `bytes` in all, for `what`: refused up front, with both numbers, if the device does not report that much free.
    void need(uint64_t bytes, const std::string& what) const
    {
        size_t freeB = 0, totalB = 0;
        HIP_CHECK(hipMemGetInfo(&freeB, &totalB));
        if (bytes > (uint64_t)freeB)
            throw LcbError(std::string(fn) + ": " + what + " needs " + std::to_string(bytes) + " bytes of device memory, " + std::to_string((uint64_t)freeB) + " are free");
    }
    template <class T>
    T* alloc(uint64_t bytes)
    {
        void* p = nullptr;
        HIP_CHECK(hipMalloc(&p, bytes ? bytes : 1));
        owned.emplace_back(p, bytes);
        live += bytes;
        peak = std::max(peak, live);
        return (T*)p;
    }
    void release(void* p)
    {
        for (auto& o : owned)
            if (o.first == p) { HIP_CHECK(hipFree(p)); live -= o.second; o.first = nullptr; }
    }
    template <class W>
    void timed(double& ms, W work)
    {
        HIP_CHECK(hipEventRecord(evA, stream));
        work();
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipEventRecord(evB, stream));
        HIP_CHECK(hipStreamSynchronize(stream));
        float t = 0;
        HIP_CHECK(hipEventElapsedTime(&t, evA, evB));
        ms += t;
    }
};

uint32_t gridFor(const char* fn, uint64_t items, uint64_t perBlock)
{
    const uint64_t n = std::max<uint64_t>(1, (items + perBlock - 1) / perBlock);
    if (n > 0x7FFFFFFFull) throw LcbError(std::string(fn) + ": the input needs more workgroups than one launch has");
    return (uint32_t)n;
}

uint64_t tilesOf(uint64_t n) { return (n + S_TILE - 1) / S_TILE; }
// What the sort holds besides the records themselves: the second record buffer, the tile histograms, the digit histograms and the scan's total.
uint64_t sortBytes(uint64_t n) { return n * sizeof(SeedRec) + tilesOf(n) * 256 * sizeof(uint32_t) + (uint64_t)S_DIGITS * 256 * 8 + 8; }

// Sorts rec[0..n) (device memory of the run); the result is in the returned buffer (rec or the run's second buffer).
SeedRec* sortRecords(Run& R, SeedRec* rec, uint64_t n, int32_t& passes, int32_t& skipped, double& ms)
{
    passes = 0; skipped = S_DIGITS;
    if (n < 2) return rec;
    const uint32_t nTiles = gridFor(R.fn, n, S_TILE);
    SeedRec* other = R.alloc<SeedRec>(n * sizeof(SeedRec));
    uint32_t* tileHist = R.alloc<uint32_t>((uint64_t)nTiles * 256 * sizeof(uint32_t));
    unsigned long long* hist = R.alloc<unsigned long long>((uint64_t)S_DIGITS * 256 * 8 + 8);
    unsigned long long* total = hist + S_DIGITS * 256;
    std::vector<unsigned long long> h((size_t)S_DIGITS * 256 + 1);
    R.timed(ms, [&]() {
        HIP_CHECK(hipMemsetAsync(hist, 0, (size_t)S_DIGITS * 256 * 8 + 8, R.stream));
        seedDigitHist<<<std::min<uint32_t>(gridFor(R.fn, n, S_T), 2048u), S_T, 0, R.stream>>>(rec, n, hist);
        HIP_CHECK(hipMemcpyAsync(h.data(), hist, (size_t)S_DIGITS * 256 * 8, hipMemcpyDeviceToHost, R.stream));
    });
    skipped = 0;
    SeedRec *in = rec, *out = other;
    for (int p = 0; p < S_DIGITS; p++) {
        bool one = false;
        unsigned long long sum = 0;
        for (int x = 0; x < 256; x++) { sum += h[(size_t)p * 256 + x]; one = one || h[(size_t)p * 256 + x] == n; }
        if (sum != n) throw LcbError(std::string(R.fn) + ": internal error: a digit histogram counts " + std::to_string(sum) + " of " + std::to_string(n) + " seeds");
        if (one) { skipped++; continue; }        // every key agrees on this digit
        R.timed(ms, [&]() {
            seedTileHist<<<nTiles, 64, 0, R.stream>>>(in, n, p, tileHist, nTiles);
            seedScan32<<<1, S_SCAN_T, 0, R.stream>>>(tileHist, (unsigned long long)nTiles * 256, total);
            seedScatter<<<nTiles, 64, 0, R.stream>>>(in, out, n, p, tileHist, nTiles);
        });
        std::swap(in, out);
        passes++;
    }
    return in;
}

}  // namespace

int64_t lcb_device_enumerate_seeds_impl(lcb_device* d, lcb_seed** out, lcb_seed_stats* stats)
{
    static const char* fn = "lcb_device_enumerate_seeds";
    const LcbSeedView V = lcb_device_seed_view_impl(d, fn);
    lcb_seed_stats X;
    memset(&X, 0, sizeof(X));
    Run R(fn, (hipStream_t)V.stream);
    const SeedTables T{V.occStart32, V.occStart64, (const uint4*)V.occRec, V.posCh, V.posRevCh, V.segBase, V.nVertex};
    X.vertices = V.nVertex;

    // ---- count: the seeds of every wave's vertices, their exclusive scan, S
    const uint64_t nWaves = ((uint64_t)V.nVertex + S_VPW - 1) / S_VPW;
    const uint32_t grid = gridFor(fn, nWaves, S_WAVES);
    const uint64_t waveBytes = ((uint64_t)grid * S_WAVES + 2) * 8 + 8;
    R.need(waveBytes, "the seed counts of " + std::to_string(V.nVertex) + " vertices");
    unsigned long long* waveCnt = R.alloc<unsigned long long>(waveBytes);
    unsigned long long* total = waveCnt + (uint64_t)grid * S_WAVES + 1;
    uint32_t* err = (uint32_t*)(total + 1);
    unsigned long long hTotal[2] = {0, 0};
    R.timed(X.count_ms, [&]() {
        HIP_CHECK(hipMemsetAsync(waveCnt, 0, waveBytes, R.stream));
        if (nWaves) seedCount<<<grid, S_T, 0, R.stream>>>(T, waveCnt);
        seedScan64<<<1, S_SCAN_T, 0, R.stream>>>(waveCnt, nWaves, total);
        HIP_CHECK(hipMemcpyAsync(hTotal, total, 8, hipMemcpyDeviceToHost, R.stream));
    });
    const uint64_t S = hTotal[0];
    if (S >= 0xFFFFFFFFull) throw LcbError(std::string(fn) + ": " + std::to_string(S) + " seeds: the device sort places fewer than 2^32");
    X.seeds = (int64_t)S;

    // ---- fill + sort: 24 B per seed for the records, as much again plus one byte for the sort
    R.need(S * sizeof(SeedRec) + (S > 1 ? sortBytes(S) : 0), std::to_string(S) + " seeds (48 bytes each and a byte of histograms)");
    SeedRec* rec = R.alloc<SeedRec>(S * sizeof(SeedRec));
    if (S) {
        R.timed(X.fill_ms, [&]() {
            seedFill<<<grid, S_T, 0, R.stream>>>(T, waveCnt, rec, S, err);
            HIP_CHECK(hipMemcpyAsync(hTotal, err, 4, hipMemcpyDeviceToHost, R.stream));
        });
        if ((uint32_t)hTotal[0]) throw LcbError(std::string(fn) + ": internal error: the writing pass found more seeds than the counting pass");
    }
    R.release(waveCnt);
    const SeedRec* sorted = sortRecords(R, rec, S, X.sort_passes, X.sort_passes_skipped, X.sort_ms);

    // ---- copy: D2H of the records, expansion to lcb_seed
    const double t0 = nowMs();
    lcb_seed* res = (lcb_seed*)malloc((S ? S : 1) * sizeof(lcb_seed));
    SeedRec* host = (SeedRec*)malloc((S ? S : 1) * sizeof(SeedRec));
    if (!res || !host) { free(res); free(host); throw LcbError("out of memory"); }
    const hipError_t ce = S ? hipMemcpy(host, sorted, S * sizeof(SeedRec), hipMemcpyDeviceToHost) : hipSuccess;
    if (ce != hipSuccess) { free(res); free(host); throw LcbError(std::string(fn) + ": copying the seeds to the host failed: " + hipGetErrorString(ce)); }
    #pragma omp parallel for schedule(static) if (S > (1u << 16))
    for (int64_t i = 0; i < (int64_t)S; i++) {
        const SeedRec& r = host[i];
        res[i] = lcb_seed{r.vid, (int32_t)(signed char)(r.chrCh & 255u), r.count, r.rank, r.pos, r.chrCh >> 8};
    }
    free(host);
    X.copy_ms = nowMs() - t0;
    X.max_count = S ? (int64_t)res[0].count : 0;      // (count descending)
    X.device_bytes = R.peak;
    *out = res;
    if (stats) *stats = X;
    return (int64_t)S;
}

void lcb_device_sort_seeds_impl(lcb_device* d, lcb_seed* seeds, int64_t n)
{
    static const char* fn = "lcb_device_sort_seeds";
    const LcbSeedView V = lcb_device_seed_view_impl(d, fn);
    if (n >= 0xFFFFFFFFll) throw LcbError(std::string(fn) + ": " + std::to_string(n) + " seeds: the device sort places fewer than 2^32");
    for (int64_t i = 0; i < n; i++) {
        const lcb_seed& s = seeds[i];
        if (s.count > 0xFFFFFFFFull || s.resolve_pos > 0xFFFFFFFFull || s.resolve_chr > 0xFFFFFFull)
            throw LcbError(std::string(fn) + ": seed " + std::to_string(i) + " has count " + std::to_string(s.count) + ", resolve_pos " + std::to_string(s.resolve_pos) + ", resolve_chr " +
                           std::to_string(s.resolve_chr) + ": the device key holds 32, 32 and 24 bits of them");
    }
    if (n < 2) return;
    const uint64_t S = (uint64_t)n;
    Run R(fn, (hipStream_t)V.stream);
    R.need(S * sizeof(SeedRec) + sortBytes(S), std::to_string(S) + " seeds (48 bytes each and a byte of histograms)");
    // the record carries the index of the caller's seed where an enumerated one carries its vertex: vid and ch never leave the host
    std::vector<SeedRec> host((size_t)S);
    #pragma omp parallel for schedule(static) if (S > (1u << 16))
    for (int64_t i = 0; i < n; i++) host[(size_t)i] = SeedRec{seeds[i].rank, (uint32_t)seeds[i].count, (uint32_t)seeds[i].resolve_pos, (int32_t)(uint32_t)i, (uint32_t)seeds[i].resolve_chr << 8};
    SeedRec* rec = R.alloc<SeedRec>(S * sizeof(SeedRec));
    HIP_CHECK(hipMemcpy(rec, host.data(), S * sizeof(SeedRec), hipMemcpyHostToDevice));
    int32_t passes = 0, skipped = 0;
    double ms = 0;
    const SeedRec* sorted = sortRecords(R, rec, S, passes, skipped, ms);
    HIP_CHECK(hipMemcpy(host.data(), sorted, S * sizeof(SeedRec), hipMemcpyDeviceToHost));
    std::vector<lcb_seed> res((size_t)S);
    #pragma omp parallel for schedule(static) if (S > (1u << 16))
    for (int64_t i = 0; i < n; i++) res[(size_t)i] = seeds[(uint32_t)host[(size_t)i].vid];
    memcpy(seeds, res.data(), (size_t)S * sizeof(lcb_seed));
}
