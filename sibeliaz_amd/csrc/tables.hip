// tables.hip — the device route of device creation (LCB_TABLES_DEVICE): the tables that are functions of the loaded graph - posWin
// (lcb_window_table of lcb_segments.h), occStart and occRec (graph.cpp's CSR, device.hip's records) - computed on one MI355X from
// the per-position arrays device.hip has uploaded. The kernels are in lcb_table_kernels.h; DESIGN.md §12 has the data read, the
// order argument and the memory formula.
//
//   windows   tableWindow
//   csr       tableKeys (counts per vertex + the sort's input) -> tableScan over nVertex + 1 entries = occStart
//   sort      tableDigitHist (all 4 digits) -> per digit that tells two keys apart: tableTileHist -> tableScan -> tableScatter
//   gather    the sort's second buffers are released, occRec is made, tableGather fills it
//   hand-over (lcb_open_fasta; LcbTableHandover): handPatch in front of the windows; between sort and gather the host CSR
//             is downloaded - occStart, the sorted payloads, handOccChr of them (lcb_handover_kernels.h)
//
// Every temporary belongs to one Run, is made through the device's own allocator (devAlloc: registered with the device's owner),
// checked against hipMemGetInfo before it is taken, and dropped before the call returns, whatever way it ends: createUsed and the
// workspaces come after.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstring>
#include <string>
#include <vector>

#include "lcb_device.h"
#include "lcb_handover_kernels.h"
#include "lcb_host.h"
#include "lcb_segments.h"
#include "lcb_table_kernels.h"

#define HIP_CHECK(x)                                                                              \
    do {                                                                                          \
        hipError_t e_ = (x);                                                                      \
        if (e_ != hipSuccess) throw LcbError(std::string(#x) + " failed: " + hipGetErrorString(e_)); \
    } while (0)

using namespace lcb_tablek;

namespace {

// Everything the build owns on the device besides its results; nothing stays behind.
struct Run {
    LcbTableJob& job;
    hipStream_t stream;
    hipEvent_t evA = nullptr, evB = nullptr;
    std::vector<std::pair<void*, uint64_t>> owned;
    uint64_t live = 0, peak = 0;
    explicit Run(LcbTableJob& j) : job(j), stream((hipStream_t)j.stream)
    {
        HIP_CHECK(hipEventCreate(&evA));
        HIP_CHECK(hipEventCreate(&evB));
    }
    ~Run()
    {
        (void)hipStreamSynchronize(stream);
        for (auto& p : owned) if (p.first) { try { job.drop(job.owner, p.first); } catch (...) {} }
        if (evA) (void)hipEventDestroy(evA);
        if (evB) (void)hipEventDestroy(evB);
    }
    template <class T>
    T* alloc(uint64_t bytes)
    {
        owned.emplace_back(nullptr, bytes);
        owned.back().first = job.alloc(job.owner, (size_t)(bytes ? bytes : 1));
        live += bytes;
        peak = std::max(peak, live);
        return (T*)owned.back().first;
    }
    void release(void* p)
    {
        for (auto& o : owned)
            if (o.first == p) { o.first = nullptr; live -= o.second; job.drop(job.owner, p); }
    }
    template <class T, class S>
    T* upload(const S* src, size_t n)
    {
        static_assert(sizeof(T) == sizeof(S), "same layout");
        T* d = alloc<T>(n * sizeof(T));
        if (n) HIP_CHECK(hipMemcpyAsync(d, src, n * sizeof(T), hipMemcpyHostToDevice, stream));
        return d;
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

// (items > 0: a launch of no workgroups is never made)
uint32_t gridFor(const char* fn, uint64_t items, uint64_t perBlock)
{
    const uint64_t n = std::max<uint64_t>(1, (items + perBlock - 1) / perBlock);
    if (n > 0x7FFFFFFFull) throw LcbError(std::string(fn) + ": the input needs more workgroups than one launch has");
    return (uint32_t)n;
}

// The 32-bit and the 64-bit instantiation of the kernels under one name each.
template <class Q> struct K;
template <> struct K<uint32_t> {
    static constexpr auto keys = tableKeys32; static constexpr auto scan = tableScan32; static constexpr auto tileHist = tableTileHist32;
    static constexpr auto scatter = tableScatter32; static constexpr auto gather = tableGather32; static constexpr auto occChr = lcb_handk::handOccChr32;
};
template <> struct K<unsigned long long> {
    static constexpr auto keys = tableKeys64; static constexpr auto scan = tableScan64; static constexpr auto tileHist = tableTileHist64;
    static constexpr auto scatter = tableScatter64; static constexpr auto gather = tableGather64; static constexpr auto occChr = lcb_handk::handOccChr64;
};

// (hand-over) n entries of Q from the device into the host's 64-bit vector: as they are, or widened chunk by chunk
template <class Q>
void drain(Run& R, const Q* src, uint64_t n, uint64_t* dst)
{
    if (!n) return;
    if constexpr (sizeof(Q) == 8) {
        HIP_CHECK(hipMemcpyAsync(dst, src, (size_t)n * 8, hipMemcpyDeviceToHost, R.stream));
        HIP_CHECK(hipStreamSynchronize(R.stream));
    } else {
        const uint64_t chunk = std::min<uint64_t>(n, 1ull << 24);
        std::vector<uint32_t> buf((size_t)chunk);
        for (uint64_t c0 = 0; c0 < n; c0 += chunk) {
            const int64_t m = (int64_t)std::min(chunk, n - c0);
            HIP_CHECK(hipMemcpyAsync(buf.data(), src + c0, (size_t)m * 4, hipMemcpyDeviceToHost, R.stream));
            HIP_CHECK(hipStreamSynchronize(R.stream));
            const uint32_t* b = buf.data();
            uint64_t* o = dst + c0;
            #pragma omp parallel for schedule(static) if (m > (1 << 16))
            for (int64_t i = 0; i < m; i++) o[i] = b[i];
        }
    }
}

template <class Q>
void build(Run& R, lcb_table_stats& X)
{
    LcbTableJob& J = R.job;
    const lcb_graph& g = *J.g;
    const LcbSegPlan& plan = *J.plan;
    const uint64_t P = g.nPos(), V1 = (uint64_t)g.nVertex + 1, C = g.nChr();
    Q* occStart = (Q*)J.occStart;
    HIP_CHECK(hipMemsetAsync(occStart, 0, V1 * sizeof(Q), R.stream));
    LcbTableHandover* const H = J.hand;
    if (!P) {                                                           // nothing survived the abundance filter: empty lists, no record
        J.occRec = J.alloc(J.owner, 1);
        HIP_CHECK(hipStreamSynchronize(R.stream));
        X.sort_passes_skipped = T_DIGITS;
        if (H) {                                                        // (the cleared lists come down like any others; no kernel is launched)
            H->g->occStart.resize((size_t)V1); H->g->occG.clear(); H->g->occChr.clear();
            drain<Q>(R, occStart, V1, H->g->occStart.data());
            H->csrBytes = sizeof(Q) * V1; H->peakBytes = 1;
        }
        return;
    }
    const uint32_t nTiles = gridFor(J.fn, P, T_TILE);
    const uint64_t planBytes = (2 * C + 1) * 8 + C * 4, histBytes = (uint64_t)T_DIGITS * 256 * 8 + 8, tileBytes = (uint64_t)nTiles * 256 * sizeof(Q);
    const uint64_t sortBytes = 2 * P * (4 + sizeof(Q)) + tileBytes + histBytes + planBytes;
    lcb_tables_need_impl(J.fn, sortBytes, "the table build of " + std::to_string(P) + " positions (" + std::to_string(2 * (4 + sizeof(Q))) + " bytes each and a byte of histograms)");

    // ---- the plan as the kernels read it
    static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "64-bit counts");
    TablePlan pl;
    pl.chrStart = R.upload<unsigned long long>(g.chrStart.data(), (size_t)C + 1);
    pl.chrDev = R.upload<unsigned long long>(plan.chrDev.data(), (size_t)C);
    pl.chrWord = R.upload<uint32_t>(plan.chrWord.data(), (size_t)C);
    pl.segBase = (const unsigned long long*)J.segBase;
    pl.nChr = (uint32_t)C;
    X.upload_bytes += planBytes;
    const uint32_t gridP = gridFor(J.fn, P, T_T);

    // ---- (hand-over) the device's copy of the letters the host has patched in its own: before anything reads posCh - no table kernel does
    if (H && H->nPatch) {
        lcb_tables_need_impl(J.fn, H->nPatch * 9, "the patch list of " + std::to_string(H->nPatch) + " characters (9 bytes each)");
        R.timed(H->patchMs, [&]() {
            const unsigned long long* pq = R.upload<unsigned long long>(H->patchQ, (size_t)H->nPatch);
            const uint8_t* pc = R.upload<uint8_t>(H->patchLetter, (size_t)H->nPatch);
            lcb_handk::handPatch<<<gridFor(J.fn, H->nPatch, lcb_handk::H_T), lcb_handk::H_T, 0, R.stream>>>(pl, pq, pc, H->nPatch, P, H->posCh);
        });
        X.upload_bytes += H->nPatch * 9;
    }

    R.timed(X.window_ms, [&]() { tableWindow<<<gridP, T_T, 0, R.stream>>>(pl, J.posPos, J.posWin, P, J.maxBranch); });

    // ---- csr: counts per vertex, their exclusive scan; the keys and payloads of the sort on the way
    uint32_t* keys = R.alloc<uint32_t>(P * 4);
    Q* pay = R.alloc<Q>(P * sizeof(Q));
    unsigned long long* hist = R.alloc<unsigned long long>(histBytes);
    unsigned long long* total = hist + T_DIGITS * 256;
    unsigned long long hTotal = 0;
    R.timed(X.csr_ms, [&]() {
        hipLaunchKernelGGL(K<Q>::keys, dim3(gridP), dim3(T_T), 0, R.stream, pl, J.posId, keys, pay, occStart, P);
        hipLaunchKernelGGL(K<Q>::scan, dim3(1), dim3(T_SCAN_T), 0, R.stream, occStart, V1, total);
        HIP_CHECK(hipMemcpyAsync(&hTotal, total, 8, hipMemcpyDeviceToHost, R.stream));
    });
    if (hTotal != P) throw LcbError(std::string(J.fn) + ": internal error: the vertex counts sum to " + std::to_string(hTotal) + ", the graph has " + std::to_string(P) + " positions");

    // ---- sort: (|id|, q) by |id|, stable, so that a vertex's occurrences ascend in q
    uint32_t* keys2 = R.alloc<uint32_t>(P * 4);
    Q* pay2 = R.alloc<Q>(P * sizeof(Q));
    Q* tileHist = R.alloc<Q>(tileBytes);
    std::vector<unsigned long long> h((size_t)T_DIGITS * 256);
    R.timed(X.sort_ms, [&]() {
        HIP_CHECK(hipMemsetAsync(hist, 0, histBytes, R.stream));
        tableDigitHist<<<gridFor(J.fn, P, (uint64_t)T_T * T_HIST_ITEMS), T_T, 0, R.stream>>>(keys, P, hist);
        HIP_CHECK(hipMemcpyAsync(h.data(), hist, (size_t)T_DIGITS * 256 * 8, hipMemcpyDeviceToHost, R.stream));
    });
    uint32_t *kin = keys, *kout = keys2;
    Q *pin = pay, *pout = pay2;
    for (int p = 0; p < T_DIGITS; p++) {
        bool one = false;
        unsigned long long sum = 0;
        for (int x = 0; x < 256; x++) { sum += h[(size_t)p * 256 + x]; one = one || h[(size_t)p * 256 + x] == P; }
        if (sum != P) throw LcbError(std::string(J.fn) + ": internal error: a digit histogram counts " + std::to_string(sum) + " of " + std::to_string(P) + " keys");
        if (one) { X.sort_passes_skipped++; continue; }       // every key agrees on this digit
        R.timed(X.sort_ms, [&]() {
            hipLaunchKernelGGL(K<Q>::tileHist, dim3(nTiles), dim3(64), 0, R.stream, kin, P, p, tileHist, nTiles);
            hipLaunchKernelGGL(K<Q>::scan, dim3(1), dim3(T_SCAN_T), 0, R.stream, tileHist, (unsigned long long)nTiles * 256, total);
            hipLaunchKernelGGL(K<Q>::scatter, dim3(nTiles), dim3(64), 0, R.stream, kin, pin, kout, pout, P, p, tileHist, nTiles);
        });
        std::swap(kin, kout); std::swap(pin, pout);
        X.sort_passes++;
    }

    // ---- gather: only the sorted payloads are still needed
    R.release(kin); R.release(kout); R.release(pout); R.release(tileHist);

    // ---- (hand-over) the host CSR from what the device has just made: occStart = the scan's result, occG = the sorted payloads (the dense
    // host position, ascending inside a vertex because the sort is stable: graph.cpp's order), occChr = handOccChr of them
    if (H) {
        const double t0 = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
        lcb_graph& hg = *H->g;
        lcb_tables_need_impl(J.fn, P * 4, "the chromosomes of " + std::to_string(P) + " occurrences (4 bytes each)");
        uint32_t* occChr = R.alloc<uint32_t>(P * 4);
        hipLaunchKernelGGL(K<Q>::occChr, dim3(gridP), dim3(lcb_handk::H_T), 0, R.stream, pl, (const Q*)pin, occChr, P);
        HIP_CHECK(hipGetLastError());
        hg.occStart.resize((size_t)V1); hg.occG.resize((size_t)P); hg.occChr.resize((size_t)P);
        drain<Q>(R, occStart, V1, hg.occStart.data());
        drain<Q>(R, pin, P, hg.occG.data());
        HIP_CHECK(hipMemcpyAsync(hg.occChr.data(), occChr, (size_t)P * 4, hipMemcpyDeviceToHost, R.stream));
        HIP_CHECK(hipStreamSynchronize(R.stream));
        R.release(occChr);
        H->csrBytes = (sizeof(Q) + 4) * P + sizeof(Q) * V1;
        H->csrMs += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count() - t0;
    }
    lcb_tables_need_impl(J.fn, P * 16, "the occurrence records of " + std::to_string(P) + " positions (16 bytes each)");
    uint4* rec = (uint4*)J.alloc(J.owner, (size_t)P * 16);
    J.occRec = rec;
    if (H) H->peakBytes = std::max(R.peak, R.live + P * 16);
    R.timed(X.gather_ms, [&]() { hipLaunchKernelGGL(K<Q>::gather, dim3(gridP), dim3(T_T), 0, R.stream, pl, pin, J.posPos, J.posId, rec, P); });
}

}  // namespace

void lcb_tables_need_impl(const char* fn, uint64_t bytes, const std::string& what)
{
    size_t freeB = 0, totalB = 0;
    HIP_CHECK(hipMemGetInfo(&freeB, &totalB));
    if (bytes > (uint64_t)freeB)
        throw LcbError(std::string(fn) + ": " + what + " needs " + std::to_string(bytes) + " bytes of device memory, " + std::to_string((uint64_t)freeB) + " are free");
}

void lcb_build_tables_impl(LcbTableJob& job, lcb_table_stats& stats)
{
    Run R(job);
    if (job.seg) build<unsigned long long>(R, stats);
    else build<uint32_t>(R, stats);
    stats.device_bytes = R.peak;
}
