// lcb_table_kernels.h — device code of the table build on the GPU (host driver: tables.hip).
// What createTables of device.hip computes on host threads from a loaded graph - the look-ahead windows (lcb_window_table of
// lcb_segments.h), the CSR over |id| (graph.cpp) and the 16-byte occurrence records - from the four per-position arrays that go to the
// device anyway. Kept in a header of its own so that the wavefront emulator of tests/emu compiles and runs the same kernels on the
// CPU (tests/test_tables_emu.py).
//
//   windows   tableWindow: one lane per position, two binary searches inside the position's chromosome, each over at most maxBranch + 1 steps.
//   CSR       tableKeys counts |id| per vertex (the counts do not depend on the order of the additions) and writes the sort's input,
//             (key |id|, payload q) for q = 0 .. P - 1; tableScan turns the counts into occStart.
//   order     stable LSD radix sort of (key, payload), 8 bits per pass, over the 4 key bytes: one histogram of all digits up front
//             (tableDigitHist; the host skips the digits on which every key agrees), then per digit tableTileHist -> tableScan ->
//             tableScatter. The input ascends in q and every pass is stable, so the occurrences of a vertex ascend in q whatever the
//             hardware does: no place in the output comes from the return value of an atomic on global memory.
//   records   tableGather: CSR slot j -> {g in its segment, chrWord, posPos[q], posId[q]}.
//
// Every kernel walks the dense HOST positions [0, P) and reaches the device tables through the plan (TablePlan): a chromosome is
// contiguous on the device, so the test gaps between segments (lcb_segments.h) are neither read nor written. Q is the type of a
// payload, a count and a tile offset: uint32_t, or unsigned long long in the segmented instantiation (P may exceed 2^32 there).
#ifndef LCB_TABLE_KERNELS_H
#define LCB_TABLE_KERNELS_H

#include <hip/hip_runtime.h>

#include <stdint.h>

#include "lcb_kernel_limits.h"

namespace lcb_tablek {

constexpr int T_T = 256;                      // lanes of a workgroup of the per-position kernels
constexpr int T_HIST_ITEMS = 16;              // keys per lane of tableDigitHist
constexpr int T_SCAN_T = 1024;                // lanes of the scan workgroup
constexpr int T_SORT_ITEMS = 16;              // records per lane of a sort tile
constexpr int T_TILE = 64 * T_SORT_ITEMS;     // records per workgroup (one wavefront) of tableTileHist / tableScatter
constexpr int T_DIGITS = 4;                   // key bytes of |id|, least significant first

// Orders the LDS accesses of the lanes of one wavefront: LDS operations of a wavefront execute in issue order, so only the compiler
// has to be kept from moving them (LCB_WAVE_SYNC_LDS of lcb_kernel.h).
#define T_WAVE_SYNC()                                             \
    do {                                                          \
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");    \
        __builtin_amdgcn_wave_barrier();                          \
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");    \
    } while (0)

// The LcbSegPlan as the kernels read it (device pointers).
struct TablePlan {
    const unsigned long long* chrStart;   // [nChr + 1] host flat index of every chromosome's first position (and the end of the last)
    const unsigned long long* chrDev;     // [nChr] device flat index of it
    const uint32_t* chrWord;              // [nChr] (segment << LCB_SEG_SHIFT) | chromosome
    const unsigned long long* segBase;    // [LCB_MAX_SEG] device flat index of g = 0 of every segment
    uint32_t nChr;
};

// The chromosome of host position q < chrStart[nChr]: the one with chrStart[c] <= q < chrStart[c + 1] (never an emptied one).
__device__ __forceinline__ uint32_t tableChrOf(const TablePlan& pl, unsigned long long q)
{
    uint32_t lo = 0, hi = pl.nChr;
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (pl.chrStart[mid] <= q) lo = mid; else hi = mid;
    }
    return lo;
}

// ---- posWin[q] = forward | backward << 16: exactly lcb_window_table (lcb_segments.h).
__global__ __launch_bounds__(T_T) void tableWindow(const TablePlan pl, const uint32_t* __restrict__ posPos, uint32_t* __restrict__ posWin, unsigned long long P, uint32_t maxBranch)
{
    const unsigned long long q = (unsigned long long)blockIdx.x * T_T + threadIdx.x;
    if (q >= P) return;
    const uint32_t c = tableChrOf(pl, q);
    const unsigned long long s = pl.chrStart[c], n = pl.chrStart[c + 1] - s, i = q - s;
    const uint32_t* pos = posPos + pl.chrDev[c];                      // the chromosome's positions: indices [0, n)
    const unsigned long long pq = pos[i];
    // forward: the last j in [i, n) with pos[j] <= pos[i] + maxBranch (positions differ by at least one per step)
    const uint32_t up = pq + maxBranch > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)(pq + maxBranch);
    unsigned long long lo = i, hi = n < i + maxBranch + 1 ? n : i + maxBranch + 1;
    while (lo < hi) {
        const unsigned long long mid = lo + (hi - lo) / 2;
        if (pos[mid] <= up) lo = mid + 1; else hi = mid;
    }
    const unsigned long long f = lo - i - 1;                          // (pos[i] <= up: lo > i)
    // backward: the first j in [0, i] with pos[j] >= pos[i] - maxBranch
    const uint32_t down = pq > maxBranch ? (uint32_t)(pq - maxBranch) : 0u;
    lo = i > maxBranch ? i - maxBranch : 0;
    hi = i + 1;
    while (lo < hi) {
        const unsigned long long mid = lo + (hi - lo) / 2;
        if (pos[mid] < down) lo = mid + 1; else hi = mid;
    }
    const unsigned long long b = i - lo;                              // (pos[i] >= down: lo <= i)
    posWin[pl.chrDev[c] + i] = (uint32_t)(f < 0xFFFF ? f : 0xFFFF) | ((uint32_t)(b < 0xFFFF ? b : 0xFFFF) << 16);
}

// ---- the sort's input and the vertex counts: keys[q] = |posId[q]|, pay[q] = q, count[|id|]++.
template <class Q>
__device__ __forceinline__ void tableKeysBody(const TablePlan& pl, const int32_t* __restrict__ posId, uint32_t* __restrict__ keys, Q* __restrict__ pay, Q* count, unsigned long long P)
{
    const unsigned long long q = (unsigned long long)blockIdx.x * T_T + threadIdx.x;
    if (q >= P) return;
    const uint32_t c = tableChrOf(pl, q);
    const int32_t id = posId[pl.chrDev[c] + (q - pl.chrStart[c])];
    const uint32_t a = id < 0 ? 0u - (uint32_t)id : (uint32_t)id;
    keys[q] = a;
    pay[q] = (Q)q;
    atomicAdd(&count[a], (Q)1);
}
__global__ __launch_bounds__(T_T) void tableKeys32(const TablePlan pl, const int32_t* posId, uint32_t* keys, uint32_t* pay, uint32_t* count, unsigned long long P) { tableKeysBody(pl, posId, keys, pay, count, P); }
__global__ __launch_bounds__(T_T) void tableKeys64(const TablePlan pl, const int32_t* posId, uint32_t* keys, unsigned long long* pay, unsigned long long* count, unsigned long long P) { tableKeysBody(pl, posId, keys, pay, count, P); }

// ---- exclusive scan of a[0..n) in place, *total = the sum. One workgroup of T_SCAN_T lanes: the array is walked in pieces of
// 4 * T_SCAN_T entries, four consecutive entries per lane, a shuffle scan inside each wavefront and the wavefronts' sums through LDS.
template <class Q>
__device__ __forceinline__ void tableScanBody(Q* a, unsigned long long n, unsigned long long* total)
{
    __shared__ Q ws[T_SCAN_T / 64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    Q carry = 0;
    for (unsigned long long p0 = 0; p0 < n; p0 += 4ull * T_SCAN_T) {            // (uniform: every lane of the workgroup takes every turn)
        const unsigned long long i = p0 + 4ull * threadIdx.x;
        Q v[4];
        for (int k = 0; k < 4; k++) v[k] = i + k < n ? a[i + k] : (Q)0;
        const Q sum = v[0] + v[1] + v[2] + v[3];
        Q inc = sum;
        for (int d = 1; d < 64; d <<= 1) {
            const Q o = (Q)__shfl_up(inc, d);
            if (lane >= d) inc += o;
        }
        if (lane == 63) ws[w] = inc;
        __syncthreads();
        Q base = 0, tot = 0;
        for (int k = 0; k < T_SCAN_T / 64; k++) {
            const Q x = ws[k];
            if (k < w) base += x;
            tot += x;
        }
        __syncthreads();
        Q run = carry + base + inc - sum;
        for (int k = 0; k < 4; k++) if (i + k < n) { a[i + k] = run; run += v[k]; }
        carry += tot;
    }
    if (threadIdx.x == 0) *total = carry;
}
__global__ __launch_bounds__(T_SCAN_T) void tableScan32(uint32_t* a, unsigned long long n, unsigned long long* total) { tableScanBody(a, n, total); }
__global__ __launch_bounds__(T_SCAN_T) void tableScan64(unsigned long long* a, unsigned long long n, unsigned long long* total) { tableScanBody(a, n, total); }

__device__ __forceinline__ uint32_t tableDigit(uint32_t key, int p) { return (key >> (8 * p)) & 255u; }

// ---- sort. hist[p * 256 + x] += the keys whose digit p is x, for all digits at once; workgroup b takes keys [b * T_T * T_HIST_ITEMS, ...).
// A wavefront whose keys agree on a digit - the high bytes of |id| - adds once, not 64 times to one LDS word.
__global__ __launch_bounds__(T_T) void tableDigitHist(const uint32_t* __restrict__ keys, unsigned long long n, unsigned long long* hist)
{
    __shared__ uint32_t h[T_DIGITS * 256];
    for (int i = threadIdx.x; i < T_DIGITS * 256; i += T_T) h[i] = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const unsigned long long b0 = (unsigned long long)blockIdx.x * (T_T * T_HIST_ITEMS) + (threadIdx.x & ~63);
    for (int k = 0; k < T_HIST_ITEMS; k++) {                                    // (uniform: the ballots inside are too)
        const unsigned long long i = b0 + (unsigned long long)k * T_T + lane;
        const bool valid = i < n;
        const uint32_t key = valid ? keys[i] : 0u;
        const unsigned long long vm = __ballot(valid);
        if (!vm) continue;                                                      // (wave-uniform)
        const int leader = __ffsll((long long)vm) - 1;
        for (int p = 0; p < T_DIGITS; p++) {
            const uint32_t x = tableDigit(key, p);
            const uint32_t f = (uint32_t)__shfl((int)x, leader);
            const unsigned long long same = __ballot(valid && x == f);
            if (same == vm) { if (lane == leader) atomicAdd(&h[p * 256 + f], (uint32_t)__popcll(vm)); }
            else if (valid) atomicAdd(&h[p * 256 + x], 1u);
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < T_DIGITS * 256; i += T_T) if (h[i]) atomicAdd(&hist[i], (unsigned long long)h[i]);
}

// Tile b = records [b * T_TILE, ...): tileHist[x * nTiles + b] = its records with digit p == x (digit-major: an exclusive scan over
// the whole array gives every (digit, tile) its first place in the output). One wavefront per tile.
template <class Q>
__device__ __forceinline__ void tableTileHistBody(const uint32_t* __restrict__ keys, unsigned long long n, int p, Q* tileHist, uint32_t nTiles)
{
    __shared__ uint32_t h[256];
    const int lane = threadIdx.x;
    for (int i = lane; i < 256; i += 64) h[i] = 0;
    T_WAVE_SYNC();
    const unsigned long long t0 = (unsigned long long)blockIdx.x * T_TILE;
    for (int k = 0; k < T_SORT_ITEMS; k++) {
        const unsigned long long i = t0 + (unsigned long long)k * 64 + lane;
        if (i < n) atomicAdd(&h[tableDigit(keys[i], p)], 1u);
    }
    T_WAVE_SYNC();
    for (int i = lane; i < 256; i += 64) tileHist[(unsigned long long)i * nTiles + blockIdx.x] = (Q)h[i];
}
__global__ __launch_bounds__(64) void tableTileHist32(const uint32_t* keys, unsigned long long n, int p, uint32_t* tileHist, uint32_t nTiles) { tableTileHistBody(keys, n, p, tileHist, nTiles); }
__global__ __launch_bounds__(64) void tableTileHist64(const uint32_t* keys, unsigned long long n, int p, unsigned long long* tileHist, uint32_t nTiles) { tableTileHistBody(keys, n, p, tileHist, nTiles); }

// The stable scatter of one tile: tileOff = the exclusive scan of tileHist. Records are taken 64 at a time in input order; within
// a step the lanes with the same digit find each other with eight ballots, and their places follow the lane order.
template <class Q>
__device__ __forceinline__ void tableScatterBody(const uint32_t* __restrict__ keysIn, const Q* __restrict__ payIn, uint32_t* __restrict__ keysOut, Q* __restrict__ payOut, unsigned long long n, int p,
                                                 const Q* __restrict__ tileOff, uint32_t nTiles)
{
    __shared__ Q run[256];
    const int lane = threadIdx.x;
    const unsigned long long below = (1ull << lane) - 1;
    for (int i = lane; i < 256; i += 64) run[i] = tileOff[(unsigned long long)i * nTiles + blockIdx.x];
    T_WAVE_SYNC();
    const unsigned long long t0 = (unsigned long long)blockIdx.x * T_TILE;
    for (int k = 0; k < T_SORT_ITEMS; k++) {
        const unsigned long long i = t0 + (unsigned long long)k * 64 + lane;
        const bool valid = i < n;
        const uint32_t key = valid ? keysIn[i] : 0u;
        const Q pay = valid ? payIn[i] : (Q)0;
        const uint32_t x = tableDigit(key, p);
        unsigned long long peers = __ballot(valid);
        for (int bit = 0; bit < 8; bit++) {
            const bool set = (x >> bit) & 1u;
            const unsigned long long b = __ballot(set);
            peers &= set ? b : ~b;
        }
        const Q base = valid ? run[x] : (Q)0;
        T_WAVE_SYNC();
        if (valid) {
            const unsigned long long at = (unsigned long long)base + (unsigned long long)__popcll(peers & below);
            if (at < n) { keysOut[at] = key; payOut[at] = pay; }       // (always: the offsets are a scan of this tile's own counts)
            if ((peers & below) == 0) run[x] = base + (Q)__popcll(peers);
        }
        T_WAVE_SYNC();
    }
}
__global__ __launch_bounds__(64) void tableScatter32(const uint32_t* keysIn, const uint32_t* payIn, uint32_t* keysOut, uint32_t* payOut, unsigned long long n, int p, const uint32_t* tileOff, uint32_t nTiles)
{
    tableScatterBody(keysIn, payIn, keysOut, payOut, n, p, tileOff, nTiles);
}
__global__ __launch_bounds__(64) void tableScatter64(const uint32_t* keysIn, const unsigned long long* payIn, uint32_t* keysOut, unsigned long long* payOut, unsigned long long n, int p,
                                                     const unsigned long long* tileOff, uint32_t nTiles)
{
    tableScatterBody(keysIn, payIn, keysOut, payOut, n, p, tileOff, nTiles);
}

// ---- occRec[j] = {g in its segment, chrWord, posPos[q], posId[q]} for the position q = pay[j] of CSR slot j.
template <class Q>
__device__ __forceinline__ void tableGatherBody(const TablePlan& pl, const Q* __restrict__ pay, const uint32_t* __restrict__ posPos, const int32_t* __restrict__ posId, uint4* __restrict__ occRec, unsigned long long P)
{
    const unsigned long long j = (unsigned long long)blockIdx.x * T_T + threadIdx.x;
    if (j >= P) return;
    const unsigned long long q = pay[j];
    if (q >= P) return;                                                // (never: the payloads are a permutation of [0, P))
    const uint32_t c = tableChrOf(pl, q);
    const uint32_t cw = pl.chrWord[c];
    const unsigned long long at = pl.chrDev[c] + (q - pl.chrStart[c]);
    occRec[j] = uint4{(uint32_t)(at - pl.segBase[cw >> LCB_SEG_SHIFT]), cw, posPos[at], (uint32_t)posId[at]};
}
__global__ __launch_bounds__(T_T) void tableGather32(const TablePlan pl, const uint32_t* pay, const uint32_t* posPos, const int32_t* posId, uint4* occRec, unsigned long long P) { tableGatherBody(pl, pay, posPos, posId, occRec, P); }
__global__ __launch_bounds__(T_T) void tableGather64(const TablePlan pl, const unsigned long long* pay, const uint32_t* posPos, const int32_t* posId, uint4* occRec, unsigned long long P) { tableGatherBody(pl, pay, posPos, posId, occRec, P); }

}  // namespace lcb_tablek
#endif
