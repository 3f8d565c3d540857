// lcb_graph_kernels.h — device code of the graph build on the GPU (host driver: junctions.hip): what graph.cpp computes
// on host threads from a junction file - the abundance of every vertex over the unfiltered records of both strands, the records kept
// by `abundance`, the four per-position arrays and chrStart - from the junction finder's records while they are still in HBM, and
// from the code bytes that are there anyway. Kept in a header of its own so that the wavefront emulator of tests/emu compiles and
// runs the same kernels on the CPU (tests/test_graph_emu.py).
//
//   count      graphCountWindows: the junction windows of the input behind a complete single table (the partitioned build knows the
//              number from its bitmap): the raw arrays are allocated once, with their size known and accounted.
//   take       graphTake, per tile: {g, id} -> raw position in its record (binary search in the record bases) and int32 id, at
//              the tile's place in the raw arrays; the first raw index of every record (atomicMin: order-free).
//   abundance  graphAbundance: counter[|id|]++ over the raw records. Integer additions: the counters do not depend on the order of
//              arrival. The WAVE instantiation adds once for the lanes of a wavefront that hold the same id (two leader rounds).
//   keep       graphKeepCount: per 256 raw records, those with counter[|id|] < abundance; graphScan turns the counts into every
//              workgroup's first kept rank.
//   compact    graphCompact: a scan inside the workgroup gives the kept rank of a record, in raw order (the compaction is stable, no
//              place comes from the return value of an atomic); posId, posPos, posCh, posRevCh are written there, chrStart[c] by
//              the lane that holds record c's first raw index. A next base that is neither ACGT nor the record's end lost its
//              letter to code 4: posCh gets G_PATCH and the host, which has the strings, writes the letter.
//
// Raw and kept indices are 64-bit; a position inside a record and an id are 32-bit, as in the junction file and the graph.
#ifndef LCB_GRAPH_KERNELS_H
#define LCB_GRAPH_KERNELS_H

#include <hip/hip_runtime.h>

#include <stdint.h>

#include "lcb_junction_kernels.h"

namespace lcb_graphk {

using lcb_junction::JRecord;
using lcb_junction::JState;

constexpr int G_T = 256;                           // lanes of a workgroup = raw records per keep-count
constexpr unsigned long long G_NONE = ~0ull;       // first raw index of a record without a junction
constexpr uint8_t G_PATCH = 0xFF;                  // posCh: the host has the letter (no sequence character has this value)
constexpr uint32_t G_LETTERS = 0x54474341u;        // code c -> byte c: "ACGT"
constexpr uint32_t G_COMPLEMENT = 0x41434754u;     // ... "TGCA"

// The largest c in [0, n) with a[c] <= x (a ascends, a[0] <= x).
__device__ __forceinline__ uint32_t graphLastNotAbove(const unsigned long long* __restrict__ a, uint32_t n, unsigned long long x)
{
    uint32_t lo = 0, hi = n;
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (a[mid] <= x) lo = mid; else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ uint32_t graphAbs(int32_t id) { return id < 0 ? 0u - (uint32_t)id : (uint32_t)id; }

// ---- *marked += the windows whose k-mer is a junction, behind a complete insertion into the single table: the sweep of
// junctionMarkPart without the partition test and without the bitmap.
__global__ __launch_bounds__(lcb_junction::JT) void graphCountWindows(const uint8_t* __restrict__ codes, uint64_t len, int k, const unsigned long long* __restrict__ key,
                                                                      const uint32_t* __restrict__ val, uint64_t mask, unsigned long long* marked, JState* st)
{
    using namespace lcb_junction;
    __shared__ uint8_t s[J_WPB + 40];
    __shared__ uint32_t found;
    const uint64_t b0 = (uint64_t)blockIdx.x * J_WPB;
    if (threadIdx.x == 0) found = 0;
    jLoadCodes(s, codes, len, b0, k);
    __syncthreads();
    uint32_t mine = 0;
    for (int j = 0; j < J_RUN; j++) {
        const int w = j * JT + threadIdx.x;
        const uint64_t g = b0 + (uint64_t)w;
        if (g >= len) break;
        uint64_t kmer, h; bool isFwd; uint32_t bits;
        if (!jWindow(s + w, k, kmer, isFwd, bits)) continue;
        if (jFind(key, mask, kmer, h)) mine += jIsJunction(val[h]) ? 1u : 0u;
        else atomicOr(&st->lost, 1u);
    }
    if (mine) atomicAdd(&found, mine);
    __syncthreads();
    if (threadIdx.x == 0 && found) atomicAdd(marked, (unsigned long long)found);
}

// ---- the n records of a tile -> raw records [rawBase, rawBase + n). base[r] = the code position of record r's first base,
// base[nRec] = the length of the code array; recFirst[r] starts as G_NONE.
__global__ __launch_bounds__(G_T) void graphTake(const JRecord* __restrict__ rec, uint32_t n, unsigned long long rawBase, const unsigned long long* __restrict__ base, uint32_t nRec,
                                                 uint32_t* __restrict__ rawPos, int32_t* __restrict__ rawId, unsigned long long* recFirst)
{
    const uint32_t q = blockIdx.x * (uint32_t)G_T + threadIdx.x;
    if (q >= n) return;
    const unsigned long long g = rec[q].g;
    const uint32_t c = graphLastNotAbove(base, nRec, g);
    rawPos[rawBase + q] = (uint32_t)(g - base[c]);
    rawId[rawBase + q] = (int32_t)rec[q].id;
    // the first record of c in this tile; an earlier tile may hold an earlier one, so the minimum decides
    if (q == 0 || rec[q - 1].g < base[c]) atomicMin(&recFirst[c], rawBase + q);
}

// ---- counter[|id|] += 1 for every raw record.
template <bool WAVE>
__device__ __forceinline__ void graphAbundanceBody(const int32_t* __restrict__ rawId, unsigned long long N, uint32_t* counter)
{
    const unsigned long long i = (unsigned long long)blockIdx.x * G_T + threadIdx.x;
    const bool valid = i < N;
    const uint32_t a = valid ? graphAbs(rawId[i]) : 0u;
    if constexpr (WAVE) {
        const int lane = threadIdx.x & 63;
        bool todo = valid;
        for (int round = 0; round < 2; round++) {              // (wave-uniform: m is)
            const unsigned long long m = __ballot(todo);
            if (!m) break;
            const int leader = __ffsll((long long)m) - 1;
            const uint32_t f = (uint32_t)__shfl((int)a, leader);
            const unsigned long long same = __ballot(todo && a == f);
            if (lane == leader) atomicAdd(&counter[f], (uint32_t)__popcll(same));
            if (a == f) todo = false;
        }
        if (todo) atomicAdd(&counter[a], 1u);
    } else if (valid) atomicAdd(&counter[a], 1u);
}
__global__ __launch_bounds__(G_T) void graphAbundance(const int32_t* rawId, unsigned long long N, uint32_t* counter) { graphAbundanceBody<false>(rawId, N, counter); }
__global__ __launch_bounds__(G_T) void graphAbundanceWave(const int32_t* rawId, unsigned long long N, uint32_t* counter) { graphAbundanceBody<true>(rawId, N, counter); }

__device__ __forceinline__ bool graphKept(const int32_t* __restrict__ rawId, const uint32_t* __restrict__ counter, uint32_t abundance, unsigned long long i)
{
    return counter[graphAbs(rawId[i])] < abundance;      // junctionstorage.h:597-617: abundance < threshold
}

// ---- blockKept[b] = the kept ones of raw records [256 b, 256 b + 256).
__global__ __launch_bounds__(G_T) void graphKeepCount(const int32_t* __restrict__ rawId, unsigned long long N, const uint32_t* __restrict__ counter, uint32_t abundance,
                                                      unsigned long long* blockKept)
{
    const unsigned long long i = (unsigned long long)blockIdx.x * G_T + threadIdx.x;
    const bool keep = i < N && graphKept(rawId, counter, abundance, i);
    const int c = __syncthreads_count(keep);
    if (threadIdx.x == 0) blockKept[blockIdx.x] = (unsigned long long)c;
}

// ---- exclusive scan of a[0..n) in place, *total = the sum: tableScan64 of lcb_table_kernels.h (one workgroup of G_SCAN_T lanes, pieces
// of 4 * G_SCAN_T entries, four consecutive entries per lane, a shuffle scan inside each wavefront, the wavefronts' sums through LDS).
constexpr int G_SCAN_T = 1024;
__global__ __launch_bounds__(G_SCAN_T) void graphScan(unsigned long long* a, unsigned long long n, unsigned long long* total)
{
    typedef unsigned long long Q;
    __shared__ Q ws[G_SCAN_T / 64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    Q carry = 0;
    for (unsigned long long p0 = 0; p0 < n; p0 += 4ull * G_SCAN_T) {            // (uniform: every lane of the workgroup takes every turn)
        const unsigned long long i = p0 + 4ull * threadIdx.x;
        Q v[4];
        for (int j = 0; j < 4; j++) v[j] = i + j < n ? a[i + j] : (Q)0;
        const Q sum = v[0] + v[1] + v[2] + v[3];
        Q inc = sum;
        for (int d = 1; d < 64; d <<= 1) {
            const Q o = (Q)__shfl_up(inc, d);
            if (lane >= d) inc += o;
        }
        if (lane == 63) ws[w] = inc;
        __syncthreads();
        Q before = 0, tot = 0;
        for (int j = 0; j < G_SCAN_T / 64; j++) {
            const Q x = ws[j];
            if (j < w) before += x;
            tot += x;
        }
        __syncthreads();
        Q run = carry + before + inc - sum;
        for (int j = 0; j < 4; j++) if (i + j < n) { a[i + j] = run; run += v[j]; }
        carry += tot;
    }
    if (threadIdx.x == 0) *total = carry;
}

// ---- blockOff = the exclusive scan of blockKept. Every record has a junction here (the host has refused anything else), so recFirst
// ascends strictly from 0 and the record of raw index i is the last one whose first index is not above i.
__global__ __launch_bounds__(G_T) void graphCompact(const uint32_t* __restrict__ rawPos, const int32_t* __restrict__ rawId, unsigned long long N, const uint32_t* __restrict__ counter,
                                                    uint32_t abundance, const unsigned long long* __restrict__ blockOff, const uint8_t* __restrict__ codes,
                                                    const unsigned long long* __restrict__ base, const unsigned long long* __restrict__ recFirst, uint32_t nRec, int k,
                                                    int32_t* __restrict__ posId, uint32_t* __restrict__ posPos, uint8_t* __restrict__ posCh, uint8_t* __restrict__ posRevCh,
                                                    unsigned long long* chrStart, unsigned long long* patched)
{
    const unsigned long long i = (unsigned long long)blockIdx.x * G_T + threadIdx.x;
    const bool valid = i < N;
    const bool keep = valid && graphKept(rawId, counter, abundance, i);
    uint32_t tot;
    const uint32_t rank = lcb_junction::jBlockExScan<G_T>(keep ? 1u : 0u, tot);
    const unsigned long long at = blockOff[blockIdx.x] + rank;
    bool patch = false;
    if (valid) {
        const uint32_t c = graphLastNotAbove(recFirst, nRec, i);
        if (recFirst[c] == i) chrStart[c] = at;
        if (keep) {
            const unsigned long long pos = rawPos[i], g = base[c] + pos, recLen = base[c + 1] - base[c] - 1;
            uint32_t ch = 0, rev = 'N';
            if (pos + (unsigned long long)k < recLen) {                               // graph.cpp: seq[pos + k], the terminator at the end
                const uint32_t code = codes[g + (unsigned long long)k];
                ch = code <= 3 ? (G_LETTERS >> (8 * code)) & 255u : (uint32_t)G_PATCH;
                patch = code > 3;
            }
            if (pos > 0) {                                                            // graph.cpp: reverseChar(seq[pos - 1])
                const uint32_t code = codes[g - 1];
                if (code <= 3) rev = (G_COMPLEMENT >> (8 * code)) & 255u;
            }
            posId[at] = rawId[i];
            posPos[at] = (uint32_t)pos;
            posCh[at] = (uint8_t)ch;
            posRevCh[at] = (uint8_t)rev;
        }
    }
    const unsigned long long pm = __ballot(patch);
    if (pm && (threadIdx.x & 63) == 0) atomicAdd(patched, (unsigned long long)__popcll(pm));
}

}  // namespace lcb_graphk
#endif
