// lcb_seed_kernels.h — device code of the seed (bundle) enumeration and ordering on the GPU (host driver: seeds.hip).
// What bundles.cpp computes with OpenMP (BlocksFinder::FindBlocks, blocksfinder.h:461-503, and the std::sort at :517), from the tables
// lcb_device_create has put into HBM. Kept in a header of its own so that the wavefront emulator of tests/emu compiles and runs the
// same kernels on the CPU (tests/test_seeds_emu.py).
//
//   enumeration  one wavefront per |v|; a wave owns S_VPW consecutive vertices, so a counting pass (seedEnumerate<false>), a scan over the
//                waves (seedScan) and the writing pass (seedEnumerate<true>) give a deterministic unsorted order in buffers sized by the
//                number of seeds. A list is walked in chunks of 64 occurrences with the per-character state (count, rank, smallest
//                positive occurrence) in LDS; the distinct characters of a chunk are taken one ballot at a time, so neither the list
//                length nor the number of distinct characters is bounded.
//   sort         stable LSD radix sort, 8 bits per pass, over the 19 key bytes of a record: one histogram of all digits up front
//                (seedDigitHist; the host skips the digits on which every key agrees), then per digit seedTileHist -> seedScan -> seedScatter.
//                The 24-byte records move with their keys (the key IS 19 of the 24 bytes).
#ifndef LCB_SEED_KERNELS_H
#define LCB_SEED_KERNELS_H

#include <hip/hip_runtime.h>

#include <stdint.h>

#include "lcb_kernel_limits.h"

namespace lcb_seedk {

constexpr int S_T = 256;                      // lanes of an enumeration workgroup
constexpr int S_WAVES = S_T / 64;
constexpr int S_VPW = 32;                     // consecutive vertices of one wavefront
constexpr int S_SCAN_T = 1024;                // lanes of the scan workgroup
constexpr int S_SORT_ITEMS = 16;              // records per lane of a sort tile
constexpr int S_TILE = 64 * S_SORT_ITEMS;     // records per workgroup (one wavefront) of seedTileHist / seedScatter
constexpr int S_DIGITS = 19;                  // key bytes, least significant first: resolve_chr 3, resolve_pos 4, rank 8, ~count 4
constexpr unsigned long long S_NONE = ~0ull;  // no positive occurrence yet

// Orders the LDS accesses of the lanes of one wavefront: LDS operations of a wavefront execute in issue order, so only the compiler
// has to be kept from moving them (LCB_WAVE_SYNC_LDS of lcb_kernel.h).
#define S_WAVE_SYNC()                                             \
    do {                                                          \
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");    \
        __builtin_amdgcn_wave_barrier();                          \
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");    \
    } while (0)

// A seed on the device. Sorted by (count descending, rank, pos, chr): seedLess of bundles.cpp.
struct SeedRec {
    unsigned long long rank;
    uint32_t count;
    uint32_t pos;         // resolve_pos
    int32_t vid;          // (lcb_device_sort_seeds: the index of the caller's seed)
    uint32_t chrCh;       // resolve_chr << 8 | the character byte
};

struct SeedTables {
    const uint32_t* occStart32;     // one of the two, as in LcbTables
    const uint64_t* occStart64;
    const uint4* occRec;            // {g, cw, Position::pos, Position::id}
    const uint8_t* posCh;
    const uint8_t* posRevCh;
    const uint64_t* segBase;
    uint32_t nVertex;
};

__host__ __device__ __forceinline__ uint32_t seedDigit(const SeedRec& r, int p)
{
    if (p < 3) return (r.chrCh >> (8 + 8 * p)) & 255u;
    if (p < 7) return (r.pos >> (8 * (p - 3))) & 255u;
    if (p < 15) return (uint32_t)(r.rank >> (8 * (p - 7))) & 255u;
    return (~r.count >> (8 * (p - 15))) & 255u;
}

__host__ __device__ __forceinline__ unsigned long long seedPow31(uint32_t i)
{
    unsigned long long r = 1, b = 31;
    for (; i; i >>= 1, b *= b) if (i & 1) r *= b;
    return r;
}

// Exclusive scan of a[0..n) in place, *total = the sum. One workgroup of S_SCAN_T lanes, a run of consecutive entries per lane.
template <class T>
__device__ __forceinline__ void seedScanBody(T* a, unsigned long long n, unsigned long long* total)
{
    __shared__ unsigned long long s[S_SCAN_T];
    const unsigned long long per = (n + S_SCAN_T - 1) / S_SCAN_T;
    const unsigned long long lo = min(n, threadIdx.x * per), hi = min(n, lo + per);
    unsigned long long sum = 0;
    for (unsigned long long q = lo; q < hi; q++) sum += a[q];
    s[threadIdx.x] = sum;
    __syncthreads();
    for (int d = 1; d < S_SCAN_T; d <<= 1) {
        const unsigned long long x = (int)threadIdx.x >= d ? s[threadIdx.x - d] : 0ull;
        __syncthreads();
        s[threadIdx.x] += x;
        __syncthreads();
    }
    unsigned long long run = s[threadIdx.x] - sum;
    for (unsigned long long q = lo; q < hi; q++) { const T v = a[q]; a[q] = (T)run; run += v; }
    if (threadIdx.x == S_SCAN_T - 1) *total = s[S_SCAN_T - 1];
}

__global__ __launch_bounds__(S_SCAN_T) void seedScan64(unsigned long long* a, unsigned long long n, unsigned long long* total) { seedScanBody(a, n, total); }

// The same for the tile histograms of the sort (32-bit entries, millions of them, once per pass): the array is walked in pieces of
// 4 * S_SCAN_T entries, four consecutive entries per lane (coalesced), a shuffle scan inside each wavefront and the wavefronts' sums
// through LDS: two barriers per piece instead of a strided walk per lane. The sum stays below 2^32 (it is the number of seeds).
__global__ __launch_bounds__(S_SCAN_T) void seedScan32(uint32_t* a, unsigned long long n, unsigned long long* total)
{
    __shared__ uint32_t ws[S_SCAN_T / 64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    uint32_t carry = 0;
    for (unsigned long long p0 = 0; p0 < n; p0 += 4ull * S_SCAN_T) {            // (uniform: every lane of the workgroup takes every turn)
        const unsigned long long i = p0 + 4ull * threadIdx.x;
        uint32_t v[4];
        for (int q = 0; q < 4; q++) v[q] = i + q < n ? a[i + q] : 0u;
        const uint32_t sum = v[0] + v[1] + v[2] + v[3];
        uint32_t inc = sum;
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t o = __shfl_up(inc, d);
            if (lane >= d) inc += o;
        }
        if (lane == 63) ws[w] = inc;
        __syncthreads();
        uint32_t base = 0, tot = 0;
        for (int q = 0; q < S_SCAN_T / 64; q++) {
            const uint32_t x = ws[q];
            if (q < w) base += x;
            tot += x;
        }
        __syncthreads();
        uint32_t run = carry + base + inc - sum;
        for (int q = 0; q < 4; q++) if (i + q < n) { a[i + q] = run; run += v[q]; }
        carry += tot;
    }
    if (threadIdx.x == 0) *total = carry;
}

// ---- enumeration. FILL = false: waveCnt[w] = the seeds of wave w's vertices. FILL = true: waveCnt holds the exclusive scan of that,
// the seeds are written to out[waveCnt[w] ...) in (vertex, +v before -v, first appearance of the character) order; a record beyond
// cap (cannot happen: both passes compute the same) is dropped and raises *err.
template <bool FILL>
__device__ __forceinline__ void seedEnumerateBody(const SeedTables T, unsigned long long* waveCnt, SeedRec* out, unsigned long long cap, uint32_t* err)
{
    __shared__ uint32_t sCnt[S_WAVES][256];
    __shared__ unsigned long long sRank[S_WAVES][256];
    __shared__ unsigned long long sRes[S_WAVES][256];      // smallest (pos << 24 | chr) over the positive occurrences
    __shared__ uint8_t sSeen[S_WAVES][256];                // the characters of the list, in order of first appearance
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const unsigned long long below = (1ull << lane) - 1;
    uint32_t* cnt = sCnt[w];
    unsigned long long* rnk = sRank[w];
    unsigned long long* res = sRes[w];
    uint8_t* seen = sSeen[w];
    for (int c = lane; c < 256; c += 64) { cnt[c] = 0; rnk[c] = 0; res[c] = S_NONE; }
    S_WAVE_SYNC();
    const unsigned long long slot = (unsigned long long)blockIdx.x * S_WAVES + w;
    const unsigned long long v0 = slot * S_VPW, v1 = min((unsigned long long)T.nVertex, v0 + S_VPW);
    unsigned long long total = 0;
    const unsigned long long dst0 = (FILL && v0 < v1) ? waveCnt[slot] : 0ull;
    for (unsigned long long av = v0; av < v1; av++) {
        const unsigned long long o0 = T.occStart32 ? T.occStart32[av] : T.occStart64[av];
        const unsigned long long o1 = T.occStart32 ? T.occStart32[av + 1] : T.occStart64[av + 1];
        if (o1 - o0 < 2) continue;                                     // count > 1 needs two occurrences (wave-uniform)
        for (int sg = 0; sg < (av ? 2 : 1); sg++) {                    // v = 0 once, as the host loop does
            const int32_t v = sg ? -(int32_t)av : (int32_t)av;
            uint32_t nSeen = 0;
            for (unsigned long long c0 = o0; c0 < o1; c0 += 64) {
                const unsigned long long j = c0 + lane;
                const bool valid = j < o1;
                uint32_t ch = 0, chr = 0, pos = 0;
                bool positive = false;
                if (valid) {
                    const uint4 r = T.occRec[j];
                    positive = (int32_t)r.w == v;                      // JunctionIterator::IsPositiveStrand
                    const unsigned long long at = T.segBase[r.y >> LCB_SEG_SHIFT] + r.x;
                    ch = positive ? T.posCh[at] : T.posRevCh[at];
                    chr = r.y & LCB_CHR_MASK;
                    pos = r.z;
                }
                unsigned long long todo = __ballot(valid);
                while (todo) {                                         // one distinct character of the chunk per turn
                    const int leader = __ffsll((long long)todo) - 1;
                    const uint32_t c = (uint32_t)__shfl((int)ch, leader);
                    const bool mine = valid && ch == c;
                    const unsigned long long m = __ballot(mine);
                    todo &= ~m;
                    const uint32_t base = cnt[c];                      // occurrences with c in the chunks in front
                    S_WAVE_SYNC();
                    if (mine) {
                        const uint32_t i = base + (uint32_t)__popcll(m & below);       // index among those with c, in CSR order
                        atomicAdd(&rnk[c], (unsigned long long)chr * seedPow31(i));   // size_t wrap-around as in the reference
                        if (positive) atomicMin(&res[c], ((unsigned long long)pos << 24) | chr);
                    }
                    if (lane == leader) {
                        if (base == 0) seen[nSeen & 255u] = (uint8_t)c;
                        cnt[c] = base + (uint32_t)__popcll(m);
                    }
                    if (base == 0) nSeen++;
                    S_WAVE_SYNC();
                }
            }
            for (uint32_t s0 = 0; s0 < nSeen; s0 += 64) {
                const uint32_t s = s0 + lane;
                const bool has = s < nSeen;
                const uint32_t c = has ? seen[s] : 0u;
                const uint32_t n = has ? cnt[c] : 0u;
                const unsigned long long rs = has ? res[c] : S_NONE;
                const bool ok = n > 1 && rs != S_NONE;
                const unsigned long long b = __ballot(ok);
                if (FILL && ok) {
                    const unsigned long long at = dst0 + total + (unsigned long long)__popcll(b & below);
                    if (at < cap) out[at] = SeedRec{rnk[c], n, (uint32_t)(rs >> 24), v, ((uint32_t)(rs & LCB_CHR_MASK) << 8) | c};
                    else atomicOr(err, 1u);
                }
                total += (unsigned long long)__popcll(b);
                if (has) { cnt[c] = 0; rnk[c] = 0; res[c] = S_NONE; }
            }
            S_WAVE_SYNC();
        }
    }
    if (!FILL && lane == 0 && v0 < v1) waveCnt[slot] = total;
}

__global__ __launch_bounds__(S_T) void seedCount(const SeedTables T, unsigned long long* waveCnt) { seedEnumerateBody<false>(T, waveCnt, nullptr, 0, nullptr); }
__global__ __launch_bounds__(S_T) void seedFill(const SeedTables T, unsigned long long* waveOff, SeedRec* out, unsigned long long cap, uint32_t* err)
{
    seedEnumerateBody<true>(T, waveOff, out, cap, err);
}

// ---- sort. hist[p * 256 + x] += the records whose digit p is x, for all digits at once (grid-stride; any grid). A wavefront whose
// records agree on a digit - the high bytes of count, of resolve_chr, often of resolve_pos - adds once, not 64 times to one LDS word.
__global__ __launch_bounds__(S_T) void seedDigitHist(const SeedRec* __restrict__ rec, unsigned long long n, unsigned long long* hist)
{
    __shared__ uint32_t h[S_DIGITS * 256];
    for (int i = threadIdx.x; i < S_DIGITS * 256; i += S_T) h[i] = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const unsigned long long stride = (unsigned long long)gridDim.x * S_T;
    // (base is wave-uniform, so the loop and the ballots inside are too)
    for (unsigned long long base = (unsigned long long)blockIdx.x * S_T + (threadIdx.x & ~63); base < n; base += stride) {
        const bool valid = base + lane < n;
        SeedRec r{0, 0, 0, 0, 0};
        if (valid) r = rec[base + lane];
        const unsigned long long vm = __ballot(valid);
        const int leader = __ffsll((long long)vm) - 1;
        for (int p = 0; p < S_DIGITS; p++) {
            const uint32_t x = seedDigit(r, p);
            const uint32_t f = (uint32_t)__shfl((int)x, leader);
            const unsigned long long same = __ballot(valid && x == f);
            if (same == vm) { if (lane == leader) atomicAdd(&h[p * 256 + f], (uint32_t)__popcll(vm)); }
            else if (valid) atomicAdd(&h[p * 256 + x], 1u);
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < S_DIGITS * 256; i += S_T) if (h[i]) atomicAdd(&hist[i], (unsigned long long)h[i]);
}

// Tile b = records [b * S_TILE, ...): tileHist[x * nTiles + b] = its records with digit p == x (digit-major: an exclusive scan over
// the whole array gives every (digit, tile) its first place in the output). One wavefront per tile.
__global__ __launch_bounds__(64) void seedTileHist(const SeedRec* __restrict__ rec, unsigned long long n, int p, uint32_t* tileHist, uint32_t nTiles)
{
    __shared__ uint32_t h[256];
    const int lane = threadIdx.x;
    for (int i = lane; i < 256; i += 64) h[i] = 0;
    S_WAVE_SYNC();
    const unsigned long long t0 = (unsigned long long)blockIdx.x * S_TILE;
    for (int q = 0; q < S_SORT_ITEMS; q++) {
        const unsigned long long i = t0 + (unsigned long long)q * 64 + lane;
        if (i < n) atomicAdd(&h[seedDigit(rec[i], p)], 1u);
    }
    S_WAVE_SYNC();
    for (int i = lane; i < 256; i += 64) tileHist[(unsigned long long)i * nTiles + blockIdx.x] = h[i];
}

// The stable scatter of one tile: tileOff = the exclusive scan of tileHist. Records are taken 64 at a time in input order; within
// a step the lanes with the same digit find each other with eight ballots, and their places follow the lane order.
__global__ __launch_bounds__(64) void seedScatter(const SeedRec* __restrict__ in, SeedRec* out, unsigned long long n, int p, const uint32_t* __restrict__ tileOff, uint32_t nTiles)
{
    __shared__ uint32_t run[256];
    const int lane = threadIdx.x;
    const unsigned long long below = (1ull << lane) - 1;
    for (int i = lane; i < 256; i += 64) run[i] = tileOff[(unsigned long long)i * nTiles + blockIdx.x];
    S_WAVE_SYNC();
    const unsigned long long t0 = (unsigned long long)blockIdx.x * S_TILE;
    for (int q = 0; q < S_SORT_ITEMS; q++) {
        const unsigned long long i = t0 + (unsigned long long)q * 64 + lane;
        const bool valid = i < n;
        SeedRec r{0, 0, 0, 0, 0};
        if (valid) r = in[i];
        const uint32_t x = seedDigit(r, p);
        unsigned long long peers = __ballot(valid);
        for (int bit = 0; bit < 8; bit++) {
            const bool set = (x >> bit) & 1u;
            const unsigned long long b = __ballot(set);
            peers &= set ? b : ~b;
        }
        const uint32_t base = valid ? run[x] : 0u;
        S_WAVE_SYNC();
        if (valid) {
            const unsigned long long at = (unsigned long long)base + (unsigned long long)__popcll(peers & below);
            if (at < n) out[at] = r;                                   // (always: the offsets are a scan of this tile's own counts)
            if ((peers & below) == 0) run[x] = base + (uint32_t)__popcll(peers);
        }
        S_WAVE_SYNC();
    }
}

}  // namespace lcb_seedk
#endif
