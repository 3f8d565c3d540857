// lcb_junction_kernels.h — device code of the GPU junction finder (host driver: junctions.hip). Kept in a header of its
// own so that the wavefront emulator of tests/emu can compile and run the same kernels on the CPU (tests/test_junctions_emu.py,
// tests/test_junction_partitions_emu.py). The table is probed in two places (jFind, jClaim); the single-table and the partitioned
// build share one insert body (jInsertBody<J_ALL | J_PART | J_MARKED>), one classify body (jClassifyBody<marked>) and the
// four tile kernels behind it; junctionMarkPart belongs to the partitioned build alone.
#ifndef LCB_JUNCTION_KERNELS_H
#define LCB_JUNCTION_KERNELS_H

#include <hip/hip_runtime.h>

#include <stdint.h>

namespace lcb_junction {

constexpr int JT = 256;                       // lanes of a workgroup
constexpr int J_RUN = 8;                      // windows per lane of the insert and classify kernels
constexpr int J_WPB = JT * J_RUN;             // windows per workgroup of those
constexpr uint32_t V_ID = 0x80000000u;        // value word: the slot's junction id is in the low 31 bits (as in the CPU tool)
constexpr uint32_t V_PEND = 0x40000000u;      // value word: junction without id, low 30 bits = 2^30 - 1 - smallest tile index seen
constexpr uint32_t V_IDX = 0x3FFFFFFFu;
constexpr uint64_t W_NONE = ~0ull;            // per-window word of a tile: not a junction
constexpr uint64_t W_FWD = 1ull << 63;        // ... the occurrence spells the canonical form
constexpr uint64_t W_FIRST = 1ull << 62;      // ... first occurrence of a slot that had no id
constexpr uint64_t W_SLOT = W_FIRST - 1;

struct JState {
    unsigned long long used;        // claimed slots (added once per workgroup)
    unsigned long long idNext;      // ids given so far
    unsigned long long tileIdBase;  // ... before the current tile
    unsigned long long totJ, totF;  // junction windows / first occurrences of the current tile
    uint32_t full;                  // the table is too full: nobody inserts any more, the host starts over with twice the slots
    uint32_t lost;                  // a lookup missed (cannot happen after a complete insertion; reported, not ignored)
};

struct JRecord { unsigned long long g; long long id; };

__host__ __device__ __forceinline__ uint64_t jMix(uint64_t x)
{
    x ^= x >> 33; x *= 0xff51afd7ed558ccdull; x ^= x >> 33; x *= 0xc4ceb9fe1a85ec53ull; x ^= x >> 33;
    return x;
}

// The partition of a canonical k-mer when the table is built in P passes (1..J_MAX_PARTS), one part of the k-mer space per pass: bits
// 40..63 of the hash. A slot index uses bits below 40 (mask < 2^40), so the k-mers of one partition still spread over all its slots.
constexpr int J_MAX_PARTS = 64;
__host__ __device__ __forceinline__ uint32_t jPartition(uint64_t kmer, uint32_t P)
{
    return (uint32_t)(jMix(kmer) >> 40) % P;
}

__device__ __forceinline__ bool jIsJunction(uint32_t v)
{
    return (v & 0x100) || __popc(v & 0xF) >= 2 || __popc((v >> 4) & 0xF) >= 2;
}

// The codes of positions [b0 - 1, b0 + J_WPB + k] -> LDS; out of the array = breaker.
__device__ __forceinline__ void jLoadCodes(uint8_t* s, const uint8_t* __restrict__ codes, uint64_t len, uint64_t b0, int k)
{
    const int n = J_WPB + k + 1;
    for (int i = threadIdx.x; i < n; i += JT) {
        const uint64_t g = b0 + (uint64_t)i;     // position g - 1
        s[i] = (g >= 1 && g - 1 < len) ? codes[g - 1] : (uint8_t)4;
    }
}

// s[0] is the code in front of the window. false: the window holds a breaker.
__device__ __forceinline__ bool jWindow(const uint8_t* s, int k, uint64_t& kmer, bool& isFwd, uint32_t& bits)
{
    uint64_t fwd = 0, rc = 0;
    uint32_t bad = 0;
    const int sh = 2 * (k - 1);
    for (int i = 1; i <= k; i++) {
        const uint32_t c = s[i];
        bad |= c;
        fwd = (fwd << 2) | (uint64_t)(c & 3);
        rc = (rc >> 2) | ((uint64_t)(3 - (c & 3)) << sh);
    }
    if (bad & 4) return false;
    const uint32_t pv = s[0], nx = s[k + 1];
    bits = (pv > 3 || nx > 3) ? 0x100u : 0u;
    isFwd = fwd < rc;
    if (isFwd) {
        if (nx <= 3) bits |= 1u << nx;
        if (pv <= 3) bits |= 1u << (4 + pv);
        kmer = fwd;
    } else {
        if (pv <= 3) bits |= 1u << (3 - pv);
        if (nx <= 3) bits |= 1u << (4 + 3 - nx);
        kmer = rc;
    }
    return true;
}

// Exclusive scan over the workgroup; every lane calls it.
template <int NT>
__device__ __forceinline__ uint32_t jBlockExScan(uint32_t v, uint32_t& total)
{
    __shared__ uint32_t ws[NT / 64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    uint32_t inc = v;
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t o = __shfl_up(inc, d);
        if (lane >= d) inc += o;
    }
    if (lane == 63) ws[w] = inc;
    __syncthreads();
    uint32_t base = 0, tot = 0;
    for (int q = 0; q < NT / 64; q++) {
        const uint32_t x = ws[q];
        if (q < w) base += x;
        tot += x;
    }
    __syncthreads();
    total = tot;
    return base + inc - v;
}

// ---- the two probe loops: linear from jMix(kmer) & mask, key = kmer + 1 (0 = empty). Find only, after a complete insertion (the
// launches in front have ended, so plain loads see every key). true: key[h] holds the k-mer.
__device__ __forceinline__ bool jFind(const unsigned long long* __restrict__ key, uint64_t mask, uint64_t kmer, uint64_t& h)
{
    const unsigned long long want = kmer + 1;
    h = jMix(kmer) & mask;
    bool found = false;
    for (uint64_t probes = 0; probes <= mask; probes++, h = (h + 1) & mask) {
        const unsigned long long cur = key[h];
        if (cur == want) { found = true; break; }
        if (cur == 0) break;
    }
    return found;
}

// Claim or find, and OR `bits` into the slot's mask. A plain load first, the atomic only if it would change something: most occurrences
// repeat what the slot already says. A plain load may be stale (the L2s of the XCDs are not coherent): an empty key that is no longer
// empty is settled by the compare-and-swap's return value, missing mask bits cost one atomicOr that changes nothing. No lane waits for
// another. `claimed` counts the slots this lane took. false: no place within the table, or somebody raised st->full (looked at every
// 256 probes) - the table must be given up. (One exit from each loop: with a return inside, the compiler keeps a three-way state.)
__device__ __forceinline__ bool jClaim(unsigned long long* key, uint32_t* val, uint64_t mask, uint64_t kmer, uint32_t bits, uint32_t& claimed, const JState* st)
{
    const unsigned long long want = kmer + 1;
    uint64_t h = jMix(kmer) & mask;
    bool done = false;
    for (uint64_t probes = 0; probes <= mask; probes++, h = (h + 1) & mask) {
        unsigned long long cur = key[h];
        if (cur == 0) {
            cur = atomicCAS(&key[h], 0ull, want);
            if (cur == 0) { claimed++; cur = want; }
        }
        if (cur == want) {
            if ((val[h] & bits) != bits) atomicOr(&val[h], bits);
            done = true;
            break;
        }
        if ((probes & 255) == 255 && __hip_atomic_load(&st->full, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) break;
    }
    return done;
}

__device__ __forceinline__ bool jMarked(const unsigned long long* __restrict__ bitmap, uint64_t g) { return (bitmap[g >> 6] >> (g & 63)) & 1ull; }

// ---- the insert kernels: one body, the windows it takes chosen at compile time (the single-table path pays for no % P and no bitmap load).
//   J_ALL      every window of the input: the single table (junctionInsert)
//   J_PART     the windows with jPartition(kmer, P) == p: the table of one pass of the partitioned build (junctionInsertPart)
//   J_MARKED   the windows with a bit in bitmap[], with 0x100 | the window's bits: the table of junction k-mers (junctionFillMarked) - jIsJunction holds for
//              every key of it; a bit without a window cannot happen and sets `lost`
// bitmap, P and p are read by the selection that needs them only.
// The `full` protocol: nobody starts a window once st->full is up; a lane whose probe gives up raises it; the workgroup adds its claimed
// slots to st->used once and raises it beyond 0.9 of the slots. The host then starts over with twice the slots.
enum JSelect { J_ALL, J_PART, J_MARKED };

template <JSelect SEL>
__device__ __forceinline__ void jInsertBody(const uint8_t* __restrict__ codes, uint64_t len, int k, const unsigned long long* __restrict__ bitmap,
                                            unsigned long long* key, uint32_t* val, uint64_t mask, JState* st, uint32_t P, uint32_t p)
{
    __shared__ uint8_t s[J_WPB + 40];
    __shared__ uint32_t claimed;
    const uint64_t b0 = (uint64_t)blockIdx.x * J_WPB;
    if (threadIdx.x == 0) claimed = 0;
    jLoadCodes(s, codes, len, b0, k);
    __syncthreads();
    uint32_t mine = 0;
    bool stop = __hip_atomic_load(&st->full, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0;
    for (int j = 0; j < J_RUN && !stop; j++) {
        const int w = j * JT + threadIdx.x;
        const uint64_t g = b0 + (uint64_t)w;
        if (g >= len) break;
        if constexpr (SEL == J_MARKED) if (!jMarked(bitmap, g)) continue;
        uint64_t kmer; bool isFwd; uint32_t bits;
        if (!jWindow(s + w, k, kmer, isFwd, bits)) { if constexpr (SEL == J_MARKED) atomicOr(&st->lost, 1u); continue; }
        if constexpr (SEL == J_PART) if (jPartition(kmer, P) != p) continue;
        if constexpr (SEL == J_MARKED) bits |= 0x100u;
        if (!jClaim(key, val, mask, kmer, bits, mine, st)) { atomicOr(&st->full, 1u); stop = true; }
    }
    if (mine) atomicAdd(&claimed, mine);
    __syncthreads();
    if (threadIdx.x == 0 && claimed) {
        const unsigned long long u = atomicAdd(&st->used, (unsigned long long)claimed) + claimed;
        if (u * 10 > (mask + 1) * 9) atomicOr(&st->full, 1u);
    }
}

__global__ __launch_bounds__(JT) void junctionInsert(const uint8_t* __restrict__ codes, uint64_t len, int k, unsigned long long* key, uint32_t* val,
                                                     uint64_t mask, JState* st)
{
    jInsertBody<J_ALL>(codes, len, k, nullptr, key, val, mask, st, 1, 0);
}

// ---- the classify kernels: tile [t0, t0 + tileLen): wslot[i] = slot | strand of window t0 + i if its k-mer is a junction, and the
// first-occurrence vote. MARKED (in front of the table of junction k-mers, bitmap[] as above): a window without a bit is W_NONE
// without a probe, every key is a junction (its value carries 0x100), and a bit without a window sets `lost` like a miss.
template <bool MARKED>
__device__ __forceinline__ void jClassifyBody(const uint8_t* __restrict__ codes, uint64_t len, int k, const unsigned long long* __restrict__ bitmap,
                                              const unsigned long long* __restrict__ key, uint32_t* val, uint64_t mask, uint64_t t0, uint32_t tileLen,
                                              unsigned long long* wslot, JState* st)
{
    __shared__ uint8_t s[J_WPB + 40];
    const uint32_t i0 = blockIdx.x * (uint32_t)J_WPB;
    jLoadCodes(s, codes, len, t0 + i0, k);
    __syncthreads();
    for (int j = 0; j < J_RUN; j++) {
        const int w = j * JT + threadIdx.x;
        const uint32_t i = i0 + (uint32_t)w;
        if (i >= tileLen) break;
        unsigned long long out = W_NONE;
        if (!MARKED || jMarked(bitmap, t0 + i)) {
            uint64_t kmer, h; bool isFwd; uint32_t bits;
            const bool window = jWindow(s + w, k, kmer, isFwd, bits);
            if (window && jFind(key, mask, kmer, h)) {
                // (a stale plain load shows an older = smaller value: at worst an atomicMax that changes nothing)
                const uint32_t v = val[h], vote = V_PEND | (V_IDX - i);
                bool junction = true;
                if (v & V_ID) {}
                else if (v & V_PEND) { if (v < vote) atomicMax(&val[h], vote); }
                else if (MARKED || jIsJunction(v)) atomicMax(&val[h], vote);
                else junction = false;
                if (junction) out = h | (isFwd ? W_FWD : 0ull);
            } else if (MARKED || window) atomicOr(&st->lost, 1u);
        }
        wslot[i] = out;
    }
}

__global__ __launch_bounds__(JT) void junctionClassify(const uint8_t* __restrict__ codes, uint64_t len, int k, const unsigned long long* __restrict__ key,
                                                       uint32_t* val, uint64_t mask, uint64_t t0, uint32_t tileLen, unsigned long long* wslot, JState* st)
{
    jClassifyBody<false>(codes, len, k, nullptr, key, val, mask, t0, tileLen, wslot, st);
}

// One window per lane from here on: workgroup b holds windows [256 b, 256 b + 256) of the tile, so scans over workgroups are in file order.
__global__ __launch_bounds__(JT) void junctionMarkFirst(unsigned long long* wslot, const uint32_t* __restrict__ val, uint32_t tileLen, uint32_t* cntJ, uint32_t* cntF)
{
    const uint32_t i = blockIdx.x * (uint32_t)JT + threadIdx.x;
    bool j = false, f = false;
    if (i < tileLen) {
        const unsigned long long w = wslot[i];
        if (w != W_NONE) {
            j = true;
            const uint32_t v = val[w & W_SLOT];
            if (!(v & V_ID) && (V_IDX - (v & V_IDX)) == i) { f = true; wslot[i] = w | W_FIRST; }
        }
    }
    const int cj = __syncthreads_count(j), cf = __syncthreads_count(f);
    if (threadIdx.x == 0) { cntJ[blockIdx.x] = (uint32_t)cj; cntF[blockIdx.x] = (uint32_t)cf; }
}

// Counts per workgroup -> exclusive offsets (in place), the tile's totals, and the id base of the tile. One workgroup.
__global__ __launch_bounds__(1024) void junctionScan(uint32_t* cntJ, uint32_t* cntF, uint32_t nb, JState* st)
{
    const uint32_t per = (nb + 1023) / 1024;
    const uint32_t lo = min(nb, threadIdx.x * per), hi = min(nb, lo + per);
    uint32_t sj = 0, sf = 0;
    for (uint32_t q = lo; q < hi; q++) { sj += cntJ[q]; sf += cntF[q]; }
    uint32_t totJ, totF;
    uint32_t ej = jBlockExScan<1024>(sj, totJ);
    uint32_t ef = jBlockExScan<1024>(sf, totF);
    for (uint32_t q = lo; q < hi; q++) {
        const uint32_t a = cntJ[q], b = cntF[q];
        cntJ[q] = ej; cntF[q] = ef;
        ej += a; ef += b;
    }
    if (threadIdx.x == 0) {
        st->totJ = totJ; st->totF = totF;
        st->tileIdBase = st->idNext;
        st->idNext += totF;
    }
}

__global__ __launch_bounds__(JT) void junctionAssignIds(const unsigned long long* __restrict__ wslot, uint32_t* val, uint32_t tileLen, const uint32_t* __restrict__ offF,
                                                        const JState* __restrict__ st)
{
    const uint32_t i = blockIdx.x * (uint32_t)JT + threadIdx.x;
    unsigned long long w = W_NONE;
    if (i < tileLen) w = wslot[i];
    const bool f = w != W_NONE && (w & W_FIRST);
    uint32_t tot;
    const uint32_t rank = jBlockExScan<JT>(f ? 1u : 0u, tot);
    if (f) val[w & W_SLOT] = V_ID | (uint32_t)(st->tileIdBase + offF[blockIdx.x] + rank + 1);
}

__global__ __launch_bounds__(JT) void junctionEmit(const unsigned long long* __restrict__ wslot, const uint32_t* __restrict__ val, uint32_t tileLen, const uint32_t* __restrict__ offJ,
                                                   uint64_t t0, JRecord* out)
{
    const uint32_t i = blockIdx.x * (uint32_t)JT + threadIdx.x;
    unsigned long long w = W_NONE;
    if (i < tileLen) w = wslot[i];
    const bool j = w != W_NONE;
    uint32_t tot;
    const uint32_t rank = jBlockExScan<JT>(j ? 1u : 0u, tot);
    if (j) {
        const long long id = (long long)(val[w & W_SLOT] & 0x7FFFFFFFu);
        out[offJ[blockIdx.x] + rank] = JRecord{t0 + i, (w & W_FWD) ? id : -id};
    }
}
// ---- the partitioned build (DESIGN.md §10 "Partitioned passes"): the table of pass p holds the k-mers with jPartition(kmer, P) == p only.
// All occurrences of a k-mer, on both strands, share the canonical form and so the pass: its masks are complete there. What survives a
// pass is one bit per position of the code array (bit g = window g is a junction occurrence); ids come from a second table that
// holds the junction k-mers alone (junctionFillMarked), through junctionClassifyMarked and the rest of the tile pipeline as it is.

__global__ __launch_bounds__(JT) void junctionInsertPart(const uint8_t* __restrict__ codes, uint64_t len, int k, unsigned long long* key, uint32_t* val,
                                                         uint64_t mask, JState* st, uint32_t P, uint32_t p)
{
    jInsertBody<J_PART>(codes, len, k, nullptr, key, val, mask, st, P, p);
}

// After a complete insertion of partition p: bit g of bitmap[] for every window g of the partition whose k-mer is a junction. Window
// w = j * 256 + lane of a workgroup whose base is a multiple of 2048: the 64 lanes of a wavefront hold, in every iteration, exactly the
// 64 windows of ONE aligned bitmap word, and no other wavefront of the launch has a window of that word. So one lane ORs the ballot in
// with a plain read-modify-write: no atomic, and no bit depends on an arrival order (the passes are launches behind each other on
// one stream). *marked += the bits set; a partition is marked once, so the sum over the passes is the number of junction windows.
__global__ __launch_bounds__(JT) void junctionMarkPart(const uint8_t* __restrict__ codes, uint64_t len, int k, const unsigned long long* __restrict__ key,
                                                       const uint32_t* __restrict__ val, uint64_t mask, uint32_t P, uint32_t p, unsigned long long* bitmap,
                                                       unsigned long long* marked, JState* st)
{
    __shared__ uint8_t s[J_WPB + 40];
    __shared__ uint32_t found;
    const uint64_t b0 = (uint64_t)blockIdx.x * J_WPB;
    if (threadIdx.x == 0) found = 0;
    jLoadCodes(s, codes, len, b0, k);
    __syncthreads();
    uint32_t mine = 0;
    for (int j = 0; j < J_RUN; j++) {               // (no lane leaves the loop early: every lane of a wavefront reaches the ballot)
        const int w = j * JT + threadIdx.x;
        const uint64_t g = b0 + (uint64_t)w;
        bool junction = false;
        uint64_t kmer, h; bool isFwd; uint32_t bits;
        if (g < len && jWindow(s + w, k, kmer, isFwd, bits) && jPartition(kmer, P) == p) {
            if (jFind(key, mask, kmer, h)) junction = jIsJunction(val[h]);
            else atomicOr(&st->lost, 1u);
        }
        const unsigned long long b = __ballot(junction);
        if (b != 0 && (threadIdx.x & 63) == 0) {    // (b != 0: a window of this word lies inside the array, so the word exists)
            bitmap[g >> 6] |= b;
            mine += (uint32_t)__popcll(b);
        }
    }
    if (mine) atomicAdd(&found, mine);
    __syncthreads();
    if (threadIdx.x == 0 && found) atomicAdd(marked, (unsigned long long)found);
}

__global__ __launch_bounds__(JT) void junctionFillMarked(const uint8_t* __restrict__ codes, uint64_t len, int k, const unsigned long long* __restrict__ bitmap,
                                                         unsigned long long* key, uint32_t* val, uint64_t mask, JState* st)
{
    jInsertBody<J_MARKED>(codes, len, k, bitmap, key, val, mask, st, 1, 0);
}

__global__ __launch_bounds__(JT) void junctionClassifyMarked(const uint8_t* __restrict__ codes, uint64_t len, int k, const unsigned long long* __restrict__ bitmap,
                                                             const unsigned long long* __restrict__ key, uint32_t* val, uint64_t mask, uint64_t t0, uint32_t tileLen,
                                                             unsigned long long* wslot, JState* st)
{
    jClassifyBody<true>(codes, len, k, bitmap, key, val, mask, t0, tileLen, wslot, st);
}

}  // namespace lcb_junction
#endif
