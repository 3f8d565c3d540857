// lcb_file_kernels.h — device code of the front end that opens a junction file on the GPU (host driver: junctions.hip):
// the bytes of the file, resident in HBM as 32-bit words, become what graphTake leaves behind for the junction finder's records - the raw
// positions and ids in file order without the separators, and the first raw index of every run between separators - so that the
// tail of the graph build (lcb_graph_kernels.h: abundance, keep-count, scan, compaction) runs on them unchanged. Two checks the FASTA
// route never needed come with it. Kept in a header of its own so that the wavefront emulator of tests/emu compiles and runs the same
// kernels on the CPU (tests/test_file_emu.py).
//
//   record     12 bytes, little-endian: uint32 pos, int64 id. The file is 4-byte aligned, not 8: a record is read as three words.
//              A separator has pos == 0xFFFFFFFF or id == INT64_MAX (junctionapi.h:93).
//   geometry   the file is cut into TILES of `tile` records (the upload unit), a tile into workgroups of F_T records: workgroup b of
//              the grid is workgroup b % bpt of tile b / bpt, bpt = ceil(tile / F_T). Lanes behind the tile's or the file's end idle.
//   count      fileCount, per tile while the next one is copied: blockSep[b] = the separators of workgroup b; tot[0] += them;
//              tot[1] = max(tot[1], |(int32) id| + 1) over the other records (= nVertex; 0 without a record). Integer additions and
//              maxima: nothing depends on the order of arrival.
//   take       fileTake: graphScan has turned blockSep into every workgroup's separators in front; a scan inside the workgroup adds
//              those of the lanes in front. A record at file index r with s separators in front has raw index r - s and belongs to
//              run s; the lane behind a separator (or at r == 0) writes recFirst[s] (atomicMin: order-free).
//   bounds     fileBounds, before anything reads codes[g + k]: a KEPT record with pos + k beyond its sequence's end raises flag[0].
//   order      fileOrder, behind the compaction: a kept position not above the one in front of it in the same chromosome raises flag[1].
//
// File, raw and kept indices are 64-bit; a position inside a record and an id are 32-bit, as in the graph.
#ifndef LCB_FILE_KERNELS_H
#define LCB_FILE_KERNELS_H

#include <hip/hip_runtime.h>

#include <stdint.h>

#include "lcb_graph_kernels.h"

namespace lcb_filek {

constexpr int F_T = 256;                           // lanes of a workgroup = file records per workgroup

// Record r of the file -> its position and its id cut to 32 bits (junctionstorage.h:129,148); true: a separator.
__device__ __forceinline__ bool fileRecord(const uint32_t* __restrict__ words, unsigned long long r, uint32_t& pos, int32_t& id)
{
    const uint32_t* w = words + 3ull * r;
    pos = w[0];
    const uint32_t lo = w[1], hi = w[2];
    id = (int32_t)lo;
    return pos == 0xFFFFFFFFu || (lo == 0xFFFFFFFFu && hi == 0x7FFFFFFFu);
}

// The file index of this lane in workgroup `wg` of tile `t`; false: the lane lies behind the tile's or the file's end.
__device__ __forceinline__ bool fileIndex(unsigned long long t, uint32_t wg, unsigned long long nRec, uint32_t tile, unsigned long long& r)
{
    const unsigned long long local = (unsigned long long)wg * F_T + threadIdx.x;
    r = t * tile + local;
    return local < tile && r < nRec;
}

// ---- one tile (grid = bpt): blockSep[blockIdx.x] = the separators of the workgroup (blockSep points at the tile's first entry).
__global__ __launch_bounds__(F_T) void fileCount(const uint32_t* __restrict__ words, unsigned long long nRec, uint32_t tile, unsigned long long t,
                                                 unsigned long long* blockSep, unsigned long long* tot)
{
    __shared__ uint32_t most;
    if (threadIdx.x == 0) most = 0;
    unsigned long long r;
    const bool valid = fileIndex(t, blockIdx.x, nRec, tile, r);
    uint32_t pos = 0; int32_t id = 0;
    const bool sep = valid && fileRecord(words, r, pos, id);
    const int c = __syncthreads_count(sep);               // (also orders the store of `most` in front of the maxima)
    if (valid && !sep) atomicMax(&most, lcb_graphk::graphAbs(id) + 1u);
    __syncthreads();
    if (threadIdx.x == 0) {
        blockSep[blockIdx.x] = (unsigned long long)c;
        if (c) atomicAdd(&tot[0], (unsigned long long)c);
        if (most) atomicMax(&tot[1], (unsigned long long)most);
    }
}

// ---- the whole file (grid = tiles * bpt): blockOff = the exclusive scan of blockSep. rawPos / rawId have N entries, recFirst has
// `runs` (= separators + 1) and starts as G_NONE.
__global__ __launch_bounds__(F_T) void fileTake(const uint32_t* __restrict__ words, unsigned long long nRec, uint32_t tile, uint32_t bpt,
                                                const unsigned long long* __restrict__ blockOff, unsigned long long N, unsigned long long runs,
                                                uint32_t* __restrict__ rawPos, int32_t* __restrict__ rawId, unsigned long long* recFirst)
{
    unsigned long long r;
    const bool valid = fileIndex(blockIdx.x / bpt, blockIdx.x % bpt, nRec, tile, r);
    uint32_t pos = 0; int32_t id = 0;
    const bool sep = valid && fileRecord(words, r, pos, id);
    uint32_t tot;
    const uint32_t rank = lcb_junction::jBlockExScan<F_T>(sep ? 1u : 0u, tot);
    if (!valid || sep) return;
    const unsigned long long s = blockOff[blockIdx.x] + rank, i = r - s;
    if (i >= N || s >= runs) return;                      // (cannot happen behind a correct count; never write outside the arrays)
    rawPos[i] = pos;
    rawId[i] = id;
    uint32_t p2; int32_t i2;
    if (r == 0 || fileRecord(words, r - 1, p2, i2)) atomicMin(&recFirst[s], i);
}

// ---- flag[0] = 1 if a kept raw record reaches beyond the end of its sequence (graph.cpp: pos + k > length). recFirst[0..nRec) ascends
// strictly from 0 (the host has refused anything else), base[c + 1] - base[c] - 1 is the length of sequence c.
__global__ __launch_bounds__(F_T) void fileBounds(const uint32_t* __restrict__ rawPos, const int32_t* __restrict__ rawId, unsigned long long N,
                                                  const uint32_t* __restrict__ counter, uint32_t abundance, const unsigned long long* __restrict__ base,
                                                  const unsigned long long* __restrict__ recFirst, uint32_t nRec, int k, unsigned long long* flag)
{
    const unsigned long long i = (unsigned long long)blockIdx.x * F_T + threadIdx.x;
    if (i >= N || !lcb_graphk::graphKept(rawId, counter, abundance, i)) return;
    const uint32_t c = lcb_graphk::graphLastNotAbove(recFirst, nRec, i);
    const unsigned long long recLen = base[c + 1] - base[c] - 1;
    if ((unsigned long long)rawPos[i] + (unsigned long long)k > recLen) atomicMax(&flag[0], 1ull);
}

// ---- flag[1] = 1 if two kept positions behind each other in one chromosome do not ascend strictly. chrStart[0..nChr) as graphCompact
// wrote it: kept index q opens a chromosome iff the last entry not above q equals q (chromosomes without a kept position repeat a value).
__global__ __launch_bounds__(F_T) void fileOrder(const uint32_t* __restrict__ posPos, unsigned long long K, const unsigned long long* __restrict__ chrStart,
                                                 uint32_t nChr, unsigned long long* flag)
{
    const unsigned long long q = (unsigned long long)blockIdx.x * F_T + threadIdx.x;
    if (q == 0 || q >= K || posPos[q] > posPos[q - 1]) return;
    if (chrStart[lcb_graphk::graphLastNotAbove(chrStart, nChr, q)] != q) atomicMax(&flag[1], 1ull);
}

}  // namespace lcb_filek
#endif
