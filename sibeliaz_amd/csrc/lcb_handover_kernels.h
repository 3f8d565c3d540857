// lcb_handover_kernels.h — device code of the hand-over route (lcb_open_fasta; host drivers: junctions.hip, device.hip, tables.hip;
// DESIGN.md §14): the graph build leaves the four per-position arrays in HBM, the device under creation takes them as its tables, and
// the two things the host used to compute in between are made here, behind the table kernels of lcb_table_kernels.h:
//
//   handPatch     the letters the code bytes do not have (the graph build's sentinel 0xFF in posCh): the host finds them in its
//                 downloaded copy and sends (q, letter) pairs; one lane per pair writes posCh at the device index of host position q.
//   handOccChr    occChr of the host CSR: CSR slot j -> the chromosome of the sorted payload pay[j] (the dense host position q, which is
//                 occG[j] itself), by the binary search of the table kernels (tableChrOf: never an emptied chromosome).
//
// Both walk dense HOST positions and reach the device tables through the TablePlan, like every table kernel: the test gaps between
// segments are neither read nor written. Kept in a header of its own so that the wavefront emulator of tests/emu compiles and runs the
// same kernels on the CPU (tests/test_handover_emu.py).
#ifndef LCB_HANDOVER_KERNELS_H
#define LCB_HANDOVER_KERNELS_H

#include <hip/hip_runtime.h>

#include <stdint.h>

#include "lcb_table_kernels.h"

namespace lcb_handk {

using lcb_tablek::TablePlan;
using lcb_tablek::tableChrOf;

constexpr int H_T = 256;                      // lanes of a workgroup: one item per lane, consecutive lanes on consecutive items

// ---- posCh[toDev(q[i])] = letter[i] for the n pairs of the patch list. P = the kept positions: a pair beyond them is skipped
// (never: the host found every q in its own copy of the array).
__global__ __launch_bounds__(H_T) void handPatch(const TablePlan pl, const unsigned long long* __restrict__ patchQ, const uint8_t* __restrict__ patchLetter, unsigned long long n,
                                                 unsigned long long P, uint8_t* __restrict__ posCh)
{
    const unsigned long long i = (unsigned long long)blockIdx.x * H_T + threadIdx.x;
    if (i >= n) return;
    const unsigned long long q = patchQ[i];
    if (q >= P) return;
    const uint32_t c = tableChrOf(pl, q);
    posCh[pl.chrDev[c] + (q - pl.chrStart[c])] = patchLetter[i];
}

// ---- occChr[j] = the last chromosome c with chrStart[c] <= pay[j], for the P slots of the CSR.
template <class Q>
__device__ __forceinline__ void handOccChrBody(const TablePlan& pl, const Q* __restrict__ pay, uint32_t* __restrict__ occChr, unsigned long long P)
{
    const unsigned long long j = (unsigned long long)blockIdx.x * H_T + threadIdx.x;
    if (j >= P) return;
    const unsigned long long q = pay[j];
    occChr[j] = q < P ? tableChrOf(pl, q) : 0u;                        // (always q < P: the payloads are a permutation of [0, P))
}
__global__ __launch_bounds__(H_T) void handOccChr32(const TablePlan pl, const uint32_t* pay, uint32_t* occChr, unsigned long long P) { handOccChrBody(pl, pay, occChr, P); }
__global__ __launch_bounds__(H_T) void handOccChr64(const TablePlan pl, const unsigned long long* pay, uint32_t* occChr, unsigned long long P) { handOccChrBody(pl, pay, occChr, P); }

}  // namespace lcb_handk
#endif
