// junction_plan.cpp — how much device memory phase A of the partitioned junction build needs, and the number of partitions that
// fits a budget. Plain arithmetic: lcb_junctions_plan answers from it without a device, junctions.hip plans with it.
#include <string>

#include "lcb_host.h"

uint64_t lcb_junction_table_bytes(uint32_t log2) { return (1ull << log2) * 12; }

uint32_t lcb_junction_default_log2(uint64_t windows, uint32_t partitions)
{
    uint32_t log2 = 20;
    while (log2 < 40 && (1ull << log2) < windows / (2ull * partitions)) log2++;
    return log2;
}

uint64_t lcb_junction_phase_a_bytes(uint64_t windows, uint64_t seqBytes, uint32_t tableLog2, uint32_t partitions)
{
    const uint32_t log2 = tableLog2 ? tableLog2 : lcb_junction_default_log2(windows, partitions);
    return seqBytes + 8 * ((seqBytes + 63) / 64) + lcb_junction_table_bytes(log2) + LCB_JUNCTION_STATE_BYTES;
}

void lcb_junctions_plan_impl(int64_t windows, int64_t seqBytes, const lcb_junction_opts_ex* opts, uint64_t budget, int32_t* partitions, uint64_t* need)
{
    if (windows < 0 || seqBytes < 0) throw LcbError("lcb_junctions_plan: windows and seq_bytes must not be negative");
    const uint32_t log2 = opts ? opts->table_log2 : 0, fixed = opts ? opts->partitions : 0;
    uint32_t P = fixed ? fixed : 1;
    uint64_t n = lcb_junction_phase_a_bytes((uint64_t)windows, (uint64_t)seqBytes, log2, P);
    if (!fixed) {
        while (n > budget && P < 64) n = lcb_junction_phase_a_bytes((uint64_t)windows, (uint64_t)seqBytes, log2, ++P);
        if (n > budget)
            throw LcbError("lcb_junctions_plan: with 64 partitions the build still needs " + std::to_string(n) + " bytes of device memory, the budget is " +
                           std::to_string(budget) + " (the sequence alone takes " + std::to_string(seqBytes) + ")");
    }
    if (partitions) *partitions = (int32_t)P;
    if (need) *need = n;
}
