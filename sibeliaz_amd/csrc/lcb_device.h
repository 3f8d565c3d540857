// lcb_device.h — one MI355X: tables + `used` bitmap resident in HBM, per-wavefront workspaces,
// kernel launches (device.hip).
#ifndef LCB_DEVICE_H
#define LCB_DEVICE_H

#include <cstdint>
#include <string>
#include <utility>
#include <vector>

#include "lcb_host.h"

struct lcb_device_impl;

struct lcb_device {
    lcb_device_impl* impl;
};

lcb_device* lcb_device_create_impl(const lcb_graph* g, const lcb_params* p, int ordinal, const lcb_device_opts* opts = nullptr);
void lcb_device_destroy_impl(lcb_device* d);
void lcb_device_reset_used_impl(lcb_device* d);
void lcb_device_mark_used_impl(lcb_device* d, const uint64_t* ranges, int64_t n);
void lcb_device_set_used_impl(lcb_device* d, const uint32_t* words, int64_t nWords);
void lcb_device_set_stats_impl(lcb_device* d, bool on);
// Processes seeds[0..n): fills offsets[n+1] and inst (resized), bestScore (optional, n entries), ctr (optional, accumulated).
void lcb_device_process_impl(lcb_device* d, const lcb_seed* seeds, int64_t n, std::vector<uint64_t>& offsets,
                             std::vector<lcb_instance>& inst, int64_t* bestScore, lcb_counters* ctr,
                             std::vector<uint64_t>* fpOffsets = nullptr, std::vector<lcb_fp>* fp = nullptr,
                             const uint32_t* view = nullptr,    // view[i]: `used` view of seed i (null = the live state)
                             std::vector<lcb_counters>* perSeedCtr = nullptr);   // stats mode: the counters of every seed
// The same for a call whose first launch overlaps with host work: begin enqueues it against the live state of this moment (false:
// not applicable, use the synchronous call), end waits and completes it.
bool lcb_device_process_begin_impl(lcb_device* d, const lcb_seed* seeds, int64_t n);
void lcb_device_process_end_impl(lcb_device* d, std::vector<uint64_t>& offsets, std::vector<lcb_instance>& inst, std::vector<uint64_t>& fpOffsets,
                                 std::vector<lcb_fp>& fp);
// Predicted `used` views 1..nViews = live state + the marks with firstView <= v (engine.cpp).
void lcb_device_build_views_impl(lcb_device* d, int nViews, const LcbViewMark* marks, int64_t nMarks);
int lcb_device_max_views_impl(lcb_device* d);
// asynchronous job batches (LcbProcessor::side*, lcb_host.h)
int lcb_device_side_lanes_impl(lcb_device* d);
int lcb_device_side_begin_impl(lcb_device* d, const lcb_seed* seeds, const uint32_t* view, int64_t n, int nViews, const LcbViewMark* marks, int64_t nMarks);
int lcb_device_side_poll_impl(lcb_device* d, int lane, int64_t k, bool wait, std::vector<lcb_instance>& inst, std::vector<lcb_fp>& fp);
void lcb_device_side_release_impl(lcb_device* d, int lane);
double lcb_device_hbm_triad_impl(lcb_device* d, uint64_t bytes, int reps);
int lcb_device_concurrency_impl(lcb_device* d);          // seeds in flight in the compact variant
void lcb_device_mode_seeds_impl(lcb_device* d, int64_t out[4]);
void lcb_device_overflows_impl(lcb_device* d, int64_t counts[16], int64_t info[5]);
void lcb_device_mode_time_impl(lcb_device* d, double ms[4], int64_t launches[4]);
// since the last call: sum of the hipEvent-timed kernel durations over all streams, launches, union of the kernels' intervals (the time
// the GPU was busy with them: side-lane kernels overlap the synchronous ones), and the part of the sum that ran on the side lanes
void lcb_device_kernel_time_impl(lcb_device* d, double* ms, int64_t* launches, double* busyMs = nullptr, double* sideMs = nullptr);
int64_t lcb_device_big_retries_impl(lcb_device* d);
void lcb_find_blocks_impl(const lcb_graph* g, lcb_device* d, const lcb_params* p, const lcb_seed* seeds, int64_t nSeeds,
                          const LcbEngineConfig& cfg, std::vector<lcb_block>& blocks, lcb_stats* stats);

// seeds.hip — seed enumeration and ordering on the device's own tables
struct LcbSeedView {                 // what the enumeration reads of a device (device pointers) and the stream it runs on (a hipStream_t)
    int ordinal;
    void* stream;
    const uint32_t* occStart32;
    const uint64_t* occStart64;
    const void* occRec;
    const uint8_t *posCh, *posRevCh;
    const uint64_t* segBase;
    uint32_t nVertex;
};
LcbSeedView lcb_device_seed_view_impl(lcb_device* d, const char* fn);     // (device.hip) fn: the caller, for the messages
int64_t lcb_device_enumerate_seeds_impl(lcb_device* d, lcb_seed** out, lcb_seed_stats* stats);
void lcb_device_sort_seeds_impl(lcb_device* d, lcb_seed* seeds, int64_t n);

// tables.hip — the device route of device creation (LCB_TABLES_DEVICE): posWin, occStart and occRec computed on the GPU from the
// per-position arrays that device.hip has uploaded
struct LcbSegPlan;
struct LcbTableJob {                 // what the build reads of a device that is being created, and where its results go (device pointers)
    const char* fn;                  // the caller, for the messages
    void* stream;                    // a hipStream_t
    const lcb_graph* g;              // (sizes and chrStart only: no per-position array of the host is read)
    const LcbSegPlan* plan;
    bool seg;                        // the 64-bit instantiation (occStart64, u64 payloads)
    uint32_t maxBranch;
    const int32_t* posId;
    const uint32_t* posPos;
    const uint64_t* segBase;
    uint32_t* posWin;                // [plan->devPositions], written at the positions only
    void* occStart;                  // [nVertex + 1] uint32_t, or uint64_t if seg
    const void* occRec = nullptr;    // OUT: [P] uint4, made by the build through alloc once the sort's second buffers are gone
    void* (*alloc)(void* owner, size_t bytes);     // devAlloc / drop of the device that is being created
    void (*drop)(void* owner, void* p);
    void* owner;
    struct LcbTableHandover* hand = nullptr;       // the hand-over route only (below)
};
// What the table build does on top on the hand-over route (lcb_open_fasta): the patch list goes up and handPatch writes
// the device's posCh before anything reads it; once the sort has finished, the host CSR of `g` is taken from the scan (occStart), the
// sorted payloads (occG) and handOccChr (occChr) instead of being computed on host threads.
struct LcbTableHandover {
    lcb_graph* g;                    // occStart / occG / occChr are filled
    uint8_t* posCh;                  // the device's table
    const uint64_t* patchQ;          // [nPatch] host: dense host positions ...
    const uint8_t* patchLetter;      // ... and the letters that belong there
    uint64_t nPatch;
    double patchMs = 0, csrMs = 0;   // OUT: hipEvent-timed patch; wall time of handOccChr + the CSR copies + their widening
    uint64_t csrBytes = 0;           // OUT: device -> host bytes of the CSR
    uint64_t peakBytes = 0;          // OUT: most the build held at one time, occRec and the CSR's occChr included
};
void lcb_tables_need_impl(const char* fn, uint64_t bytes, const std::string& what);   // refuses a request beyond what hipMemGetInfo reports free, with both numbers
void lcb_build_tables_impl(LcbTableJob& job, lcb_table_stats& stats);
lcb_device* lcb_device_create_tables_impl(const lcb_graph* g, const lcb_params* p, int ordinal, const lcb_device_opts* opts, int tables, lcb_table_stats* stats);
void lcb_device_table_read_impl(lcb_device* d, int table, uint64_t first, uint64_t n, void* out, uint64_t outBytes);

// the hand-over route: junctions.hip builds the graph's arrays in HBM and passes them on, device.hip makes them its tables
//
// The four kept per-position arrays on their way from the junction run to the device that is being created. Movable, not copyable:
// one owner at any moment. Whoever holds it when it dies frees what it still holds; the device takes an array out of it (take) in
// the same step that registers it with its LcbOwner. Plain C++ without any HIP call: the maker says how an array is freed.
struct LcbKeptArrays {
    int32_t* posId = nullptr;
    uint32_t* posPos = nullptr;
    uint8_t *posCh = nullptr, *posRevCh = nullptr;
    uint64_t K = 0;                          // kept positions; every array was made for max(1, K) elements
    int (*release)(void*) = nullptr;         // hipFree in junctions.hip
    LcbKeptArrays() = default;
    LcbKeptArrays(const LcbKeptArrays&) = delete;
    LcbKeptArrays& operator=(const LcbKeptArrays&) = delete;
    LcbKeptArrays(LcbKeptArrays&& o) noexcept { *this = std::move(o); }
    LcbKeptArrays& operator=(LcbKeptArrays&& o) noexcept
    {
        if (this != &o) {
            reset();
            posId = o.posId; posPos = o.posPos; posCh = o.posCh; posRevCh = o.posRevCh; K = o.K; release = o.release;
            o.posId = nullptr; o.posPos = nullptr; o.posCh = o.posRevCh = nullptr; o.K = 0;
        }
        return *this;
    }
    ~LcbKeptArrays() { reset(); }
    template <class T>
    static T* take(T*& p) { T* q = p; p = nullptr; return q; }      // the caller owns q from here on
    bool empty() const { return !posId && !posPos && !posCh && !posRevCh; }
    void reset()
    {
        for (void* p : {(void*)take(posId), (void*)take(posPos), (void*)take(posCh), (void*)take(posRevCh)})
            if (p && release) (void)release(p);
    }
};
struct LcbHandover {
    const char* fn;                  // the call the messages name
    LcbKeptArrays kept;
    int threads;
    uint64_t patched;                // characters the compaction marked for the host
    uint64_t junctionPeak;           // peak of the junction run, by its own account
    lcb_open_stats* stats;           // never null
};
// g: nVertex, chrStart, names and sequences are final, the four per-position vectors are sized and not yet filled, no CSR. On return
// the graph is complete. Whatever way the call ends, `ho.kept` holds nothing.
lcb_device* lcb_device_create_handover_impl(lcb_graph* g, const lcb_params* p, int ordinal, const lcb_device_opts* opts, LcbHandover& ho);
void lcb_open_fasta_impl(const std::vector<std::string>& fasta, int k, int abundance, int threads, const lcb_params* p, int ordinal, const lcb_junction_opts_ex& jopts,
                         const lcb_device_opts* dopts, lcb_graph** graph, lcb_device** device, lcb_open_stats* stats);
void lcb_open_junctions_impl(const std::string& file, const std::vector<std::string>& fasta, int k, int abundance, int threads, const lcb_params* p, int ordinal,
                             const lcb_junction_opts_ex& jopts, const lcb_device_opts* dopts, lcb_graph** graph, lcb_device** device, lcb_open_stats* stats);

// comm.hip — RCCL all-gather between the ranks of the round engine
struct lcb_comm;
void lcb_comm_unique_id_impl(unsigned char* id128);
lcb_comm* lcb_comm_create_impl(int ordinal, const unsigned char* id128, int rank, int world);
void lcb_comm_destroy_impl(lcb_comm* c);
void lcb_comm_fill_config(lcb_comm* c, LcbEngineConfig& cfg);
int lcb_device_ordinal_impl(lcb_device* d);
void lcb_find_blocks_gpus_impl(const lcb_graph* g, const int* ordinals, int n, const lcb_params* p, const lcb_device_opts* opts,
                               const lcb_seed* seeds, int64_t nSeeds, LcbEngineConfig cfg, std::vector<lcb_block>& blocks, lcb_stats* stats);

// a persistent set of GPUs of this node driven from one process (one host thread per GPU inside every pass)
struct lcb_gpus_impl;
lcb_gpus_impl* lcb_gpus_create_impl(const lcb_graph* g, const int* ordinals, int n, const lcb_params* p, const lcb_device_opts* opts, bool alwaysComm);
void lcb_gpus_find_blocks_impl(lcb_gpus_impl* m, const lcb_seed* seeds, int64_t nSeeds, LcbEngineConfig cfg, std::vector<lcb_block>& blocks, lcb_stats* stats);
void lcb_gpus_destroy_impl(lcb_gpus_impl* m);
int lcb_gpus_count_impl(const lcb_gpus_impl* m);
lcb_device* lcb_gpus_device_impl(lcb_gpus_impl* m, int i);

#endif
