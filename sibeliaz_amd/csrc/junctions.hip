// junctions.hip — the junction finder on one MI355X: what tools/mkgraph.cpp computes on the CPU (and `twopaco` in the reference
// pipeline, sibeliaz:145), byte for byte, with the k-mer table and the sequence resident in HBM. DESIGN.md §10 has the layout, the
// memory formula and the argument why the output does not depend on the order in which atomics arrive.
//
//   sequence   one byte per base (0..3, 4 = anything that breaks a window), all records in file order behind each other with one
//              breaker in front of the first and one after every record: a sequence end is a breaker like any other, so a WINDOW
//              INDEX g is simply a position of this array (64-bit), and the record of a window is found by the host from g.
//   table      open addressing, linear probing: key[] = canonical k-mer + 1 (0 = empty, claimed with a 64-bit atomicCAS),
//              val[] = successor mask | predecessor mask << 4 | forced << 8 (atomicOr) - the CPU tool's bit layout.
//   ids        tiles of consecutive windows, in file order. In a tile every junction window whose slot has no id yet raises the
//              slot's value word to PENDING | (2^30 - 1 - its index in the tile) with an atomicMax: the maximum is the first
//              occurrence, whatever the arrival order. A scan over the first occurrences gives the ids, a scan over the junction
//              windows the places of the records.
//   partitions the table can be built in P passes over the input, one part of the canonical k-mer space per pass (jPartition), when
//              the whole table does not fit: a pass leaves one bit per window in a bitmap, the ids then come from a table of the
//              junction k-mers alone, through the same tile pipeline. One partition = the single-table path above.
//   sinks      the pipeline (junctionPipeline) has two callers. lcb_junctions_build_impl copies a tile's records to the host and writes
//              the junction file; lcb_graph_build_impl keeps them in HBM and makes the graph of them with the kernels of
//              lcb_graph_kernels.h - what lcb_graph_load makes of the file, without the file.
//   file       the tail of that graph build (graphTail: abundance, keep-count, scan, compaction) has a second front half: a junction
//              file read on the device (graphFromFile, kernels in lcb_file_kernels.h) puts the file's records where
//              graphTake puts the junction finder's. No k-mer table, no pipeline: lcb_graph_load with the work on the GPU.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <functional>
#include <memory>
#include <string>
#include <vector>

#include "lcb_device.h"
#include "lcb_fasta.h"
#include "lcb_file_host.h"
#include "lcb_file_kernels.h"
#include "lcb_graph_kernels.h"
#include "lcb_host.h"
#include "lcb_junction_kernels.h"

#define HIP_CHECK(x)                                                                              \
    do {                                                                                          \
        hipError_t e_ = (x);                                                                      \
        if (e_ != hipSuccess) throw LcbError(std::string(#x) + " failed: " + hipGetErrorString(e_)); \
    } while (0)

using namespace lcb_junction;

namespace {

double nowMs() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

uint32_t gridFor(uint64_t items, uint64_t perBlock, const char* fn = "lcb_junctions_build")
{
    const uint64_t n = std::max<uint64_t>(1, (items + perBlock - 1) / perBlock);
    if (n > 0x7FFFFFFFull) throw LcbError(std::string(fn) + ": the input needs more workgroups than one launch has");
    return (uint32_t)n;
}

// Everything the run owns; whatever way it ends, nothing stays behind (device memory, pinned memory, a partial file).
struct Run {
    hipStream_t stream = nullptr;
    hipEvent_t evA = nullptr, evB = nullptr, evCopy[2] = {nullptr, nullptr};
    uint8_t* dCodes = nullptr;
    unsigned long long* dKey = nullptr;
    uint32_t* dVal = nullptr;
    unsigned long long* dBitmap = nullptr;
    unsigned long long* dWslot = nullptr;
    JRecord* dOut = nullptr;
    uint32_t *dCntJ = nullptr, *dCntF = nullptr;
    JState* dState = nullptr;       // LCB_JUNCTION_STATE_BYTES: the JState, and behind it the count of marked windows
    JState* hState = nullptr;       // (pinned, the same block)
    JRecord* hOut[2] = {nullptr, nullptr};
    FILE* f = nullptr;
    std::string part;
    // the graph build (lcb_graph_build_impl) on top of the junction finder's: raw records, counters, the kept arrays; staging for the codes
    uint32_t* dRawPos = nullptr;
    int32_t* dRawId = nullptr;
    unsigned long long *dBase = nullptr, *dRecFirst = nullptr, *dBlockKept = nullptr, *dChrStart = nullptr, *dTotals = nullptr;
    uint32_t* dCounter = nullptr;
    int32_t* dPosId = nullptr;
    uint32_t* dPosPos = nullptr;
    uint8_t *dPosCh = nullptr, *dPosRevCh = nullptr;
    uint8_t* hStage[2] = {nullptr, nullptr};
    // the junction file opened on the device (lcb_graph_load_device_impl): its words, the separators per workgroup, the two flags
    uint32_t* dFile = nullptr;
    unsigned long long *dBlockSep = nullptr, *dFlags = nullptr;
    std::string fn = "lcb_junctions_build";      // the call the messages name
    uint64_t budget = 0, live = 0, peak = 0;     // the run's own account of its device memory
    uint64_t tableBytesKey = 0, tableBytesVal = 0, tileBytes[4] = {0, 0, 0, 0}, bitmapBytes = 0;   // what the pipeline holds when it returns
    ~Run()
    {
        if (stream) (void)hipStreamSynchronize(stream);
        for (void* p : {(void*)dCodes, (void*)dKey, (void*)dVal, (void*)dBitmap, (void*)dWslot, (void*)dOut, (void*)dCntJ, (void*)dCntF, (void*)dState, (void*)dRawPos,
                        (void*)dRawId, (void*)dBase, (void*)dRecFirst, (void*)dBlockKept, (void*)dChrStart, (void*)dTotals, (void*)dCounter, (void*)dPosId, (void*)dPosPos,
                        (void*)dPosCh, (void*)dPosRevCh, (void*)dFile, (void*)dBlockSep, (void*)dFlags})
            if (p) (void)hipFree(p);
        if (hState) (void)hipHostFree(hState);
        for (JRecord* p : hOut) if (p) (void)hipHostFree(p);
        for (uint8_t* p : hStage) if (p) (void)hipHostFree(p);
        for (hipEvent_t e : {evA, evB, evCopy[0], evCopy[1]}) if (e) (void)hipEventDestroy(e);
        if (stream) (void)hipStreamDestroy(stream);
        if (f) fclose(f);
        if (!part.empty()) remove(part.c_str());
    }
    // The stream and the events of the run.
    void start()
    {
        HIP_CHECK(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
        HIP_CHECK(hipEventCreate(&evA));
        HIP_CHECK(hipEventCreate(&evB));
        HIP_CHECK(hipEventCreate(&evCopy[0]));
        HIP_CHECK(hipEventCreate(&evCopy[1]));
    }
    // Would `bytes` more fit? Against the budget by the run's own account, and against what the device reports free.
    bool fits(uint64_t bytes) const
    {
        size_t freeB = 0, totalB = 0;
        return live + bytes <= budget && hipMemGetInfo(&freeB, &totalB) == hipSuccess && bytes <= (uint64_t)freeB;
    }
    template <class T>
    void alloc(T*& p, uint64_t bytes, const char* what)
    {
        size_t freeB = 0, totalB = 0;
        HIP_CHECK(hipMemGetInfo(&freeB, &totalB));
        if (live + bytes > budget || bytes > (uint64_t)freeB)
            throw LcbError(fn + ": " + what + " needs " + std::to_string(bytes) + " bytes of device memory on top of the " + std::to_string(live) +
                           " in use: the budget is " + std::to_string(budget) + ", " + std::to_string((uint64_t)freeB) + " are free");
        HIP_CHECK(hipMalloc((void**)&p, bytes));
        live += bytes;
        peak = std::max(peak, live);
    }
    template <class T>
    void release(T*& p, uint64_t bytes)
    {
        if (!p) return;
        HIP_CHECK(hipFree(p));
        p = nullptr;
        live -= bytes;
    }
    // One timed step: `work` (launches and memsets on the stream) between two events, the state block to the host behind it, `meanwhile`
    // on the host while the device works, and the device time of the step added to a phase.
    template <class W, class H = void (*)()>
    void timed(double& phaseMs, W work, H meanwhile = [] {})
    {
        HIP_CHECK(hipEventRecord(evA, stream));
        work();
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipEventRecord(evB, stream));
        HIP_CHECK(hipMemcpyAsync(hState, dState, LCB_JUNCTION_STATE_BYTES, hipMemcpyDeviceToHost, stream));
        meanwhile();
        HIP_CHECK(hipStreamSynchronize(stream));
        float ms = 0;
        HIP_CHECK(hipEventElapsedTime(&ms, evA, evB));
        phaseMs += ms;
    }
};

// The junction file, written while the device works on the next tile: the records of a tile, with the separators of the sequences
// that end in front of them.
struct Writer {
    Run& R;
    const std::vector<uint64_t>&base, &recLen;
    double& writeMs;
    std::vector<unsigned char> buf;
    size_t curRec = 0;
    void flushBuf()
    {
        if (!buf.empty() && fwrite(buf.data(), 1, buf.size(), R.f) != buf.size()) throw LcbError("cannot write " + R.part);
        buf.clear();
    }
    void put(uint32_t pos, int64_t id)
    {
        const size_t at = buf.size();
        buf.resize(at + 12);
        memcpy(&buf[at], &pos, 4); memcpy(&buf[at + 4], &id, 8);
        if (buf.size() >= (64u << 20)) flushBuf();
    }
    void drain(int slot, uint64_t n)
    {
        HIP_CHECK(hipEventSynchronize(R.evCopy[slot]));
        const double t0 = nowMs();
        const JRecord* o = R.hOut[slot];
        for (uint64_t q = 0; q < n; q++) {
            while (o[q].g >= base[curRec] + recLen[curRec]) { put(0xFFFFFFFFu, INT64_MAX); curRec++; }
            put((uint32_t)(o[q].g - base[curRec]), (int64_t)o[q].id);
        }
        flushBuf();
        writeMs += nowMs() - t0;
    }
};

static_assert(sizeof(JState) + sizeof(unsigned long long) <= LCB_JUNCTION_STATE_BYTES, "the state block holds the JState and the count of marked windows");

void needDevice(const char* fn, const char* cpuWay, int ordinal)
{
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0)
        throw LcbError(std::string("no HIP device available: ") + fn + " runs only on the GPU (there is no CPU fallback; " + cpuWay + ")");
    if (ordinal < 0 || ordinal >= count) throw LcbError("HIP device ordinal out of range");
}

// The input as the pipeline sees it: where the records lie in the code array, and the code bytes when the device has room for them.
struct Source {
    std::vector<uint64_t> base, recLen;      // base[r]: the code position of record r's first base; base[records] = len
    uint64_t len = 1, nWindows = 0;
    std::function<void(Run&)> upload;        // the records' codes -> R.dCodes (which holds a breaker everywhere), on or behind R.stream
    void layout(int k)
    {
        base.resize(recLen.size() + 1);
        len = 1; nWindows = 0;
        for (size_t r = 0; r < recLen.size(); r++) {
            base[r] = len;
            len += recLen[r] + 1;
            if (recLen[r] >= (uint64_t)k) nWindows += recLen[r] - k + 1;
        }
        base[recLen.size()] = len;
    }
};

// Where a tile's records go: the junction file (lcb_junctions_build_impl) or the raw arrays of the graph build (lcb_graph_build_impl).
struct Sink {
    bool countFirst = false;                                              // begin() is told the number of junction windows of the whole input
    std::function<void(uint64_t junctionWindows, uint32_t tileBuf)> begin;// the tables are complete, no tile has run
    std::function<void(int64_t tile)> meanwhile;                          // on the host, while the device works on `tile`
    std::function<void(int64_t tile, uint64_t n, uint64_t before)> tileDone;   // R.dOut holds the tile's n records; `before` = those of the tiles in front
};

// opts.partitions == 1: the single-table path. 0: as many partitions as lcb_junctions_plan finds for the budget. Otherwise that many.
// Insert, classify, ids and emit; what becomes of a tile's records is the sink's. -> the junction k-mers (= the largest id).
uint64_t junctionPipeline(Run& R, const Source& src, int k, int ordinal, const lcb_junction_opts_ex& opts, Sink& sink, lcb_junction_stats_ex& X, double& countMs)
{
    lcb_junction_stats& S = X.base;
    const uint32_t tableLog2 = opts.table_log2;
    uint32_t P = opts.partitions;
    const uint64_t len = src.len, nWindows = src.nWindows;
    const std::string fn = R.fn;
    S.records = (int64_t)src.recLen.size();
    S.windows = (int64_t)nWindows;

    // ---- plan: the budget, the number of partitions, and whether the first phase fits, before anything is allocated
    HIP_CHECK(hipSetDevice(ordinal));
    size_t freeB = 0, totalB = 0;
    HIP_CHECK(hipMemGetInfo(&freeB, &totalB));
    R.budget = opts.mem_budget ? std::min<uint64_t>(opts.mem_budget, freeB) : (uint64_t)freeB;
    const uint32_t tileWindows = opts.tile_windows ? opts.tile_windows : (1u << 22);
    const uint32_t tileBuf = (uint32_t)std::min<uint64_t>(tileWindows, len);
    const uint32_t nbMax = gridFor(tileBuf, JT);
    const uint64_t tileBytes = (uint64_t)tileBuf * (sizeof(unsigned long long) + sizeof(JRecord)) + (uint64_t)nbMax * 8;
    const uint64_t bitmapWords = (len + 63) / 64;
    if (P == 0) {
        lcb_junction_opts_ex o;
        memset(&o, 0, sizeof(o));
        o.table_log2 = tableLog2;
        int32_t planned = 0;
        lcb_junctions_plan_impl((int64_t)nWindows, (int64_t)len, &o, R.budget, &planned, nullptr);
        P = (uint32_t)planned;
    }
    const uint32_t capLog2 = tableLog2 ? tableLog2 : lcb_junction_default_log2(nWindows, P);
    const uint64_t need = P == 1 ? len + tileBytes + LCB_JUNCTION_STATE_BYTES + lcb_junction_table_bytes(capLog2) : lcb_junction_phase_a_bytes(nWindows, len, tableLog2, P);
    if (need > R.budget)
        throw LcbError(fn + ": the input needs " + std::to_string(need) + " bytes of device memory with " + std::to_string(P) + " partition(s), " +
                       std::to_string(R.budget) + " may be used (sequence " + std::to_string(len) + " + 12 bytes per table slot + " +
                       (P == 1 ? "24 bytes per tile window)" : "one bit per base)"));
    X.partitions = P;

    R.start();
    R.alloc(R.dCodes, len, "the sequence");
    R.alloc(R.dState, LCB_JUNCTION_STATE_BYTES, "the state");
    auto allocTiles = [&]() {
        R.alloc(R.dWslot, (uint64_t)tileBuf * sizeof(unsigned long long), "the tile buffers");
        R.alloc(R.dOut, (uint64_t)tileBuf * sizeof(JRecord), "the tile buffers");
        R.alloc(R.dCntJ, (uint64_t)nbMax * sizeof(uint32_t), "the tile buffers");
        R.alloc(R.dCntF, (uint64_t)nbMax * sizeof(uint32_t), "the tile buffers");
    };
    if (P == 1) allocTiles();
    HIP_CHECK(hipHostMalloc((void**)&R.hState, LCB_JUNCTION_STATE_BYTES, hipHostMallocDefault));

    // ---- upload
    float ms = 0;
    HIP_CHECK(hipEventRecord(R.evA, R.stream));
    HIP_CHECK(hipMemsetAsync(R.dCodes, 4, len, R.stream));
    HIP_CHECK(hipMemsetAsync(R.dState, 0, LCB_JUNCTION_STATE_BYTES, R.stream));
    HIP_CHECK(hipStreamSynchronize(R.stream));
    src.upload(R);
    HIP_CHECK(hipEventRecord(R.evB, R.stream));
    HIP_CHECK(hipEventSynchronize(R.evB));
    HIP_CHECK(hipEventElapsedTime(&ms, R.evA, R.evB));
    S.upload_ms = ms;

    // ---- table(s). One attempt to fill a fresh table of 2^log2 slots with `insert` (a launch on R.stream); false: too full, the
    // table is freed again.
    uint64_t mask = 0;
    auto tryTable = [&](uint32_t log2, const std::string& what, double& phaseMs, auto insert) {
        const uint64_t cap = 1ull << log2;
        mask = cap - 1;
        R.alloc(R.dKey, cap * sizeof(unsigned long long), what.c_str());
        R.alloc(R.dVal, cap * sizeof(uint32_t), what.c_str());
        R.timed(phaseMs, [&]() {
            HIP_CHECK(hipMemsetAsync(R.dKey, 0, cap * sizeof(unsigned long long), R.stream));
            HIP_CHECK(hipMemsetAsync(R.dVal, 0, cap * sizeof(uint32_t), R.stream));
            HIP_CHECK(hipMemsetAsync(R.dState, 0, sizeof(JState), R.stream));
            insert();
        });
        if (!R.hState->full && R.hState->used * 10 <= cap * 9) return true;
        S.table_rebuilds++;
        R.release(R.dKey, cap * sizeof(unsigned long long));
        R.release(R.dVal, cap * sizeof(uint32_t));
        return false;
    };
    // A table that may take whatever it needs: too full -> twice the slots, from the start.
    auto growTable = [&](uint32_t log2, const std::string& name, const char* note, double& phaseMs, auto insert) {
        for (;; log2++) {
            if (log2 > 40) throw LcbError(fn + ": " + name + " would need more than 2^40 slots");
            if (tryTable(log2, name + note, phaseMs, insert)) return;
        }
    };
    const uint32_t gridAll = gridFor(len, J_WPB);
    unsigned long long* const dMarked = (unsigned long long*)((char*)R.dState + sizeof(JState));

    if (P == 1) {
        growTable(capLog2, "the k-mer table", "", S.insert_ms,
                  [&]() { junctionInsert<<<gridAll, JT, 0, R.stream>>>(R.dCodes, len, k, R.dKey, R.dVal, mask, R.dState); });
        S.table_slots = (int64_t)(mask + 1);
        X.passes = 1;
        if (sink.countFirst) {       // the sweep of a marking pass with the final masks, for the number alone
            R.timed(countMs, [&]() {
                lcb_graphk::graphCountWindows<<<gridAll, JT, 0, R.stream>>>(R.dCodes, len, k, R.dKey, R.dVal, mask, dMarked, R.dState);
            });
            if (R.hState->lost) throw LcbError(fn + ": internal error: a k-mer of the input is missing from the table");
            X.junction_windows = (int64_t) * (const unsigned long long*)((const char*)R.hState + sizeof(JState));
        }
    } else {
        // ---- phase A: partition after partition, insert + mark. (M, r) = the k-mers with jPartition(kmer, M) == r. A table too full is
        // doubled; where the doubled table would not fit the budget, the partition is split instead: (M, r) = (2M, r) + (2M, r + M).
        R.alloc(R.dBitmap, bitmapWords * 8, "the bitmap of junction windows");
        HIP_CHECK(hipMemsetAsync(R.dBitmap, 0, bitmapWords * 8, R.stream));
        struct Part { uint32_t M, r, log2; };
        std::vector<Part> todo;
        for (uint32_t p = P; p-- > 0;) todo.push_back(Part{P, p, capLog2});
        while (!todo.empty()) {
            Part q = todo.back();
            todo.pop_back();
            bool split = false;
            while (!tryTable(q.log2, "the k-mer table of a partition", S.insert_ms, [&]() {
                junctionInsertPart<<<gridAll, JT, 0, R.stream>>>(R.dCodes, len, k, R.dKey, R.dVal, mask, R.dState, q.M, q.r);
            })) {
                if (q.log2 < 40 && R.fits(lcb_junction_table_bytes(q.log2 + 1))) { q.log2++; continue; }
                if (2 * q.M > (uint32_t)J_MAX_PARTS)
                    throw LcbError(fn + ": the k-mer table of partition " + std::to_string(q.r) + " of " + std::to_string(q.M) + " is too full at 2^" +
                                   std::to_string(q.log2) + " slots, and twice the slots (" + std::to_string(lcb_junction_table_bytes(q.log2 + 1)) + " bytes on top of " +
                                   std::to_string(R.live) + " in use) do not fit the budget of " + std::to_string(R.budget));
                todo.push_back(Part{2 * q.M, q.r + q.M, q.log2});
                todo.push_back(Part{2 * q.M, q.r, q.log2});
                split = true;
                break;
            }
            if (split) continue;
            S.table_slots = std::max<int64_t>(S.table_slots, (int64_t)(mask + 1));
            R.timed(X.mark_ms, [&]() {
                junctionMarkPart<<<gridAll, JT, 0, R.stream>>>(R.dCodes, len, k, R.dKey, R.dVal, mask, q.M, q.r, R.dBitmap, dMarked, R.dState);
            });
            if (R.hState->lost) throw LcbError(fn + ": internal error: a k-mer of the input is missing from the table of its partition");
            R.release(R.dKey, (mask + 1) * sizeof(unsigned long long));
            R.release(R.dVal, (mask + 1) * sizeof(uint32_t));
            X.passes++;
        }
        // ---- phase B: the table of the junction k-mers (every key of it is a junction), then the tiles as with one table
        const uint64_t nJ = *(const unsigned long long*)((const char*)R.hState + sizeof(JState));
        X.junction_windows = (int64_t)nJ;
        allocTiles();
        growTable(lcb_junction_default_log2(nJ, 1), "the table of junction k-mers", " (phase B is not partitioned)", S.emit_ms,
                  [&]() { junctionFillMarked<<<gridAll, JT, 0, R.stream>>>(R.dCodes, len, k, R.dBitmap, R.dKey, R.dVal, mask, R.dState); });
        if (R.hState->lost) throw LcbError(fn + ": internal error: a marked position holds no window");
        X.junction_table_slots = (int64_t)(mask + 1);
    }

    // ---- tiles: classify + emit in file order; the sink takes tile t - 1 while the device works on tile t
    R.tableBytesKey = (mask + 1) * sizeof(unsigned long long);
    R.tableBytesVal = (mask + 1) * sizeof(uint32_t);
    R.tileBytes[0] = (uint64_t)tileBuf * sizeof(unsigned long long); R.tileBytes[1] = (uint64_t)tileBuf * sizeof(JRecord);
    R.tileBytes[2] = R.tileBytes[3] = (uint64_t)nbMax * sizeof(uint32_t);
    R.bitmapBytes = P == 1 ? 0 : bitmapWords * 8;
    const bool counted = P > 1 || sink.countFirst;
    sink.begin(counted ? (uint64_t)X.junction_windows : 0, tileBuf);
    uint64_t prevN = 0, ids = 0;
    int64_t tile = 0;
    for (uint64_t t0 = 0; t0 < len; t0 += tileWindows, tile++) {
        const uint32_t tileLen = (uint32_t)std::min<uint64_t>(tileWindows, len - t0);
        const uint32_t nb = gridFor(tileLen, JT), nbRun = gridFor(tileLen, J_WPB);
        R.timed(S.emit_ms, [&]() {
            if (P == 1) junctionClassify<<<nbRun, JT, 0, R.stream>>>(R.dCodes, len, k, R.dKey, R.dVal, mask, t0, tileLen, R.dWslot, R.dState);
            else junctionClassifyMarked<<<nbRun, JT, 0, R.stream>>>(R.dCodes, len, k, R.dBitmap, R.dKey, R.dVal, mask, t0, tileLen, R.dWslot, R.dState);
            junctionMarkFirst<<<nb, JT, 0, R.stream>>>(R.dWslot, R.dVal, tileLen, R.dCntJ, R.dCntF);
            junctionScan<<<1, 1024, 0, R.stream>>>(R.dCntJ, R.dCntF, nb, R.dState);
            junctionAssignIds<<<nb, JT, 0, R.stream>>>(R.dWslot, R.dVal, tileLen, R.dCntF, R.dState);
            junctionEmit<<<nb, JT, 0, R.stream>>>(R.dWslot, R.dVal, tileLen, R.dCntJ, t0, R.dOut);
        }, [&]() { sink.meanwhile(tile); });
        if (R.hState->lost) throw LcbError(fn + ": internal error: a k-mer of the input is missing from the table");
        prevN = R.hState->totJ;
        ids = R.hState->idNext;
        if (ids > 0x7FFFFFFFull) throw LcbError(fn + ": more than 2^31 - 1 junction k-mers (the value word holds 31 bits of id)");
        if (prevN > tileLen) throw LcbError(fn + ": internal error: more records than windows in a tile");
        sink.tileDone(tile, prevN, (uint64_t)S.occurrences);
        S.occurrences += (int64_t)prevN;
    }
    sink.meanwhile(tile);
    if (!counted) X.junction_windows = S.occurrences;
    else if (S.occurrences != X.junction_windows) throw LcbError(fn + ": internal error: the tiles found another number of junction windows than the passes marked");
    S.junction_kmers = (int64_t)ids;
    S.tiles = tile;
    return ids;
}

}  // namespace

void lcb_junctions_build_impl(const std::vector<std::string>& fasta, int k, int ordinal, const lcb_junction_opts_ex& opts, const std::string& outFile,
                              lcb_junction_stats_ex* stats)
{
    needDevice("lcb_junctions_build", "the CPU tool is lcb-mkgraph", ordinal);
    lcb_junction_stats_ex X;
    memset(&X, 0, sizeof(X));
    lcb_junction_stats& S = X.base;

    // ---- read + encode (in place: the sequence strings become the code bytes)
    double t = nowMs();
    std::vector<lcb_fasta::Record> rec;
    for (const std::string& f : fasta) {
        try { lcb_fasta::readFasta(f, rec); } catch (std::exception& e) { throw LcbError(e.what()); }
    }
    Source src;
    for (const lcb_fasta::Record& r : rec) src.recLen.push_back(r.seq.size());
    src.layout(k);
    for (lcb_fasta::Record& r : rec) {
        char* p = &r.seq[0];
        const int64_t n = (int64_t)r.seq.size();
        #pragma omp parallel for schedule(static) if (n > (1 << 16))
        for (int64_t i = 0; i < n; i++) { const int c = lcb_fasta::code(p[i]); p[i] = (char)(c < 0 ? 4 : c); }
    }
    S.read_ms = nowMs() - t;
    src.upload = [&](Run& R) {
        for (size_t r = 0; r < rec.size(); r++)
            if (!rec[r].seq.empty()) HIP_CHECK(hipMemcpy(R.dCodes + src.base[r], rec[r].seq.data(), rec[r].seq.size(), hipMemcpyHostToDevice));
        std::vector<lcb_fasta::Record>().swap(rec);      // (the host copy of the sequence is no longer needed)
    };

    // ---- the file sink: the host turns tile t - 1 into records while the device works on tile t
    Run R;
    Writer W{R, src.base, src.recLen, S.write_ms};
    uint64_t prevN = 0;
    Sink sink;
    sink.begin = [&](uint64_t, uint32_t tileBuf) {
        HIP_CHECK(hipHostMalloc((void**)&R.hOut[0], (size_t)tileBuf * sizeof(JRecord), hipHostMallocDefault));
        HIP_CHECK(hipHostMalloc((void**)&R.hOut[1], (size_t)tileBuf * sizeof(JRecord), hipHostMallocDefault));
        R.part = outFile + ".part";
        R.f = fopen(R.part.c_str(), "wb");
        if (!R.f) { const std::string p = R.part; R.part.clear(); throw LcbError("cannot create " + p); }
    };
    sink.meanwhile = [&](int64_t tile) { if (tile > 0) W.drain((int)((tile - 1) & 1), prevN); };
    sink.tileDone = [&](int64_t tile, uint64_t n, uint64_t) {
        prevN = n;
        if (n) HIP_CHECK(hipMemcpyAsync(R.hOut[tile & 1], R.dOut, n * sizeof(JRecord), hipMemcpyDeviceToHost, R.stream));
        HIP_CHECK(hipEventRecord(R.evCopy[tile & 1], R.stream));
    };
    double countMs = 0;
    junctionPipeline(R, src, k, ordinal, opts, sink, X, countMs);
    const std::vector<uint64_t>& recLen = src.recLen;

    // ---- finish: the separators of the sequences behind the last record, and the file under its name
    const double tw = nowMs();
    for (; W.curRec < recLen.size(); W.curRec++) W.put(0xFFFFFFFFu, INT64_MAX);
    W.flushBuf();
    FILE* f = R.f;
    R.f = nullptr;
    if (fclose(f) != 0) throw LcbError("cannot write " + R.part);
    if (rename(R.part.c_str(), outFile.c_str()) != 0) throw LcbError("cannot rename " + R.part + " to " + outFile);
    R.part.clear();
    S.write_ms += nowMs() - tw;
    X.peak_device_bytes = R.peak;
    if (stats) *stats = X;
}

// ---- the graph from the FASTA files alone: the same pipeline with a sink that keeps a tile's records on the device,
// then the kernels of lcb_graph_kernels.h. The host parses the FASTA (graph.cpp's parser: names, strings, validation), downloads the
// kept arrays and builds the CSR (graph.cpp's code); it makes no pass over the raw records.
//
// The device part is shared by its two callers (graphOnDevice): lcb_graph_build_impl downloads the kept arrays and releases the device,
// lcb_open_fasta_impl passes them on to the device that is being created.
namespace {

// The FASTA files with the loader's parser (the strings stay in the graph) -> where the records lie in the code array.
Source parseSource(const char* const FN, lcb_graph* g, const std::vector<std::string>& fasta, int k, int threads)
{
    g->k = k;
    const size_t nRec = lcb_graph_parse_fasta(*g, fasta, threads);
    Source src;
    for (size_t r = 0; r < nRec; r++) src.recLen.push_back(g->seq[r].size());
    src.layout(k);
    if (nRec > 0x7FFFFFFFull) throw LcbError(std::string(FN) + ": more than 2^31 - 1 FASTA records");
    return src;
}

// The code bytes of the graph's strings -> R.dCodes (which holds a breaker everywhere): made chunk by chunk in the run's two pinned
// staging buffers (never in place: the strings are the graph's) and copied behind each other.
void uploadCodes(Run& R, const lcb_graph* g, const Source& src, int threads)
{
    const std::vector<uint64_t>& base = src.base;
    const uint64_t len = src.len;
    const size_t nRec = src.recLen.size();
    const uint64_t chunk = std::min<uint64_t>(len, 32ull << 20);
    for (uint8_t*& p : R.hStage) HIP_CHECK(hipHostMalloc((void**)&p, chunk, hipHostMallocDefault));
    size_t r = 0;
    int64_t n = 0;
    for (uint64_t c0 = 0; c0 < len; c0 += chunk, n++) {
        const int slot = (int)(n & 1);
        if (n >= 2) HIP_CHECK(hipEventSynchronize(R.evCopy[slot]));
        uint8_t* s = R.hStage[slot];
        const uint64_t c1 = std::min(len, c0 + chunk);
        memset(s, 4, c1 - c0);
        while (r < nRec && base[r] + src.recLen[r] <= c0) r++;
        for (size_t q = r; q < nRec && base[q] < c1; q++) {
            const int64_t lo = (int64_t)std::max(base[q], c0), hi = (int64_t)std::min(base[q] + src.recLen[q], c1);
            const char* p = g->seq[q].data();
            const int64_t b = (int64_t)base[q], s0 = (int64_t)c0;
            #pragma omp parallel for num_threads(threads) schedule(static) if (hi - lo > (1 << 16))
            for (int64_t i = lo; i < hi; i++) { const int c = lcb_fasta::code(p[i - b]); s[i - s0] = (uint8_t)(c < 0 ? 4 : c); }
        }
        HIP_CHECK(hipMemcpyAsync(R.dCodes + c0, s, c1 - c0, hipMemcpyHostToDevice, R.stream));
        HIP_CHECK(hipEventRecord(R.evCopy[slot], R.stream));
    }
    HIP_CHECK(hipStreamSynchronize(R.stream));
    for (uint8_t*& p : R.hStage) { HIP_CHECK(hipHostFree(p)); p = nullptr; }
}

uint64_t graphTail(Run& R, const char* const FN, lcb_graph* g, uint64_t N, size_t runs, size_t nRec, int k, int abundance, bool fromFile, lcb_graph_build_stats& B,
                   uint64_t& K);

// The front half for the FASTA files alone: parse, junction pipeline with a sink that keeps a tile's records on the device (graphTake),
// then the tail. -> what the tail returns.
uint64_t graphOnDevice(Run& R, const char* const FN, lcb_graph* g, const std::vector<std::string>& fasta, int k, int abundance, int threads, int ordinal,
                       const lcb_junction_opts_ex& opts, lcb_graph_build_stats& B, uint64_t& K)
{
    using namespace lcb_graphk;
    lcb_junction_stats_ex& X = B.junctions;

    // ---- parse once, with the loader's parser; the strings stay in the graph
    double t = nowMs();
    Source src = parseSource(FN, g, fasta, k, threads);
    const size_t nRec = src.recLen.size();
    const std::vector<uint64_t>& base = src.base;
    B.parse_ms = nowMs() - t;

    uint64_t N = 0, ids = 0;
    {
        R.fn = FN;
        src.upload = [&](Run& R) {
            const double t0 = nowMs();
            uploadCodes(R, g, src, threads);
            B.parse_ms += nowMs() - t0;
        };
        Sink sink;
        sink.countFirst = true;
        sink.begin = [&](uint64_t junctionWindows, uint32_t) {
            N = junctionWindows;
            R.alloc(R.dRawPos, std::max<uint64_t>(1, N) * sizeof(uint32_t), "the raw positions");
            R.alloc(R.dRawId, std::max<uint64_t>(1, N) * sizeof(int32_t), "the raw ids");
            R.alloc(R.dBase, (nRec + 1) * 8, "the record bases");
            R.alloc(R.dRecFirst, (nRec + 1) * 8, "the first raw index of every record");
            HIP_CHECK(hipMemcpyAsync(R.dBase, base.data(), (nRec + 1) * 8, hipMemcpyHostToDevice, R.stream));
            HIP_CHECK(hipMemsetAsync(R.dRecFirst, 0xFF, (nRec + 1) * 8, R.stream));
            HIP_CHECK(hipStreamSynchronize(R.stream));
        };
        sink.meanwhile = [](int64_t) {};
        sink.tileDone = [&](int64_t, uint64_t n, uint64_t before) {
            if (before + n > N) throw LcbError(std::string(FN) + ": internal error: the tiles hold more junction windows than the count found");
            if (n) R.timed(B.take_ms, [&]() { graphTake<<<gridFor(n, G_T, FN), G_T, 0, R.stream>>>(R.dOut, (uint32_t)n, before, R.dBase, (uint32_t)nRec, R.dRawPos, R.dRawId, R.dRecFirst); });
        };
        ids = junctionPipeline(R, src, k, ordinal, opts, sink, X, B.count_ms);
        X.base.read_ms = B.parse_ms;
        B.raw_occurrences = (int64_t)N;

        // ---- the junction finder's tables are done with
        R.release(R.dKey, R.tableBytesKey);
        R.release(R.dVal, R.tableBytesVal);
        R.release(R.dBitmap, R.bitmapBytes);
        R.release(R.dWslot, R.tileBytes[0]);
        R.release(R.dOut, R.tileBytes[1]);
        R.release(R.dCntJ, R.tileBytes[2]);
        R.release(R.dCntF, R.tileBytes[3]);
    }
    g->nVertex = N ? (uint32_t)(ids + 1) : 0u;
    return graphTail(R, FN, g, N, nRec, nRec, k, abundance, false, B, K);
}

// The tail of its two front halves (the FASTA files alone, above; a junction file, graphFromFile below): abundance filter and compaction.
// In: R holds the N raw records (dRawPos, dRawId), the first raw index of each of the `runs` runs of records (dRecFirst; a run is a FASTA
// record that has junctions, or what lies between two separators of a file), the code bytes and the bases of the nRec FASTA records
// (dCodes, dBase); g has its names, sequences and nVertex. On return R holds the four kept arrays (K positions each) besides what is
// left of the run, g has chrStart, and its per-position vectors have their size (nothing in them yet). The per-chromosome limit is
// checked; fromFile: so is what a junction finder of ours cannot get wrong (fileBounds, fileOrder). -> the characters the compaction
// marked for the host (the sentinel in posCh).
uint64_t graphTail(Run& R, const char* const FN, lcb_graph* g, uint64_t N, size_t runs, size_t nRec, int k, int abundance, bool fromFile, lcb_graph_build_stats& B,
                   uint64_t& K)
{
    using namespace lcb_graphk;
    // ---- what the loader refuses in a junction file: a chromosome without junctions in front of a later one; another number of
    // FASTA records than chromosomes (a junction file has no way to say that records behind the last chromosome exist)
    double td = nowMs();
    std::vector<unsigned long long> recFirst(runs);
    if (runs) HIP_CHECK(hipMemcpy(recFirst.data(), R.dRecFirst, runs * 8, hipMemcpyDeviceToHost));
    B.download_bytes += runs * 8;
    const size_t C = lcb_file::chromosomes(recFirst.data(), runs, N);
    lcb_file::sameRecords(nRec, C);
    B.junctions.base.records = (int64_t)C;
    B.download_ms += nowMs() - td;

    // ---- abundance over the unfiltered records of both strands, keep-counts, their scan
    const uint32_t nb = N ? gridFor(N, G_T, FN) : 0;
    R.alloc(R.dCounter, ((uint64_t)g->nVertex + 1) * sizeof(uint32_t), "the abundance counters");
    R.alloc(R.dBlockKept, ((uint64_t)nb + 1) * 8, "the keep-counts");
    R.alloc(R.dTotals, 16, "the totals");
    const char* aggEnv = getenv("LCB_GRAPH_ABUNDANCE");          // wave (aggregate equal ids within a wavefront) or plain; a measurement hook
    const bool wave = aggEnv && std::string(aggEnv) == "wave";
    R.timed(B.abundance_ms, [&]() {
        HIP_CHECK(hipMemsetAsync(R.dCounter, 0, ((uint64_t)g->nVertex + 1) * sizeof(uint32_t), R.stream));
        HIP_CHECK(hipMemsetAsync(R.dTotals, 0, 16, R.stream));
        if (!N) return;
        if (wave) graphAbundanceWave<<<nb, G_T, 0, R.stream>>>(R.dRawId, N, R.dCounter);
        else graphAbundance<<<nb, G_T, 0, R.stream>>>(R.dRawId, N, R.dCounter);
    });
    unsigned long long totals[2] = {0, 0}, flags[2] = {0, 0};      // (R.dFlags: the front half of a file made and cleared it)
    if (N) {
        R.timed(B.compact_ms, [&]() {
            graphKeepCount<<<nb, G_T, 0, R.stream>>>(R.dRawId, N, R.dCounter, (uint32_t)abundance, R.dBlockKept);
            graphScan<<<1, G_SCAN_T, 0, R.stream>>>(R.dBlockKept, nb, R.dTotals);
            // a kept junction beyond the end of its sequence is refused before the compaction reads the code bytes around it
            if (fromFile) lcb_filek::fileBounds<<<nb, G_T, 0, R.stream>>>(R.dRawPos, R.dRawId, N, R.dCounter, (uint32_t)abundance, R.dBase, R.dRecFirst, (uint32_t)C, k, R.dFlags);
        });
        HIP_CHECK(hipMemcpy(totals, R.dTotals, 8, hipMemcpyDeviceToHost));
        B.download_bytes += 8;
        if (fromFile) {
            HIP_CHECK(hipMemcpy(flags, R.dFlags, 8, hipMemcpyDeviceToHost));
            B.download_bytes += 8;
            if (flags[0]) throw LcbError("a junction lies beyond the end of its sequence (junction file and FASTA do not match)");
        }
    }
    K = totals[0];
    if (K > N) throw LcbError(std::string(FN) + ": internal error: more kept than raw occurrences");

    // ---- compaction: the four per-position arrays and chrStart
    R.alloc(R.dPosId, std::max<uint64_t>(1, K) * 4, "the kept ids");
    R.alloc(R.dPosPos, std::max<uint64_t>(1, K) * 4, "the kept positions");
    R.alloc(R.dPosCh, std::max<uint64_t>(1, K), "the characters");
    R.alloc(R.dPosRevCh, std::max<uint64_t>(1, K), "the characters");
    R.alloc(R.dChrStart, (C + 1) * 8, "chrStart");
    if (N)
        R.timed(B.compact_ms, [&]() {
            graphCompact<<<nb, G_T, 0, R.stream>>>(R.dRawPos, R.dRawId, N, R.dCounter, (uint32_t)abundance, R.dBlockKept, R.dCodes, R.dBase, R.dRecFirst, (uint32_t)C, k,
                                                   R.dPosId, R.dPosPos, R.dPosCh, R.dPosRevCh, R.dChrStart, R.dTotals + 1);
            if (fromFile && K > 1) lcb_filek::fileOrder<<<gridFor(K, G_T, FN), G_T, 0, R.stream>>>(R.dPosPos, K, R.dChrStart, (uint32_t)C, R.dFlags);
        });
    if (fromFile && K > 1) {
        HIP_CHECK(hipMemcpy(&flags[1], R.dFlags + 1, 8, hipMemcpyDeviceToHost));
        B.download_bytes += 8;
        if (flags[1]) throw LcbError("junction positions must strictly increase within a chromosome");
    }

    // ---- download: chrStart, the number of characters to patch (both tiny); the per-chromosome limit
    td = nowMs();
    g->posId.resize(K); g->posPos.resize(K); g->posCh.resize(K); g->posRevCh.resize(K);
    g->chrStart.assign(C + 1, 0);
    if (C && N) HIP_CHECK(hipMemcpy(g->chrStart.data(), R.dChrStart, C * 8, hipMemcpyDeviceToHost));
    g->chrStart[C] = K;
    if (N) HIP_CHECK(hipMemcpy(&totals[1], R.dTotals + 1, 8, hipMemcpyDeviceToHost));
    B.download_bytes += 8 * C + 8;
    B.download_ms += nowMs() - td;
    for (size_t c = 0; c < C; c++) {
        if (g->chrStart[c + 1] < g->chrStart[c]) throw LcbError(std::string(FN) + ": internal error: chrStart does not ascend");
        if (g->chrStart[c + 1] - g->chrStart[c] >= LCB_SEG_POSITIONS) throw LcbError("a chromosome with 2^32 - 2^20 or more junctions is not supported (the reference's own limit is 2^32 bp, hence fewer than 2^32 junctions, per chromosome)");
    }
    B.kept_occurrences = (int64_t)K;
    B.vertices = (int64_t)g->nVertex;
    return totals[1];
}

}  // namespace

uint64_t lcb_graph_patch_chars(lcb_graph* g, int threads, std::vector<uint64_t>* patchQ, std::vector<uint8_t>* patchLetter)
{
    const size_t C = g->chrStart.size() - 1;
    const int k = g->k;
    std::vector<std::vector<uint64_t>> hits(patchQ ? C : 0);           // per chromosome: the list ascends without a sort
    uint64_t found = 0;
    #pragma omp parallel for num_threads(threads) schedule(dynamic, 1) reduction(+ : found)
    for (int64_t c = 0; c < (int64_t)C; c++) {
        const std::string& s = g->seq[(size_t)c];
        uint8_t* const ch = g->posCh.data();
        uint64_t i = g->chrStart[(size_t)c];
        const uint64_t end = g->chrStart[(size_t)c + 1];
        while (i < end) {
            const uint8_t* hit = (const uint8_t*)memchr(ch + i, lcb_graphk::G_PATCH, end - i);
            if (!hit) break;
            i = (uint64_t)(hit - ch);
            ch[i] = (uint8_t)s[(size_t)g->posPos[i] + (size_t)k];
            if (patchQ) hits[(size_t)c].push_back(i);
            found++;
            i++;
        }
    }
    if (patchQ) {
        patchQ->clear(); patchLetter->clear();
        for (const std::vector<uint64_t>& h : hits)
            for (uint64_t q : h) { patchQ->push_back(q); patchLetter->push_back(g->posCh[(size_t)q]); }
    }
    return found;
}

namespace {

// ---- the front half for a junction file: what lcb_graph_load_impl reads on host threads, read on the device. The file
// goes up tile by tile through the run's two pinned staging buffers and stays resident as words until its records are taken:
// fileCount per tile (the host reads tile n + 1 meanwhile), a scan, fileTake; then the file is released, the FASTA is parsed, its code
// bytes go up, and the tail runs. Of `opts`, tile_windows (records per tile) and mem_budget are read. -> what the tail returns.
uint64_t graphFromFile(Run& R, const char* const FN, lcb_graph* g, const std::string& file, const std::vector<std::string>& fasta, int k, int abundance, int threads,
                       int ordinal, const lcb_junction_opts_ex& opts, lcb_graph_build_stats& B, uint64_t& K)
{
    using namespace lcb_filek;
    lcb_junction_stats& S = B.junctions.base;
    R.fn = FN;
    lcb_file::Reader in(file);
    const lcb_file::Tiling T = lcb_file::tiling(in.bytes, opts.tile_windows);
    const uint64_t blocks = T.blocks();
    HIP_CHECK(hipSetDevice(ordinal));
    size_t freeB = 0, totalB = 0;
    HIP_CHECK(hipMemGetInfo(&freeB, &totalB));
    R.budget = opts.mem_budget ? std::min<uint64_t>(opts.mem_budget, freeB) : (uint64_t)freeB;
    R.start();
    R.alloc(R.dState, LCB_JUNCTION_STATE_BYTES, "the state");
    R.alloc(R.dFlags, 32, "the counts and the flags of the file");       // [0] fileBounds, [1] fileOrder, [2] separators, [3] max |id| + 1
    R.alloc(R.dFile, std::max<uint64_t>(4, T.nRec * 12), "the junction file");
    R.alloc(R.dBlockSep, (blocks + 1) * 8, "the separator counts");
    HIP_CHECK(hipHostMalloc((void**)&R.hState, LCB_JUNCTION_STATE_BYTES, hipHostMallocDefault));
    HIP_CHECK(hipMemsetAsync(R.dState, 0, LCB_JUNCTION_STATE_BYTES, R.stream));
    HIP_CHECK(hipMemsetAsync(R.dFlags, 0, 32, R.stream));

    // ---- the file: read, copy, count
    float ms = 0;
    if (T.nRec)
        for (uint8_t*& p : R.hStage) HIP_CHECK(hipHostMalloc((void**)&p, (size_t)T.tile * 12, hipHostMallocDefault));
    HIP_CHECK(hipEventRecord(R.evA, R.stream));
    for (uint64_t t = 0; t < T.tiles; t++) {
        const int slot = (int)(t & 1);
        if (t >= 2) HIP_CHECK(hipEventSynchronize(R.evCopy[slot]));
        const double t0 = nowMs();
        in.read(T, t, R.hStage[slot]);
        S.read_ms += nowMs() - t0;
        HIP_CHECK(hipMemcpyAsync(R.dFile + 3 * T.first(t), R.hStage[slot], T.count(t) * 12, hipMemcpyHostToDevice, R.stream));
        HIP_CHECK(hipEventRecord(R.evCopy[slot], R.stream));
        fileCount<<<T.bpt, F_T, 0, R.stream>>>(R.dFile, T.nRec, T.tile, t, R.dBlockSep + t * T.bpt, R.dFlags + 2);
    }
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipEventRecord(R.evB, R.stream));
    HIP_CHECK(hipEventSynchronize(R.evB));
    HIP_CHECK(hipEventElapsedTime(&ms, R.evA, R.evB));
    S.upload_ms = ms;
    S.tiles = (int64_t)T.tiles;
    for (uint8_t*& p : R.hStage) if (p) { HIP_CHECK(hipHostFree(p)); p = nullptr; }

    // ---- the raw records and the first raw index of every run
    unsigned long long counts[2] = {0, 0};
    HIP_CHECK(hipMemcpy(counts, R.dFlags + 2, 16, hipMemcpyDeviceToHost));
    B.download_bytes += 16;
    if (counts[0] > T.nRec) throw LcbError(std::string(FN) + ": internal error: more separators than records");
    const uint64_t N = T.nRec - counts[0];
    const size_t runs = (size_t)counts[0] + 1;
    R.alloc(R.dRawPos, std::max<uint64_t>(1, N) * sizeof(uint32_t), "the raw positions");
    R.alloc(R.dRawId, std::max<uint64_t>(1, N) * sizeof(int32_t), "the raw ids");
    R.alloc(R.dRecFirst, (uint64_t)runs * 8, "the first raw index of every run");
    HIP_CHECK(hipMemsetAsync(R.dRecFirst, 0xFF, (uint64_t)runs * 8, R.stream));
    if (N)
        R.timed(B.take_ms, [&]() {
            lcb_graphk::graphScan<<<1, lcb_graphk::G_SCAN_T, 0, R.stream>>>(R.dBlockSep, blocks, R.dBlockSep + blocks);
            fileTake<<<gridFor(blocks, 1, FN), F_T, 0, R.stream>>>(R.dFile, T.nRec, T.tile, T.bpt, R.dBlockSep, N, runs, R.dRawPos, R.dRawId, R.dRecFirst);
        });
    else HIP_CHECK(hipStreamSynchronize(R.stream));
    R.release(R.dFile, std::max<uint64_t>(4, T.nRec * 12));
    R.release(R.dBlockSep, (blocks + 1) * 8);
    B.raw_occurrences = (int64_t)N;
    g->nVertex = N ? (uint32_t)counts[1] : 0u;

    // ---- the FASTA: parsed with the loader's parser, its code bytes and record bases go up
    double t = nowMs();
    const Source src = parseSource(FN, g, fasta, k, threads);
    const size_t nRec = src.recLen.size();
    R.alloc(R.dCodes, src.len, "the sequence");
    R.alloc(R.dBase, (nRec + 1) * 8, "the record bases");
    HIP_CHECK(hipEventRecord(R.evA, R.stream));
    HIP_CHECK(hipMemsetAsync(R.dCodes, 4, src.len, R.stream));
    HIP_CHECK(hipMemcpyAsync(R.dBase, src.base.data(), (nRec + 1) * 8, hipMemcpyHostToDevice, R.stream));
    uploadCodes(R, g, src, threads);
    HIP_CHECK(hipEventRecord(R.evB, R.stream));
    HIP_CHECK(hipEventSynchronize(R.evB));
    HIP_CHECK(hipEventElapsedTime(&ms, R.evA, R.evB));
    S.upload_ms += ms;
    B.parse_ms = nowMs() - t;
    return graphTail(R, FN, g, N, runs, nRec, k, abundance, true, B, K);
}

// What produces the kept arrays in a run: one of the two front halves with its arguments bound.
typedef std::function<uint64_t(Run&, lcb_graph*, lcb_graph_build_stats&, uint64_t&)> Front;

// The graph as a host object: the kept arrays come down (10 bytes per kept occurrence), the device is released, the host patches the
// letters the code bytes do not have and builds the CSR with the loader's code.
lcb_graph* graphToHost(const char* const FN, const Front& front, int threads, lcb_graph_build_stats* stats)
{
    if (threads < 1) threads = 1;
    lcb_graph_build_stats B;
    memset(&B, 0, sizeof(B));
    std::unique_ptr<lcb_graph> g(new lcb_graph());
    uint64_t K = 0, patched = 0;
    {
        Run R;
        patched = front(R, g.get(), B, K);

        // ---- download: 10 bytes per kept occurrence
        const double td = nowMs();
        if (K) {
            HIP_CHECK(hipMemcpy(g->posId.data(), R.dPosId, K * 4, hipMemcpyDeviceToHost));
            HIP_CHECK(hipMemcpy(g->posPos.data(), R.dPosPos, K * 4, hipMemcpyDeviceToHost));
            HIP_CHECK(hipMemcpy(g->posCh.data(), R.dPosCh, K, hipMemcpyDeviceToHost));
            HIP_CHECK(hipMemcpy(g->posRevCh.data(), R.dPosRevCh, K, hipMemcpyDeviceToHost));
        }
        B.download_bytes += 10 * K;
        B.download_ms += nowMs() - td;
        B.peak_device_bytes = R.peak;
        B.junctions.peak_device_bytes = R.peak;
    }   // (the device is released here: everything below is the host's)

    // ---- the letters the code bytes do not have
    const double tp = nowMs();
    const uint64_t found = lcb_graph_patch_chars(g.get(), threads);
    if (found != patched) throw LcbError(std::string(FN) + ": internal error: the device marked " + std::to_string(patched) + " characters for the host, " + std::to_string(found) + " were found");
    B.patched = (int64_t)patched;
    B.download_ms += nowMs() - tp;

    // ---- the host CSR, by the loader's code
    const double t = nowMs();
    lcb_graph_build_csr(g.get(), threads);
    B.csr_ms = nowMs() - t;
    if (stats) *stats = B;
    return g.release();
}

// Graph + device in one call: the junction run is released except for the four kept arrays, which travel in a holder to
// the device that is being created (device.hip: placement, the one download, the patch of both copies, the table build with the host
// CSR taken from it).
void graphToDevice(const char* const FN, const Front& front, int threads, const lcb_params* p, int ordinal, const lcb_device_opts* dopts, lcb_graph** graph,
                   lcb_device** device, lcb_open_stats* stats)
{
    if (threads < 1) threads = 1;
    lcb_open_stats S;
    memset(&S, 0, sizeof(S));
    lcb_graph_build_stats& B = S.graph;
    std::unique_ptr<lcb_graph> g(new lcb_graph());
    LcbHandover ho;
    ho.fn = FN; ho.threads = threads; ho.stats = &S;
    uint64_t K = 0;
    {
        Run R;
        ho.patched = front(R, g.get(), B, K);
        // the holder takes the four arrays out of the run's account; everything else of the run goes with it (raw arrays, counters,
        // codes, record bases, stream and events)
        ho.kept.release = [](void* q) { return (int)hipFree(q); };
        ho.kept.K = K;
        ho.kept.posId = LcbKeptArrays::take(R.dPosId); ho.kept.posPos = LcbKeptArrays::take(R.dPosPos);
        ho.kept.posCh = LcbKeptArrays::take(R.dPosCh); ho.kept.posRevCh = LcbKeptArrays::take(R.dPosRevCh);
        B.peak_device_bytes = R.peak;
        B.junctions.peak_device_bytes = R.peak;
        ho.junctionPeak = R.peak;
    }
    lcb_device* d = lcb_device_create_handover_impl(g.get(), p, ordinal, dopts, ho);
    if (stats) *stats = S;
    *graph = g.release();
    *device = d;
}

}  // namespace

lcb_graph* lcb_graph_build_impl(const std::vector<std::string>& fasta, int k, int abundance, int threads, int ordinal, const lcb_junction_opts_ex& opts,
                                lcb_graph_build_stats* stats)
{
    const char* const FN = "lcb_graph_build";
    needDevice(FN, "the two-step route is lcb-mkgraph + lcb_graph_load", ordinal);
    return graphToHost(FN, [&](Run& R, lcb_graph* g, lcb_graph_build_stats& B, uint64_t& K) {
        return graphOnDevice(R, FN, g, fasta, k, abundance, std::max(1, threads), ordinal, opts, B, K);
    }, threads, stats);
}

// ---- FASTA -> graph + device in one call
void lcb_open_fasta_impl(const std::vector<std::string>& fasta, int k, int abundance, int threads, const lcb_params* p, int ordinal, const lcb_junction_opts_ex& jopts,
                         const lcb_device_opts* dopts, lcb_graph** graph, lcb_device** device, lcb_open_stats* stats)
{
    const char* const FN = "lcb_open_fasta";
    needDevice(FN, "the two-step route is lcb-mkgraph + lcb_graph_load + lcb_device_create", ordinal);
    graphToDevice(FN, [&](Run& R, lcb_graph* g, lcb_graph_build_stats& B, uint64_t& K) {
        return graphOnDevice(R, FN, g, fasta, k, abundance, std::max(1, threads), ordinal, jopts, B, K);
    }, threads, p, ordinal, dopts, graph, device, stats);
}

// ---- junction file + FASTA -> the graph of lcb_graph_load, with the work on the device
lcb_graph* lcb_graph_load_device_impl(const std::string& file, const std::vector<std::string>& fasta, int k, int abundance, int threads, int ordinal,
                                      const lcb_junction_opts_ex& opts, lcb_graph_build_stats* stats)
{
    const char* const FN = "lcb_graph_load_device";
    needDevice(FN, "the CPU way is lcb_graph_load", ordinal);
    return graphToHost(FN, [&](Run& R, lcb_graph* g, lcb_graph_build_stats& B, uint64_t& K) {
        return graphFromFile(R, FN, g, file, fasta, k, abundance, std::max(1, threads), ordinal, opts, B, K);
    }, threads, stats);
}

// ---- ... and graph + device in one call, the graph handed over in HBM
void lcb_open_junctions_impl(const std::string& file, const std::vector<std::string>& fasta, int k, int abundance, int threads, const lcb_params* p, int ordinal,
                             const lcb_junction_opts_ex& jopts, const lcb_device_opts* dopts, lcb_graph** graph, lcb_device** device, lcb_open_stats* stats)
{
    const char* const FN = "lcb_open_junctions";
    needDevice(FN, "the CPU way is lcb_graph_load + lcb_device_create", ordinal);
    graphToDevice(FN, [&](Run& R, lcb_graph* g, lcb_graph_build_stats& B, uint64_t& K) {
        return graphFromFile(R, FN, g, file, fasta, k, abundance, std::max(1, threads), ordinal, jopts, B, K);
    }, threads, p, ordinal, dopts, graph, device, stats);
}

