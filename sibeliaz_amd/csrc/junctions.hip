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
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "lcb_fasta.h"
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

uint32_t gridFor(uint64_t items, uint64_t perBlock)
{
    const uint64_t n = std::max<uint64_t>(1, (items + perBlock - 1) / perBlock);
    if (n > 0x7FFFFFFFull) throw LcbError("lcb_junctions_build: the input needs more workgroups than one launch has");
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
    uint64_t budget = 0, live = 0, peak = 0;     // the run's own account of its device memory
    ~Run()
    {
        if (stream) (void)hipStreamSynchronize(stream);
        for (void* p : {(void*)dCodes, (void*)dKey, (void*)dVal, (void*)dBitmap, (void*)dWslot, (void*)dOut, (void*)dCntJ, (void*)dCntF, (void*)dState})
            if (p) (void)hipFree(p);
        if (hState) (void)hipHostFree(hState);
        for (JRecord* p : hOut) if (p) (void)hipHostFree(p);
        for (hipEvent_t e : {evA, evB, evCopy[0], evCopy[1]}) if (e) (void)hipEventDestroy(e);
        if (stream) (void)hipStreamDestroy(stream);
        if (f) fclose(f);
        if (!part.empty()) remove(part.c_str());
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
            throw LcbError(std::string("lcb_junctions_build: ") + what + " needs " + std::to_string(bytes) + " bytes of device memory on top of the " + std::to_string(live) +
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

}  // namespace

// opts.partitions == 1: the single-table path. 0: as many partitions as lcb_junctions_plan finds for the budget. Otherwise that many.
void lcb_junctions_build_impl(const std::vector<std::string>& fasta, int k, int ordinal, const lcb_junction_opts_ex& opts, const std::string& outFile,
                              lcb_junction_stats_ex* stats)
{
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0)
        throw LcbError("no HIP device available: lcb_junctions_build runs only on the GPU (there is no CPU fallback; the CPU tool is lcb-mkgraph)");
    if (ordinal < 0 || ordinal >= count) throw LcbError("HIP device ordinal out of range");
    lcb_junction_stats_ex X;
    memset(&X, 0, sizeof(X));
    lcb_junction_stats& S = X.base;
    const uint32_t tableLog2 = opts.table_log2;
    uint32_t P = opts.partitions;

    // ---- read + encode (in place: the sequence strings become the code bytes)
    double t = nowMs();
    std::vector<lcb_fasta::Record> rec;
    for (const std::string& f : fasta) {
        try { lcb_fasta::readFasta(f, rec); } catch (std::exception& e) { throw LcbError(e.what()); }
    }
    std::vector<uint64_t> base(rec.size() + 1), recLen(rec.size());
    uint64_t len = 1, nWindows = 0;
    for (size_t r = 0; r < rec.size(); r++) {
        base[r] = len;
        recLen[r] = rec[r].seq.size();
        len += recLen[r] + 1;
        if (recLen[r] >= (size_t)k) nWindows += recLen[r] - k + 1;
    }
    base[rec.size()] = len;
    for (lcb_fasta::Record& r : rec) {
        char* p = &r.seq[0];
        const int64_t n = (int64_t)r.seq.size();
        #pragma omp parallel for schedule(static) if (n > (1 << 16))
        for (int64_t i = 0; i < n; i++) { const int c = lcb_fasta::code(p[i]); p[i] = (char)(c < 0 ? 4 : c); }
    }
    S.records = (int64_t)rec.size();
    S.windows = (int64_t)nWindows;
    S.read_ms = nowMs() - t;

    // ---- plan: the budget, the number of partitions, and whether the first phase fits, before anything is allocated
    Run R;
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
        throw LcbError("lcb_junctions_build: the input needs " + std::to_string(need) + " bytes of device memory with " + std::to_string(P) + " partition(s), " +
                       std::to_string(R.budget) + " may be used (sequence " + std::to_string(len) + " + 12 bytes per table slot + " +
                       (P == 1 ? "24 bytes per tile window)" : "one bit per base)"));
    X.partitions = P;

    HIP_CHECK(hipStreamCreateWithFlags(&R.stream, hipStreamNonBlocking));
    HIP_CHECK(hipEventCreate(&R.evA));
    HIP_CHECK(hipEventCreate(&R.evB));
    HIP_CHECK(hipEventCreate(&R.evCopy[0]));
    HIP_CHECK(hipEventCreate(&R.evCopy[1]));
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
    for (size_t r = 0; r < rec.size(); r++)
        if (!rec[r].seq.empty()) HIP_CHECK(hipMemcpy(R.dCodes + base[r], rec[r].seq.data(), rec[r].seq.size(), hipMemcpyHostToDevice));
    HIP_CHECK(hipEventRecord(R.evB, R.stream));
    HIP_CHECK(hipEventSynchronize(R.evB));
    HIP_CHECK(hipEventElapsedTime(&ms, R.evA, R.evB));
    S.upload_ms = ms;
    std::vector<lcb_fasta::Record>().swap(rec);      // (the host copy of the sequence is no longer needed)

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
            if (log2 > 40) throw LcbError("lcb_junctions_build: " + name + " would need more than 2^40 slots");
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
                    throw LcbError("lcb_junctions_build: the k-mer table of partition " + std::to_string(q.r) + " of " + std::to_string(q.M) + " is too full at 2^" +
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
            if (R.hState->lost) throw LcbError("lcb_junctions_build: internal error: a k-mer of the input is missing from the table of its partition");
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
        if (R.hState->lost) throw LcbError("lcb_junctions_build: internal error: a marked position holds no window");
        X.junction_table_slots = (int64_t)(mask + 1);
    }

    // ---- tiles: classify + emit in file order; the host turns tile t - 1 into records while the device works on tile t
    HIP_CHECK(hipHostMalloc((void**)&R.hOut[0], (size_t)tileBuf * sizeof(JRecord), hipHostMallocDefault));
    HIP_CHECK(hipHostMalloc((void**)&R.hOut[1], (size_t)tileBuf * sizeof(JRecord), hipHostMallocDefault));
    R.part = outFile + ".part";
    R.f = fopen(R.part.c_str(), "wb");
    if (!R.f) { const std::string p = R.part; R.part.clear(); throw LcbError("cannot create " + p); }
    Writer W{R, base, recLen, S.write_ms};
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
        }, [&]() { if (tile > 0) W.drain((int)((tile - 1) & 1), prevN); });
        if (R.hState->lost) throw LcbError("lcb_junctions_build: internal error: a k-mer of the input is missing from the table");
        prevN = R.hState->totJ;
        ids = R.hState->idNext;
        if (ids > 0x7FFFFFFFull) throw LcbError("lcb_junctions_build: more than 2^31 - 1 junction k-mers (the value word holds 31 bits of id)");
        if (prevN > tileLen) throw LcbError("lcb_junctions_build: internal error: more records than windows in a tile");
        if (prevN) HIP_CHECK(hipMemcpyAsync(R.hOut[tile & 1], R.dOut, prevN * sizeof(JRecord), hipMemcpyDeviceToHost, R.stream));
        HIP_CHECK(hipEventRecord(R.evCopy[tile & 1], R.stream));
        S.occurrences += (int64_t)prevN;
    }
    if (tile > 0) W.drain((int)((tile - 1) & 1), prevN);
    if (P == 1) X.junction_windows = S.occurrences;
    else if (S.occurrences != X.junction_windows) throw LcbError("lcb_junctions_build: internal error: the tiles found another number of junction windows than the passes marked");

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
    S.junction_kmers = (int64_t)ids;
    S.tiles = tile;
    X.peak_device_bytes = R.peak;
    if (stats) *stats = X;
}
