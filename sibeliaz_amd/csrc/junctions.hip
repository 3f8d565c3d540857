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
    unsigned long long* dWslot = nullptr;
    JRecord* dOut = nullptr;
    uint32_t *dCntJ = nullptr, *dCntF = nullptr;
    JState* dState = nullptr;
    JState* hState = nullptr;
    JRecord* hOut[2] = {nullptr, nullptr};
    FILE* f = nullptr;
    std::string part;
    ~Run()
    {
        if (stream) (void)hipStreamSynchronize(stream);
        for (void* p : {(void*)dCodes, (void*)dKey, (void*)dVal, (void*)dWslot, (void*)dOut, (void*)dCntJ, (void*)dCntF, (void*)dState})
            if (p) (void)hipFree(p);
        if (hState) (void)hipHostFree(hState);
        for (JRecord* p : hOut) if (p) (void)hipHostFree(p);
        for (hipEvent_t e : {evA, evB, evCopy[0], evCopy[1]}) if (e) (void)hipEventDestroy(e);
        if (stream) (void)hipStreamDestroy(stream);
        if (f) fclose(f);
        if (!part.empty()) remove(part.c_str());
    }
};

}  // namespace

void lcb_junctions_build_impl(const std::vector<std::string>& fasta, int k, int ordinal, const lcb_junction_opts* opts, const std::string& outFile,
                              lcb_junction_stats* stats)
{
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0)
        throw LcbError("no HIP device available: lcb_junctions_build runs only on the GPU (there is no CPU fallback; the CPU tool is lcb-mkgraph)");
    if (ordinal < 0 || ordinal >= count) throw LcbError("HIP device ordinal out of range");
    lcb_junction_stats S;
    memset(&S, 0, sizeof(S));

    // ---- read + encode (in place: the sequence strings become the code bytes)
    double t = nowMs();
    std::vector<lcb_fasta::Record> rec;
    for (const std::string& f : fasta) {
        try { lcb_fasta::readFasta(f, rec); } catch (std::exception& e) { throw LcbError(e.what()); }
    }
    std::vector<uint64_t> base(rec.size() + 1);
    uint64_t len = 1, nWindows = 0;
    for (size_t r = 0; r < rec.size(); r++) {
        base[r] = len;
        len += rec[r].seq.size() + 1;
        if (rec[r].seq.size() >= (size_t)k) nWindows += rec[r].seq.size() - k + 1;
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

    // ---- sizes, and whether they fit, before anything is allocated
    const uint32_t tileWindows = opts && opts->tile_windows ? opts->tile_windows : (1u << 22);
    const uint32_t tileBuf = (uint32_t)std::min<uint64_t>(tileWindows, len);
    const uint32_t nbMax = gridFor(tileBuf, JT);
    uint32_t capLog2 = 20;
    if (opts && opts->table_log2) capLog2 = opts->table_log2;
    else while ((1ull << capLog2) < nWindows / 2) capLog2++;
    const uint64_t fixedBytes = len + (uint64_t)tileBuf * (sizeof(unsigned long long) + sizeof(JRecord)) + (uint64_t)nbMax * 8 + sizeof(JState);
    auto tableBytes = [](uint32_t log2) { return (1ull << log2) * (sizeof(unsigned long long) + sizeof(uint32_t)); };
    HIP_CHECK(hipSetDevice(ordinal));
    auto needFits = [&](uint64_t need, const char* what) {
        size_t freeB = 0, totalB = 0;
        HIP_CHECK(hipMemGetInfo(&freeB, &totalB));
        if (need > (uint64_t)freeB)
            throw LcbError(std::string("lcb_junctions_build: ") + what + " needs " + std::to_string(need) + " bytes of device memory, " + std::to_string((uint64_t)freeB) +
                           " are free (sequence " + std::to_string(len) + " + 12 bytes per table slot + 24 bytes per tile window)");
    };
    needFits(fixedBytes + tableBytes(capLog2), "the input");

    Run R;
    HIP_CHECK(hipStreamCreateWithFlags(&R.stream, hipStreamNonBlocking));
    HIP_CHECK(hipEventCreate(&R.evA));
    HIP_CHECK(hipEventCreate(&R.evB));
    HIP_CHECK(hipEventCreate(&R.evCopy[0]));
    HIP_CHECK(hipEventCreate(&R.evCopy[1]));
    HIP_CHECK(hipMalloc((void**)&R.dCodes, len));
    HIP_CHECK(hipMalloc((void**)&R.dWslot, (size_t)tileBuf * sizeof(unsigned long long)));
    HIP_CHECK(hipMalloc((void**)&R.dOut, (size_t)tileBuf * sizeof(JRecord)));
    HIP_CHECK(hipMalloc((void**)&R.dCntJ, (size_t)nbMax * sizeof(uint32_t)));
    HIP_CHECK(hipMalloc((void**)&R.dCntF, (size_t)nbMax * sizeof(uint32_t)));
    HIP_CHECK(hipMalloc((void**)&R.dState, sizeof(JState)));
    HIP_CHECK(hipHostMalloc((void**)&R.hState, sizeof(JState), hipHostMallocDefault));
    float ms = 0;

    // ---- upload
    HIP_CHECK(hipEventRecord(R.evA, R.stream));
    HIP_CHECK(hipMemsetAsync(R.dCodes, 4, len, R.stream));
    HIP_CHECK(hipStreamSynchronize(R.stream));
    for (size_t r = 0; r < rec.size(); r++)
        if (!rec[r].seq.empty()) HIP_CHECK(hipMemcpy(R.dCodes + base[r], rec[r].seq.data(), rec[r].seq.size(), hipMemcpyHostToDevice));
    HIP_CHECK(hipEventRecord(R.evB, R.stream));
    HIP_CHECK(hipEventSynchronize(R.evB));
    HIP_CHECK(hipEventElapsedTime(&ms, R.evA, R.evB));
    S.upload_ms = ms;
    std::vector<uint64_t> recLen(rec.size());
    for (size_t r = 0; r < rec.size(); r++) recLen[r] = rec[r].seq.size();
    std::vector<lcb_fasta::Record>().swap(rec);      // (the host copy of the sequence is no longer needed)

    // ---- the k-mer table: insert everything; too full -> twice the slots, from the start
    uint64_t mask = 0;
    for (;; capLog2++) {
        if (capLog2 > 40) throw LcbError("lcb_junctions_build: the k-mer table would need more than 2^40 slots");
        if (R.dKey) { HIP_CHECK(hipFree(R.dKey)); R.dKey = nullptr; }
        if (R.dVal) { HIP_CHECK(hipFree(R.dVal)); R.dVal = nullptr; }
        needFits(tableBytes(capLog2), "the k-mer table");
        const uint64_t cap = 1ull << capLog2;
        mask = cap - 1;
        HIP_CHECK(hipMalloc((void**)&R.dKey, cap * sizeof(unsigned long long)));
        HIP_CHECK(hipMalloc((void**)&R.dVal, cap * sizeof(uint32_t)));
        HIP_CHECK(hipEventRecord(R.evA, R.stream));
        HIP_CHECK(hipMemsetAsync(R.dKey, 0, cap * sizeof(unsigned long long), R.stream));
        HIP_CHECK(hipMemsetAsync(R.dVal, 0, cap * sizeof(uint32_t), R.stream));
        HIP_CHECK(hipMemsetAsync(R.dState, 0, sizeof(JState), R.stream));
        junctionInsert<<<gridFor(len, J_WPB), JT, 0, R.stream>>>(R.dCodes, len, k, R.dKey, R.dVal, mask, R.dState);
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipEventRecord(R.evB, R.stream));
        HIP_CHECK(hipMemcpyAsync(R.hState, R.dState, sizeof(JState), hipMemcpyDeviceToHost, R.stream));
        HIP_CHECK(hipStreamSynchronize(R.stream));
        HIP_CHECK(hipEventElapsedTime(&ms, R.evA, R.evB));
        S.insert_ms += ms;
        if (!R.hState->full && R.hState->used * 10 <= cap * 9) break;
        S.table_rebuilds++;
    }
    S.table_slots = (int64_t)(mask + 1);

    // ---- classify + emit, tile by tile in file order; the host turns tile t - 1 into records while the device works on tile t
    HIP_CHECK(hipHostMalloc((void**)&R.hOut[0], (size_t)tileBuf * sizeof(JRecord), hipHostMallocDefault));
    HIP_CHECK(hipHostMalloc((void**)&R.hOut[1], (size_t)tileBuf * sizeof(JRecord), hipHostMallocDefault));
    R.part = outFile + ".part";
    R.f = fopen(R.part.c_str(), "wb");
    if (!R.f) { const std::string p = R.part; R.part.clear(); throw LcbError("cannot create " + p); }
    std::vector<unsigned char> buf;
    auto flushBuf = [&]() {
        if (!buf.empty() && fwrite(buf.data(), 1, buf.size(), R.f) != buf.size()) throw LcbError("cannot write " + R.part);
        buf.clear();
    };
    auto put = [&](uint32_t pos, int64_t id) {
        const size_t at = buf.size();
        buf.resize(at + 12);
        memcpy(&buf[at], &pos, 4); memcpy(&buf[at + 4], &id, 8);
        if (buf.size() >= (64u << 20)) flushBuf();
    };
    size_t curRec = 0;
    auto drain = [&](int slot, uint64_t n) {          // the records of one tile, with the separators of the sequences that end in front of them
        HIP_CHECK(hipEventSynchronize(R.evCopy[slot]));
        const double t0 = nowMs();
        const JRecord* o = R.hOut[slot];
        for (uint64_t q = 0; q < n; q++) {
            while (o[q].g >= base[curRec] + recLen[curRec]) { put(0xFFFFFFFFu, INT64_MAX); curRec++; }
            put((uint32_t)(o[q].g - base[curRec]), (int64_t)o[q].id);
        }
        flushBuf();
        S.write_ms += nowMs() - t0;
    };
    uint64_t prevN = 0, ids = 0;
    int64_t tile = 0;
    for (uint64_t t0 = 0; t0 < len; t0 += tileWindows, tile++) {
        const uint32_t tileLen = (uint32_t)std::min<uint64_t>(tileWindows, len - t0);
        const uint32_t nb = gridFor(tileLen, JT);
        HIP_CHECK(hipEventRecord(R.evA, R.stream));
        junctionClassify<<<gridFor(tileLen, J_WPB), JT, 0, R.stream>>>(R.dCodes, len, k, R.dKey, R.dVal, mask, t0, tileLen, R.dWslot, R.dState);
        junctionMarkFirst<<<nb, JT, 0, R.stream>>>(R.dWslot, R.dVal, tileLen, R.dCntJ, R.dCntF);
        junctionScan<<<1, 1024, 0, R.stream>>>(R.dCntJ, R.dCntF, nb, R.dState);
        junctionAssignIds<<<nb, JT, 0, R.stream>>>(R.dWslot, R.dVal, tileLen, R.dCntF, R.dState);
        junctionEmit<<<nb, JT, 0, R.stream>>>(R.dWslot, R.dVal, tileLen, R.dCntJ, t0, R.dOut);
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipEventRecord(R.evB, R.stream));
        HIP_CHECK(hipMemcpyAsync(R.hState, R.dState, sizeof(JState), hipMemcpyDeviceToHost, R.stream));
        if (tile > 0) drain((int)((tile - 1) & 1), prevN);
        HIP_CHECK(hipStreamSynchronize(R.stream));
        HIP_CHECK(hipEventElapsedTime(&ms, R.evA, R.evB));
        S.emit_ms += ms;
        if (R.hState->lost) throw LcbError("lcb_junctions_build: internal error: a k-mer of the input is missing from the table");
        prevN = R.hState->totJ;
        ids = R.hState->idNext;
        if (ids > 0x7FFFFFFFull) throw LcbError("lcb_junctions_build: more than 2^31 - 1 junction k-mers (the value word holds 31 bits of id)");
        if (prevN > tileLen) throw LcbError("lcb_junctions_build: internal error: more records than windows in a tile");
        if (prevN) HIP_CHECK(hipMemcpyAsync(R.hOut[tile & 1], R.dOut, prevN * sizeof(JRecord), hipMemcpyDeviceToHost, R.stream));
        HIP_CHECK(hipEventRecord(R.evCopy[tile & 1], R.stream));
        S.occurrences += (int64_t)prevN;
    }
    if (tile > 0) drain((int)((tile - 1) & 1), prevN);
    const double tw = nowMs();
    for (; curRec < recLen.size(); curRec++) put(0xFFFFFFFFu, INT64_MAX);
    flushBuf();
    FILE* f = R.f;
    R.f = nullptr;
    if (fclose(f) != 0) throw LcbError("cannot write " + R.part);
    if (rename(R.part.c_str(), outFile.c_str()) != 0) throw LcbError("cannot rename " + R.part + " to " + outFile);
    R.part.clear();
    S.write_ms += nowMs() - tw;
    S.junction_kmers = (int64_t)ids;
    S.tiles = tile;
    if (stats) *stats = S;
}
