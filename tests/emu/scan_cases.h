// tests/emu/scan_cases.h — TEST-ONLY: what the `scan` modes of seeds_emu, tables_emu, graph_emu and junction_emu share: the generated
// arrays and the comparison of a one-workgroup scan kernel's output with a serial 64-bit prefix sum. Include it behind <vector>/<string>.
//   ones     every entry 1
//   hist     random in [0, 1024]: the range of a tile-histogram entry
//   kept     random in [0, 256] with runs of zeros: blockKept with emptied blocks
//   first / last / second    one non-zero entry, at index 0 / n - 1 / `piece` (the first entry of the second piece; the middle where n <= piece)
//   big      (64-bit entries only) random just below 2^31: the total and the sums of whole wavefronts pass 2^32
#ifndef LCB_SCAN_CASES_H
#define LCB_SCAN_CASES_H
#include <cstdint>
#include <cstdio>
#include <random>
#include <string>
#include <vector>

static const char* const SCAN_CONTENTS[] = {"ones", "hist", "kept", "first", "last", "second", "big"};

// false: the content does not exist for this entry type.
template <class T> static bool scanFill(std::vector<T>& a, uint64_t n, const std::string& content, uint64_t piece, uint64_t seed)
{
    std::mt19937_64 rng(seed * 1000003ull + n);
    a.assign((size_t)n, (T)0);
    if (content == "ones") for (T& x : a) x = 1;
    else if (content == "hist") for (T& x : a) x = (T)(rng() % 1025);
    else if (content == "kept") {
        for (uint64_t i = 0; i < n;) {
            const uint64_t run = 1 + rng() % 700;
            const bool zero = rng() % 3 == 0;
            for (uint64_t j = 0; j < run && i < n; j++, i++) a[(size_t)i] = zero ? (T)0 : (T)(rng() % 257);
        }
    } else if (content == "first") { if (n) a[0] = 1000; }
    else if (content == "last") { if (n) a[(size_t)n - 1] = 1000; }
    else if (content == "second") { if (n) a[(size_t)(piece < n ? piece : n / 2)] = 1000; }
    else if (content == "big") {
        if (sizeof(T) < 8) return false;
        for (T& x : a) x = (T)((1ull << 31) - rng() % 1025);
    } else { fprintf(stderr, "unknown content %s\n", content.c_str()); exit(2); }
    return true;
}

// Serial exclusive prefix sum in 64 bits -> the total.
template <class T> static unsigned long long scanSerial(const std::vector<T>& a, std::vector<unsigned long long>& ex)
{
    unsigned long long run = 0;
    ex.resize(a.size());
    for (size_t i = 0; i < a.size(); i++) { ex[i] = run; run += a[i]; }
    return run;
}

// run(a, n, &total) launches the kernel on a[0..n); a[n] is a guard. 0 = every entry and the total equal the serial scan.
template <class T, class F> static int scanCheck(const char* kernel, uint64_t n, const std::string& content, uint64_t piece, F run)
{
    std::vector<T> a;
    if (!scanFill(a, n, content, piece, 1)) return 0;
    std::vector<unsigned long long> want;
    const unsigned long long wantTotal = scanSerial(a, want);
    if (content == "big" && wantTotal <= (1ull << 32)) { fprintf(stderr, "%s n %llu %s: the serial total %llu does not pass 2^32\n", kernel, (unsigned long long)n, content.c_str(), wantTotal); return 1; }
    if (sizeof(T) < 8 && wantTotal >= (1ull << 32)) { fprintf(stderr, "%s n %llu %s: the serial total %llu does not fit the 32-bit entries\n", kernel, (unsigned long long)n, content.c_str(), wantTotal); return 1; }
    const T guard = (T)0xEEEEEEEEEEEEEEEEull;
    a.push_back(guard);
    unsigned long long total = 0xEEEEEEEEEEEEEEEEull;
    run(a.data(), n, &total);
    if (a[(size_t)n] != guard) { fprintf(stderr, "%s n %llu %s: the kernel wrote behind the array\n", kernel, (unsigned long long)n, content.c_str()); return 1; }
    for (uint64_t i = 0; i < n; i++)
        if ((unsigned long long)a[(size_t)i] != want[(size_t)i]) {
            fprintf(stderr, "%s n %llu %s: entry %llu is %llu, the serial scan has %llu\n", kernel, (unsigned long long)n, content.c_str(), (unsigned long long)i, (unsigned long long)a[(size_t)i], want[(size_t)i]);
            return 1;
        }
    if (total != wantTotal) { fprintf(stderr, "%s n %llu %s: total %llu, the serial scan has %llu\n", kernel, (unsigned long long)n, content.c_str(), total, wantTotal); return 1; }
    printf("scan %s n %llu %s total %llu\n", kernel, (unsigned long long)n, content.c_str(), wantTotal);
    return 0;
}

// Every content in turn. 0 = all equal.
template <class T, class F> static int scanCheckAll(const char* kernel, uint64_t n, uint64_t piece, F run)
{
    for (const char* c : SCAN_CONTENTS) {
        if (std::string(c) == "big" && n < 3) continue;        // (two entries below 2^31 cannot pass 2^32)
        if (scanCheck<T>(kernel, n, c, piece, run)) return 1;
    }
    return 0;
}
#endif
