// vote_scan_emu.cpp — TEST-ONLY: the two pure parts of stage A of the look-ahead vote (lcb_used_fetch8, lcb_used_first in
// lcb_kernel.h) against the definition: the first used step of a walk is the first step d = 1 .. L whose bit - flat bit fb + (d - 1)
// going up, fb - (d - 1) going down - is set, read one bit at a time with lcb_used_bit; the - strand walking down onto its
// chromosome's first position (step d == rem) reads no bit for that step (lcb_it_used). Built by tests/test_vote_scan_emu.py with
// -DLCB_PAGE_SHIFT=2u (pages of four words), once plain and once with the address and undefined-behaviour sanitizers.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "lcb_kernel.h"

namespace {

constexpr uint32_t kWords = 40;                       // words of the bitmap: nPos / 32 + 2
constexpr uint32_t kNPos = 38 * 32 + 19;              // positions (the last word index a window may name is maxW = nPos >> 5 = 38)
constexpr uint32_t kPageWords = 1u << LCB_PAGE_SHIFT;
constexpr uint32_t kPages = kWords / kPageWords;
static_assert(LCB_PAGE_SHIFT == 2u && kWords % kPageWords == 0, "build with -DLCB_PAGE_SHIFT=2u");

// One `used` state in both forms the kernels read: flat (no page table), and as a view whose pages 1, 2, 3 (mod 4) are private copies
// behind the live bitmap in a non-identity order, the live words of those pages holding the complement (a read that skips the table
// is wrong in every bit); pages 0 (mod 4) are shared with the live bitmap (table entry 0).
struct State {
    std::vector<uint32_t> flat, paged, tab;
    explicit State(const std::vector<uint32_t>& bits) : flat(bits), paged(2 * kWords), tab(kPages)
    {
        for (uint32_t p = 0; p < kPages; p++) {
            const uint32_t q = (3 * p + 1) % kPages;             // where the private copy of page p lives
            const bool shared = p % 4 == 0;
            tab[p] = shared ? 0u : kWords + q * kPageWords - p * kPageWords;
            for (uint32_t w = 0; w < kPageWords; w++) {
                const uint32_t v = bits[p * kPageWords + w];
                paged[p * kPageWords + w] = shared ? v : ~v;
                if (!shared) paged[kWords + q * kPageWords + w] = v;
            }
        }
    }
    LcbUsed used(bool viaTable) const { LcbUsed U; U.live = viaTable ? paged.data() : flat.data(); U.tab = viaTable ? tab.data() : nullptr; return U; }
};

uint64_t g_rng = 0x9E3779B97F4A7C15ull;               // fixed seed: the same fills in every run
uint32_t rnd()
{
    g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17;
    return (uint32_t)(g_rng >> 32);
}

template <class F>
uint32_t first_by_definition(const LcbUsed& U, F fb, bool up, bool positive, uint32_t L, uint32_t rem)
{
    for (uint32_t d = 1; d <= L; d++) {
        if (!positive && !up && d == rem) continue;              // the chromosome's first position on the - strand: no bit
        if (lcb_used_bit(U, (F)(up ? fb + (d - 1u) : fb - (d - 1u)))) return d;
    }
    return 0;
}

unsigned long long g_cases = 0;

template <class F>
void check(const State& st, uint32_t fb, bool up, bool positive, uint32_t L, uint32_t rem, const char* what)
{
    for (int viaTable = 0; viaTable < 2; viaTable++) {
        const LcbUsed U = st.used(viaTable != 0);
        uint32_t uw[8];
        lcb_used_fetch8(U, (F)fb, up, kNPos >> 5, uw);
        const uint32_t got = lcb_used_first(U, uw, (F)fb, up, positive, L, rem);
        const uint32_t want = first_by_definition(U, (F)fb, up, positive, L, rem);
        g_cases++;
        if (got != want) {
            fprintf(stderr, "MISMATCH (%s, %s, %u-bit positions): fb %u, %s, %c strand, L %u, rem %u: first used step %u, by definition %u\n", what,
                    viaTable ? "page table" : "flat", (unsigned)(8 * sizeof(F)), fb, up ? "up" : "down", positive ? '+' : '-', L, rem, got, want);
            exit(1);
        }
    }
}

}   // namespace

int main()
{
    const uint32_t origins[] = { 0, 1, 31, 32, 33, 63, 64, 1023, 1024, kNPos - 3, kNPos - 2, kNPos - 1 };
    const uint32_t lengths[] = { 0, 1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 191, 192, 193, 224, 225, 226, 255, 256, 257, 300 };
    std::vector<State> fills;
    for (int density = 0; density < 2; density++)                // 1/64 and 1/4
        for (int f = 0; f < 20; f++) {
            std::vector<uint32_t> bits(kWords, 0u);
            for (uint32_t b = 0; b < kNPos; b++) if (rnd() % (density ? 4u : 64u) == 0) bits[b >> 5] |= 1u << (b & 31);
            fills.emplace_back(bits);
        }
    const State none(std::vector<uint32_t>(kWords, 0u));
    for (uint32_t fb : origins)
        for (int up = 0; up < 2; up++)
            for (int positive = 0; positive < 2; positive++)
                for (int last = 0; last < 2; last++) {           // last: the window ends with the chromosome (L == rem)
                    const bool noBit = last && !up && !positive;                  // ... whose final step then reads one bit fewer
                    if (last && !noBit) continue;                                 // (rem matters to the scan in that one case only)
                    for (uint32_t L0 : lengths) {
                        // clipped to what the map allows: every step that reads a bit reads one of the map
                        const uint32_t room = up ? kNPos - fb : fb + 1u;
                        const uint32_t L = L0 < room + (noBit ? 1u : 0u) ? L0 : room + (noBit ? 1u : 0u);
                        if (last && L == 0) continue;                             // (rem == 0: such a voter does not walk)
                        const uint32_t rem = last ? L : L + 7u;
                        check<uint32_t>(none, fb, up, positive, L, rem, "no used bit");
                        check<uint64_t>(none, fb, up, positive, L, rem, "no used bit");
                        const uint32_t steps[] = { 1u, L - 1u, L, L + 1u };
                        for (uint32_t d : steps) {
                            if (d == 0 || d == ~0u || d > L + 1u) continue;
                            if (up ? d > kNPos - fb : d > fb + 1u) continue;      // the step's bit is outside the map
                            std::vector<uint32_t> bits(kWords, 0u);
                            const uint32_t b = up ? fb + (d - 1u) : fb - (d - 1u);
                            bits[b >> 5] |= 1u << (b & 31);
                            const State one(bits);
                            check<uint32_t>(one, fb, up, positive, L, rem, "one used bit");
                            check<uint64_t>(one, fb, up, positive, L, rem, "one used bit");
                        }
                        for (const State& st : fills) {
                            check<uint32_t>(st, fb, up, positive, L, rem, "random fill");
                            check<uint64_t>(st, fb, up, positive, L, rem, "random fill");
                        }
                    }
                }
    printf("vote-scan: %llu cases, all equal to the definition\n", g_cases);
    return 0;
}
