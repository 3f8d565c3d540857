// TEST-ONLY: the resource owner of the device layer (csrc/lcb_owned.h) driven with stub allocate / free functions in place of
// the hip* calls. Every stub allocation is a real malloc(1) that lives until the end of its case (addresses stay unique), where the
// released ones are freed: under -fsanitize=address one that was never released is reported by the leak check as well as here.
//   1. registering and releasing          2. re-registering on growth          3. a create that throws after the k-th allocation, every k
#include <cstdio>
#include <cstdlib>
#include <map>
#include <stdexcept>
#include <vector>

#include "lcb_owned.h"

namespace {

struct Record { LcbOwnedKind kind; int frees; long order; };
std::map<void*, Record> made;            // every stub allocation ever made
long failAt = -1, allocs = 0, releases = 0;
int failures = 0;

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "owned_emu: %s:%d: %s\n", __FILE__, __LINE__, #c); failures++; } } while (0)

void* stubAlloc(LcbOwnedKind kind)
{
    if (allocs == failAt) { allocs++; throw std::runtime_error("stub allocation failed"); }
    allocs++;
    void* p = malloc(1);
    made[p] = Record{kind, 0, 0};
    return p;
}

int stubRelease(LcbOwnedKind kind, void* p)
{
    auto it = made.find(p);
    CHECK(it != made.end());
    if (it == made.end()) return 1;
    CHECK(it->second.kind == kind);
    CHECK(it->second.frees == 0);
    it->second.frees++;
    it->second.order = ++releases;
    return 0;
}

void* makeOne(LcbOwner& own, LcbOwnedKind kind) { return own.make(kind, [kind] { return stubAlloc(kind); }); }

void reset()
{
    for (auto& kv : made) if (kv.second.frees) free(kv.first);
    made.clear(); failAt = -1; allocs = 0; releases = 0;
}

void expectAllFreedOnce()
{
    for (auto& kv : made) CHECK(kv.second.frees == 1);
}

// the shape of a device's creation: a stream and its events, tables, a buffer that is made again in another size (a workspace, an
// arena), pinned buffers, then per-lane streams, events and buffers
const LcbOwnedKind kCreate[] = {LCB_OWN_STREAM, LCB_OWN_EVENT, LCB_OWN_EVENT, LCB_OWN_DEVICE, LCB_OWN_DEVICE, LCB_OWN_DEVICE, LCB_OWN_PINNED, LCB_OWN_PINNED,
                                LCB_OWN_STREAM, LCB_OWN_STREAM, LCB_OWN_EVENT, LCB_OWN_PINNED, LCB_OWN_DEVICE};
const int kCreateN = (int)(sizeof(kCreate) / sizeof(kCreate[0]));

void mockCreate(LcbOwner& own)
{
    void* grown = nullptr;
    for (int i = 0; i < kCreateN; i++) {
        void* p = makeOne(own, kCreate[i]);
        if (i == 4) grown = p;
        if (i == 7) {                     // growth half-way: the old buffer goes first, as the device's allocWork / allocArena do
            CHECK(own.drop(grown) == 0);
            grown = nullptr;
            grown = makeOne(own, LCB_OWN_DEVICE);
        }
    }
}

}  // namespace

int main()
{
    long cases = 0;
    {   // 1. registering and releasing: everything once, the youngest first, each with its own kind
        reset();
        LcbOwner own(stubRelease);
        std::vector<void*> ps;
        for (int i = 0; i < 12; i++) ps.push_back(makeOne(own, (LcbOwnedKind)(i % 4)));
        CHECK(own.size() == 12);
        own.releaseAll();
        CHECK(own.size() == 0);
        expectAllFreedOnce();
        for (size_t i = 0; i < ps.size(); i++) CHECK(made[ps[i]].order == (long)(ps.size() - i));
        own.releaseAll();                 // a second release finds nothing
        CHECK(releases == 12);
        cases++;
    }
    {   // ... and by the destructor
        reset();
        { LcbOwner own(stubRelease); for (int i = 0; i < 5; i++) makeOne(own, LCB_OWN_PINNED); }
        CHECK(releases == 5);
        expectAllFreedOnce();
        cases++;
    }
    {   // 2. re-registering on growth: the old buffer is released at once and only then, the new one at the end
        reset();
        LcbOwner own(stubRelease);
        void* a = makeOne(own, LCB_OWN_DEVICE);
        void* b = makeOne(own, LCB_OWN_PINNED);
        void* c = makeOne(own, LCB_OWN_EVENT);
        CHECK(own.drop(nullptr) == 0 && releases == 0);
        int notOurs = 0;
        CHECK(own.drop(&notOurs) == -1 && releases == 0 && own.size() == 3);
        CHECK(own.drop(b) == 0);
        CHECK(made[b].frees == 1 && releases == 1 && own.size() == 2);
        CHECK(own.drop(b) == -1 && releases == 1);     // forgotten: not released again
        void* b2 = makeOne(own, LCB_OWN_PINNED);
        for (int g = 0; g < 3; g++) { CHECK(own.drop(b2) == 0); b2 = makeOne(own, LCB_OWN_PINNED); }     // ... and again and again
        CHECK(own.size() == 3);
        own.releaseAll();
        expectAllFreedOnce();
        CHECK(made.size() == 7 && releases == 7);
        CHECK(made[a].order == 7 && made[c].order == 6 && made[b2].order == 5);
        cases++;
    }
    // 3. a create that throws after the k-th allocation: whatever was made by then is released once by the clean-up, nothing else
    for (long k = 0; k <= kCreateN + 1; k++) {
        reset();
        failAt = k;
        LcbOwner own(stubRelease);
        bool threw = false;
        try { mockCreate(own); } catch (const std::runtime_error&) { threw = true; }
        CHECK(threw == (k <= kCreateN));                 // (kCreateN + 1 allocations: the list and the one growth)
        CHECK((long)made.size() == (threw ? k : kCreateN + 1));
        own.releaseAll();
        CHECK(own.size() == 0);
        expectAllFreedOnce();
        CHECK(releases == (long)made.size());
        cases++;
    }
    reset();
    if (failures) { fprintf(stderr, "owned_emu: %d checks failed\n", failures); return 1; }
    printf("owned_emu: %ld cases, every allocation released exactly once\n", cases);
    return 0;
}
