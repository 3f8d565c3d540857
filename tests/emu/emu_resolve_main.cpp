// emu_resolve_main.cpp — TEST-ONLY: the emu_check harness (emu_main.cpp, included unchanged) for the resolved heavy vote of the wide and
// big variants (lcb_vote_resolve / lcb_vote_items in lcb_kernel.h), built by tests/test_vote_resolve_emu.py with a tiny
// LCB_VOTE_RESOLVE_MIN and -DLCB_TEST_RESOLVE_EVENT=lcb_test_resolve_event. It adds two things to emu_check:
//   * the event counters of the resolved path, printed to stderr when the process ends ("resolve-events: ...");
//   * the modes `medium-final` / `big-final`: every seed in the wide / big variant against the oracle in the `used` state a whole
//     FindBlocks leaves behind (emu_check has that state only for the compact variant, `seeds-final`), and `medium-runs` / `big-runs`:
//     the same with pseudo-random runs of used positions (any bitmap is a legal state for the kernels) - sparse enough that a voter's
//     window ends at a used position several chunks into it.
#include <atomic>

#define main emu_check_main
#include "emu_main.cpp"
#undef main

static std::atomic<unsigned long long> g_resolveEvents[LCB_RV_COUNT];
void lcb_test_resolve_event(int what) { g_resolveEvents[what]++; }

namespace {

struct ResolveReport {
    ~ResolveReport()
    {
        fprintf(stderr, "resolve-events: resolved=%llu chunk1=%llu used_beyond_64=%llu repeat_hit=%llu above_max=%llu items_full=%llu round2=%llu\n",
                g_resolveEvents[LCB_RV_RESOLVED].load(), g_resolveEvents[LCB_RV_CHUNK1].load(), g_resolveEvents[LCB_RV_USED_BEYOND_64].load(),
                g_resolveEvents[LCB_RV_REPEAT_HIT].load(), g_resolveEvents[LCB_RV_ABOVE_MAX].load(), g_resolveEvents[LCB_RV_ITEMS_FULL].load(), g_resolveEvents[LCB_RV_ROUND2].load());
    }
} g_resolveReport;

int usedMode(int argc, char** argv, int kernelMode, bool runs)
{
    const char* graph = argv[1]; const char* fasta = argv[2];
    lcb_params p; p.k = atoi(argv[3]); p.max_branch = p.max_flank = atoi(argv[4]); p.min_block = atoi(argv[5]); p.looking_depth = 8; p.phase_size = 256;
    const int a = atoi(argv[6]);
    (void)argc;
    lcb_graph* g = lcb_graph_load_impl(graph, {fasta}, p.k, a, 4);
    std::vector<lcb_seed> seeds;
    lcb_enumerate_seeds_impl(*g, 4, seeds);
    char err[512];
    const char* fa[1] = {fasta};
    orc_graph* og = orc_load(graph, fa, 1, p.k, a, err, sizeof(err));
    if (!og) { fprintf(stderr, "oracle load: %s\n", err); return 1; }
    orc_params op{p.k, p.min_block, p.max_branch, p.max_flank, p.looking_depth};
    if (orc_build_bundles(og) != (int64_t)seeds.size()) { fprintf(stderr, "FAIL: seed count differs\n"); return 1; }
    Emu emu(g, p, kernelMode);
    {   // the state after a whole FindBlocks, or runs of 20 .. 300 used positions (one per 2 000 positions), in the oracle and in the emulated bitmap
        const size_t stride = orc_used_stride();
        if (!runs) {
            orc_block* ob = nullptr; orc_stats st;
            orc_find_blocks(og, &op, &ob, &st, nullptr);
            orc_free_blocks(ob);
        } else {
            uint64_t x = 0x9E3779B97F4A7C15ull;
            auto next = [&]() { x ^= x << 13; x ^= x >> 7; x ^= x << 17; return x; };
            for (int64_t c = 0; c < orc_n_chr(og); c++) {
                uint8_t* u = orc_chr_used(og, c);
                const int64_t n = orc_chr_n_pos(og, c);
                for (int64_t r = 0; r < n / 2000 + 1; r++) {
                    const int64_t q0 = (int64_t)(next() % (uint64_t)std::max<int64_t>(n, 1)), len = 20 + (int64_t)(next() % 281);
                    for (int64_t q = q0; q < n && q < q0 + len; q++) u[(size_t)q * stride] = 1;
                }
            }
        }
        for (int64_t c = 0; c < orc_n_chr(og); c++) {
            const uint8_t* u = orc_chr_used(og, c);
            for (int64_t i = 0; i < orc_chr_n_pos(og, c); i++)
                if (u[(size_t)i * stride]) { const uint64_t q = emu.plan.toDev(g->chrStart[c] + i); emu.used[q >> 5] |= 1u << (q & 31); }
        }
    }
    if (getenv("EMU_LIMIT") && (size_t)atoi(getenv("EMU_LIMIT")) < seeds.size()) seeds.resize((size_t)atoi(getenv("EMU_LIMIT")));   // the heavy seeds come first
    std::vector<LcbKSeed> ks;
    for (auto& s : seeds) ks.push_back(LcbKSeed{s.vid, s.ch, 0u, 0u});
    emu.runRetry(ks);
    orc_counters octr; memset(&octr, 0, sizeof(octr));
    std::vector<orc_inst> ref(1 << 16);
    int bad = 0;
    for (size_t i = 0; i < seeds.size() && bad <= 8; i++) {
        int64_t score = 0;
        const int64_t n = orc_process_seed(og, &op, seeds[i].vid, seeds[i].ch, ref.data(), (int64_t)ref.size(), &score, &octr);
        bad += compareSeed((int64_t)i, seeds[i], emu.out[i], emu.arena.data(), ref.data(), n, score);
        if (getenv("EMU_FP_CHECK") && emu.out[i].status == 0) {
            // footprint completeness as in emu_check: every unused position outside the seed's footprint set to used -> same result
            const LcbSeedOut& o = emu.out[i];
            std::vector<uint8_t> keep((size_t)g->nPos(), 0);
            for (uint32_t e = 0; e < o.nFp; e++) { const LcbFpOut f = emu.fpArena[o.fpOff + e]; for (uint64_t q = emu.plan.toHost(f.lo); q <= emu.plan.toHost(f.hi) && q < keep.size(); q++) keep[q] = 1; }
            const size_t stride = orc_used_stride();
            std::vector<uint8_t*> flipped;
            for (int64_t c = 0; c < orc_n_chr(og); c++) {
                uint8_t* u = orc_chr_used(og, c);
                const uint64_t base = g->chrStart[c];
                for (int64_t q = 0; q < orc_chr_n_pos(og, c); q++) if (!keep[(size_t)(base + q)] && !u[(size_t)q * stride]) { u[(size_t)q * stride] = 1; flipped.push_back(&u[(size_t)q * stride]); }
            }
            int64_t score2 = 0;
            const int64_t n2 = orc_process_seed(og, &op, seeds[i].vid, seeds[i].ch, ref.data(), (int64_t)ref.size(), &score2, nullptr);
            for (uint8_t* u : flipped) *u = 0;
            if (compareSeed((int64_t)i, seeds[i], o, emu.arena.data(), ref.data(), n2, score2)) { fprintf(stderr, "FAIL: the footprint of seed %zu does not cover what it read\n", i); bad++; }
        }
    }
    fprintf(stderr, "%s: %zu seeds, %d mismatches\n", argv[7], seeds.size(), bad);
    if (!bad && !getenv("EMU_NOSTATS") && (emu.ctr.n_walk != octr.n_walk || emu.ctr.n_occ != octr.n_occ || emu.ctr.n_compat_call != octr.n_compat_call ||
                                           emu.ctr.n_compat_step != octr.n_compat_step || emu.ctr.n_inst_out != octr.n_inst_out)) {
        fprintf(stderr, "FAIL: event counters differ (walk %llu vs %llu)\n", (unsigned long long)emu.ctr.n_walk, (unsigned long long)octr.n_walk);
        bad++;
    }
    return bad ? 1 : 0;
}

}  // namespace

int main(int argc, char** argv)
{
    const std::string mode = argc >= 8 ? argv[7] : "";
    if (mode == "medium-final" || mode == "big-final" || mode == "medium-runs" || mode == "big-runs") {
        try { return usedMode(argc, argv, mode[0] == 'b' ? 2 : 1, mode.find("runs") != std::string::npos); }
        catch (const std::exception& e) { fprintf(stderr, "error: %s\n", e.what()); return 1; }
    }
    return emu_check_main(argc, argv);
}
