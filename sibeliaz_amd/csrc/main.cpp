// main.cpp — `sibeliaz-lcb`: drop-in replacement of the reference executable (sibeliaz.cpp:37-157).
//
// Same flags, defaults, stdout banners, output files and exit codes, so line 146 of the reference's
// `sibeliaz` wrapper script keeps working verbatim:
//   sibeliaz-lcb --graph <junctions> <fasta...> -k <odd> -b <int> -o <dir> -m <int> -t <int> --abundance <int> [--noseq] --chunks <int>
// `-t` stays "host threads" (loading, seed enumeration). Everything else is chosen by the environment, never by a new flag; unset and
// empty mean the default, any other spelling and any unsupported combination is refused before anything is loaded (the list in main()):
//   LCB_DEVICE=i / LCB_GPUS=N  the GPU (default 0; HIP_VISIBLE_DEVICES also applies), or HIP devices 0..N-1 driven from this process
//   LCB_SEEDS=host|device      where the seeds are enumerated: host threads, or the device's own tables
//   LCB_TABLES=host|device     where the device's tables are computed (device: one GPU)
//   LCB_JUNCTIONS=file|device  the way to the graph: the junction file of --graph, or lcb_graph_build - the junctions come from the
//                              FASTA arguments on the GPU, --graph is still required by the parser but never opened
//   LCB_HANDOVER=host|device   the way the graph reaches the device: the graph build releases the GPU and the device uploads its tables, or
//                              lcb_open_fasta - needs LCB_JUNCTIONS=device and one GPU: the graph's arrays stay in HBM and become the tables
//   LCB_LOAD=host|device       where the junction file is read: lcb_graph_load on host threads, or lcb_open_junctions - needs
//                              LCB_JUNCTIONS=file and one GPU: the file goes up as it is and graph and device come from one call
// Which of the four opening calls runs is one value of `Opening`, chosen in one place.
// The block finder itself runs on the MI355X through the C ABI in include/lcb.h.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <string>
#include <utility>
#include <vector>

#include "lcb.h"

namespace {

struct Args {
    unsigned k = 25, b = 200, m = 200, t = 1, a = 150, chunks = 0;   // sibeliaz.cpp:45-110
    std::string graph, outDir;
    bool noSeq = false;
    std::vector<std::string> fasta;
};

[[noreturn]] void parseError(const std::string& arg, const std::string& msg)
{
    std::cerr << "PARSE ERROR: Argument: " << arg << "\n             " << msg << "\n\n"
              << "Brief USAGE: \n   sibeliaz-lcb  [--chunks <integer>] [--noseq] [-o <directory name>] --graph <file name> [-a <integer>] "
                 "[-t <integer>] [-m <integer>] [-b <integer>] [-k <oddc>] [--] [--version] [-h] <fasta files with genomes> ...\n\n"
              << "For complete USAGE and HELP type: \n   sibeliaz-lcb --help\n" << std::endl;
    exit(1);
}

unsigned toUnsigned(const std::string& flag, const char* v)
{
    char* end = nullptr;
    if (!v || !*v || *v == '-') parseError(flag, "Couldn't read argument value from string '" + std::string(v ? v : "") + "'");
    const unsigned long x = strtoul(v, &end, 10);
    if (*end) parseError(flag, "Couldn't read argument value from string '" + std::string(v) + "'");
    return (unsigned)x;
}

void usage()
{
    std::cout << "\nUSAGE: \n\n   sibeliaz-lcb  [--chunks <integer>] [--noseq] [-o <directory name>] --graph <file name>\n"
                 "                 [-a <integer>] [-t <integer>] [-m <integer>] [-b <integer>] [-k <oddc>] [--] [--version] [-h]\n"
                 "                 <fasta files with genomes> ...\n\n"
                 "Where: \n\n"
                 "   --chunks <integer>\n     Split blocks for alignment into a number of chunks\n\n"
                 "   --noseq\n     Do not output blocks sequences\n\n"
                 "   -o <directory name>,  --outdir <directory name>\n     Output dir for blocks sequences\n\n"
                 "   --graph <file name>\n     (required)  Binary file containing the graph\n\n"
                 "   -a <integer>,  --abundance <integer>\n     Max abundance of a junction\n\n"
                 "   -t <integer>,  --threads <integer>\n     Number of worker threads\n\n"
                 "   -m <integer>,  --blocksize <integer>\n     Minimum block size\n\n"
                 "   -b <integer>,  --branchsize <integer>\n     Maximum branch size\n\n"
                 "   -k <oddc>,  --kvalue <oddc>\n     Value of k\n\n"
                 "   --,  --ignore_rest\n     Ignores the rest of the labeled arguments following this flag.\n\n"
                 "   --version\n     Displays version information and exits.\n\n"
                 "   -h,  --help\n     Displays usage information and exits.\n\n"
                 "   <fasta files with genomes>  (accepted multiple times)\n     (required)  FASTA file(s) with nucleotide sequences.\n\n\n"
                 "   SibeliaZ-LCB, a program for construction of locally-collinear blocks from\n   complete genomes (MI355X build)\n" << std::endl;
}

Args parse(int argc, char** argv)
{
    Args a;
    bool rest = false, haveGraph = false;
    for (int i = 1; i < argc; i++) {
        std::string s = argv[i];
        if (rest || s.empty() || s[0] != '-' || s == "-") { a.fasta.push_back(s); continue; }
        if (s == "--" || s == "--ignore_rest") { rest = true; continue; }
        if (s == "-h" || s == "--help") { usage(); exit(0); }
        if (s == "--version") { std::cout << "\nsibeliaz-lcb  version: 1.2.7 (" << lcb_version() << ")\n" << std::endl; exit(0); }
        if (s == "--noseq") { a.noSeq = true; continue; }
        std::string flag = s, val;
        bool hasVal = false;
        const size_t eq = s.find('=');
        if (eq != std::string::npos) { flag = s.substr(0, eq); val = s.substr(eq + 1); hasVal = true; }
        auto value = [&]() -> const char* {
            if (hasVal) return val.c_str();
            if (i + 1 >= argc) parseError(flag, "Missing a value for this argument!");
            return argv[++i];
        };
        if (flag == "-k" || flag == "--kvalue") {
            a.k = toUnsigned(flag, value());
            if (a.k % 2 != 1) parseError("-k (--kvalue)", "Value '" + std::to_string(a.k) + "' does not meet constraint: value of K must be odd");
        } else if (flag == "-b" || flag == "--branchsize") a.b = toUnsigned(flag, value());
        else if (flag == "-m" || flag == "--blocksize") a.m = toUnsigned(flag, value());
        else if (flag == "-t" || flag == "--threads") a.t = toUnsigned(flag, value());
        else if (flag == "-a" || flag == "--abundance") a.a = toUnsigned(flag, value());
        else if (flag == "--chunks") a.chunks = toUnsigned(flag, value());
        else if (flag == "--graph") { a.graph = value(); haveGraph = true; }
        else if (flag == "-o" || flag == "--outdir") a.outDir = value();
        else parseError(s, "Couldn't find match for argument");
    }
    if (!haveGraph) parseError("(--graph)", "Required argument missing: graph");
    if (a.fasta.empty()) parseError("(--filenames)", "Required argument missing: filenames");
    return a;
}

// An environment variable's value; unset and empty are the same: null.
const char* env(const char* name)
{
    const char* v = getenv(name);
    return v && *v ? v : nullptr;
}
int deviceOrdinal() { return env("LCB_DEVICE") ? atoi(env("LCB_DEVICE")) : 0; }
int gpuCount() { return env("LCB_GPUS") ? atoi(env("LCB_GPUS")) : 1; }

// One switch of the environment with two values: `def` (also when unset or empty) and `other`.
struct Route {
    bool other = false;       // it says `other`
    std::string error;        // it says something else: the line to refuse it with
};
Route route(const char* name, const char* def, const char* other)
{
    Route r;
    const std::string v = env(name) ? env(name) : def;
    r.other = v == other;
    if (!r.other && v != def) r.error = std::string("error: ") + name + " is '" + v + "': it is " + def + " (the default) or " + other;
    return r;
}

// How graph and device come to be. A new way is a value here, a line in the choice and a case in the switch of main().
enum Opening {
    OPEN_LOAD,          // lcb_graph_load: the junction file of --graph, read on host threads
    OPEN_GRAPH_BUILD,   // lcb_graph_build (LCB_JUNCTIONS=device): the junctions come from the FASTA files on the GPU, the graph is a host object
    OPEN_FASTA,         // lcb_open_fasta (+ LCB_HANDOVER=device): the same, and the graph's arrays stay in HBM as the device's tables
    OPEN_JUNCTIONS      // lcb_open_junctions (LCB_LOAD=device): the junction file goes up as it is, graph and device come from one call
};

// LCB_VERBOSE: what the two one-call routes report alike, in front of and behind the times that are their own
void openCounts(const lcb_open_stats& os)
{
    std::cerr << " raw=" << os.graph.raw_occurrences << " kept=" << os.graph.kept_occurrences << " vertices=" << os.graph.vertices << " patched=" << os.graph.patched
              << " download_bytes=" << os.graph.download_bytes << " upload_bytes=" << os.tables.upload_bytes << " csr_download_bytes=" << os.csr_download_bytes
              << " peak_device_bytes=" << os.peak_device_bytes;
}
void openTimes(const lcb_open_stats& os)
{
    std::cerr << " compact_ms=" << os.graph.compact_ms << " place_ms=" << os.place_ms << " download_ms=" << os.graph.download_ms << " patch_ms=" << os.patch_ms
              << " window_ms=" << os.tables.window_ms << " csr_ms=" << os.tables.csr_ms << " sort_ms=" << os.tables.sort_ms << " csr_download_ms=" << os.csr_download_ms
              << " gather_ms=" << os.tables.gather_ms << std::endl;
}

}  // namespace

int main(int argc, char** argv)
{
    const Args a = parse(argc, argv);
    // The routes are chosen like the GPU, from the environment, and what is wrong with them is said before anything is loaded: the
    // first line of this list whose condition holds (the order is part of the tool's behaviour).
    const Route seedsRoute = route("LCB_SEEDS", "host", "device"), tablesRoute = route("LCB_TABLES", "host", "device"), junctionsRoute = route("LCB_JUNCTIONS", "file", "device"),
                handoverRoute = route("LCB_HANDOVER", "host", "device"), loadRoute = route("LCB_LOAD", "host", "device");
    const bool tablesHost = env("LCB_TABLES") && !tablesRoute.other;      // said, not defaulted
    const int nGpus = gpuCount();
    const std::string gpus = std::string("LCB_GPUS=") + (env("LCB_GPUS") ? env("LCB_GPUS") : "");
    const std::pair<bool, std::string> refusals[] = {
        {!seedsRoute.error.empty(), seedsRoute.error},
        {!tablesRoute.error.empty(), tablesRoute.error},
        {!junctionsRoute.error.empty(), junctionsRoute.error},
        {tablesRoute.other && nGpus > 1, "error: LCB_TABLES=device together with " + gpus + " is not supported: the tables are built on the device of a single-GPU run (LCB_GPUS unset or 1)"},
        {!handoverRoute.error.empty(), handoverRoute.error},
        {handoverRoute.other && !junctionsRoute.other, "error: LCB_HANDOVER=device requires LCB_JUNCTIONS=device: it is the graph built on the device that is handed over"},
        {handoverRoute.other && tablesHost, "error: LCB_HANDOVER=device together with LCB_TABLES=host is not supported: the tables of a handed-over graph are built on the device (LCB_TABLES unset or device)"},
        {handoverRoute.other && nGpus > 1, "error: LCB_HANDOVER=device together with " + gpus + " is not supported: the graph is handed over to the device of a single-GPU run (LCB_GPUS unset or 1)"},
        {!loadRoute.error.empty(), loadRoute.error},
        {loadRoute.other && junctionsRoute.other, "error: LCB_LOAD=device together with LCB_JUNCTIONS=device is not supported: there is no file to load (the junctions come from the FASTA files)"},
        {loadRoute.other && tablesHost, "error: LCB_LOAD=device together with LCB_TABLES=host is not supported: the tables of a graph opened on the device are built there (LCB_TABLES unset or device)"},
        {loadRoute.other && nGpus > 1, "error: LCB_LOAD=device together with " + gpus + " is not supported: the file is opened on the device of a single-GPU run (LCB_GPUS unset or 1)"},
    };
    for (const auto& r : refusals)
        if (r.first) { std::cerr << r.second << std::endl; return 1; }
    const bool deviceSeeds = seedsRoute.other, deviceTables = tablesRoute.other;
    const Opening opening = handoverRoute.other ? OPEN_FASTA : junctionsRoute.other ? OPEN_GRAPH_BUILD : loadRoute.other ? OPEN_JUNCTIONS : OPEN_LOAD;
    lcb_graph* g = nullptr;
    lcb_device* dev = nullptr;
    lcb_gpus* set = nullptr;
    lcb_seed* seeds = nullptr;
    lcb_block* blocks = nullptr;
    int rc = 0;
    auto fail = [&]() { std::cerr << "error: " << lcb_last_error() << std::endl; rc = 1; };   // sibeliaz.cpp:150-154
    do {
        std::cout << "Loading the graph..." << std::endl;                                      // sibeliaz.cpp:124
        std::vector<const char*> fa;
        for (auto& f : a.fasta) fa.push_back(f.c_str());
        const int nFa = (int)fa.size(), k = (int)a.k, abundance = (int)a.a, threads = (int)a.t;
        lcb_params p;
        p.k = (int)a.k; p.min_block = (int)a.m; p.max_branch = (int)a.b; p.max_flank = (int)a.b;   // sibeliaz.cpp:133-138
        p.looking_depth = 8; p.phase_size = 256;
        const bool verbose = getenv("LCB_VERBOSE") != nullptr;
        lcb_open_stats os;
        lcb_graph_build_stats gs;
        bool opened = false;
        switch (opening) {
        case OPEN_LOAD:
            g = lcb_graph_load(a.graph.c_str(), fa.data(), nFa, k, abundance, threads);
            opened = g != nullptr;
            break;
        case OPEN_GRAPH_BUILD:
            // on LCB_DEVICE (device 0 of an LCB_GPUS=N set); the graph is a host object and the build has released the device when it returns
            g = lcb_graph_build(fa.data(), nFa, k, abundance, threads, nGpus > 1 ? 0 : deviceOrdinal(), nullptr, &gs);
            opened = g != nullptr;
            if (opened && verbose)
                std::cerr << "lcb: graph=device records=" << gs.junctions.base.records << " raw=" << gs.raw_occurrences << " kept=" << gs.kept_occurrences << " vertices=" << gs.vertices
                          << " patched=" << gs.patched << " partitions=" << gs.junctions.partitions << " download_bytes=" << gs.download_bytes << " peak_device_bytes="
                          << gs.peak_device_bytes << " parse_ms=" << gs.parse_ms << " upload_ms=" << gs.junctions.base.upload_ms << " insert_ms=" << gs.junctions.base.insert_ms
                          << " mark_ms=" << gs.junctions.mark_ms << " count_ms=" << gs.count_ms << " emit_ms=" << gs.junctions.base.emit_ms << " take_ms=" << gs.take_ms
                          << " abundance_ms=" << gs.abundance_ms << " compact_ms=" << gs.compact_ms << " download_ms=" << gs.download_ms << " csr_ms=" << gs.csr_ms << std::endl;
            break;
        case OPEN_FASTA:
            // graph and device in one call, on LCB_DEVICE: the device exists from here on, createDevices below finds it made
            opened = lcb_open_fasta(fa.data(), nFa, k, abundance, threads, &p, deviceOrdinal(), nullptr, nullptr, &g, &dev, &os) == LCB_OK;
            if (opened && verbose) {
                std::cerr << "lcb: handover=device records=" << os.graph.junctions.base.records;
                openCounts(os);
                std::cerr << " parse_ms=" << os.graph.parse_ms;
                openTimes(os);
            }
            break;
        case OPEN_JUNCTIONS:
            // the junction file, opened on LCB_DEVICE: graph and device in one call, as with LCB_HANDOVER=device
            opened = lcb_open_junctions(a.graph.c_str(), fa.data(), nFa, k, abundance, threads, &p, deviceOrdinal(), nullptr, nullptr, &g, &dev, &os) == LCB_OK;
            if (opened && verbose) {
                std::cerr << "lcb: load=device chromosomes=" << os.graph.junctions.base.records << " tiles=" << os.graph.junctions.base.tiles;
                openCounts(os);
                std::cerr << " read_ms=" << os.graph.junctions.base.read_ms << " upload_ms=" << os.graph.junctions.base.upload_ms << " take_ms=" << os.graph.take_ms
                          << " parse_ms=" << os.graph.parse_ms << " abundance_ms=" << os.graph.abundance_ms;
                openTimes(os);
            }
            break;
        }
        if (!opened) { fail(); break; }
        std::cout << "Analyzing the graph..." << std::endl;                                    // sibeliaz.cpp:132
        // GPU selection comes from the environment, never from argv (the wrapper's command line, sibeliaz:146, stays as it is):
        // LCB_GPUS=N uses HIP devices 0..N-1 (as filtered by HIP_VISIBLE_DEVICES), LCB_DEVICE=i uses device i; default one GPU.
        // So does the seed route: LCB_SEEDS=host (default) enumerates with -t host threads before the device exists, LCB_SEEDS=device
        // creates the device first and enumerates on its tables (with LCB_GPUS=N on device 0 of the set).
        auto createDevices = [&]() -> bool {
            if (dev) return true;             // (LCB_HANDOVER=device: made with the graph)
            if (nGpus > 1) {
                std::vector<int> ord;
                for (int i = 0; i < nGpus; i++) ord.push_back(i);
                // the same handle bench.py --gpus N times: devices + tables + RCCL once, then one pass
                set = lcb_gpus_create(g, ord.data(), nGpus, &p, nullptr, 0);
                return set != nullptr;
            }
            lcb_table_stats ts;
            dev = lcb_device_create_tables(g, &p, deviceOrdinal(), nullptr, deviceTables ? LCB_TABLES_DEVICE : LCB_TABLES_HOST, &ts);
            if (dev && getenv("LCB_VERBOSE"))
                std::cerr << "lcb: device tables=" << (deviceTables ? "device" : "host") << " positions=" << ts.positions << " vertices=" << ts.vertices << " sort_passes=" << ts.sort_passes << " (+"
                          << ts.sort_passes_skipped << " skipped) upload_bytes=" << ts.upload_bytes << " device_bytes=" << ts.device_bytes << " upload_ms=" << ts.upload_ms
                          << " window_ms=" << ts.window_ms << " csr_ms=" << ts.csr_ms << " sort_ms=" << ts.sort_ms << " gather_ms=" << ts.gather_ms << std::endl;
            return dev != nullptr;
        };
        int64_t nSeeds = -1;
        if (deviceSeeds) {
            if (!createDevices()) { fail(); break; }
            lcb_device* d0 = nGpus > 1 ? lcb_gpus_device(set, 0) : dev;
            if (!d0) { fail(); break; }
            lcb_seed_stats ss;
            nSeeds = lcb_device_enumerate_seeds(d0, &seeds, &ss);
            if (nSeeds >= 0 && getenv("LCB_VERBOSE"))
                std::cerr << "lcb: device seeds=" << ss.seeds << " vertices=" << ss.vertices << " max_count=" << ss.max_count << " sort_passes=" << ss.sort_passes << " (+"
                          << ss.sort_passes_skipped << " skipped) device_bytes=" << ss.device_bytes << " count_ms=" << ss.count_ms << " fill_ms=" << ss.fill_ms
                          << " sort_ms=" << ss.sort_ms << " copy_ms=" << ss.copy_ms << std::endl;
        } else
            nSeeds = lcb_enumerate_seeds(g, (int)a.t, &seeds);
        if (nSeeds < 0) { fail(); break; }
        if (!deviceSeeds && !createDevices()) { fail(); break; }
        int64_t nBlocks = 0;
        lcb_stats st;
        if (nGpus > 1) {
            lcb_hooks hk;
            memset(&hk, 0, sizeof(hk));
            hk.abi = LCB_ABI_VERSION; hk.world = 1; hk.progress = 1;
            const int rc = lcb_gpus_find_blocks(set, seeds, nSeeds, &hk, &blocks, &nBlocks, &st);
            lcb_gpus_destroy(set);
            set = nullptr;
            if (rc != LCB_OK) { fail(); break; }
        } else {
            if (lcb_find_blocks(g, dev, &p, seeds, nSeeds, 1, &blocks, &nBlocks, &st) != LCB_OK) { fail(); break; }
        }
        if (getenv("LCB_VERBOSE"))
            std::cerr << "lcb: seeds=" << st.seeds << " blocks=" << st.blocks_found << " conflicts=" << st.failures << " launches=" << st.launches
                      << " big_retries=" << st.big_retries << " kernel_ms=" << st.kernel_ms << " loop_ms=" << st.wall_ms << " | rounds=" << st.rounds
                      << " job_launches=" << st.recompute_launches << " (" << st.conflict_launches << " at a conflict) jobs=" << st.recomputed_seeds << " used="
                      << st.jobs_used << " views=" << st.views_built << " over_predicted=" << st.over_predicted << " process_ms=" << st.process_ms << " plan_ms=" << st.plan_ms << std::endl;
        std::cout << "Generating the output..." << std::endl;                                  // sibeliaz.cpp:142
        // Blocks found / Coverage are printed by GenerateOutput before the files are written (blocksfinder.h:658-661);
        // the counts are only known after trimming, which lcb_generate_output does, so print right after it.
        int64_t nTrimmed = 0;
        double coverage = 0;
        const int orc = lcb_generate_output(g, a.m, blocks, nBlocks, st.blocks_found, a.outDir.c_str(), a.noSeq ? 0 : 1, a.chunks, &nTrimmed, &coverage);
        char buf[64];
        snprintf(buf, sizeof(buf), "%.2f", coverage);
        if (orc != LCB_OK) { fail(); break; }
        std::cout << "Blocks found: " << nTrimmed << std::endl << "Coverage: " << buf << std::endl;
    } while (false);
    lcb_free(blocks);
    lcb_free(seeds);
    lcb_gpus_destroy(set);
    lcb_device_destroy(dev);
    lcb_graph_free(g);
    return rc;
}
