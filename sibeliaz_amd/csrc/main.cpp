// main.cpp — `sibeliaz-lcb`: drop-in replacement of the reference executable (sibeliaz.cpp:37-157).
//
// Same flags, defaults, stdout banners, output files and exit codes, so line 146 of the reference's
// `sibeliaz` wrapper script keeps working verbatim:
//   sibeliaz-lcb --graph <junctions> <fasta...> -k <odd> -b <int> -o <dir> -m <int> -t <int> --abundance <int> [--noseq] --chunks <int>
// `-t` stays "host threads" (loading, seed enumeration); the GPU is chosen by the environment
// (LCB_DEVICE, default 0; HIP_VISIBLE_DEVICES also applies), never by a new flag, and so are the place where the seeds are
// enumerated (LCB_SEEDS=host, the default, or device), the place where the device's tables are computed (LCB_TABLES=host, the
// default, or device) and the way to the graph (LCB_JUNCTIONS=file, the default: the junction file of --graph; or device: the
// junctions come from the FASTA arguments on the GPU, --graph is still required by the parser but never opened) and the way the graph
// reaches the device (LCB_HANDOVER=host, the default: the graph build releases the GPU and the device uploads its tables; or device,
// which needs LCB_JUNCTIONS=device and one GPU: lcb_open_fasta, the graph's arrays stay in HBM and become the device's tables) and the
// place where the junction file is read (LCB_LOAD=host, the default: lcb_graph_load on host threads; or device, which needs
// LCB_JUNCTIONS=file and one GPU: lcb_open_junctions, the file goes up as it is and graph and device come from one call).
// The block finder itself runs on the MI355X through the C ABI in include/lcb.h.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <string>
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

}  // namespace

int main(int argc, char** argv)
{
    const Args a = parse(argc, argv);
    // where the seeds are enumerated: chosen like the GPU, from the environment; refused before anything is loaded
    const char* seedsEnv = getenv("LCB_SEEDS");
    const std::string seedRoute = seedsEnv && *seedsEnv ? seedsEnv : "host";
    if (seedRoute != "host" && seedRoute != "device") {
        std::cerr << "error: LCB_SEEDS is '" << seedRoute << "': it is host (the default) or device" << std::endl;
        return 1;
    }
    const bool deviceSeeds = seedRoute == "device";
    // ... and where the device's tables are computed (LCB_TABLES=host, the default, or device), the same way
    const char* tablesEnv = getenv("LCB_TABLES");
    const std::string tableRoute = tablesEnv && *tablesEnv ? tablesEnv : "host";
    if (tableRoute != "host" && tableRoute != "device") {
        std::cerr << "error: LCB_TABLES is '" << tableRoute << "': it is host (the default) or device" << std::endl;
        return 1;
    }
    const bool deviceTables = tableRoute == "device";
    // ... and the way to the graph (LCB_JUNCTIONS=file, the default, or device)
    const char* junctionsEnv = getenv("LCB_JUNCTIONS");
    const std::string junctionRoute = junctionsEnv && *junctionsEnv ? junctionsEnv : "file";
    if (junctionRoute != "file" && junctionRoute != "device") {
        std::cerr << "error: LCB_JUNCTIONS is '" << junctionRoute << "': it is file (the default) or device" << std::endl;
        return 1;
    }
    const bool deviceJunctions = junctionRoute == "device";
    {
        const char* gpus = getenv("LCB_GPUS");
        if (deviceTables && gpus && *gpus && atoi(gpus) > 1) {
            std::cerr << "error: LCB_TABLES=device together with LCB_GPUS=" << gpus << " is not supported: the tables are built on the device of a single-GPU run (LCB_GPUS unset or 1)" << std::endl;
            return 1;
        }
    }
    // ... and the way the graph reaches the device (LCB_HANDOVER=host, the default, or device: one call from the FASTA files to graph and device)
    const char* handoverEnv = getenv("LCB_HANDOVER");
    const std::string handoverRoute = handoverEnv && *handoverEnv ? handoverEnv : "host";
    if (handoverRoute != "host" && handoverRoute != "device") {
        std::cerr << "error: LCB_HANDOVER is '" << handoverRoute << "': it is host (the default) or device" << std::endl;
        return 1;
    }
    const bool deviceHandover = handoverRoute == "device";
    if (deviceHandover) {
        const char* gpus = getenv("LCB_GPUS");
        if (!deviceJunctions) {
            std::cerr << "error: LCB_HANDOVER=device requires LCB_JUNCTIONS=device: it is the graph built on the device that is handed over" << std::endl;
            return 1;
        }
        if (tablesEnv && *tablesEnv && !deviceTables) {
            std::cerr << "error: LCB_HANDOVER=device together with LCB_TABLES=host is not supported: the tables of a handed-over graph are built on the device (LCB_TABLES unset or device)" << std::endl;
            return 1;
        }
        if (gpus && *gpus && atoi(gpus) > 1) {
            std::cerr << "error: LCB_HANDOVER=device together with LCB_GPUS=" << gpus << " is not supported: the graph is handed over to the device of a single-GPU run (LCB_GPUS unset or 1)" << std::endl;
            return 1;
        }
    }
    // ... and where the junction file of --graph is read (LCB_LOAD=host, the default, or device: one call from the file to graph and device)
    const char* loadEnv = getenv("LCB_LOAD");
    const std::string loadRoute = loadEnv && *loadEnv ? loadEnv : "host";
    if (loadRoute != "host" && loadRoute != "device") {
        std::cerr << "error: LCB_LOAD is '" << loadRoute << "': it is host (the default) or device" << std::endl;
        return 1;
    }
    const bool deviceLoad = loadRoute == "device";
    if (deviceLoad) {
        const char* gpus = getenv("LCB_GPUS");
        if (deviceJunctions) {
            std::cerr << "error: LCB_LOAD=device together with LCB_JUNCTIONS=device is not supported: there is no file to load (the junctions come from the FASTA files)" << std::endl;
            return 1;
        }
        if (tablesEnv && *tablesEnv && !deviceTables) {
            std::cerr << "error: LCB_LOAD=device together with LCB_TABLES=host is not supported: the tables of a graph opened on the device are built there (LCB_TABLES unset or device)" << std::endl;
            return 1;
        }
        if (gpus && *gpus && atoi(gpus) > 1) {
            std::cerr << "error: LCB_LOAD=device together with LCB_GPUS=" << gpus << " is not supported: the file is opened on the device of a single-GPU run (LCB_GPUS unset or 1)" << std::endl;
            return 1;
        }
    }
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
        lcb_params p;
        p.k = (int)a.k; p.min_block = (int)a.m; p.max_branch = (int)a.b; p.max_flank = (int)a.b;   // sibeliaz.cpp:133-138
        p.looking_depth = 8; p.phase_size = 256;
        if (deviceHandover) {
            // graph and device in one call, on LCB_DEVICE: the device exists from here on, createDevices below finds it made
            const char* ordEnv = getenv("LCB_DEVICE");
            lcb_open_stats os;
            if (lcb_open_fasta(fa.data(), (int)fa.size(), (int)a.k, (int)a.a, (int)a.t, &p, ordEnv && *ordEnv ? atoi(ordEnv) : 0, nullptr, nullptr, &g, &dev, &os) != LCB_OK) { fail(); break; }
            if (getenv("LCB_VERBOSE"))
                std::cerr << "lcb: handover=device records=" << os.graph.junctions.base.records << " raw=" << os.graph.raw_occurrences << " kept=" << os.graph.kept_occurrences
                          << " vertices=" << os.graph.vertices << " patched=" << os.graph.patched << " download_bytes=" << os.graph.download_bytes << " upload_bytes=" << os.tables.upload_bytes
                          << " csr_download_bytes=" << os.csr_download_bytes << " peak_device_bytes=" << os.peak_device_bytes << " parse_ms=" << os.graph.parse_ms
                          << " compact_ms=" << os.graph.compact_ms << " place_ms=" << os.place_ms << " download_ms=" << os.graph.download_ms << " patch_ms=" << os.patch_ms
                          << " window_ms=" << os.tables.window_ms << " csr_ms=" << os.tables.csr_ms << " sort_ms=" << os.tables.sort_ms << " csr_download_ms=" << os.csr_download_ms
                          << " gather_ms=" << os.tables.gather_ms << std::endl;
        } else if (deviceJunctions) {
            // on LCB_DEVICE (device 0 of an LCB_GPUS=N set); the graph is a host object and the build has released the device when it returns
            const char* ordEnv = getenv("LCB_DEVICE");
            const char* setEnv = getenv("LCB_GPUS");
            const bool several = setEnv && *setEnv && atoi(setEnv) > 1;
            lcb_graph_build_stats gs;
            g = lcb_graph_build(fa.data(), (int)fa.size(), (int)a.k, (int)a.a, (int)a.t, !several && ordEnv && *ordEnv ? atoi(ordEnv) : 0, nullptr, &gs);
            if (g && getenv("LCB_VERBOSE"))
                std::cerr << "lcb: graph=device records=" << gs.junctions.base.records << " raw=" << gs.raw_occurrences << " kept=" << gs.kept_occurrences << " vertices=" << gs.vertices
                          << " patched=" << gs.patched << " partitions=" << gs.junctions.partitions << " download_bytes=" << gs.download_bytes << " peak_device_bytes="
                          << gs.peak_device_bytes << " parse_ms=" << gs.parse_ms << " upload_ms=" << gs.junctions.base.upload_ms << " insert_ms=" << gs.junctions.base.insert_ms
                          << " mark_ms=" << gs.junctions.mark_ms << " count_ms=" << gs.count_ms << " emit_ms=" << gs.junctions.base.emit_ms << " take_ms=" << gs.take_ms
                          << " abundance_ms=" << gs.abundance_ms << " compact_ms=" << gs.compact_ms << " download_ms=" << gs.download_ms << " csr_ms=" << gs.csr_ms << std::endl;
        } else if (deviceLoad) {
            // the junction file, opened on LCB_DEVICE: graph and device in one call, as with LCB_HANDOVER=device
            const char* ordEnv = getenv("LCB_DEVICE");
            lcb_open_stats os;
            if (lcb_open_junctions(a.graph.c_str(), fa.data(), (int)fa.size(), (int)a.k, (int)a.a, (int)a.t, &p, ordEnv && *ordEnv ? atoi(ordEnv) : 0, nullptr, nullptr, &g, &dev, &os) != LCB_OK) { fail(); break; }
            if (getenv("LCB_VERBOSE"))
                std::cerr << "lcb: load=device chromosomes=" << os.graph.junctions.base.records << " tiles=" << os.graph.junctions.base.tiles << " raw=" << os.graph.raw_occurrences
                          << " kept=" << os.graph.kept_occurrences << " vertices=" << os.graph.vertices << " patched=" << os.graph.patched << " download_bytes=" << os.graph.download_bytes
                          << " upload_bytes=" << os.tables.upload_bytes << " csr_download_bytes=" << os.csr_download_bytes << " peak_device_bytes=" << os.peak_device_bytes
                          << " read_ms=" << os.graph.junctions.base.read_ms << " upload_ms=" << os.graph.junctions.base.upload_ms << " take_ms=" << os.graph.take_ms
                          << " parse_ms=" << os.graph.parse_ms << " abundance_ms=" << os.graph.abundance_ms << " compact_ms=" << os.graph.compact_ms << " place_ms=" << os.place_ms
                          << " download_ms=" << os.graph.download_ms << " patch_ms=" << os.patch_ms << " window_ms=" << os.tables.window_ms << " csr_ms=" << os.tables.csr_ms
                          << " sort_ms=" << os.tables.sort_ms << " csr_download_ms=" << os.csr_download_ms << " gather_ms=" << os.tables.gather_ms << std::endl;
        } else
            g = lcb_graph_load(a.graph.c_str(), fa.data(), (int)fa.size(), (int)a.k, (int)a.a, (int)a.t);
        if (!g) { fail(); break; }
        std::cout << "Analyzing the graph..." << std::endl;                                    // sibeliaz.cpp:132
        // GPU selection comes from the environment, never from argv (the wrapper's command line, sibeliaz:146, stays as it is):
        // LCB_GPUS=N uses HIP devices 0..N-1 (as filtered by HIP_VISIBLE_DEVICES), LCB_DEVICE=i uses device i; default one GPU.
        // So does the seed route: LCB_SEEDS=host (default) enumerates with -t host threads before the device exists, LCB_SEEDS=device
        // creates the device first and enumerates on its tables (with LCB_GPUS=N on device 0 of the set).
        const char* devEnv = getenv("LCB_DEVICE");
        const char* gpusEnv = getenv("LCB_GPUS");
        const int nGpus = gpusEnv && *gpusEnv ? atoi(gpusEnv) : 1;
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
            dev = lcb_device_create_tables(g, &p, devEnv && *devEnv ? atoi(devEnv) : 0, nullptr, deviceTables ? LCB_TABLES_DEVICE : LCB_TABLES_HOST, &ts);
            if (dev && getenv("LCB_VERBOSE"))
                std::cerr << "lcb: device tables=" << tableRoute << " positions=" << ts.positions << " vertices=" << ts.vertices << " sort_passes=" << ts.sort_passes << " (+"
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
