// TEST-ONLY: the argument checks of the five calls that open a graph or a device (capi.cpp), driven from a program of its own so that
// they can run under -fsanitize=address,undefined (`make -C tests/emu build_san/capi_args`, then run it: no GPU, no preloading). Every
// call here is refused before a device is looked for; the program prints each refusal and fails if a call succeeded or said nothing.
#include <cstdio>
#include <cstring>
#include <string>

#include "lcb.h"

static int bad = 0;

static void refused(const char* what, bool failed)
{
    const char* msg = lcb_last_error();
    printf("%-52s %s\n", what, failed ? msg : "NOT REFUSED");
    if (!failed || !*msg) bad++;
}

int main(int, char** argv)
{
    const std::string self = argv[0], missing = self + ".no-such-file";     // a file that exists (this program) and one that does not
    const char* one[] = {self.c_str()};
    const char* withNull[] = {self.c_str(), nullptr};
    const char* withMissing[] = {self.c_str(), missing.c_str()};
    lcb_params p = {15, 50, 200, 200, 8, 256}, deep = {15, 50, 65000, 200, 8, 256};
    lcb_junction_opts_ex jo;
    memset(&jo, 0, sizeof(jo));
    jo.abi = LCB_ABI_VERSION - 1;
    lcb_device_opts dopts;
    memset(&dopts, 0, sizeof(dopts));
    dopts.abi = LCB_ABI_VERSION + 1;
    lcb_graph* g = nullptr;
    lcb_device* d = nullptr;
    const char* out = "/dev/null";

    struct { const char* name; const char* const* fa; int n; int k; const lcb_junction_opts_ex* jo; } cases[] = {
        {"null list", nullptr, 1, 15, nullptr}, {"n = 0", one, 0, 15, nullptr}, {"even k", one, 1, 16, nullptr}, {"k = 0", one, 1, 0, nullptr},
        {"wrong abi", one, 1, 15, &jo}, {"null path", withNull, 2, 15, nullptr}, {"missing file", withMissing, 2, 15, nullptr}};
    for (const auto& c : cases) {
        const std::string n = c.name;
        refused(("lcb_junctions_build_ex: " + n).c_str(), lcb_junctions_build_ex(c.fa, c.n, c.k, 0, c.jo, out, nullptr) != LCB_OK);
        if (n != "missing file")       // (lcb_graph_build leaves the files to the parser, behind the device check)
            refused(("lcb_graph_build: " + n).c_str(), lcb_graph_build(c.fa, c.n, c.k, 150, 1, 0, c.jo, nullptr) == nullptr);
        refused(("lcb_open_fasta: " + n).c_str(), lcb_open_fasta(c.fa, c.n, c.k, 150, 1, &p, 0, c.jo, nullptr, &g, &d, nullptr) != LCB_OK && !g && !d);
        refused(("lcb_graph_load_device: " + n).c_str(), lcb_graph_load_device(self.c_str(), c.fa, c.n, c.k, 150, 1, 0, c.jo, nullptr) == nullptr);
        refused(("lcb_open_junctions: " + n).c_str(), lcb_open_junctions(self.c_str(), c.fa, c.n, c.k, 150, 1, &p, 0, c.jo, nullptr, &g, &d, nullptr) != LCB_OK && !g && !d);
    }
    refused("lcb_junctions_build_ex: no output file", lcb_junctions_build_ex(one, 1, 15, 0, nullptr, nullptr, nullptr) != LCB_OK);
    refused("lcb_graph_load_device: null junction file", lcb_graph_load_device(nullptr, one, 1, 15, 150, 1, 0, nullptr, nullptr) == nullptr);
    refused("lcb_graph_load_device: missing junction file", lcb_graph_load_device(missing.c_str(), one, 1, 15, 150, 1, 0, nullptr, nullptr) == nullptr);
    refused("lcb_open_junctions: missing junction file", lcb_open_junctions(missing.c_str(), one, 1, 15, 150, 1, &p, 0, nullptr, nullptr, &g, &d, nullptr) != LCB_OK);
    refused("lcb_open_fasta: null outputs", lcb_open_fasta(one, 1, 15, 150, 1, &p, 0, nullptr, nullptr, nullptr, nullptr, nullptr) != LCB_OK);
    refused("lcb_open_fasta: null params", lcb_open_fasta(one, 1, 15, 150, 1, nullptr, 0, nullptr, nullptr, &g, &d, nullptr) != LCB_OK);
    refused("lcb_open_junctions: null outputs", lcb_open_junctions(self.c_str(), one, 1, 15, 150, 1, &p, 0, nullptr, nullptr, nullptr, nullptr, nullptr) != LCB_OK);
    refused("lcb_open_fasta: device opts of another abi", lcb_open_fasta(one, 1, 15, 150, 1, &p, 0, nullptr, &dopts, &g, &d, nullptr) != LCB_OK);
    refused("lcb_open_junctions: device opts of another abi", lcb_open_junctions(self.c_str(), one, 1, 15, 150, 1, &p, 0, nullptr, &dopts, &g, &d, nullptr) != LCB_OK);
    refused("lcb_open_fasta: maxBranchSize 65000", lcb_open_fasta(one, 1, 15, 150, 1, &deep, 0, nullptr, nullptr, &g, &d, nullptr) != LCB_OK);
    refused("lcb_open_junctions: maxBranchSize 65000", lcb_open_junctions(self.c_str(), one, 1, 15, 150, 1, &deep, 0, nullptr, nullptr, &g, &d, nullptr) != LCB_OK);
    printf("%s\n", bad ? "FAILED" : "every call was refused with a message");
    return bad ? 1 : 0;
}
