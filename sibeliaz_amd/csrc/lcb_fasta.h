// lcb_fasta.h — the FASTA reader of the junction finders (tools/mkgraph.cpp on the CPU, junctions.hip on the GPU): both must
// see the same records, so there is one reader. Name = first token of the header; whitespace is dropped, everything is
// upper-cased; what is not ACGT stays in the sequence (it breaks k-mer windows). Files are appended to `out` in call order.
#ifndef LCB_FASTA_H
#define LCB_FASTA_H

#include <cctype>
#include <cstdio>
#include <stdexcept>
#include <string>
#include <vector>

namespace lcb_fasta {

struct Record { std::string name; std::string seq; };

inline void readFasta(const std::string& file, std::vector<Record>& out) {
    FILE* f = fopen(file.c_str(), "rb");
    if (!f) throw std::runtime_error("cannot open " + file);
    std::vector<char> buf(1 << 20);
    bool inHeader = false;
    std::string header;
    size_t n;
    while ((n = fread(buf.data(), 1, buf.size(), f)) > 0) {
        for (size_t i = 0; i < n; i++) {
            char c = buf[i];
            if (inHeader) {
                if (c == '\n') {
                    inHeader = false;
                    size_t e = 0;
                    while (e < header.size() && !isspace((unsigned char)header[e])) e++;
                    out.push_back({header.substr(0, e), std::string()});
                } else header.push_back(c);
            } else if (c == '>') { inHeader = true; header.clear(); }
            else if (!isspace((unsigned char)c) && !out.empty()) out.back().seq.push_back((char)toupper((unsigned char)c));
        }
    }
    fclose(f);
}

inline int code(char c) {
    switch (c) { case 'A': return 0; case 'C': return 1; case 'G': return 2; case 'T': return 3; }
    return -1;
}

}  // namespace lcb_fasta
#endif
