// bdx-sites-check FILE MASKS NAME...: FILE through the --sites parser (sites.cpp) against the sequence names NAME..., with the type masks
// MASKS = "DEL=4,INS=8,INV=34,ITX=16,CTX=256" (a type left out or 0: no read class maps to it).  Prints one line per kept site --
// "k chr1 pos1 chr2 pos2 type size|. tid1 pos1 tid2 pos2 mask" -- then "unknown <lines>"; a parser error goes to stderr with exit 1.
// Test tooling for sites.cpp: it links nothing else, so that the parser can be built and run under a sanitizer on its own.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <exception>
#include <string>
#include <utility>
#include <vector>

#include "sites.h"

int main(int argc, char** argv) {
    if (argc < 3) {
        fprintf(stderr, "usage: bdx-sites-check FILE MASKS NAME...\n");
        return 2;
    }
    std::vector<std::pair<std::string, uint32_t>> masks;
    const std::string m(argv[2]);
    for (size_t i = 0; i < m.size();) {
        const size_t j = m.find(',', i), e = std::min(j, m.size());
        const size_t q = m.find('=', i);
        if (q != std::string::npos && q < e) masks.emplace_back(m.substr(i, q - i), (uint32_t)strtoul(m.substr(q + 1, e - q - 1).c_str(), nullptr, 10));
        i = e + 1;
    }
    std::vector<std::string> names(argv + 3, argv + argc);
    bdhost::SiteTable t;
    try {
        bdhost::read_sites(argv[1], names, masks, t);
    } catch (std::exception const& ex) {
        fprintf(stderr, "ERROR: %s\n", ex.what());
        return 1;
    }
    for (size_t k = 0; k < t.sites.size(); ++k) {
        const bdhost::SiteLine& s = t.sites[k];
        printf("%zu %d %d %d %d %s %s %d %d %d %d %u\n", k + 1, s.chr1, s.pos1, s.chr2, s.pos2, s.type.c_str(),
               s.has_size ? std::to_string(s.size).c_str() : ".", s.site.tid1, s.site.pos1, s.site.tid2, s.site.pos2, s.site.flag_mask);
    }
    printf("unknown %zu\n", t.unknown_lines);
    return 0;
}
