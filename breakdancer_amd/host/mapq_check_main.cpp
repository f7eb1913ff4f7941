// bdx-mapq-check: every line of stdin -- the two ends of a site as --mapq counted it and whether the record prints them the other way
// round, 17 integers "HELD N NALL NLOW QMIN Q1 MEDIAN QMAX" x 2 and SWAPPED -- through the writer's own formatting (vcf.cpp mapq_info),
// one INFO fragment per line; a malformed line is exit 2.
// Test tooling for vcf.cpp: it links nothing else, so that the formatting can be built and run without a GPU (tests/test_mapq.py).
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>

#include "vcf.h"

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        if (line.empty()) continue;
        std::istringstream in(line);
        long long v[17];
        for (long long& x : v)
            if (!(in >> x) || x < 0 || x > 0xFFFFFFFFll) {
                fprintf(stderr, "not 17 integers from 0 to 2^32 - 1: '%s'\n", line.c_str());
                return 2;
            }
        std::string rest;
        if (in >> rest) {
            fprintf(stderr, "more than 17 fields: '%s'\n", line.c_str());
            return 2;
        }
        bdhost::EndQuality e[2];
        for (int k = 0; k < 2; ++k) {
            const long long* w = v + 8 * k;
            e[k].held = w[0] != 0;
            e[k].n = (uint32_t)w[1]; e[k].n_all = (uint32_t)w[2]; e[k].n_low = (uint32_t)w[3];
            e[k].qmin = (unsigned)w[4]; e[k].q1 = (unsigned)w[5]; e[k].median = (unsigned)w[6]; e[k].qmax = (unsigned)w[7];
        }
        printf("%s\n", bdhost::mapq_info(e[0], e[1], v[16] != 0).c_str());
    }
    return 0;
}
