// bdx-depth-check RCI RCF POS1 POS2 FLANK CONTIG_LEN ...: every six through --depth's arithmetic (vcf.cpp depth_spans and depth_ratio), one
// line "len_in len_flank RDR" each; a malformed or incomplete argument list is exit 2.
// Test tooling for vcf.cpp: it links nothing else, so that the arithmetic can be built and run without a GPU, or under a sanitizer.
#include <cerrno>
#include <cstdio>
#include <cstdlib>

#include "vcf.h"

int main(int argc, char** argv) {
    if (argc < 7 || (argc - 1) % 6) {
        fprintf(stderr, "usage: bdx-depth-check RCI RCF POS1 POS2 FLANK CONTIG_LEN [RCI RCF POS1 POS2 FLANK CONTIG_LEN ...]\n");
        return 2;
    }
    for (int i = 1; i < argc; i += 6) {
        long long v[6];
        for (int k = 0; k < 6; ++k) {
            char* end = nullptr;
            errno = 0;
            v[k] = strtoll(argv[i + k], &end, 10);
            if (end == argv[i + k] || *end || errno) {
                fprintf(stderr, "not an integer: '%s'\n", argv[i + k]);
                return 2;
            }
        }
        const bdhost::DepthSpans s = bdhost::depth_spans(v[2], v[3], v[4], v[5]);
        printf("%lld %lld %s\n", (long long)s.len_in(), (long long)s.len_flank(), bdhost::depth_ratio(v[0], v[1], s.len_in(), s.len_flank()).c_str());
    }
    return 0;
}
