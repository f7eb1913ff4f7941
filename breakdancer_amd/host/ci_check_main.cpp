// bdx-ci-check LO HI P ...: every triple through --ci's interval arithmetic (vcf.cpp ci_offsets), one line "a b" each; a malformed or
// incomplete argument list is exit 2.
// Test tooling for vcf.cpp: it links nothing else, so that the arithmetic can be built and run under a sanitizer on its own.
#include <cerrno>
#include <cstdio>
#include <cstdlib>

#include "vcf.h"

int main(int argc, char** argv) {
    if (argc < 4 || (argc - 1) % 3) {
        fprintf(stderr, "usage: bdx-ci-check LO HI P [LO HI P ...]\n");
        return 2;
    }
    for (int i = 1; i < argc; i += 3) {
        long long v[3];
        for (int k = 0; k < 3; ++k) {
            char* end = nullptr;
            errno = 0;
            v[k] = strtoll(argv[i + k], &end, 10);
            if (end == argv[i + k] || *end || errno) {
                fprintf(stderr, "not an integer: '%s'\n", argv[i + k]);
                return 2;
            }
        }
        const bdhost::CiOffsets c = bdhost::ci_offsets(v[0], v[1], v[2]);
        printf("%lld %lld\n", (long long)c.a, (long long)c.b);
    }
    return 0;
}
