// bdx-clip-check: the host half of --clip on its own, without a GPU and without libbdx (tests/test_clip.py).
//   bdx-clip-check words           every line of stdin "CIGAR L_SEQ FLAG" (CIGAR '*': none) -> "LEFT RIGHT SPAN WORD", the clip word
//                                  of csrc/bdx_clip.h, the one function of every reader
//   bdx-clip-check bam FILE        every record of the BAM through the host reader (bam_reader.cpp parse_record), in file order ->
//                                  "TID POS FLAG WORD"
//   bdx-clip-check keys SUPPORT    every line of stdin -- the two ends of a site as --clip asked them and whether the record prints them the
//                                  other way round, 17 integers "HELD P NLEFT NRIGHT POSLEFT POSRIGHT PEAKLEFT PEAKRIGHT" x 2 and SWAPPED --
//                                  through the writer's own formatting (vcf.cpp clip_info), one INFO fragment per line
// A malformed line or argument is exit 2.
#include <cstdio>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../csrc/bdx_clip.h"
#include "bam_reader.h"
#include "vcf.h"

namespace {

int words() {
    std::string line;
    while (std::getline(std::cin, line)) {
        if (line.empty()) continue;
        std::istringstream in(line);
        std::string cigar, rest;
        long long l_seq = 0, flag = 0;
        if (!(in >> cigar >> l_seq >> flag) || (in >> rest) || l_seq < 0 || l_seq > 0x7FFFFFFFll || flag < 0 || flag > 0xFFFF) {
            fprintf(stderr, "not 'CIGAR L_SEQ FLAG': '%s'\n", line.c_str());
            return 2;
        }
        std::vector<uint8_t> bytes;
        if (cigar != "*") {
            unsigned long long len = 0;
            bool digits = false, ok = true;   // (digits: a length is open; a CIGAR ends behind an operation)
            for (size_t i = 0; i < cigar.size() && ok; ++i) {
                const char ch = cigar[i];
                if (ch >= '0' && ch <= '9') {
                    len = len * 10 + (unsigned)(ch - '0');
                    digits = true;
                    ok = len < (1ull << 28);
                    continue;
                }
                const char* ops = "MIDNSHP=X";
                const char* at = strchr(ops, ch);
                ok = at && digits;
                if (!ok) break;
                const uint32_t w = (uint32_t)(len << 4) | (uint32_t)(at - ops);
                for (int k = 0; k < 4; ++k) bytes.push_back((uint8_t)(w >> (8 * k)));
                len = 0;
                digits = false;
            }
            if (!ok || digits || bytes.empty() || bytes.size() / 4 > 65535) {
                fprintf(stderr, "not a CIGAR: '%s'\n", cigar.c_str());
                return 2;
            }
        }
        const uint32_t w = bdx::clip_word(bytes.data(), (uint32_t)(bytes.size() / 4), (int32_t)l_seq, (uint32_t)flag);
        printf("%u %u %u %u\n", w & 255u, (w >> 8) & 255u, w >> 16, w);
    }
    return 0;
}

int bam(const char* path) {
    bdhost::BamReader rd(path, 2);
    bdhost::BamRecord r;
    while (rd.next(r)) printf("%d %d %u %u\n", r.tid, r.pos, (unsigned)r.flag, r.clip);
    return 0;
}

int keys(const char* support_arg) {
    char* end = nullptr;
    const long support = strtol(support_arg, &end, 10);
    if (end == support_arg || *end || support < 1 || support > (1L << 30)) {
        fprintf(stderr, "SUPPORT is an integer from 1 to 2^30, not '%s'\n", support_arg);
        return 2;
    }
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
        bdhost::EndClips e[2];
        for (int k = 0; k < 2; ++k) {
            const long long* w = v + 8 * k;
            e[k].held = w[0] != 0;
            e[k].pos = w[1];
            e[k].n_left = (uint32_t)w[2]; e[k].n_right = (uint32_t)w[3];
            e[k].pos_left = (int32_t)w[4]; e[k].pos_right = (int32_t)w[5];
            e[k].peak_left = (uint32_t)w[6]; e[k].peak_right = (uint32_t)w[7];
        }
        printf("%s\n", bdhost::clip_info(e[0], e[1], v[16] != 0, (uint32_t)support).c_str());
    }
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    try {
        if (argc == 2 && !strcmp(argv[1], "words")) return words();
        if (argc == 3 && !strcmp(argv[1], "bam")) return bam(argv[2]);
        if (argc == 3 && !strcmp(argv[1], "keys")) return keys(argv[2]);
    } catch (std::exception const& e) {
        fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    fprintf(stderr, "usage: bdx-clip-check words | bam FILE | keys SUPPORT\n");
    return 2;
}
