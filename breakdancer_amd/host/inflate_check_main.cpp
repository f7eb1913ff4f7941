// bdx-inflate-check <bgzf file>...: every BGZF block of the files through fast_inflate and through zlib; reports
// mismatches (exit 1) and the two decoders' throughput.  Test tooling for fast_inflate.cpp.
// bdx-inflate-check --members FILE [AVAIL]: the members the shared parser (bgzf.h) finds in FILE when it may look at the
// first AVAIL bytes only (default: all) -- one line "offset total payload_off payload_len ulen" each, then "end <offset>
// <status>" for what ended the walk.  Test tooling for bgzf.h.
// bdx-inflate-check --each FILE: one line "index zlib_ok fast_ok bytes_equal" per member of FILE, empty ones included; a member that
// zlib rejects is no failure here (tests/test_deflate_cases.py feeds it members that must be rejected).  fast_inflate reads each payload
// from a heap copy with exactly the 32 bytes behind it that its callers guarantee, so that a sanitizer build sees a read beyond them.
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iterator>
#include <vector>

#include "bgzf.h"
#include "fast_inflate.h"

using bdhost::BgzfMember;
using bdhost::BgzfStatus;

static const char* status_name(BgzfStatus s) {
    switch (s) {
        case BgzfStatus::kMember: return "member";
        case BgzfStatus::kEnd: return "end";
        case BgzfStatus::kNeedBytes: return "need-bytes";
        case BgzfStatus::kNotBgzf: return "not-bgzf";
        case BgzfStatus::kNoBsize: return "no-bc-field";
        case BgzfStatus::kBadBsize: return "bad-bsize";
        case BgzfStatus::kTooLarge: return "too-large";
    }
    return "?";
}

static int list_members(const char* path, const char* avail_arg) {
    std::ifstream in(path, std::ios::binary);
    if (!in) { fprintf(stderr, "cannot open %s\n", path); return 2; }
    const std::vector<uint8_t> d((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
    size_t avail = d.size();
    if (avail_arg) avail = std::min(avail, (size_t)strtoull(avail_arg, nullptr, 10));
    size_t off = 0;
    BgzfMember m;
    BgzfStatus s;
    while ((s = bdhost::bgzf_parse(d.data() + off, avail - off, &m)) == BgzfStatus::kMember) {
        printf("%zu %zu %zu %zu %u\n", off, m.total, m.payload_off, m.payload_len, m.ulen);
        off += m.total;
    }
    printf("end %zu %s\n", off, status_name(s));
    return 0;
}

static int each_member(const char* path) {
    try {
        const bdhost::MappedFile file(path, false);
        const uint8_t* m = file.data();
        const size_t size = file.size();
        size_t off = 0, index = 0;
        BgzfMember mem;
        while (bdhost::bgzf_member_at(m, size, off, path, &mem)) {
            const size_t coff = off + mem.payload_off, clen = mem.payload_len;
            const uint32_t ulen = mem.ulen;
            off += mem.total;
            std::vector<uint8_t> a((size_t)ulen + 64), b((size_t)ulen + 1);
            const bool okz = bdhost::bgzf_try_inflate_zlib(m + coff, clen, b.data(), ulen);
            bool okf = false;
            if (coff + clen + 32 <= size) {
                const std::vector<uint8_t> in(m + coff, m + coff + clen + 32);
                okf = bdhost::fast_inflate(in.data(), clen, a.data(), ulen, 64);
            }
            printf("%zu %d %d %d\n", index++, (int)okz, (int)okf, (int)(okz && okf && memcmp(a.data(), b.data(), ulen) == 0));
        }
    } catch (std::exception const& e) {
        fprintf(stderr, "%s\n", e.what());
        return 2;
    }
    return 0;
}

int main(int argc, char** argv) {
    if (argc >= 3 && !strcmp(argv[1], "--members")) return list_members(argv[2], argc > 3 ? argv[3] : nullptr);
    if (argc == 3 && !strcmp(argv[1], "--each")) return each_member(argv[2]);
    size_t blocks = 0, bad = 0, rejected = 0, bytes = 0;
    double t_fast = 0, t_zlib = 0;
    std::vector<uint8_t> a(65536 + 64), b(65536 + 64);
    for (int f = 1; f < argc; ++f) {
        try {
            const bdhost::MappedFile file(argv[f], false);
            const uint8_t* m = file.data();
            const size_t size = file.size();
            size_t off = 0;
            BgzfMember mem;
            while (bdhost::bgzf_member_at(m, size, off, argv[f], &mem)) {
                const size_t coff = off + mem.payload_off, clen = mem.payload_len;
                const uint32_t ulen = mem.ulen;
                off += mem.total;
                if (!ulen) continue;
                ++blocks;
                bytes += ulen;
                auto t0 = std::chrono::steady_clock::now();
                const bool okz = bdhost::bgzf_try_inflate_zlib(m + coff, clen, b.data(), ulen);
                auto t1 = std::chrono::steady_clock::now();
                bool okf = false;
                if (coff + clen + 32 <= size) okf = bdhost::fast_inflate(m + coff, clen, a.data(), ulen, 64);
                auto t2 = std::chrono::steady_clock::now();
                t_zlib += std::chrono::duration<double>(t1 - t0).count();
                t_fast += std::chrono::duration<double>(t2 - t1).count();
                if (!okz) { fprintf(stderr, "%s: zlib rejects the block at %zu\n", argv[f], coff); ++bad; continue; }
                if (!okf) { ++rejected; continue; }
                if (memcmp(a.data(), b.data(), ulen) != 0) { fprintf(stderr, "%s: MISMATCH in the block at %zu\n", argv[f], coff); ++bad; }
            }
        } catch (std::exception const& e) {
            fprintf(stderr, "%s\n", e.what());
            return 2;
        }
    }
    printf("blocks %zu bytes %zu mismatches %zu left_to_zlib %zu fast %.1f MB/s zlib %.1f MB/s\n", blocks, bytes, bad, rejected,
           t_fast > 0 ? bytes / t_fast / 1e6 : 0.0, t_zlib > 0 ? bytes / t_zlib / 1e6 : 0.0);
    return bad ? 1 : 0;
}
