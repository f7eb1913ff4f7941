// bdx-feed-check: the device feeder's pure parts (feed_plan.h) on their own, for tests/test_feed.py -- no GPU and no libbdx.
//   bdx-feed-check cut FILE PIECE_BYTES MAX_BLOCKS [BEGIN END]
//       PieceCutter over bytes [BEGIN, END) of FILE (default: all of it) as device_feed.cpp's feed() drives it: pieces of PIECE_BYTES read
//       kLead bytes into a buffer, the carry in front.  Per piece "piece <file offset of the first byte submitted> <bytes> <nblocks> <last>",
//       per table entry "m <file offset of the payload> <payload_len> <inflated_len>".  An error: its text on stderr, status 1;
//       more than MAX_BLOCKS members in a piece: "too many members", status 2.
//   bdx-feed-check plan FILE_SIZE MEMBER_OFF SPAN_BYTES SIZED_FOR COMP INFL
//       every field of plan_decoder's answer as name=value, the knobs taken from the environment (FeedKnobs::from_env)
//   bdx-feed-check tie FILE
//       file_that_emitted_last for the two files and the sequence FILE describes:
//         t T                      the sequence whose first records tie
//         has F TID...             the sequences file F (0 or 1) holds records of
//         last F TID POS STRAND    the key of file F's last record on TID (no line: it has none)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <map>
#include <sstream>
#include <stdexcept>

#include "feed_plan.h"

using namespace bdhost;

namespace {

size_t num(const char* s) { return (size_t)strtoull(s, nullptr, 10); }

int cut(int argc, char** argv) {
    if (argc != 5 && argc != 7) throw std::runtime_error("usage: bdx-feed-check cut FILE PIECE_BYTES MAX_BLOCKS [BEGIN END]");
    const std::string path = argv[2];
    const MappedFile file(path, false);
    const size_t piece = num(argv[3]), max_blocks = num(argv[4]), file_size = file.size();
    const size_t begin = argc == 7 ? num(argv[5]) : 0;
    const size_t read_end = argc == 7 ? std::min(file_size, num(argv[6])) : file_size;
    std::vector<uint8_t> buf(kLead + piece + 65536);
    std::vector<bdx_bgzf_block> tab(max_blocks);
    PieceCutter cutter(path);
    for (size_t next_off = begin;;) {
        const size_t at = next_off, want = std::min(piece, read_end - std::min(read_end, next_off));
        if (want) memcpy(buf.data() + kLead, file.data() + at, want);
        next_off += want;
        const bool at_eof = next_off >= file_size;
        const PieceCutter::Cut c = cutter.cut(buf.data(), want, at_eof, next_off < read_end, tab.data(), max_blocks);
        if (c.too_many_members) {
            printf("too many members\n");
            return 2;
        }
        // (buffer offset kLead is file offset `at`)
        printf("piece %zu %zu %zu %d\n", at + c.base - kLead, c.bytes, c.nblocks, at_eof ? 1 : 0);
        for (size_t i = 0; i < c.nblocks; ++i)
            printf("m %zu %u %u\n", at + (size_t)tab[i].offset - kLead, tab[i].payload_len, tab[i].inflated_len);
        if (at_eof || next_off >= read_end) return 0;
    }
}

int plan(int argc, char** argv) {
    if (argc != 8) throw std::runtime_error("usage: bdx-feed-check plan FILE_SIZE MEMBER_OFF SPAN_BYTES SIZED_FOR COMP INFL");
    FeedExtent x;
    x.file_size = num(argv[2]); x.member_off = num(argv[3]); x.span_bytes = num(argv[4]); x.sized_for = num(argv[5]);
    x.comp = num(argv[6]); x.infl = num(argv[7]);
    const FeedPlan p = plan_decoder(x, FeedKnobs::from_env());
    printf("batch_bytes=%zu\nexpected_bytes=%zu\nbatch_blocks=%zu\nbatch_rounds=%d\nring_bytes=%zu\npiece_bytes=%zu\npiece_blocks=%zu\ntime_kernels=%d\n"
           "this_span=%zu\nread_end=%zu\n", p.batch_bytes, p.expected_bytes, p.batch_blocks, p.batch_rounds, p.ring_bytes, p.piece_bytes, p.piece_blocks,
           p.time_kernels, p.this_span, p.read_end);
    return 0;
}

int tie(int argc, char** argv) {
    if (argc != 3) throw std::runtime_error("usage: bdx-feed-check tie FILE");
    std::ifstream in(argv[2]);
    if (!in.is_open()) throw std::runtime_error(std::string("unable to open '") + argv[2] + "'");
    int t = -1;
    std::vector<std::vector<FileSpan>> span(2);
    std::map<std::pair<size_t, int>, std::pair<int32_t, int>> last;
    std::string line, word;
    while (std::getline(in, line)) {
        std::istringstream ls(line);
        if (!(ls >> word)) continue;
        size_t f = 0;
        int tid = 0;
        if (word == "t") ls >> t;
        else if (word == "has") {
            ls >> f;
            if (f > 1) throw std::runtime_error("malformed line: " + line);
            while (ls >> tid) {
                if (tid < 0) throw std::runtime_error("malformed line: " + line);
                if (span[f].size() <= (size_t)tid) span[f].resize((size_t)tid + 1);
                span[f][tid].has = true;
            }
        } else if (word == "last") {
            int32_t pos = 0;
            int strand = 0;
            if (!(ls >> f >> tid >> pos >> strand) || f > 1) throw std::runtime_error("malformed line: " + line);
            last[{f, tid}] = {pos, strand};
        } else throw std::runtime_error("unknown line: " + line);
    }
    if (t < 0) throw std::runtime_error("no sequence given");
    for (auto& s : span) s.resize(std::max(s.size(), (size_t)t + 1));
    printf("%d\n", file_that_emitted_last(span, {0, 1}, t, [&](size_t f, int tid, int32_t* pos, int* strand) {
               const auto hit = last.find({f, tid});
               if (hit == last.end()) return false;
               *pos = hit->second.first; *strand = hit->second.second;
               return true;
           }));
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    try {
        const std::string what = argc > 1 ? argv[1] : "";
        if (what == "cut") return cut(argc, argv);
        if (what == "plan") return plan(argc, argv);
        if (what == "tie") return tie(argc, argv);
        throw std::runtime_error("usage: bdx-feed-check cut|plan|tie ...");
    } catch (std::exception const& e) {
        std::cerr << e.what() << "\n";
        return 1;
    }
}
