// The device decode's feeder (device_feed.cpp), its pure parts: the knobs of the environment, the sizes a decoder is created with,
// the cut of a piece of the file into whole BGZF members, and the tie-break between two files at a chromosome's first position.
// Arithmetic over bytes only -- no libbdx symbol, no GPU: bin/bdx-feed-check drives every function here (tests/test_feed.py).
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "bdx.h"
#include "bgzf.h"

namespace bdhost {

// A piece's file bytes land kLead bytes into its staging buffer: the tail of the piece before it -- the member cut at that piece's
// end, known only once that piece has been cut -- is put in front of them.
constexpr size_t kLead = 65536;

// Test / measurement knobs of the CLI (the library reads no environment variable for them: they travel in the parameters).
struct FeedKnobs {
    size_t piece_bytes = (size_t)8 << 20;   // BDX_BAM_PIECE_BYTES (a staging buffer costs ~0.22 ms per MiB to pin and is reused dozens of times)
    size_t batch_blocks = 0;                // BDX_BAM_BATCH_BLOCKS; 0: the decoder's
    int32_t batch_rounds = 0;               // BDX_BAM_BATCH_ROUNDS, 1..16; 0: from the ratio probe
    size_t ring_bytes = 0;                  // BDX_BAM_RING_BYTES; 0: planned
    int ahead = 4;                          // BDX_BAM_AHEAD, 1..4: pieces on their way into staging buffers
    bool read_by_pread = false;             // BDX_READ=pread: the system call instead of the copy out of the mapping
    bool timing = false;                    // BDX_TIMING: the [bdx timing] lines, and HIP events around the inflate launches
    static FeedKnobs from_env() {
        FeedKnobs k;
        if (const char* v = getenv("BDX_BAM_PIECE_BYTES")) k.piece_bytes = (size_t)std::max(1ll, atoll(v));
        if (const char* v = getenv("BDX_BAM_BATCH_BLOCKS")) k.batch_blocks = (size_t)std::max(1ll, atoll(v));
        if (const char* v = getenv("BDX_BAM_BATCH_ROUNDS")) k.batch_rounds = std::max(1, std::min(16, atoi(v)));
        if (const char* v = getenv("BDX_BAM_RING_BYTES")) k.ring_bytes = (size_t)std::max(1ll, atoll(v));
        if (const char* v = getenv("BDX_BAM_AHEAD")) k.ahead = std::max(1, std::min(4, atoi(v)));
        const char* how = getenv("BDX_READ");
        k.read_by_pread = how && !strcmp(how, "pread");
        k.timing = getenv("BDX_TIMING") != nullptr;
        return k;
    }
};

// What is to be decoded, in bytes of the file.
struct FeedExtent {
    size_t file_size = 0;
    size_t member_off = 0;    // the member that holds the first record
    size_t span_bytes = 0;    // sharded runs: what the sequence takes of the file; 0: the rest of the file
    size_t sized_for = 0;     // a decoder that is armed again: the largest span it will be used for (its buffers are sized once)
    size_t comp = 0, infl = 0;   // compressed and inflated bytes of the first members (BSIZE / ISIZE of their headers), at most 64
    void probe_ratio(const uint8_t* map) {
        comp = infl = 0;
        size_t off = member_off;
        BgzfMember m;
        for (int k = 0; k < 64 && off < file_size && bgzf_parse(map + off, file_size - off, &m) == BgzfStatus::kMember; ++k) {
            comp += m.total; infl += m.ulen;
            off += m.total;
        }
    }
};

struct FeedPlan {   // the size fields of bdx_bamdec_params, and where the feeder's reading ends
    size_t batch_bytes = 0, expected_bytes = 0, batch_blocks = 0, ring_bytes = 0, piece_bytes = 0, piece_blocks = 0;
    int32_t batch_rounds = 0, time_kernels = 0;
    size_t this_span = 0;   // the bytes of THIS stretch (what a decoder armed again is told to expect)
    size_t read_end = 0;    // file offset behind which nothing is read
    void apply(bdx_bamdec_params& p) const {
        p.batch_bytes = batch_bytes; p.expected_bytes = expected_bytes; p.batch_blocks = batch_blocks; p.batch_rounds = batch_rounds;
        p.ring_bytes = ring_bytes; p.piece_bytes = piece_bytes; p.piece_blocks = piece_blocks; p.time_kernels = time_kernels;
    }
};

// pieces (transfer units) of 8 MiB; the decoder gathers them into batches of >= 8192 members before it launches kernels.
// Small files get small buffers.
inline FeedPlan plan_decoder(const FeedExtent& x, const FeedKnobs& k) {
    FeedPlan p;
    size_t rest = x.file_size - std::min(x.file_size, x.member_off);
    if (x.span_bytes) rest = std::min(rest, x.span_bytes);
    p.this_span = rest;
    if (x.sized_for) rest = std::max(rest, std::min(x.sized_for, x.file_size));   // (the buffers of a decoder that is armed again: for its largest stretch)
    // (a file of less than a batch: buffers of its size; else the decoder picks the batches -- up to four rounds of the wave slots for a large input)
    p.batch_bytes = rest < ((size_t)384 << 20) ? ((rest + ((size_t)1 << 20)) >> 20) << 20 : 0;
    p.expected_bytes = rest;
    p.batch_blocks = k.batch_blocks;
    // The ring of inflated bytes holds FOUR batches (the one whose records are being read, its successor, the one being inflated, slack).
    // A batch is at most the decoder's largest -- rounds x 7,680 members and the piece that took it there, 64 KiB each -- or everything that
    // is read (a BGZF member inflates to at most ~16 x its size; 8 x is assumed of a whole stretch: beyond that the decoder says BDX_ELIMIT
    // and the host reader takes the file).  Sharded runs keep one decoder per rank for all of its sequences: sized for the largest.
    //
    // An inflate launch should take several rounds of the GPU's wave slots once the input is large (a one-round launch ends with the slots
    // draining: 58 against 68-70 GB/s of inflated bytes on the level-1 file, 109 against 168 on a level-6 file of reference-drawn reads) --
    // and "large" is about the INFLATED bytes: a real 30x BAM compresses 5 x, the random-base test files 1.57 x.  The ratio is read off
    // the first members (FeedExtent::probe_ratio); one round per 4 GB of inflated bytes expected, at most four.
    if (x.comp && x.infl && !p.batch_blocks) {
        const double expected_inflated = (double)rest * (double)x.infl / (double)x.comp;
        p.batch_rounds = (int32_t)std::max(1.0, std::min(4.0, expected_inflated / (double)((size_t)4 << 30)));
    }
    if (k.batch_rounds) p.batch_rounds = k.batch_rounds;
    if (k.timing) p.time_kernels = 1;   // (the timing lines say what the inflate kernel took inside the pipeline)
    const size_t rounds = p.batch_rounds ? (size_t)p.batch_rounds : std::max<size_t>(1, std::min<size_t>(4, rest / ((size_t)2560 << 20)));
    const size_t blocks = p.batch_blocks ? p.batch_blocks : 7680 * rounds;
    const size_t batch_inflated = (blocks + k.piece_bytes / 16384 + 64) * 65536;
    p.ring_bytes = std::max<size_t>((size_t)64 << 20, std::min<size_t>(rest * 32, 4 * batch_inflated));
    if (x.span_bytes) p.ring_bytes = std::max<size_t>(p.ring_bytes, (size_t)256 << 20);
    if (k.ring_bytes) p.ring_bytes = k.ring_bytes;
    // (what bdx_bamdec_acquire will ask for: a piece, a member cut at the piece's end carried over from the one before, and slack)
    p.piece_bytes = std::min(k.piece_bytes, rest) + 65536 + 65536;   // (in front: the tail of the piece before; behind: slack)
    p.piece_blocks = k.piece_bytes / 512 + 4096;   // (a piece of more members than that -- 512 bytes each on average -- is left to the host reader)
    // (a sequence read through the index: its records end where the index says -- nothing behind that is read, let alone inflated)
    p.read_end = x.span_bytes ? std::min(x.file_size, x.member_off + x.span_bytes) : x.file_size;
    return p;
}

// Pieces of about piece_bytes, cut at member boundaries: the bytes behind the last whole member of a piece (`carry`) open the next.
class PieceCutter {
public:
    struct Cut {
        size_t base = 0;      // where the piece begins in the staging buffer: kLead less what was carried over
        size_t bytes = 0;     // whole members from there on (the caller submits base + bytes: the bytes in front of `base` travel with
                              // the piece -- at most 64 KiB of 8 MiB -- and no table entry points at them)
        size_t nblocks = 0;   // table entries written; their offsets are relative to the buffer
        bool too_many_members = false;   // more than max_blocks members: nothing is to be submitted
    };
    explicit PieceCutter(const std::string& path) : path_(path) {}
    // buf: a staging buffer with `want` bytes of the file from buf + kLead on (and room for kLead in front); at_eof: they end the file;
    // more: the caller is going to read further.  Members that inflate to nothing (the EOF marker, flush blocks) stay out of the table.
    Cut cut(uint8_t* buf, size_t want, bool at_eof, bool more, bdx_bgzf_block* tab, size_t max_blocks) {
        if (carry_.size() > kLead) throw std::runtime_error("BGZF member larger than 64 KiB: " + path_);
        Cut c;
        c.base = kLead - carry_.size();
        uint8_t* b = buf + c.base;
        if (!carry_.empty()) memcpy(b, carry_.data(), carry_.size());
        const size_t have = carry_.size() + want;
        size_t q = 0;
        for (;;) {
            BgzfMember m;
            const BgzfStatus st = bgzf_parse(b + q, have - q, &m);
            if (st == BgzfStatus::kEnd || st == BgzfStatus::kNeedBytes) break;   // (the rest of a member cut at the piece's end comes with the next piece)
            if (st != BgzfStatus::kMember) bgzf_throw(st, path_);
            if (m.ulen) {
                if (c.nblocks >= max_blocks) { c.too_many_members = true; return c; }
                tab[c.nblocks].offset = c.base + q + m.payload_off;
                tab[c.nblocks].payload_len = (uint32_t)m.payload_len;
                tab[c.nblocks].inflated_len = m.ulen;
                ++c.nblocks;
            }
            q += m.total;
        }
        if (at_eof && q != have) throw std::runtime_error("truncated BGZF file: " + path_);
        carry_.assign(b + q, b + have);
        if (q == 0 && !at_eof && want && more) throw std::runtime_error("BGZF member larger than a piece: " + path_);
        c.bytes = q;
        return c;
    }

private:
    std::string path_;
    std::vector<uint8_t> carry_;
};

struct FileSpan { size_t begin = 0, end = 0; bool has = false; };   // what a file's index says of one sequence: [begin, end) of the file

// The reference keeps ONE queue across chromosome boundaries (io/BamMerger.cpp:40-126): where the files' first records of a
// chromosome tie (same position and strand -- the first mappable base behind a telomere's Ns), the file whose record has been
// waiting at the top wins, and that is the one that did NOT emit the genome's last record in front of the chromosome.  Two
// files (the tumour / normal pair): worked out from the files' last records on the chromosomes before -- whoever's rank they
// were on.  More files: the tie goes to the lowest file index, as a queue filled afresh would have it (only the
// order of equal-key records at a chromosome's first position can differ from the reference there).
// span[file][tid]; files: the two that hold records of sequence t; last_key(file, tid, &pos, &strand): the key of the file's last
// record on tid, false if it has none.  Returns 0 or 1: which of the two emitted last in front of t (merge_order's emitted_last).
template <class LastKey>
int file_that_emitted_last(const std::vector<std::vector<FileSpan>>& span, const std::vector<size_t>& files, int t, LastKey&& last_key) {
    int prev[2] = {-1, -1};
    for (int x = 0; x < 2; ++x)
        for (int tp = t - 1; tp >= 0 && prev[x] < 0; --tp)
            if (span[files[x]][tp].has) prev[x] = tp;
    if (prev[0] >= 0 && prev[1] < 0) return 0;
    if (prev[0] < 0) return 1;   // (file 1 alone emitted before; or neither did: the queue's first fill, file 0 on top)
    if (prev[0] != prev[1]) return prev[0] > prev[1] ? 0 : 1;
    int32_t lp[2] = {0, 0};
    int ls[2] = {0, 0};
    for (int x = 0; x < 2; ++x)
        if (!last_key(files[x], prev[x], &lp[x], &ls[x])) return 1;
    if (lp[0] != lp[1] || ls[0] != ls[1]) return (lp[0] > lp[1] || (lp[0] == lp[1] && ls[0] > ls[1])) ? 0 : 1;
    return 1;   // (equal last keys as well: what happened in front of THAT tie decides -- left as a fresh queue would have it)
}

}  // namespace bdhost
