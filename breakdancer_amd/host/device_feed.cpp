#include "device_feed.h"

#include <algorithm>
#include <chrono>
#include <condition_variable>
#include <cstdio>
#include <cstring>
#include <deque>
#include <fcntl.h>
#include <mutex>
#include <stdexcept>
#include <sys/mman.h>
#include <thread>
#include <unistd.h>

#include "column_reader.h"
#include "feed_plan.h"
#include "producer.h"

namespace bdhost {

namespace {

std::vector<bdx_bamdec*> g_retired;
std::mutex g_retired_mu;

// Pieces of a file read AHEAD of the one being cut into members: a pool of threads that lives as long as the decode, fed with slices of 1 MiB.
// The slices are copied out of the file's MAPPING (the reader's own, ColumnReader::mapped) when there is one: pread() of the same bytes from the
// page cache fed the copy engine 39-42 GB/s, memcpy from the mapping 51 -- the engine's own rate -- with half the threads
// (tools/feed_probe.hip, profiles/r05_feed_probe.txt); BDX_READ=pread keeps the system call.
// (Page cache -> pinned memory is a plain copy, one core moves 2-5 GB/s of it through pread.  Until round 4 every piece was read by threads started for
// it -- 244 pieces x 7 threads for a 2 GB file, the piece all they had to work on: 26 GB/s on 16 CPUs; a pool working on up to four pieces at
// a time moves 40 GB/s on the same box, tools/register_probe.hip.)
class ReadPool {
public:
    struct Piece {
        std::mutex mu;
        std::condition_variable cv;
        size_t left = 0;
        bool failed = false;
    };
    explicit ReadPool(int n) {
        for (int i = 0; i < std::max(1, n); ++i) th_.emplace_back([this] { work(); });
    }
    ~ReadPool() {
        { std::lock_guard<std::mutex> lk(mu_); stop_ = true; }
        cv_.notify_all();
        for (auto& t : th_) t.join();
    }
    // bytes [off, off + n) of fd into dst; pc->left counts the slices still on their way
    void read(int fd, const uint8_t* map, size_t off, uint8_t* dst, size_t n, Piece* pc) {
        const size_t slice = (size_t)1 << 20;
        const size_t k = (n + slice - 1) / slice;
        { std::lock_guard<std::mutex> lk(pc->mu); pc->left += k; }
        {
            std::lock_guard<std::mutex> lk(mu_);
            for (size_t o = 0; o < n; o += slice) q_.push_back(Task{fd, map, off + o, dst + o, std::min(slice, n - o), pc});
        }
        cv_.notify_all();
    }
    static bool wait(Piece* pc) {   // true: every byte arrived
        std::unique_lock<std::mutex> lk(pc->mu);
        pc->cv.wait(lk, [pc] { return pc->left == 0; });
        return !pc->failed;
    }

private:
    struct Task { int fd; const uint8_t* map; size_t off; uint8_t* dst; size_t n; Piece* pc; };
    void work() {
        for (;;) {
            Task t;
            {
                std::unique_lock<std::mutex> lk(mu_);
                cv_.wait(lk, [this] { return stop_ || !q_.empty(); });
                if (q_.empty()) return;
                t = q_.front();
                q_.pop_front();
            }
            bool ok = true;
            if (t.map) {
                memcpy(t.dst, t.map + t.off, t.n);
                // (the pages' mappings go again at once, here, on sixteen threads: left to the end, tearing down 16 GB of populated page
                // tables took the thread that unmaps the file 0.2 s)
                const uintptr_t lo = ((uintptr_t)(t.map + t.off) + 4095) & ~(uintptr_t)4095, hi = (uintptr_t)(t.map + t.off + t.n) & ~(uintptr_t)4095;
                if (hi > lo) (void)madvise((void*)lo, hi - lo, MADV_DONTNEED);
            } else for (size_t done = 0; done < t.n;) {
                const ssize_t r = pread(t.fd, t.dst + done, t.n - done, (off_t)(t.off + done));
                if (r <= 0) { ok = false; break; }
                done += (size_t)r;
            }
            std::lock_guard<std::mutex> lk(t.pc->mu);
            if (!ok) t.pc->failed = true;
            if (--t.pc->left == 0) t.pc->cv.notify_all();
        }
    }
    std::vector<std::thread> th_;
    std::deque<Task> q_;
    std::mutex mu_;
    std::condition_variable cv_;
    bool stop_ = false;
};

using Clock = std::chrono::steady_clock;
double since(Clock::time_point a) { return std::chrono::duration<double>(Clock::now() - a).count(); }

void check(int rc, const char* what, const bdx_bamdec* dec, const std::string& path) {
    if (rc != BDX_OK) throw std::runtime_error(std::string(what) + ": " + bdx_strerror(rc) + " (" + bdx_bamdec_last_error(dec) + ") in " + path);
}

struct Located {
    RecordFilter filter;
    size_t member_off = 0;   // the member that holds the first record to look at
    uint64_t rec_off = 0;    // the record's offset in that member's inflated bytes
    bool seeked = false;     // the index was used to get there: a region's reading stops at the first record behind it
};

Located locate(const DecodeJob& job, ColumnReader& hdr, const std::string& path) {
    Located at;
    RecordFilter& f = at.filter;
    if (job.whole_tid >= 0) {
        f.only_tid = job.whole_tid;
        f.beg = 0;                // (every placed record of the sequence: the device's overlap test compares unsigned)
        f.end = 0x7FFFFFFF;
    } else if (!job.region.empty() && !parse_region(hdr, job.region, f.only_tid, f.beg, f.end))
        throw std::runtime_error("Failed to parse bam region '" + job.region + "' in file " + path + ". ");
    if (job.targets) *job.targets = hdr.target_names();
    hdr.locate(f, &at.member_off, &at.rec_off, &at.seeked);
    return at;
}

FeedPlan plan(const DecodeJob& job, const ColumnReader& hdr, const Located& at, const FeedKnobs& knobs) {
    FeedExtent x;
    x.file_size = hdr.mapped_size();
    x.member_off = at.member_off;
    x.span_bytes = job.span_bytes;
    x.sized_for = job.sized_for;
    x.probe_ratio(hdr.mapped());
    return plan_decoder(x, knobs);
}

// job.rearm armed again, or a new decoder with the --exclude table: *own holds what this call set up
bdx_bamdec* open_decoder(const DecodeJob& job, const ColumnReader& hdr, const Located& at, const FeedPlan& fp, OwnedDecoder* own) {
    const RecordFilter& f = at.filter;
    if (bdx_bamdec* dec = job.rearm) {
        const int rc = bdx_bamdec_rearm(dec, f.only_tid, f.beg, f.end, at.rec_off, fp.this_span);
        if (rc != BDX_OK) throw std::runtime_error(std::string("bdx_bamdec_rearm: ") + bdx_strerror(rc) + " (" + bdx_bamdec_last_error(dec) + ")");
        return dec;
    }
    std::vector<std::string> ids;
    std::vector<uint8_t> libs;
    for (auto const& kv : job.cfg.readgroup_index()) { ids.push_back(kv.first); libs.push_back((uint8_t)kv.second); }
    std::vector<const char*> idp;
    for (auto const& s : ids) idp.push_back(s.c_str());
    bdx_bamdec_params p{};
    p.device = job.device;
    p.n_targets = (int32_t)hdr.target_names().size();
    p.bam_index = (int32_t)job.bam_index;
    p.only_tid = f.only_tid; p.region_beg = f.beg; p.region_end = f.end;
    p.n_read_groups = (uint32_t)ids.size();
    p.rg_ids = idp.empty() ? nullptr : idp.data();
    p.rg_lib = libs.empty() ? nullptr : libs.data();
    p.fallback_lib = (uint8_t)job.cfg.fallback_library();
    p.first_record_offset = at.rec_off;
    fp.apply(p);
    if (job.clips) p.record_mode |= 4;
    bdx_bamdec* dec = nullptr;
    int rc = bdx_bamdec_create(&dec, job.sink, &p);
    if (rc != BDX_OK) throw std::runtime_error(std::string("bdx_bamdec_create: ") + bdx_strerror(rc));
    own->reset(dec);
    const ExcludeTable* ex = job.exclude;
    if (ex && !ex->intervals.empty()) {
        rc = bdx_bamdec_set_exclude(dec, ex->intervals.data(), ex->intervals.size());
        if (rc != BDX_OK) {
            const std::string msg = std::string("bdx_bamdec_set_exclude: ") + bdx_strerror(rc) + " (" + bdx_bamdec_last_error(dec) + ")";
            bdx_bamdec_destroy(own->release());
            throw std::runtime_error(msg);
        }
    }
    return dec;
}

struct FeedTimes { double create = 0, acquire = 0, read = 0, scan = 0, submit = 0, finish = 0; size_t npieces = 0; };
enum class FeedEnd { kFed, kTooManyMembers, kRefusedInSubmit };

// The file is read AHEAD of the piece being cut: up to `ahead` pieces are on their way into staging buffers (ReadPool) while this
// thread finds the members of the oldest one and submits it.  Returns with no reader still writing into a staging buffer, whatever
// ends the loop -- an exception too: the decoder may go on (bdx_bamdec_finish) as soon as this is through.
FeedEnd feed(bdx_bamdec* dec, const DecodeJob& job, const ColumnReader& hdr, const std::string& path, const Located& at, const FeedPlan& fp,
             const FeedKnobs& knobs, FeedTimes& tm) {
    const int fd = open(path.c_str(), O_RDONLY);
    if (fd < 0) throw std::runtime_error("Failed to open samfile " + path);
    struct Fd { int fd; ~Fd() { close(fd); } } fdg{fd};
    const size_t file_size = hdr.mapped_size(), read_end = fp.read_end, max_blocks = fp.piece_blocks;
    // (a region read through the index stops at the first record behind it: nothing is read in vain)
    const int n_ahead = at.seeked ? 1 : knobs.ahead;
    const uint8_t* read_map = knobs.read_by_pread ? nullptr : hdr.mapped();
    struct Ahead { uint8_t* b = nullptr; bdx_bgzf_block* tab = nullptr; size_t off = 0, want = 0; ReadPool::Piece pc; };
    ReadPool pool(job.threads);
    struct Queue : std::deque<std::unique_ptr<Ahead>> {   // (pieces read ahead and not needed: their readers are through before the decoder is)
        ~Queue() { for (auto& x : *this) (void)ReadPool::wait(&x->pc); }
    } ahead;
    PieceCutter cutter(path);
    size_t next_off = at.member_off;
    bool queued_all = false;
    for (;;) {
        while (!queued_all && (int)ahead.size() < n_ahead) {
            std::unique_ptr<Ahead> a(new Ahead);
            a->off = next_off;
            a->want = std::min(knobs.piece_bytes, read_end - std::min(read_end, next_off));
            void* buf = nullptr;
            const auto t0 = Clock::now();
            check(bdx_bamdec_acquire(dec, kLead + a->want + 65536, max_blocks, &buf, &a->tab), "bdx_bamdec_acquire", dec, path);
            tm.acquire += since(t0);
            a->b = (uint8_t*)buf;
            if (a->want) pool.read(fd, read_map, a->off, a->b + kLead, a->want, &a->pc);
            next_off += a->want;
            if (next_off >= read_end) queued_all = true;
            ahead.push_back(std::move(a));
        }
        if (ahead.empty()) return FeedEnd::kFed;
        std::unique_ptr<Ahead> cur = std::move(ahead.front());
        ahead.pop_front();
        ++tm.npieces;
        auto t0 = Clock::now();
        const bool read_ok = ReadPool::wait(&cur->pc);
        tm.read += since(t0);
        t0 = Clock::now();
        if (!read_ok) throw std::runtime_error("cannot read " + path);
        const size_t off = cur->off + cur->want;
        const bool at_eof = off >= file_size;
        const PieceCutter::Cut c = cutter.cut(cur->b, cur->want, at_eof, off < read_end, cur->tab, max_blocks);
        if (c.too_many_members) return FeedEnd::kTooManyMembers;
        tm.scan += since(t0);
        t0 = Clock::now();
        const int src = bdx_bamdec_submit(dec, c.base + c.bytes, c.nblocks, at_eof ? 1 : 0);
        // (a stretch that inflates beyond what the ring was sized for, ...: the host reader's)
        if (src == BDX_ELIMIT && job.may_be_unsupported) return FeedEnd::kRefusedInSubmit;
        check(src, "bdx_bamdec_submit", dec, path);
        tm.submit += since(t0);
        if (at_eof) return FeedEnd::kFed;
        if (off >= read_end) return FeedEnd::kFed;   // (the end of the sequence's span: the stream is cut here, bdx_bamdec_finish drops a record that runs past it)
        if (at.seeked) {   // a region read through the index: nothing of it lies behind the first record past it
            int past = 0;
            check(bdx_bamdec_progress(dec, nullptr, nullptr, &past, nullptr), "bdx_bamdec_progress", dec, path);
            if (past) return FeedEnd::kFed;
        }
    }
}

enum HostMs {   // bdx_bamdec_host_ms, include/bdx.h
    kStagingWait, kStagingPinning, kSlotWait, kSlotBuffers, kCopyCalls, kBatchLaunches, kRecordStages, kClassifierFeed,
    kFirstInflateAt, kFinishedAt, kSizingLaterStages, kClassifierLaunches, kInflateKernel, kInflateLaunches, kHostMsCount
};

void report_feed_timing(const bdx_bamdec* dec, const FeedTimes& tm, size_t fed_bytes, int threads) {
    float hm[kHostMsCount];
    if (bdx_bamdec_host_ms(dec, hm, kHostMsCount) == BDX_OK) {
        if (hm[kInflateLaunches] > 0) {
            uint64_t cb = 0, ib = 0, np_ = 0, tw = 0;
            (void)bdx_bamdec_stats(dec, &cb, &ib, &np_, &tw);
            fprintf(stderr, "[bdx timing] inflate kernel in the pipeline: %.1f ms in %d launches (HIP events), %.3f GB inflated from %.3f GB: %.1f GB/s of inflated bytes\n",
                    hm[kInflateKernel], (int)hm[kInflateLaunches], (double)ib * 1e-9, (double)cb * 1e-9, hm[kInflateKernel] > 0 ? (double)ib * 1e-6 / hm[kInflateKernel] : 0.0);
        }
        fprintf(stderr, "[bdx timing] of the classifier feed: sizing the later stages %.1f ms, classifier launches %.1f ms\n", hm[kSizingLaterStages], hm[kClassifierLaunches]);
        // (the rate the file moves at once the GPU has its first batch: what a file of any size approaches)
        const double steady = (hm[kFinishedAt] - hm[kFirstInflateAt]) * 1e-3;
        fprintf(stderr, "[bdx timing] steady state: %.3f GB of BAM (%zu pieces) between the first inflate launch (%.3f s after the decoder's set-up) and the last record "
                        "(%.3f s): %.3f s, %.2f GB/s\n", (double)fed_bytes * 1e-9, tm.npieces, hm[kFirstInflateAt] * 1e-3, hm[kFinishedAt] * 1e-3, steady,
                steady > 0 ? (double)fed_bytes * 1e-9 / steady : 0.0);
        fprintf(stderr, "[bdx timing] inside the decoder (ms): staging wait %.1f, staging pinning %.1f, slot wait %.1f, slot buffers %.1f, copy calls %.1f, "
                        "batch launches %.1f (of which record stages %.1f), classifier feed %.1f\n", hm[kStagingWait], hm[kStagingPinning], hm[kSlotWait], hm[kSlotBuffers],
                hm[kCopyCalls], hm[kBatchLaunches], hm[kRecordStages], hm[kClassifierFeed]);
    }
    fprintf(stderr, "[bdx timing] device decode: decoder set up in %.3f s; %zu pieces; waiting for a staging buffer %.3f s, reading the file %.3f s (%d threads), member tables %.3f s, "
                    "enqueueing %.3f s, waiting for the GPU at the end %.3f s\n", tm.create, tm.npieces, tm.acquire, tm.read, threads, tm.scan, tm.submit, tm.finish);
}

}  // namespace

void retire(bdx_bamdec* d) {
    if (!d) return;
    std::lock_guard<std::mutex> lk(g_retired_mu);
    g_retired.push_back(d);
}

void release_device_decoders() {
    std::lock_guard<std::mutex> lk(g_retired_mu);
    for (bdx_bamdec* d : g_retired) bdx_bamdec_destroy(d);
    g_retired.clear();
}

DecodeResult decode_on_device(const DecodeJob& job) {
    const std::string& path = job.cfg.bam_files()[job.bam_index];
    const FeedKnobs knobs = FeedKnobs::from_env();
    ColumnReader hdr(path, 1, nullptr);   // (the header: reference names, where the first record lies; the index for -o)
    const Located at = locate(job, hdr, path);
    const FeedPlan fp = plan(job, hdr, at, knobs);
    DecodeResult res;
    FeedTimes tm;
    const auto t_create = Clock::now();
    bdx_bamdec* dec = open_decoder(job, hdr, at, fp, &res.decoder);
    tm.create = since(t_create);
    const FeedEnd end = feed(dec, job, hdr, path, at, fp, knobs, tm);
    uint64_t n = 0;
    const auto tf = Clock::now();
    int rc = bdx_bamdec_finish(dec, &n);   // (also when a piece was refused: what is in flight is waited for before the caller starts over)
    if (end == FeedEnd::kRefusedInSubmit) rc = BDX_ELIMIT;
    tm.finish = since(tf);
    if (knobs.timing) report_feed_timing(dec, tm, fp.read_end - at.member_off, job.threads);
    if ((rc == BDX_ELIMIT || end == FeedEnd::kTooManyMembers) && job.may_be_unsupported) { res.unsupported = true; return res; }
    if (end == FeedEnd::kTooManyMembers) throw std::runtime_error("too many BGZF members in a piece: " + path);
    check(rc, "bdx_bamdec_finish", dec, path);
    if (job.exclude) check(bdx_bamdec_excluded(dec, &res.excluded), "bdx_bamdec_excluded", dec, path);
    res.n = (size_t)n;
    return res;
}

}  // namespace bdhost
