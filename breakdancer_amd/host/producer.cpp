#include "producer.h"

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <thread>
#include <queue>
#include <stdexcept>
#include <future>
#include <unordered_map>

#include "bam_reader.h"
#include "column_reader.h"
#include "device_feed.h"
#include "feed_plan.h"

namespace bdhost {

bdx_batch ReadStream::batch() const {
    bdx_batch b;
    b.tid = tid.data(); b.pos = pos.data(); b.mtid = mtid.data(); b.mpos = mpos.data(); b.isize = isize.data();
    b.flag = flag.data(); b.qlen = qlen.data(); b.mapq = mapq.data(); b.lib = lib.data(); b.bam = bam.data();
    b.name_key = name_key.data();
    b.name_check = name_check.data();
    b.n = size();
    return b;
}

namespace {

struct Stream {
    std::unique_ptr<BamReader> rd;
    int bam_index = 0;
    int only_tid = -1;
    int beg = 0, end = 1 << 29;
    bdx::ExcludeMask exclude{nullptr, nullptr, nullptr, 0};   // --exclude (csrc/bdx_exclude.h); ntids == 0: none
    uint64_t excluded = 0;   // records the mask dropped
    BamRecord cur{};
    bool valid = false;
    // reader filter of the reference: primary (not secondary / supplementary) and tid >= 0
    // (io/AlignmentFilter.hpp:24-34, io/BamIo.cpp:11-18); -o keeps one tid (RegionLimitedBamReader.hpp:63-71)
    bool advance() {
        while (rd->next(cur)) {
            if (cur.flag & (0x100 | 0x800)) continue;
            if (cur.tid < 0) continue;
            // bam_iter_read keeps the records of the region that overlap it (bam_index.c:571-576 is_overlap)
            if (only_tid >= 0 && (cur.tid != only_tid || !((uint32_t)cur.end_pos > (uint32_t)beg && (uint32_t)cur.pos < (uint32_t)end))) continue;
            if (exclude.ntids && bdx::exclude_record(exclude, cur.tid, cur.pos, cur.mtid, cur.mpos)) { ++excluded; continue; }
            return valid = true;
        }
        return valid = false;
    }
};

struct StreamGreater {  // BamMerger::Stream::operator> (io/BamMerger.cpp:40-61), adapted through deref_compare
    bool operator()(const Stream* a, const Stream* b) const {
        const BamRecord &x = a->cur, &y = b->cur;
        if (x.tid > y.tid) return true;
        if (y.tid > x.tid) return false;
        if (x.pos > y.pos) return true;
        if (y.pos > x.pos) return false;
        return ((x.flag >> 4) & 1) > ((y.flag >> 4) & 1);
    }
};


// opens the BAMs and runs the k-way merge, calling f(stream_index, record, bam_index, library) per merged record; returns the records
// the --exclude mask dropped
template <class F>
uint64_t merge_streams(const BamConfig& cfg, const std::string& chr, const ExcludeTable* ex, int threads, std::vector<std::string>* targets, F&& f) {
    std::vector<std::unique_ptr<Stream>> streams;
    for (size_t b = 0; b < cfg.num_bams(); ++b) {
        std::unique_ptr<Stream> s(new Stream);
        s->rd.reset(new BamReader(cfg.bam_files()[b], threads));
        s->bam_index = (int)b;
        if (ex) s->exclude = ex->mask();
        if (!chr.empty() && !parse_region(*s->rd, chr, s->only_tid, s->beg, s->end))
            throw std::runtime_error("Failed to parse bam region '" + chr + "' in file " + cfg.bam_files()[b] + ". ");
        streams.push_back(std::move(s));
    }
    if (streams.empty()) throw std::runtime_error("BamMerger created with no input streams!");
    if (targets) *targets = streams[0]->rd->target_names();

    // read-group string -> library index (io/BamConfig.hpp:62-72), cached per distinct RG value
    std::unordered_map<std::string, uint8_t> rg_cache;
    for (auto const& kv : cfg.readgroup_index()) rg_cache[kv.first] = (uint8_t)kv.second;
    const uint8_t fallback = (uint8_t)cfg.fallback_library();

    std::priority_queue<Stream*, std::vector<Stream*>, StreamGreater> pq;
    for (auto& s : streams)
        if (s->advance()) pq.push(s.get());
    // The records were decoded on other cores: their bytes are cold here, so runs of one read group are recognised by the
    // 64-bit key the decoder computed, and the RG string itself is only read the first time a key is seen.
    std::string rgtmp;
    std::unordered_map<uint64_t, uint8_t> by_key;
    uint64_t last_key = ~0ull;
    uint8_t last_lib = fallback;
    uint64_t index = 0;
    auto excluded = [&] {
        uint64_t n = 0;
        for (auto& s : streams) n += s->excluded;
        return n;
    };
    auto lib_of = [&](const BamRecord& r) {
        if (r.rg_key == last_key) return last_lib;  // runs of one RG
        auto hit = by_key.find(r.rg_key);  // (a key stands for its string: two RG ids with one 64-bit key are not expected)
        if (hit == by_key.end()) {
            rgtmp.assign(r.rg ? r.rg : "", r.rg ? r.l_rg : 0);
            auto it = rg_cache.find(rgtmp);
            hit = by_key.emplace(r.rg_key, it != rg_cache.end() ? it->second : fallback).first;
        }
        last_key = r.rg_key;
        return last_lib = hit->second;
    };
    if (pq.size() == 1) {  // one BAM: nothing to merge
        Stream* s = pq.top();
        do {
            f(index++, s->cur, s->bam_index, lib_of(s->cur));
        } while (s->advance());
        return excluded();
    }
    while (!pq.empty()) {
        Stream* s = pq.top();
        pq.pop();
        const BamRecord& r = s->cur;
        f(index++, r, s->bam_index, lib_of(r));
        if (s->advance()) pq.push(s);
    }
    return excluded();
}

}  // namespace

namespace {

// appends records to the sink's current batch and submits it when it is full
class BatchWriter {
public:
    BatchWriter(BatchSink& sink, size_t batch_records) : sink_(sink), batch_(batch_records) {}
    void append_range(const ColumnChunk& c, size_t lo, size_t hi, uint8_t bam) {
        while (lo < hi) {
            if (!open_) open();
            const size_t m = std::min(hi - lo, buf_.capacity - used_);
            memcpy(buf_.tid + used_, c.tid.data() + lo, m * 4); memcpy(buf_.pos + used_, c.pos.data() + lo, m * 4);
            memcpy(buf_.mtid + used_, c.mtid.data() + lo, m * 4); memcpy(buf_.mpos + used_, c.mpos.data() + lo, m * 4);
            memcpy(buf_.isize + used_, c.isize.data() + lo, m * 4);
            memcpy(buf_.flag + used_, c.flag.data() + lo, m * 2); memcpy(buf_.qlen + used_, c.qlen.data() + lo, m * 2);
            memcpy(buf_.mapq + used_, c.mapq.data() + lo, m); memcpy(buf_.lib + used_, c.lib.data() + lo, m);
            memset(buf_.bam + used_, bam, m);
            memcpy(buf_.name_key + used_, c.name_key.data() + lo, m * 8);
            memcpy(buf_.name_check + used_, c.name_check.data() + lo, m * 8);
            memcpy(clip_.data() + used_, c.clip.data() + lo, m * 4);
            used_ += m; lo += m; total_ += m;
            if (used_ == buf_.capacity) close();
        }
    }
    void append_one(const ColumnChunk& c, size_t i, uint8_t bam) {
        if (!open_) open();
        const size_t u = used_;
        buf_.tid[u] = c.tid[i]; buf_.pos[u] = c.pos[i]; buf_.mtid[u] = c.mtid[i]; buf_.mpos[u] = c.mpos[i]; buf_.isize[u] = c.isize[i];
        buf_.flag[u] = c.flag[i]; buf_.qlen[u] = c.qlen[i]; buf_.mapq[u] = c.mapq[i]; buf_.lib[u] = c.lib[i]; buf_.bam[u] = bam;
        buf_.name_key[u] = c.name_key[i];
        buf_.name_check[u] = c.name_check[i];
        clip_[u] = c.clip[i];
        ++used_; ++total_;
        if (used_ == buf_.capacity) close();
    }
    void finish() { if (open_) close(); }
    size_t total() const { return total_; }

private:
    void open() {
        const auto t0 = std::chrono::steady_clock::now();
        buf_ = sink_.acquire(batch_); used_ = 0; open_ = true;
        if (clip_.size() < buf_.capacity) clip_.resize(buf_.capacity);
        acquire_s_ += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    }
    void close() {
        const auto t0 = std::chrono::steady_clock::now();
        sink_.clip = clip_.data();
        sink_.submit(used_); open_ = false;
        sink_.clip = nullptr;
        submit_s_ += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    }
public:
    double acquire_s_ = 0, submit_s_ = 0, copy_s_ = 0;
private:
    BatchSink& sink_;
    size_t batch_;
    bdx_batch_buf buf_{};
    std::vector<uint32_t> clip_;   // the clip words of the batch being filled (BatchSink::clip)
    size_t used_ = 0, total_ = 0;
    bool open_ = false;
};

struct Cursor {  // one file's position in the merge: record i of the chunk the reader handed out last
    std::unique_ptr<ColumnReader> rd;
    const ColumnChunk* chunk = nullptr;
    size_t i = 0;
    uint8_t bam = 0;
    bool advance() {  // to the next record; false at the end of the file
        if (chunk && ++i < chunk->size()) return true;
        do {
            chunk = rd->next();
            i = 0;
        } while (chunk && chunk->size() == 0);
        return chunk != nullptr;
    }
    bool first() {
        do {
            chunk = rd->next();
            i = 0;
        } while (chunk && chunk->size() == 0);
        return chunk != nullptr;
    }
};

struct CursorGreater {  // BamMerger::Stream::operator> (io/BamMerger.cpp:40-61): tid, pos, strand
    bool operator()(const Cursor* a, const Cursor* b) const {
        const ColumnChunk &x = *a->chunk, &y = *b->chunk;
        const size_t i = a->i, j = b->i;
        if (x.tid[i] > y.tid[j]) return true;
        if (y.tid[j] > x.tid[i]) return false;
        if (x.pos[i] > y.pos[j]) return true;
        if (y.pos[j] > x.pos[i]) return false;
        return ((x.flag[i] >> 4) & 1) > ((y.flag[j] >> 4) & 1);
    }
};

struct VectorSink : BatchSink {  // batches appended to a ReadStream
    ReadStream& out;
    size_t base = 0;
    explicit VectorSink(ReadStream& o) : out(o) {}
    bdx_batch_buf acquire(size_t cap) override {
        base = out.size();
        const size_t n = base + cap;
        out.tid.resize(n); out.pos.resize(n); out.mtid.resize(n); out.mpos.resize(n); out.isize.resize(n); out.flag.resize(n);
        out.qlen.resize(n); out.mapq.resize(n); out.lib.resize(n); out.bam.resize(n); out.name_key.resize(n); out.name_check.resize(n);
        bdx_batch_buf b{};
        b.tid = out.tid.data() + base; b.pos = out.pos.data() + base; b.mtid = out.mtid.data() + base; b.mpos = out.mpos.data() + base;
        b.isize = out.isize.data() + base; b.flag = out.flag.data() + base; b.qlen = out.qlen.data() + base;
        b.mapq = out.mapq.data() + base; b.lib = out.lib.data() + base; b.bam = out.bam.data() + base;
        b.name_key = out.name_key.data() + base;
        b.name_check = out.name_check.data() + base;
        b.capacity = cap;
        return b;
    }
    void submit(size_t n) override {
        const size_t m = base + n;
        out.tid.resize(m); out.pos.resize(m); out.mtid.resize(m); out.mpos.resize(m); out.isize.resize(m); out.flag.resize(m);
        out.qlen.resize(m); out.mapq.resize(m); out.lib.resize(m); out.bam.resize(m); out.name_key.resize(m); out.name_check.resize(m);
    }
};

}  // namespace

size_t produce_stream(const BamConfig& cfg, const std::string& chr, const ExcludeTable* ex, int threads, std::vector<std::string>* targets, BatchSink& sink,
                      size_t batch_records) {
    const LibraryResolver libs(cfg);
    const size_t nb = cfg.num_bams();
    if (nb == 0) throw std::runtime_error("BamMerger created with no input streams!");
    const int per = std::max(1, threads / (int)nb);
    std::vector<std::unique_ptr<Cursor>> cur;
    for (size_t b = 0; b < nb; ++b) {
        std::unique_ptr<Cursor> c(new Cursor);
        c->rd.reset(new ColumnReader(cfg.bam_files()[b], per, &libs));
        c->bam = (uint8_t)b;
        RecordFilter f;
        if (ex) f.exclude = ex->mask();
        if (!chr.empty() && !parse_region(*c->rd, chr, f.only_tid, f.beg, f.end))
            throw std::runtime_error("Failed to parse bam region '" + chr + "' in file " + cfg.bam_files()[b] + ". ");
        c->rd->start(f);
        cur.push_back(std::move(c));
    }
    if (targets) *targets = cur[0]->rd->target_names();
    BatchWriter w(sink, batch_records);
    if (nb == 1) {  // one file: nothing to merge, whole chunks are copied
        Cursor& c = *cur[0];
        while (const ColumnChunk* ch = c.rd->next()) {
            const auto t0 = std::chrono::steady_clock::now();
            if (ch->size()) w.append_range(*ch, 0, ch->size(), c.bam);
            w.copy_s_ += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        }
        w.finish();
        if (getenv("BDX_BAM_PROFILE"))
            fprintf(stderr, "[producer] consumer: copying into batches %.3f s (of which acquire %.3f s, submit %.3f s)\n", w.copy_s_, w.acquire_s_, w.submit_s_);
        if (ex) ex->dropped += c.rd->excluded();
        return w.total();
    }
    // the reference's k-way merge: a priority queue on (tid, pos, strand), same push / pop sequence as BamMerger
    std::priority_queue<Cursor*, std::vector<Cursor*>, CursorGreater> pq;
    for (auto& c : cur)
        if (c->first()) pq.push(c.get());
    while (!pq.empty()) {
        Cursor* c = pq.top();
        pq.pop();
        w.append_one(*c->chunk, c->i, c->bam);
        if (c->advance()) pq.push(c);
    }
    w.finish();
    if (ex)
        for (auto& c : cur) ex->dropped += c->rd->excluded();
    return w.total();
}


namespace {

// BamMerger's order over the files' (tid, pos, strand) columns: the same priority queue, the same push / pop sequence as the host
// producer's merge (io/BamMerger.cpp:40-61, 78-110).  One short cut, for queues that hold at most ONE other file (two files in all,
// the tumour / normal case): while the file just taken from stays STRICTLY below the other it would come out on top again, so its
// records are taken without touching the queue.  With more files every record goes through the queue: a push that rises to the top
// and the pop behind it rearrange the others, and their arrangement is what decides the ties that follow.
struct KeyCursor {
    const int32_t *tid, *pos;
    const uint16_t* flag;
    size_t i, n;
    uint8_t file;
};
struct KeyGreater {
    bool operator()(const KeyCursor* a, const KeyCursor* b) const {
        const size_t i = a->i, j = b->i;
        if (a->tid[i] > b->tid[j]) return true;
        if (b->tid[j] > a->tid[i]) return false;
        if (a->pos[i] > b->pos[j]) return true;
        if (b->pos[j] > a->pos[i]) return false;
        return ((a->flag[i] >> 4) & 1) > ((b->flag[j] >> 4) & 1);
    }
};

}  // namespace

namespace {

// Two files.  What the priority queue does with two streams is a rule with one bit of memory: the file that emitted last goes on
// only while its next record is STRICTLY below the other file's; otherwise the other file is taken (ties: the file that waited).
// Nothing ahead of a key influences what happens below it, so the merge can be cut wherever the memory cannot matter -- at a key
// that only ONE of the files holds -- and the pieces merged by threads of their own.
struct TwoWay {
    const int32_t *tid[2], *pos[2];
    const uint16_t* flag[2];
    size_t n[2];
    bool less(int a, size_t i, int b, size_t j) const {   // (tid, pos, strand): io/BamMerger.cpp:40-61
        if (tid[a][i] != tid[b][j]) return tid[a][i] < tid[b][j];
        if (pos[a][i] != pos[b][j]) return pos[a][i] < pos[b][j];
        return ((flag[a][i] >> 4) & 1) < ((flag[b][j] >> 4) & 1);
    }
    // records [i, ie) of file 0 and [j, je) of file 1 into the output from i + j on; `last`: the file that emitted before them
    void merge(size_t i, size_t ie, size_t j, size_t je, int last, uint8_t* src_file, uint32_t* src_index) const {
        size_t o = i + j;
        while (i < ie && j < je) {
            const bool take0 = last == 0 ? less(0, i, 1, j) : !less(1, j, 0, i);
            if (take0) { src_file[o] = 0; src_index[o] = (uint32_t)i; ++i; last = 0; }
            else { src_file[o] = 1; src_index[o] = (uint32_t)j; ++j; last = 1; }
            ++o;
        }
        for (; i < ie; ++i, ++o) { src_file[o] = 0; src_index[o] = (uint32_t)i; }
        for (; j < je; ++j, ++o) { src_file[o] = 1; src_index[o] = (uint32_t)j; }
    }
    // (a file is sorted by reference and position; the strands at one position come in any order: seams are sought by position)
    bool before(int a, size_t i, int b, size_t j) const { return tid[a][i] != tid[b][j] ? tid[a][i] < tid[b][j] : pos[a][i] < pos[b][j]; }
    size_t lower_bound(int f, int kf, size_t ki) const {   // first record of file f whose position is not before that of record ki of file kf
        size_t lo = 0, hi = n[f];
        while (lo < hi) {
            const size_t mid = (lo + hi) / 2;
            if (before(f, mid, kf, ki)) lo = mid + 1; else hi = mid;
        }
        return lo;
    }
};

void merge_two(const TwoWay& w, int threads, uint8_t* src_file, uint32_t* src_index, int first_last = 1) {
    // seams: (i, j) with every record before them at a position before every record behind them, and file 1 holding nothing at record i's position
    std::vector<std::pair<size_t, size_t>> seam{{0, 0}};
    const int want = std::max(1, threads);
    for (int t = 1; t < want; ++t) {
        size_t i = w.n[0] * (size_t)t / (size_t)want;
        bool found = false;
        for (int tries = 0; tries < 64 && i < w.n[0]; ++tries) {
            i = w.lower_bound(0, 0, i);                    // the first record of file 0 at this position
            const size_t j = w.lower_bound(1, 0, i);
            if (j == w.n[1] || w.before(0, i, 1, j)) {     // file 1 has no record there: the seam cannot see a tie
                if (i > seam.back().first || j > seam.back().second) seam.emplace_back(i, j);
                found = true;
                break;
            }
            size_t lo = i, hi = w.n[0];                    // on to file 0's next position
            while (lo < hi) {
                const size_t mid = (lo + hi) / 2;
                if (!w.before(0, i, 0, mid)) lo = mid + 1; else hi = mid;
            }
            i = lo;
        }
        (void)found;   // (no seam here: the piece before it is simply longer)
    }
    seam.emplace_back(w.n[0], w.n[1]);
    std::vector<std::thread> th;
    for (size_t s = 0; s + 1 < seam.size(); ++s) {
        // (the file that emitted before a seam: nothing at a seam depends on it; the very first piece starts as the queue does -- file 0 on a tie)
        // (first_last: the caller merges a stretch of a longer stream and knows which file emitted in front of it)
        const int last = s == 0 ? first_last : 1;
        auto job = [&w, &seam, s, last, src_file, src_index] { w.merge(seam[s].first, seam[s + 1].first, seam[s].second, seam[s + 1].second, last, src_file, src_index); };
        if (s + 2 < seam.size()) th.emplace_back(job); else job();
    }
    for (auto& t : th) t.join();
}

}  // namespace

void merge_order(const std::vector<const int32_t*>& tid, const std::vector<const int32_t*>& pos, const std::vector<const uint16_t*>& flag,
                 const std::vector<size_t>& n, std::vector<uint8_t>& src_file, std::vector<uint32_t>& src_index, int threads, int emitted_last) {
    const size_t k = n.size();
    size_t total = 0;
    for (size_t b = 0; b < k; ++b) total += n[b];
    src_file.resize(total);
    src_index.resize(total);
    if (k == 2 && threads > 0) {
        const TwoWay w{{tid[0], tid[1]}, {pos[0], pos[1]}, {flag[0], flag[1]}, {n[0], n[1]}};
        merge_two(w, total < ((size_t)1 << 16) && threads < 1000 ? 1 : std::min(threads, 64), src_file.data(), src_index.data(), emitted_last == 0 ? 0 : 1);
        return;
    }
    std::vector<KeyCursor> cur(k);
    std::priority_queue<KeyCursor*, std::vector<KeyCursor*>, KeyGreater> pq;
    for (size_t b = 0; b < k; ++b) {
        cur[b] = KeyCursor{tid[b], pos[b], flag[b], 0, n[b], (uint8_t)b};
        if (n[b]) pq.push(&cur[b]);
    }
    const KeyGreater greater;
    size_t o = 0;
    while (!pq.empty()) {
        KeyCursor* c = pq.top();
        pq.pop();
        src_file[o] = c->file; src_index[o] = (uint32_t)c->i; ++o;
        ++c->i;
        while (c->i < c->n && (pq.empty() || (pq.size() == 1 && greater(pq.top(), c)))) {   // strictly below the only other file
            src_file[o] = c->file; src_index[o] = (uint32_t)c->i; ++o;
            ++c->i;
        }
        if (c->i < c->n) pq.push(c);
    }
}

namespace {

// tid, pos and flag of a decoder's records, on the host: what BamMerger's order looks at (io/BamMerger.cpp:40-61)
struct KeyColumns {
    std::vector<int32_t> tid, pos;
    std::vector<uint16_t> flag;
    void fetch(bdx_bamdec* dec, size_t n) {
        tid.resize(n); pos.resize(n); flag.resize(n);
        bdx_batch_buf out{};
        out.tid = tid.data(); out.pos = pos.data(); out.flag = flag.data();
        out.capacity = n;
        const int rc = bdx_bamdec_fetch(dec, 0, n, &out);
        if (rc != BDX_OK) throw std::runtime_error(std::string("bdx_bamdec_fetch: ") + bdx_strerror(rc) + " (" + bdx_bamdec_last_error(dec) + ")");
    }
};

struct MergeTimes { double decoded = 0, keys = 0, ordered = 0, gathered = 0; };   // seconds from the start to the end of each step

// Several files over one stretch: each decoded into its decoder's own columns, the merge order worked out from three of them, one
// gather in HBM.  false: the device path gives the stretch up (nothing of it counts); else *total records were gathered.
//   decode(b, &dec)              file b through a decoder without a sink: *dec and its records; false: unsupported
//   emitted_last(pos, flag, n)   what merge_order is to assume of the stream in front of these records
//   gather(decs, k, src_file, src_index, total)   bdx_merge_decoded or bdx_append_decoded; false: unsupported
// overlap: a file's key columns come to the host while the next file is decoded
template <class Decode, class EmittedLast, class Gather>
bool decode_merge_gather(const std::vector<size_t>& files, std::vector<KeyColumns>& keys, bool overlap, int threads, Decode&& decode,
                         EmittedLast&& emitted_last, Gather&& gather, size_t* total, MergeTimes* tm = nullptr) {
    const auto t0 = std::chrono::steady_clock::now();
    auto since = [&] { return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(); };
    MergeTimes times;
    std::vector<size_t> n;
    std::vector<bdx_bamdec*> decs;
    std::vector<std::future<void>> fetched;   // (their destructors wait: whatever ends the loop, no fetch outlives it)
    *total = 0;
    for (size_t b : files) {
        bdx_bamdec* dec = nullptr;
        size_t nr = 0;
        if (!decode(b, &dec, &nr)) return false;
        n.push_back(nr); decs.push_back(dec);
        *total += nr;
        KeyColumns& k = keys[b];
        if (overlap) fetched.push_back(std::async(std::launch::async, [&k, dec, nr] { k.fetch(dec, nr); }));
        else k.fetch(dec, nr);
    }
    times.decoded = since();
    for (auto& f : fetched) f.get();
    times.keys = since();
    std::vector<const int32_t*> ptid, ppos;
    std::vector<const uint16_t*> pflag;
    for (size_t b : files) { ptid.push_back(keys[b].tid.data()); ppos.push_back(keys[b].pos.data()); pflag.push_back(keys[b].flag.data()); }
    std::vector<uint8_t> src_file;
    std::vector<uint32_t> src_index;
    // (BamMerger's order among the files that hold the stretch: a file without records of it is not in the queue at that point either)
    merge_order(ptid, ppos, pflag, n, src_file, src_index, std::max(1, threads), emitted_last(ppos, pflag, n));
    times.ordered = since();
    const bool ok = gather(decs.data(), (int)decs.size(), src_file.data(), src_index.data(), *total);
    times.gathered = since();
    if (tm) *tm = times;
    return ok;
}

// (tid, pos, strand) of the LAST record of sequence tid in a file, by the host reader through the index: the tail of the sequence is
// decoded (a window of 32 kb in front of the sequence's end, widened while it holds no record).  false: the file has none
bool last_key_of(const std::string& path, int tid, const ExcludeTable* ex, int32_t* pos, int* strand) {
    for (int64_t back = 2 * 16384;; back *= 32) {
        ColumnReader rd(path, 1, nullptr);
        const int64_t len = (size_t)tid < rd.target_lengths().size() ? (int64_t)rd.target_lengths()[tid] : ((int64_t)1 << 29);
        RecordFilter f;
        f.only_tid = tid;
        f.beg = (int)std::max<int64_t>(0, len - back);
        f.end = 0x7FFFFFFF;
        if (ex) f.exclude = ex->mask();   // (a record the run does not see did not emit anything)
        rd.start(f);
        bool any = false;
        while (const ColumnChunk* c = rd.next())
            if (c->size()) { any = true; *pos = c->pos.back(); *strand = (c->flag.back() >> 4) & 1; }
        if (any) return true;
        if (f.beg == 0) return false;
    }
}

struct ShardedRun {   // what the ranks' threads share, read only
    const BamConfig& cfg;
    const ExcludeTable* ex;
    const std::vector<std::string>& names;
    const std::vector<std::vector<FileSpan>>& span;   // [file][sequence]
    const std::vector<bdx_dist*>& ranks;
    const std::vector<int>& devices;
    const std::vector<int>& rank_of;
    int per;   // threads of a rank
    bool timing;
    bool clips;   // --clip: the ranks' contexts and the decoders keep clip words
};

struct RankOutcome {
    size_t n = 0;
    uint64_t excluded = 0;   // (added to ex->dropped only when every rank came through: a run that starts over counts afresh)
    bool gave_up = false;    // a stretch the device path does not take: the caller starts over with the host producer
    std::string error;
};

// Rank r's chromosomes, one after the other, into bdx_dist_chromosome(ranks[r], t): ONE decoder per file, armed again for every chromosome
void decode_rank(const ShardedRun& run, int r, RankOutcome& out) {
    const size_t nb = run.cfg.num_bams();
    size_t bytes_mine = 0;
    std::vector<size_t> largest(nb, 0);
    for (size_t b = 0; b < nb; ++b)
        for (size_t t = 0; t < run.names.size(); ++t)
            if (run.rank_of[t] == r && run.span[b][t].has) {
                bytes_mine += run.span[b][t].end - run.span[b][t].begin;
                largest[b] = std::max(largest[b], run.span[b][t].end - run.span[b][t].begin);
            }
    const size_t largest_any = *std::max_element(largest.begin(), largest.end());
    bool reserved = false;
    std::vector<OwnedDecoder> decs(nb);
    std::vector<KeyColumns> keys(nb);
    for (size_t t = 0; t < run.names.size() && !out.gave_up; ++t) {
        if (run.rank_of[t] != r) continue;
        std::vector<size_t> files;   // the files that hold records of this chromosome
        for (size_t b = 0; b < nb; ++b)
            if (run.span[b][t].has) files.push_back(b);
        if (files.empty()) continue;
        bdx_ctx* c = bdx_dist_chromosome(run.ranks[r], (int)t);
        if (!c) throw std::runtime_error(std::string("bdx_dist_chromosome: ") + bdx_dist_last_error(run.ranks[r]));
        if (bdx_use_name_check(c, 1) != BDX_OK) throw std::runtime_error("bdx_use_name_check");
        if (run.clips && bdx_use_clips(c, 1) != BDX_OK) throw std::runtime_error(std::string("bdx_use_clips: ") + bdx_last_error(c));
        if (!reserved) {   // the rank's store for ALL of its chromosomes (a record takes 50-150 bytes of BAM): no growing between them
            // (plus what the decoder must assume of a batch in flight before its records are counted: 36 bytes is the smallest record)
            if (bdx_reserve(c, std::min<size_t>(bytes_mine / 48 + largest_any * 8 / 36 + ((size_t)1 << 20), 0xFFFFFFFFull - 1024)) != BDX_OK) throw std::runtime_error("bdx_reserve");
            reserved = true;
        }
        const auto tc = std::chrono::steady_clock::now();
        auto decode = [&](size_t b, bdx_ctx* sink, bdx_bamdec** dec, size_t* n) {
            DecodeJob job{run.cfg, b};
            job.whole_tid = (int)t; job.span_bytes = run.span[b][t].end - run.span[b][t].begin;
            job.exclude = run.ex; job.threads = run.per; job.device = run.devices[r]; job.sink = sink;
            job.rearm = decs[b].get(); job.sized_for = largest[b]; job.may_be_unsupported = true; job.clips = run.clips;
            DecodeResult res = decode_on_device(job);
            if (res.decoder) decs[b] = std::move(res.decoder);
            out.excluded += res.excluded;
            *dec = decs[b].get(); *n = res.n;
            return !res.unsupported;
        };
        if (nb == 1) {
            bdx_bamdec* dec = nullptr;
            out.gave_up = !decode(0, c, &dec, &out.n);   // (the decoder reports the store's record count: the rank's total so far)
        } else {
            size_t total = 0;
            out.gave_up = !decode_merge_gather(
                files, keys, false, run.per, [&](size_t b, bdx_bamdec** dec, size_t* n) { return decode(b, nullptr, dec, n); },
                [&](const std::vector<const int32_t*>& pos, const std::vector<const uint16_t*>& flag, const std::vector<size_t>& n) {
                    if (files.size() != 2 || !n[0] || !n[1] || pos[0][0] != pos[1][0] || ((flag[0][0] >> 4) & 1) != ((flag[1][0] >> 4) & 1)) return 1;
                    return file_that_emitted_last(run.span, files, (int)t, [&](size_t file, int tid, int32_t* p, int* strand) {
                        return last_key_of(run.cfg.bam_files()[file], tid, run.ex, p, strand);
                    });
                },
                [&](bdx_bamdec* const* d, int k, const uint8_t* src_file, const uint32_t* src_index, size_t n) {
                    const int rc = bdx_append_decoded(c, d, k, src_file, src_index, n);
                    if (rc != BDX_OK && rc != BDX_ELIMIT) throw std::runtime_error(std::string("bdx_append_decoded: ") + bdx_strerror(rc) + " (" + bdx_last_error(c) + ")");
                    return rc == BDX_OK;
                },
                &total);
            if (!out.gave_up) out.n += total;
        }
        if (run.timing && !out.gave_up)
            fprintf(stderr, "[bdx timing] rank %d: %s (%zu file%s) in %.3f s\n", r, run.names[t].c_str(), files.size(), files.size() == 1 ? "" : "s",
                    std::chrono::duration<double>(std::chrono::steady_clock::now() - tc).count());
    }
}

}  // namespace

// Indexed BAMs, the chromosomes of one whole-genome run spread over ranks (bdx_dist_*): every rank's thread reads the BGZF ranges of ITS
// chromosomes (the index says where they lie) and decodes them on ITS GPU -- the reference's answer to "one chromosome" is the same indexed
// seek (io/RegionLimitedBamReader.hpp:43-71: bam_index_load, bam_iter_query).  ONE file: straight into the rank's context.  SEVERAL files
// (the tumour / normal pair): per chromosome one decoder per file over that file's range (the decoders are the rank's, armed again for every
// chromosome), the merge order worked out from three columns as for one GPU (merge_order: BamMerger's queue, io/BamMerger.cpp:40-126),
// one gather in HBM behind what the rank's store holds (bdx_append_decoded).  Nothing is decoded twice and no record crosses the host.
// unsupported: a file without an index (or one that does not cover the header's sequences), nothing was done.
size_t produce_sharded_on_device(const BamConfig& cfg, const ExcludeTable* ex, int threads, std::vector<std::string>* targets, const std::vector<bdx_dist*>& ranks,
                                 const std::vector<int>& devices, const std::vector<int>& rank_of, bool* unsupported, bool clips) {
    *unsupported = true;
    const size_t nb = cfg.num_bams();
    if (nb < 1 || nb > 16) return 0;
    std::vector<std::string> names;
    std::vector<std::vector<FileSpan>> span(nb);
    for (size_t b = 0; b < nb; ++b) {
        ColumnReader hdr(cfg.bam_files()[b], 1, nullptr);
        if (b == 0) names = hdr.target_names();
        else if (hdr.target_names() != names) return 0;   // (files that disagree about the sequences: the host reader's error message)
        span[b].resize(names.size());
        bool any_index = false;
        for (size_t t = 0; t < names.size(); ++t) {
            bool empty = false;
            span[b][t].has = hdr.index_span((int)t, &span[b][t].begin, &span[b][t].end, &empty);
            if (span[b][t].has || empty) any_index = true;
            if (!span[b][t].has && !empty) return 0;   // (no index, or one that does not cover the header's sequences: the host producer takes the files)
        }
        if (!any_index) return 0;
    }
    if (targets) *targets = names;
    const int world = (int)ranks.size();
    const ShardedRun run{cfg, ex, names, span, ranks, devices, rank_of, std::max(2, threads / std::max(1, world)), getenv("BDX_TIMING") != nullptr, clips};
    std::vector<RankOutcome> outcome(world);
    std::vector<std::thread> th;
    for (int r = 0; r < world; ++r)
        th.emplace_back([&run, &outcome, r] {
            try {
                decode_rank(run, r, outcome[r]);
            } catch (std::exception const& e) {
                outcome[r].error = e.what();
            }
        });
    for (auto& t : th) t.join();
    for (auto const& o : outcome)
        if (!o.error.empty()) throw std::runtime_error(o.error);
    for (auto const& o : outcome)
        if (o.gave_up) return 0;   // (a record the device path does not take: the caller starts over with the host producer)
    *unsupported = false;
    size_t n = 0;
    for (auto const& o : outcome) {
        n += o.n;
        if (ex) ex->dropped += o.excluded;
    }
    return n;
}

size_t produce_on_device(const BamConfig& cfg, const std::string& chr, const ExcludeTable* ex, int threads, std::vector<std::string>* targets, bdx_ctx* ctx,
                         bool* unsupported, bool clips) {
    if (unsupported) *unsupported = false;
    const size_t nb = cfg.num_bams();
    if (nb == 0) throw std::runtime_error("BamMerger created with no input streams!");
    if (nb > 16) { if (unsupported) *unsupported = true; return 0; }
    uint64_t excluded = 0;   // (added to ex->dropped only when the device path came through: the host reader that takes over counts afresh)
    std::vector<OwnedDecoder> decs(nb);
    auto decode = [&](size_t b, bdx_ctx* sink, bdx_bamdec** dec, size_t* n) {
        DecodeJob job{cfg, b};
        job.region = chr; job.exclude = ex; job.threads = threads; job.sink = sink; job.device = sink ? 0 : bdx_device(ctx);
        job.may_be_unsupported = unsupported != nullptr || !sink; job.targets = b == 0 ? targets : nullptr; job.clips = clips;
        DecodeResult res = decode_on_device(job);
        decs[b] = std::move(res.decoder);
        excluded += res.excluded;
        *dec = decs[b].get(); *n = res.n;
        return !res.unsupported;
    };
    size_t total = 0;
    bool ok;
    MergeTimes tm;
    if (nb == 1) {
        bdx_bamdec* dec = nullptr;
        ok = decode(0, ctx, &dec, &total);
    } else {
        // several files: each decoded into its decoder's own columns, the merge order worked out from three of them, one gather in HBM
        std::vector<size_t> files(nb);
        for (size_t b = 0; b < nb; ++b) files[b] = b;
        std::vector<KeyColumns> keys(nb);
        ok = decode_merge_gather(
            files, keys, true, threads, [&](size_t b, bdx_bamdec** dec, size_t* n) { return decode(b, nullptr, dec, n); },
            [](const std::vector<const int32_t*>&, const std::vector<const uint16_t*>&, const std::vector<size_t>&) { return 1; },
            [&](bdx_bamdec* const* d, int k, const uint8_t* src_file, const uint32_t* src_index, size_t n) {
                if (n > 0xFFFFFFFFull - 1024) return false;
                const int rc = bdx_merge_decoded(ctx, d, k, src_file, src_index, n);
                if (rc != BDX_OK) throw std::runtime_error(std::string("bdx_merge_decoded: ") + bdx_strerror(rc) + " (" + bdx_last_error(ctx) + ")");
                return true;
            },
            &total, &tm);
    }
    if (!ok) { if (unsupported) *unsupported = true; return 0; }
    if (ex) ex->dropped += excluded;
    if (nb > 1 && getenv("BDX_TIMING"))
        fprintf(stderr, "[bdx timing] %zu files decoded on the GPU in %.3f s, their keys fetched in %.3f s, merge order in %.3f s, gather in %.3f s\n", nb, tm.decoded,
                tm.keys - tm.decoded, tm.ordered - tm.keys, tm.gathered - tm.ordered);
    return total;
}

void read_targets(const BamConfig& cfg, std::vector<std::string>& names, std::vector<uint32_t>& lengths) {
    if (cfg.num_bams() == 0) throw std::runtime_error("BamMerger created with no input streams!");
    ColumnReader rd(cfg.bam_files()[0], 1, nullptr);  // (parses the header only: nothing is decoded before start())
    names = rd.target_names();
    lengths = rd.target_lengths();
}

int region_tid(const std::vector<std::string>& names, const std::string& chr) {
    struct Names {
        const std::vector<std::string>& names;
        int tid_of(const std::string& name) const {   // (the first of equal names, as tid_of of the readers)
            const auto f = std::find(names.begin(), names.end(), name);
            return f == names.end() ? -1 : (int)(f - names.begin());
        }
    } header{names};
    int tid = -1, beg = 0, end = 0;
    return parse_region(header, chr, tid, beg, end) ? tid : -1;
}

void produce_merged_by_columns(const BamConfig& cfg, const std::string& chr, const ExcludeTable* ex, int threads, ReadStream& out) {
    const LibraryResolver libs(cfg);
    const size_t nb = cfg.num_bams();
    if (nb == 0) throw std::runtime_error("BamMerger created with no input streams!");
    std::vector<ReadStream> per(nb);
    for (size_t b = 0; b < nb; ++b) {
        ColumnReader rd(cfg.bam_files()[b], std::max(1, threads), &libs);
        RecordFilter f;
        if (ex) f.exclude = ex->mask();
        if (!chr.empty() && !parse_region(rd, chr, f.only_tid, f.beg, f.end))
            throw std::runtime_error("Failed to parse bam region '" + chr + "' in file " + cfg.bam_files()[b] + ". ");
        rd.start(f);
        if (b == 0) out.targets = rd.target_names();
        VectorSink sink(per[b]);
        BatchWriter w(sink, 1 << 16);
        while (const ColumnChunk* ch = rd.next())
            if (ch->size()) w.append_range(*ch, 0, ch->size(), (uint8_t)b);
        w.finish();
        if (ex) ex->dropped += rd.excluded();
    }
    std::vector<const int32_t*> tid(nb), pos(nb);
    std::vector<const uint16_t*> flag(nb);
    std::vector<size_t> n(nb);
    for (size_t b = 0; b < nb; ++b) { tid[b] = per[b].tid.data(); pos[b] = per[b].pos.data(); flag[b] = per[b].flag.data(); n[b] = per[b].size(); }
    std::vector<uint8_t> src_file;
    std::vector<uint32_t> src_index;
    // (BDX_DUMP_MERGE=queue: the priority queue itself; =pieces: the two-file rule cut into many pieces even on a small input)
    const char* how = getenv("BDX_DUMP_MERGE");
    merge_order(tid, pos, flag, n, src_file, src_index, how && !strcmp(how, "queue") ? 0 : how && !strcmp(how, "pieces") ? 1007 : 4);
    const size_t total = src_file.size();
    out.tid.resize(total); out.pos.resize(total); out.mtid.resize(total); out.mpos.resize(total); out.isize.resize(total); out.flag.resize(total);
    out.qlen.resize(total); out.mapq.resize(total); out.lib.resize(total); out.bam.resize(total); out.name_key.resize(total); out.name_check.resize(total);
    for (size_t i = 0; i < total; ++i) {
        const ReadStream& s = per[src_file[i]];
        const size_t j = src_index[i];
        out.tid[i] = s.tid[j]; out.pos[i] = s.pos[j]; out.mtid[i] = s.mtid[j]; out.mpos[i] = s.mpos[j]; out.isize[i] = s.isize[j]; out.flag[i] = s.flag[j];
        out.qlen[i] = s.qlen[j]; out.mapq[i] = s.mapq[j]; out.lib[i] = s.lib[j]; out.bam[i] = s.bam[j]; out.name_key[i] = s.name_key[j];
        out.name_check[i] = s.name_check[j];
    }
}

void produce(const BamConfig& cfg, const std::string& chr, const ExcludeTable* ex, int threads, ReadStream& out) {
    VectorSink sink(out);
    produce_stream(cfg, chr, ex, threads, &out.targets, sink);
}

uint64_t collect_reads(const BamConfig& cfg, const std::string& chr, const ExcludeTable* ex, int threads, const std::vector<uint64_t>& wanted,
                       std::vector<SupportRead>& out) {
    out.assign(wanted.size(), SupportRead());
    size_t w = 0;
    static const char* nt16 = "=ACMGRSVTWYHKDBN";  // bam_nt16_rev_table
    return merge_streams(cfg, chr, ex, threads, nullptr, [&](uint64_t index, const BamRecord& r, int, uint8_t lib) {
        if (w >= wanted.size() || wanted[w] != index) return;
        SupportRead& sr = out[w++];
        sr.tid = r.tid; sr.pos = r.pos; sr.l_qseq = r.l_qseq; sr.bdqual = r.bdqual; sr.lib = lib; sr.rev = (r.flag & 0x10) != 0;
        sr.name.assign(r.qname, r.l_qname);
        sr.bases.resize(r.l_qseq > 0 ? r.l_qseq : 0);
        for (int i = 0; i < r.l_qseq; ++i) sr.bases[i] = nt16[(r.seq[i >> 1] >> ((~i & 1) << 2)) & 0xf];
        sr.has_qual = r.l_qseq > 0 && r.qual[0] != 0xff;
        if (sr.has_qual) sr.qual.assign((const char*)r.qual, r.l_qseq);
    });
}

}  // namespace bdhost
