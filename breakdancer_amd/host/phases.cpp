#include "phases.h"

#include <sys/stat.h>

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <iostream>
#include <stdexcept>

#include "anchor.h"
#include "mini.h"
#include "store_counts.h"

namespace bdhost {

namespace {

Clock::time_point now() { return Clock::now(); }

// Sharded runs: the merged stream is position sorted, so every chromosome is one run of records; each run goes into the
// staging ring of the context that owns the chromosome (bdx_dist_chromosome of its rank).
struct RoutingSink : BatchSink {
    const std::vector<bdx_dist*>& ranks;
    const std::vector<int>& rank_of;
    std::vector<char> store;
    bdx_batch_buf cur{};
    bool clips;                                   // --clip: the contexts keep clip words, put behind every batch
    std::vector<std::pair<bdx_ctx*, size_t>> held;   // ... at the row their context has reached
    RoutingSink(const std::vector<bdx_dist*>& r, const std::vector<int>& ro, bool with_clips) : ranks(r), rank_of(ro), clips(with_clips) {}
    bdx_batch_buf acquire(size_t capacity) override {
        const size_t K = (capacity + 63) / 64 * 64;
        store.resize(K * 43 + 64);
        char* p = store.data();
        cur.name_key = (uint64_t*)p; p += K * 8;
        cur.name_check = (uint64_t*)p; p += K * 8;
        cur.tid = (int32_t*)p; p += K * 4; cur.pos = (int32_t*)p; p += K * 4; cur.mtid = (int32_t*)p; p += K * 4;
        cur.mpos = (int32_t*)p; p += K * 4; cur.isize = (int32_t*)p; p += K * 4;
        cur.flag = (uint16_t*)p; p += K * 2; cur.qlen = (uint16_t*)p; p += K * 2;
        cur.mapq = (uint8_t*)p; p += K; cur.lib = (uint8_t*)p; p += K; cur.bam = (uint8_t*)p;
        cur.capacity = K;
        return cur;
    }
    void submit(size_t n) override {
        size_t lo = 0;
        while (lo < n) {
            const int tid = cur.tid[lo];
            size_t hi = lo + 1;
            while (hi < n && cur.tid[hi] == tid) ++hi;
            if (tid < 0 || (size_t)tid >= rank_of.size()) throw std::runtime_error("record with a reference id beyond the header's sequences");
            bdx_ctx* c = bdx_dist_chromosome(ranks[rank_of[tid]], tid);
            if (!c) throw std::runtime_error("bdx_dist_chromosome failed");
            check(c, bdx_use_name_check(c, 1), "bdx_use_name_check");
            if (clips) check(c, bdx_use_clips(c, 1), "bdx_use_clips");
            const size_t m = hi - lo;
            bdx_batch_buf b{};
            check(c, bdx_acquire_batch(c, m, &b), "bdx_acquire_batch");
            memcpy(b.tid, cur.tid + lo, m * 4); memcpy(b.pos, cur.pos + lo, m * 4); memcpy(b.mtid, cur.mtid + lo, m * 4);
            memcpy(b.mpos, cur.mpos + lo, m * 4); memcpy(b.isize, cur.isize + lo, m * 4);
            memcpy(b.flag, cur.flag + lo, m * 2); memcpy(b.qlen, cur.qlen + lo, m * 2);
            memcpy(b.mapq, cur.mapq + lo, m); memcpy(b.lib, cur.lib + lo, m); memcpy(b.bam, cur.bam + lo, m);
            memcpy(b.name_key, cur.name_key + lo, m * 8);
            memcpy(b.name_check, cur.name_check + lo, m * 8);
            check(c, bdx_submit_batch(c, m), "bdx_submit_batch");
            if (clips) {
                auto at = std::find_if(held.begin(), held.end(), [c](const std::pair<bdx_ctx*, size_t>& h) { return h.first == c; });
                if (at == held.end()) at = held.insert(held.end(), {c, 0});
                check(c, bdx_put_clips(c, at->second, clip + lo, m), "bdx_put_clips");
                at->second += m;
            }
            lo = hi;
        }
    }
};

// The producer's batches go straight into the context's pinned staging ring: while the decode threads work on the next
// pieces of the BAMs, the previous batch crosses PCIe and the classifier runs over it (AlignmentSource.hpp:48-65: one
// record stream, consumed as it is produced).  The context is created on a helper thread (the HIP runtime takes ~0.1 s
// to come up) and only waited for when the first batch is ready.
struct GpuSink : BatchSink {
    Session& s;
    size_t reserve;
    bool up = false;
    bool clips;          // --clip: the context keeps clip words, put behind every batch ...
    size_t held = 0;     // ... at the row the store has reached
    GpuSink(Session& session, size_t res, bool with_clips) : s(session), reserve(res), clips(with_clips) {}
    void bring_up(bool with_store = true) {
        if (up) return;
        if (s.ctx_ready.valid()) check(nullptr, s.ctx_ready.get(), "bdx_create");
        if (!with_store) return;   // (the device-side decoder sizes the store itself, and the later stages once it knows the record density)
        check(s.ctx, bdx_reserve(s.ctx, reserve), "bdx_reserve");
        up = true;
    }
    bdx_batch_buf acquire(size_t capacity) override {
        bring_up();
        bdx_batch_buf b{};
        check(s.ctx, bdx_acquire_batch(s.ctx, capacity, &b), "bdx_acquire_batch");
        return b;
    }
    void submit(size_t n) override {
        check(s.ctx, bdx_submit_batch(s.ctx, n), "bdx_submit_batch");
        if (clips) check(s.ctx, bdx_put_clips(s.ctx, held, clip, n), "bdx_put_clips");
        held += n;
    }
};

// --estimate: from the summed histograms to the run's libraries in `in`; returns them for bdx_set_libs / bdx_dist_set_libs
EstimatePlan estimate_from(Inputs& in, const Env& env, const std::vector<uint64_t>& hist, const std::vector<uint64_t>& n_over, Clock::time_point t0) {
    EstimatePlan plan = plan_estimate(in.cfg, in.config_text, in.opts.o.cut_sd, hist.data(), n_over.data());
    for (const std::string& w : plan.warnings) fprintf(stderr, "WARNING: %s\n", w.c_str());
    if (!plan.fatal.empty()) throw std::runtime_error(plan.fatal);
    in.apply_estimate(plan);
    if (env.timing) fprintf(stderr, "[bdx timing] --estimate: %s; window %d; %.4f s\n", estimate_summary(in.cfg, plan).c_str(), plan.window, secs(t0, now()));
    return plan;
}

}  // namespace

Session::~Session() {
    if (ctx_ready.valid()) ctx_ready.wait();
    if (trimmer.joinable()) trimmer.join();
    release_device_decoders();
    if (ranks.empty() && ctx) bdx_destroy(ctx);
    for (bdx_dist* d : ranks)
        if (d) bdx_dist_destroy(d);
}

void Session::start_trimmer() {
    bdx_ctx* tc = ctx;
    trimmer = std::thread([tc] { (void)bdx_trim_results(tc); });
}

Fed feed_and_run_single(Inputs& in, const Env& env, Session& s, Clock::time_point t_start) {
    const Options& opts = in.opts;
    Fed fed;
    // the GPU context (HIP runtime start-up, ~0.1 s) comes up on a helper thread while the BAMs are decoded
    // (the thread has copies of what it reads: it may outlive everything but the session)
    s.ctx_ready = std::async(std::launch::async, [ctx = &s.ctx, o = opts.o, libs = in.libs, nbams = (int)in.cfg.num_bams(), w0 = in.cfg.max_read_window_size(),
                                                   device = opts.device, mark_dup = opts.mark_dup, clips = opts.clip] {
        int rc = bdx_create(ctx, &o, libs.data(), (int)libs.size(), nbams, 0, w0, device);
        if (rc == BDX_OK) rc = bdx_use_name_check(*ctx, 1);   // mates are joined on two hashes of the read name
        if (rc == BDX_OK && clips) rc = bdx_use_clips(*ctx, 1);
        if (rc == BDX_OK && mark_dup) rc = bdx_set_mark_duplicates(*ctx, 1);
        return rc;
    });
    // resident store sized from the compressed files (a record takes 50-150 bytes of BAM; a store that is too small
    // grows, at the price of classifying from the first tile again)
    size_t reserve = 1 << 20;
    for (auto const& f : in.cfg.bam_files()) {
        struct stat st;
        if (stat(f.c_str(), &st) == 0) reserve += (size_t)st.st_size / 48;
    }
    reserve = std::min<size_t>(reserve, 0xFFFFFFFFull - 1024);
    GpuSink sink(s, reserve, opts.clip);
    // One BAM: the file goes to the GPU as it is and is decoded there (bdx_bamdec_*: inflate, record boundaries, fields,
    // RG -> library, reader filter in HBM).  Several BAMs are merged in the reference's order by the host producer, which
    // also takes the files the device path does not (BDX_DECODE=host forces it).
    if (in.cfg.num_bams() <= 16 && !env.decode_host) {
        const auto tb = now();
        sink.bring_up(false);
        if (env.timing) fprintf(stderr, "[bdx timing] GPU context + resident store ready %.3f s after start (waited %.3f s for it)\n", secs(t_start, now()), secs(tb, now()));
        bool unsupported = false;
        fed.n_reads = produce_on_device(in.cfg, opts.chr, in.exclude.get(), env.read_threads ? env.read_threads : (int)std::min(std::max(usable_cpus(), 2u), 16u),
                                        &fed.targets, s.ctx, &unsupported, opts.clip);
        if (unsupported) check(s.ctx, bdx_reset_reads(s.ctx), "bdx_reset_reads");
        else { fed.device_decoded = true; sink.up = true; }
    }
    if (!fed.device_decoded) {
        fed.n_reads = produce_stream(in.cfg, opts.chr, in.exclude.get(), (int)in.io_threads, &fed.targets, sink, env.batch_records ? env.batch_records : (size_t)1 << 20);
        sink.bring_up();  // (an input without records never asked for a batch)
    }
    fed.t_decoded = now();
    if (in.want_dumps) check(s.ctx, bdx_set_collect_support(s.ctx, 1), "bdx_set_collect_support");
    if (in.restored) check(s.ctx, bdx_set_pass1_statistics(s.ctx, in.cache.counters.data(), in.cache.covered_ref_len), "bdx_set_pass1_statistics");
    if (opts.estimate) {
        const auto te = now();
        const size_t nlibs = in.libs.size();
        std::vector<uint64_t> hist(nlibs * (size_t)BDX_ISIZE_BINS), n_over(nlibs);
        check(s.ctx, bdx_insert_size_histogram(s.ctx, hist.data(), n_over.data()), "bdx_insert_size_histogram");
        const EstimatePlan plan = estimate_from(in, env, hist, n_over, te);
        check(s.ctx, bdx_set_libs(s.ctx, plan.libs.data(), (int)plan.libs.size(), plan.window), "bdx_set_libs");
    }
    check(s.ctx, bdx_run(s.ctx), "bdx_run");
    fed.t_ran = now();
    return fed;
}

// BDX_GPUS=N (devices 0..N-1) or a list "0,1,2,3": ONE whole-genome run with the chromosomes spread over several
// GPUs (bdx_dist_*: one rank per device, here as threads of this process) -- same output as on one GPU
Fed feed_and_run_sharded(Inputs& in, const Env& env, Session& s, Clock::time_point t_start) {
    const Options& opts = in.opts;
    Fed fed;
    if (in.restored) throw std::runtime_error("-R is not supported with BDX_GPUS");
    const std::vector<uint32_t>& lengths = in.header.lengths();
    const int ntids = (int)std::max<size_t>(in.header.names().size(), 1), world = (int)in.devices.size();
    const int nlibs = (int)in.libs.size(), nbams = (int)in.cfg.num_bams();
    s.ranks.assign(world, nullptr);
    const auto t_create = now();
    int rc = bdx_dist_create_threads(s.ranks.data(), &opts.o, in.libs.data(), nlibs, nbams, ntids, in.cfg.max_read_window_size(), in.devices.data(), world);
    if (rc != BDX_OK) throw std::runtime_error(std::string("bdx_dist_create_threads: ") + bdx_strerror(rc));
    const auto t_created = now();
    if (opts.mark_dup)
        for (bdx_dist* r : s.ranks)
            if (bdx_dist_set_mark_duplicates(r, 1) != BDX_OK) throw std::runtime_error(std::string("bdx_dist_set_mark_duplicates: ") + bdx_dist_last_error(r));
    if (in.want_dumps)   // -g / -d: the supporting reads come with the result (gathered compact records, walked read by read on rank 0)
        for (bdx_dist* r : s.ranks) bdx_dist_set_collect_support(r, 1);
    std::vector<uint64_t> weight(lengths.begin(), lengths.end());  // chromosomes -> ranks by sequence length
    weight.resize(ntids, 0);
    fed.rank_of.assign(ntids, 0);
    bdx_dist_plan(weight.data(), ntids, world, fed.rank_of.data());
    // BAMs with their indexes: every rank pulls the BGZF ranges of ITS chromosomes and decodes them on ITS GPU (bdx_bamdec_*), as the
    // reference reads one chromosome through the index (io/RegionLimitedBamReader.hpp:43-71); several files are merged per
    // chromosome in the reference's order by a gather in HBM.  Without an index or with BDX_DECODE=host: the host producer
    // decodes everything once and routes the records to the ranks.
    if (!env.decode_host) {
        bool unsupported = true;
        fed.n_reads = produce_sharded_on_device(in.cfg, in.exclude.get(), (int)std::min(std::max(usable_cpus(), 2u), 32u), &fed.targets, s.ranks, in.devices,
                                                fed.rank_of, &unsupported, opts.clip);
        fed.device_decoded = !unsupported;
        if (unsupported)   // (no index: nothing was appended; a file the device path gave up on half way: what it appended goes again)
            for (bdx_dist* r : s.ranks)
                if (bdx_dist_reset_reads(r) != BDX_OK) throw std::runtime_error(std::string("bdx_dist_reset_reads: ") + bdx_dist_last_error(r));
    }
    if (!fed.device_decoded) {
        RoutingSink sink(s.ranks, fed.rank_of, opts.clip);
        fed.n_reads = produce_stream(in.cfg, opts.chr, in.exclude.get(), (int)in.io_threads, &fed.targets, sink, env.batch_records ? env.batch_records : (size_t)1 << 20);
    }
    if (env.timing)
        fprintf(stderr, "[bdx timing] sharded run over %d ranks: %s\n", world,
                fed.device_decoded ? "every rank decoded its chromosomes' BGZF ranges on its own GPU (through the BAM index)"
                                   : "records decoded by the host producer and routed to the ranks");
    const auto t_fed = now();
    {   // (device code loaded, the later stages' buffers sized: beside nothing, but outside the run; every rank on its own thread)
        std::vector<std::thread> pt;
        for (bdx_dist* r : s.ranks) pt.emplace_back([r] { (void)bdx_dist_prepare(r); });
        for (auto& t : pt) t.join();
    }
    fed.t_decoded = now();
    if (env.timing)
        fprintf(stderr, "[bdx timing] sharded run: ranks created %.3f s after start, in %.3f s; reads on the ranks %.3f s later; prepared in %.3f s\n",
                secs(t_start, t_create), secs(t_create, t_created), secs(t_created, t_fed), secs(t_fed, fed.t_decoded));
    if (opts.estimate) {   // (the ranks are threads of this process: their histograms are summed here, no collective)
        const auto te = now();
        std::vector<uint64_t> hist((size_t)nlibs * BDX_ISIZE_BINS, 0), n_over(nlibs, 0), h(hist.size()), o(nlibs);
        for (bdx_dist* r : s.ranks) {
            if (bdx_dist_insert_size_histogram(r, h.data(), o.data()) != BDX_OK)
                throw std::runtime_error(std::string("bdx_dist_insert_size_histogram: ") + bdx_dist_last_error(r));
            for (size_t i = 0; i < hist.size(); ++i) hist[i] += h[i];
            for (int i = 0; i < nlibs; ++i) n_over[i] += o[i];
        }
        const EstimatePlan plan = estimate_from(in, env, hist, n_over, te);
        for (bdx_dist* r : s.ranks)
            if (bdx_dist_set_libs(r, plan.libs.data(), nlibs, plan.window) != BDX_OK)
                throw std::runtime_error(std::string("bdx_dist_set_libs: ") + bdx_dist_last_error(r));
    }
    std::vector<int> rcs(world, BDX_OK);
    std::vector<std::thread> th;
    for (int r = 0; r < world; ++r) th.emplace_back([&, r] { rcs[r] = bdx_dist_run(s.ranks[r]); });
    for (auto& t : th) t.join();
    for (int r = 0; r < world; ++r)
        if (rcs[r] != BDX_OK)
            throw std::runtime_error(std::string("bdx_dist_run: ") + bdx_strerror(rcs[r]) + " (" + bdx_dist_last_error(s.ranks[r]) + ")");
    s.ctx = bdx_dist_result(s.ranks[0]);
    if (!s.ctx) throw std::runtime_error("bdx_dist_result: no result on rank 0");
    fed.t_ran = now();
    return fed;
}

Statistics fetch_statistics(const Inputs& in, const Session& s) {
    Statistics st;
    if (in.opts.mark_dup) {
        if (in.sharded) {
            for (bdx_dist* r : s.ranks) {
                uint64_t m = 0, g = 0;
                if (bdx_dist_get_duplicates(r, &m, &g) != BDX_OK) throw std::runtime_error(std::string("bdx_dist_get_duplicates: ") + bdx_dist_last_error(r));
                st.dup_marked += m; st.dup_groups += g;
            }
        } else {
            check(s.ctx, bdx_get_duplicates(s.ctx, &st.dup_marked, &st.dup_groups), "bdx_get_duplicates");
        }
    }
    check(s.ctx, bdx_get_summary(s.ctx, &st.sum), "bdx_get_summary");
    const size_t nlibs = in.libs.size(), nbams = in.cfg.num_bams();
    TableCounters& c = st.counters;
    c.covered_ref_len = st.sum.covered_ref_len;
    c.lib_count.resize(nlibs); c.bam_count.resize(nbams); c.flag_hist.resize(nlibs * BDX_NUM_FLAGS);
    c.seqcov.resize(nlibs); c.density.resize(nlibs);
    check(s.ctx, bdx_get_counters(s.ctx, c.lib_count.data(), c.bam_count.data(), c.flag_hist.data(), c.seqcov.data(), c.density.data()), "bdx_get_counters");
    return st;
}

void write_pass1_cache(const Inputs& in, const Statistics& st) {
    const std::vector<std::string>& argv = in.opts.orig_argv;
    Pass1Cache w;
    for (size_t i = 0; i < argv.size(); ++i) {
        if (argv[i] == "-C" && i + 1 < argv.size()) { ++i; continue; }
        if (argv[i].compare(0, 2, "-C") == 0 && argv[i].size() > 2) continue;
        w.argv.push_back(argv[i]);
    }
    w.config_text = in.config_text;
    w.covered_ref_len = st.sum.covered_ref_len;
    w.nlibs = (int)in.libs.size(); w.nbams = (int)in.cfg.num_bams();
    w.counters = st.counters.flag_hist;
    w.counters.insert(w.counters.end(), st.counters.lib_count.begin(), st.counters.lib_count.end());
    w.counters.insert(w.counters.end(), st.counters.bam_count.begin(), st.counters.bam_count.end());
    write_cache(in.opts.cache_file, w);
}

Calls fetch_calls(const Session& s, size_t n_svs) {
    Calls c;
    c.svs.resize(n_svs);
    check(s.ctx, bdx_get_svs(s.ctx, c.svs.data(), c.svs.size()), "bdx_get_svs");
    size_t nl = 0, nc = 0;
    for (auto const& sv : c.svs) { nl = std::max<size_t>(nl, sv.lib_begin + sv.lib_count); nc = std::max<size_t>(nc, sv.cn_begin + sv.cn_count); }
    SvLists& l = c.lists;
    l.lib_index.resize(nl); l.lib_pairs.resize(nl); l.cn_key.resize(nc); l.cn_value.resize(nc);
    check(s.ctx, bdx_get_sv_lists(s.ctx, l.lib_index.data(), l.lib_pairs.data(), nl, l.cn_key.data(), l.cn_value.data(), nc), "bdx_get_sv_lists");
    for (size_t i = 0; i < c.svs.size(); ++i)
        if (c.svs[i].printed) c.printed_rows.push_back(i);
    return c;
}

Genotypes count_on_store(const Inputs& in, const Env& env, const Session& s, const Fed& fed, const Calls& calls) {
    Genotypes gt;
    if (!in.vcf && !in.sites_vcf) return gt;
    const Options& opts = in.opts;
    const int only_tid = opts.chr.empty() ? -1 : region_tid(in.header.names(), opts.chr);   // (the producer has parsed the same argument)
    const RunContexts rc{s.ctx, s.ranks, fed.rank_of, only_tid};
    if (in.vcf) {
        const auto tv = now();
        gt.vcf_rows = vcf_records(opts, in.cfg, calls.svs, calls.printed_rows, calls.lists.lib_index, calls.lists.lib_pairs, rc);
        if (env.timing) fprintf(stderr, "[bdx timing] --vcf: junction counts of %zu rows %.4f s\n", calls.printed_rows.size(), secs(tv, now()));
    }
    if (in.sites_vcf) {
        const auto tv = now();
        gt.site_rows = site_records(opts, in.cfg, in.site_table, in.sites_window, rc);
        if (env.timing)
            fprintf(stderr, "[bdx timing] --sites: pair and junction counts of %zu sites (window %d, %zu lines on unknown sequences ignored) %.4f s\n",
                    in.site_table.sites.size(), in.sites_window, in.site_table.unknown_lines, secs(tv, now()));
    }
    if (opts.ci) {
        const auto tv = now();
        fill_ci(opts, rc, in.ci_window, gt.vcf_rows);
        fill_ci(opts, rc, in.ci_window, gt.site_rows);
        size_t with = 0;
        for (auto const* rows : {&gt.vcf_rows, &gt.site_rows})
            for (auto const& r : *rows) with += r.has_ci;
        if (env.timing)
            fprintf(stderr, "[bdx timing] --ci: breakpoint bounds of %zu records (window %d, %zu with supporting pairs) %.4f s\n",
                    gt.vcf_rows.size() + gt.site_rows.size(), in.ci_window, with, secs(tv, now()));
    }
    if (opts.mapq) {
        const auto tv = now();
        fill_quality(opts, rc, in.mapq_window, gt.vcf_rows);
        fill_quality(opts, rc, in.mapq_window, gt.site_rows);
        size_t ends = 0;
        for (auto const* rows : {&gt.vcf_rows, &gt.site_rows})
            for (auto const& r : *rows) ends += r.has_mapq ? (size_t)r.mq[0].held + (size_t)r.mq[1].held : 0;
        if (env.timing)
            fprintf(stderr, "[bdx timing] --mapq: mapping quality at %zu ends of %zu records (window %d) %.4f s\n", ends,
                    gt.vcf_rows.size() + gt.site_rows.size(), in.mapq_window, secs(tv, now()));
    }
    if (opts.clip) {
        const auto tv = now();
        uint64_t observations = 0;
        size_t ends = 0;
        for (auto* rows : {&gt.vcf_rows, &gt.site_rows}) {
            observations += fill_clips(opts, rc, in.clip_window, opts.min_clip(), *rows);
            for (auto const& r : *rows) ends += r.has_clip ? (size_t)r.cl[0].held + (size_t)r.cl[1].held : 0;
        }
        if (env.timing)
            fprintf(stderr, "[bdx timing] --clip: piles of clipped reads at %zu ends of %zu records, %llu clipped observations (window %d, min %d) %.4f s\n", ends,
                    gt.vcf_rows.size() + gt.site_rows.size(), (unsigned long long)observations, in.clip_window, opts.min_clip(), secs(tv, now()));
    }
    if (opts.depth) {
        const auto tv = now();
        const size_t ns = sample_names(opts, in.cfg).size();
        size_t with = 0;
        for (auto* rows : {&gt.vcf_rows, &gt.site_rows}) {
            fill_depth(opts, rc, opts.flank(), in.header.lengths(), ns, *rows);
            for (auto const& r : *rows) with += r.has_depth;
        }
        if (env.timing)
            fprintf(stderr, "[bdx timing] --depth: read starts inside and beside %zu records (flank %d, %zu with both ends on one sequence) %.4f s\n",
                    gt.vcf_rows.size() + gt.site_rows.size(), opts.flank(), with, secs(tv, now()));
    }
    return gt;
}

// --mini: behind the run -- the store's histogram (after the run, so --mark-dup's marks are honoured) becomes the null of every context, the
// grid windows of every sequence the run read go to the GPU in batches, and what reaches the threshold is merged and written (mini.h)
void call_mini(Inputs& in, const Env& env, const Session& s, const Fed& fed) {
    if (in.opts.mini.empty()) return;
    const Options& opts = in.opts;
    const auto t0 = now();
    const int only_tid = opts.chr.empty() ? -1 : region_tid(in.header.names(), opts.chr);
    const RunContexts rc{s.ctx, s.ranks, fed.rank_of, only_tid};
    const size_t nlibs = in.libs.size();
    MiniParams p;
    p.window = opts.mini_window > 0 ? opts.mini_window : mini_mean_window(in.libs);
    p.step = opts.mini_step > 0 ? opts.mini_step : std::max<int64_t>(p.window / 2, 1);
    p.min_pairs = opts.mini_min_pairs > 0 ? opts.mini_min_pairs : Options::kMiniMinPairsDefault;
    p.score = opts.mini_score;
    std::vector<uint64_t> hist;
    store_insert_histogram(rc, nlibs, hist);
    const MiniNull null = mini_null(hist.data(), nlibs);
    for (size_t l = 0; l < nlibs; ++l)
        if (!null.usable[l])
            fprintf(stderr, "WARNING: --mini: library %s has %llu usable pairs, fewer than %llu: skipped\n", in.cfg.library_config(l).name.c_str(),
                    (unsigned long long)null.N[l], (unsigned long long)kMiniUsable);
    set_insert_null(rc, hist.data());
    const auto t1 = now();
    double t_gpu = 0;
    // (a sequence is taken to end at 2^31 - 2 at the latest, as --depth takes it: positions and window ends are int32 in the store and the ABI)
    std::vector<uint32_t> lengths = in.header.lengths();
    for (uint32_t& l : lengths) l = std::min<uint32_t>(l, 2147483646u);
    const size_t batch = std::max<size_t>(((size_t)1 << 22) / nlibs, 1);   // (a call's rows stay at or below 160 MiB)
    const double keep_from = p.score >= 0 ? (double)p.score : 20.0;       // (no threshold is below it)
    std::vector<MiniKept> kept;
    uint64_t windows = 0, scoring = 0, saturated = 0;
    std::vector<bdx_interval> iv;
    std::vector<std::pair<int32_t, int64_t>> which;
    std::vector<bdx_insert_shift> rows;
    auto flush = [&] {
        if (iv.empty()) return;
        const auto tg = now();
        window_insert_shift(rc, iv, nlibs, rows);
        t_gpu += secs(tg, now());
        for (size_t i = 0; i < iv.size(); ++i) {
            const MiniWindow w = mini_window(rows.data() + i * nlibs, null, p.min_pairs);
            scoring += w.scoring;
            saturated += w.saturated;
            if (w.scoring && w.score >= keep_from) kept.push_back(MiniKept{which[i].first, which[i].second, w});
        }
        windows += iv.size();
        iv.clear();
        which.clear();
    };
    for (size_t t = 0; t < lengths.size(); ++t) {
        if (!rc.held((int)t)) continue;
        const int64_t len = lengths[t];
        const uint64_t nw = mini_grid((uint64_t)len, p.step);
        for (uint64_t j = 0; j < nw; ++j) {
            const int64_t beg = (int64_t)j * p.step;
            iv.push_back(bdx_interval{(int32_t)t, (int32_t)beg, (int32_t)std::min<int64_t>(beg + p.window, len)});
            which.emplace_back((int32_t)t, (int64_t)j);
            if (iv.size() == batch) flush();
        }
    }
    flush();
    const int threshold = p.score >= 0 ? p.score : mini_default_threshold(scoring);
    const std::vector<MiniCall> calls = mini_merge(kept, threshold, p, lengths);
    std::ofstream& out = in.mini_out;
    out << "#Software: breakdancer-max --mini\n#Command: ";
    for (auto const& a : opts.orig_argv) out << a << " ";
    out << "\n#Window: " << p.window << "\n#Step: " << p.step << "\n#MinPairs: " << p.min_pairs << "\n#Threshold: " << threshold << "\n";
    mini_write_table(out, calls, in.header.names());
    out.close();
    if (out.fail()) throw std::runtime_error("unable to write --mini file '" + opts.mini + "'");
    if (env.timing)
        fprintf(stderr, "[bdx timing] --mini: %llu windows (window %lld, step %lld), %llu scoring, %llu saturated, %zu calls, threshold %d; histogram %.4f s, kernel calls %.4f s, host %.4f s\n",
                (unsigned long long)windows, (long long)p.window, (long long)p.step, (unsigned long long)scoring, (unsigned long long)saturated, calls.size(), threshold,
                secs(t0, t1), t_gpu, secs(t1, now()) - t_gpu);
}

// --anchor: behind the run and behind --mini -- the grid windows of every sequence the run read go to the GPU in batches (KA), the windows
// that call are merged and written (anchor.h).  The rule does not look at BDX_CLS_PASS, so -t changes nothing here
void call_anchor(Inputs& in, const Env& env, const Session& s, const Fed& fed) {
    if (in.opts.anchor.empty()) return;
    const Options& opts = in.opts;
    const auto t0 = now();
    const int only_tid = opts.chr.empty() ? -1 : region_tid(in.header.names(), opts.chr);
    const RunContexts rc{s.ctx, s.ranks, fed.rank_of, only_tid};
    AnchorParams p;
    p.window = opts.anchor_window > 0 ? opts.anchor_window : anchor_default_window(in.libs);
    p.step = opts.anchor_step > 0 ? opts.anchor_step : anchor_default_step(p.window);
    p.min = opts.anchor_min > 0 ? opts.anchor_min : Options::kAnchorMinDefault;
    p.mapq = opts.anchor_mapq;
    // (every `tile`-th window, when the step divides the window: those windows cut the sequence without overlap, so their sums count a record once)
    const uint64_t tile = p.window % p.step == 0 ? (uint64_t)(p.window / p.step) : 0;
    double t_gpu = 0;
    // (a sequence is taken to end at 2^31 - 2 at the latest, as --mini takes it)
    std::vector<uint32_t> lengths = in.header.lengths();
    for (uint32_t& l : lengths) l = std::min<uint32_t>(l, 2147483646u);
    const size_t batch = (size_t)1 << 22;
    std::vector<AnchorCall> called;
    uint64_t windows = 0, candidates = 0, anchors = 0, any_candidate = 0, any_anchor = 0;
    std::vector<bdx_interval> iv;
    std::vector<std::pair<int32_t, uint64_t>> which;
    std::vector<bdx_anchor_split> rows;
    auto flush = [&] {
        if (iv.empty()) return;
        const auto tg = now();
        window_anchor_split(rc, iv, p.mapq, rows);
        t_gpu += secs(tg, now());
        for (size_t i = 0; i < iv.size(); ++i) {
            const bdx_anchor_split& r = rows[i];
            const uint64_t a = (uint64_t)r.n_fwd + r.n_rev;
            any_candidate += a + r.n_low;
            any_anchor += a;
            if (tile && which[i].second % tile == 0) { candidates += a + r.n_low; anchors += a; }
            if (anchor_calls(r, p.min)) called.push_back(AnchorCall{which[i].first, r, 1});
        }
        windows += iv.size();
        iv.clear();
        which.clear();
    };
    for (size_t t = 0; t < lengths.size(); ++t) {
        if (!rc.held((int)t)) continue;
        const int64_t len = lengths[t];
        const uint64_t nw = mini_grid((uint64_t)len, p.step);
        for (uint64_t j = 0; j < nw; ++j) {
            const int64_t beg = (int64_t)j * p.step;
            iv.push_back(bdx_interval{(int32_t)t, (int32_t)beg, (int32_t)std::min<int64_t>(beg + p.window, len)});
            which.emplace_back((int32_t)t, j);
            if (iv.size() == batch) flush();
        }
    }
    flush();
    if (any_candidate && !any_anchor)
        fprintf(stderr, "WARNING: --anchor: the run holds reads whose mate is unmapped, and none passes the quality test.  The store keeps the AM tag where "
                        "the aligner wrote one, the smaller quality of the two mates, which is 0 for these reads: give --anchor-mapq 0\n");
    const std::vector<AnchorCall> calls = anchor_merge(std::move(called));
    std::ofstream& out = in.anchor_out;
    out << "#Software: breakdancer-max --anchor\n#Command: ";
    for (auto const& a : opts.orig_argv) out << a << " ";
    out << "\n#Window: " << p.window << "\n#Step: " << p.step << "\n#Min: " << p.min << "\n#Mapq: " << p.mapq << "\n";
    anchor_write_table(out, calls, in.header.names());
    out.close();
    if (out.fail()) throw std::runtime_error("unable to write --anchor file '" + opts.anchor + "'");
    if (env.timing) {
        char seen[96] = "";
        if (tile) snprintf(seen, sizeof seen, " %llu candidates, %llu anchors,", (unsigned long long)candidates, (unsigned long long)anchors);
        fprintf(stderr, "[bdx timing] --anchor: %llu windows (window %lld, step %lld),%s %zu calls; kernel calls %.4f s, host %.4f s\n", (unsigned long long)windows,
                (long long)p.window, (long long)p.step, seen, calls.size(), t_gpu, secs(t0, now()) - t_gpu);
    }
}

// supporting reads of the printed SVs: a second decode pass fetches just those records (the reference keeps
// sequence data for every anomalous read in memory instead)
Support fetch_support(const Inputs& in, const Session& s, const Fed& fed, const Calls& calls) {
    Support sup;
    if (!in.want_dumps) return sup;
    const Options& opts = in.opts;
    if (!opts.prefix_fastq.empty()) sup.fastq.reset(new FastqDump(opts.prefix_fastq, in.cfg));
    if (!opts.dump_BED.empty()) sup.bed.reset(new BedDump(opts.dump_BED, in.cfg, fed.targets));
    size_t total = 0;
    sup.off.resize(calls.svs.size() + 1);
    check(s.ctx, bdx_get_sv_support(s.ctx, sup.off.data(), nullptr, nullptr, 0, &total), "bdx_get_sv_support");
    sup.idx.resize(total);
    sup.flag.resize(total);
    check(s.ctx, bdx_get_sv_support(s.ctx, sup.off.data(), sup.idx.data(), sup.flag.data(), total, &total), "bdx_get_sv_support");
    for (size_t i : calls.printed_rows) sup.wanted.insert(sup.wanted.end(), sup.idx.begin() + sup.off[i], sup.idx.begin() + sup.off[i + 1]);
    std::sort(sup.wanted.begin(), sup.wanted.end());
    sup.wanted.erase(std::unique(sup.wanted.begin(), sup.wanted.end()), sup.wanted.end());
    // (the replay drops what the run's reader dropped: the indices are positions in the masked stream)
    const uint64_t replay_dropped = collect_reads(in.cfg, opts.chr, in.exclude.get(), (int)in.io_threads, sup.wanted, sup.reads);
    if (in.exclude && replay_dropped != in.exclude->dropped.load())
        throw std::runtime_error("--exclude: the dump pass dropped " + std::to_string(replay_dropped) + " records, the run's reader " +
                                 std::to_string(in.exclude->dropped.load()));
    return sup;
}

void write_table(const Inputs& in, const Env& env, const TableFormat& table, const Calls& calls, Support& sup) {
    const size_t rows = calls.printed_rows.size();
    if (!in.want_dumps) {
        // (a table below 8,192 rows is not worth the threads.  BDX_FORMAT_THREADS -- tests, A/B: 1 = the sequential loop; n = n threads
        // whatever the table's size)
        size_t threads = rows < 8192 ? 1 : std::min<size_t>(std::min<size_t>(in.io_threads, 8), rows / 2048);
        if (env.format_threads_set) threads = std::max<size_t>(1, std::min<size_t>((size_t)env.format_threads, std::max<size_t>(rows, 1)));
        table.write_rows(std::cout, calls.svs, calls.printed_rows, calls.lists, threads);
        return;
    }
    // The dumps (-g / -d) keep the sequential loop: a dump per printed row
    for (size_t i : calls.printed_rows) {
        const bdx_sv& s = calls.svs[i];
        table.row(std::cout, s, calls.lists);
        SvForDump d;
        d.chr0 = table.target_name(s.chr[0]); d.pos0 = s.pos[0]; d.type = in.opts.sv_type(s.flag); d.size = s.size; d.flag = s.flag;
        for (uint32_t k = sup.off[i]; k < sup.off[i + 1]; ++k) {
            const size_t w = std::lower_bound(sup.wanted.begin(), sup.wanted.end(), sup.idx[k]) - sup.wanted.begin();
            d.reads.push_back(&sup.reads[w]);
            d.read_flags.push_back(sup.flag[k]);
        }
        if (sup.bed) sup.bed->write(d);
        if (sup.fastq) sup.fastq->write(d);
    }
}

void write_vcfs(const Inputs& in, Genotypes& gt) {
    if (!in.vcf && !in.sites_vcf) return;
    const Options& opts = in.opts;
    const std::vector<std::string> samples = sample_names(opts, in.cfg);
    const VcfCi ci_info{in.ci_window};
    const VcfCi* ci = opts.ci ? &ci_info : nullptr;
    const VcfDepth depth_info{opts.flank()};
    const VcfDepth* depth = opts.depth ? &depth_info : nullptr;
    const VcfMapq mapq_header{in.mapq_window};
    const VcfMapq* mapq = opts.mapq ? &mapq_header : nullptr;
    const VcfClip clip_header{in.clip_window, opts.min_clip(), opts.clip_needed()};
    const VcfClip* clip = opts.clip ? &clip_header : nullptr;
    if (in.vcf) in.vcf->write(opts.orig_argv, in.header.names(), in.header.lengths(), samples, std::move(gt.vcf_rows), opts.exclude, nullptr, opts.mark_dup, ci, depth, mapq, opts.estimate, clip);
    if (in.sites_vcf) {
        const VcfSites info{opts.sites, in.sites_window};
        in.sites_vcf->write(opts.orig_argv, in.header.names(), in.header.lengths(), samples, std::move(gt.site_rows), opts.exclude, &info, opts.mark_dup, ci, depth, mapq, opts.estimate, clip);
    }
}

void print_timing(const Inputs& in, const Session& s, const Fed& fed, const Statistics& st, Clock::time_point t_start) {
    if (in.exclude) print_exclude_timing(*in.exclude);
    if (in.opts.mark_dup)
        fprintf(stderr, "[bdx timing] --mark-dup: marked %llu duplicate records in %llu groups\n", (unsigned long long)st.dup_marked, (unsigned long long)st.dup_groups);
    float ms[8] = {0};
    bdx_get_timings(s.ctx, ms, 8);
    fprintf(stderr, "[bdx timing] reads=%zu decode+merge+stream=%.3fs (%s, single pass, %s) bdx_run=%.4fs format=%.3fs total=%.3fs\n",
            fed.n_reads, secs(t_start, fed.t_decoded), fed.device_decoded ? "BGZF inflate and record decode on the GPU" : "host decode threads",
            in.opts.mark_dup ? "records marked and classified inside bdx_run" : "records classified as they are produced",
            secs(fed.t_decoded, fed.t_ran), secs(fed.t_ran, now()), secs(t_start, now()));
    fprintf(stderr, "[bdx timing] inside bdx_run (ms): classify kernel %.3f, host waits for its share of the groups %.3f, host walk %.3f, "
                    "final wait + scores %.3f, whole call %.3f\n", ms[0], ms[4], ms[5], ms[6], ms[7]);
}

}  // namespace bdhost
