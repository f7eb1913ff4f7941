#include "store_counts.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <stdexcept>
#include <thread>

#include "table.h"

namespace bdhost {

void check(bdx_ctx* ctx, int rc, const char* what) {
    if (rc == BDX_OK) return;
    std::string msg = std::string(what) + ": " + bdx_strerror(rc);
    if (ctx && bdx_last_error(ctx)[0]) msg += std::string(" (") + bdx_last_error(ctx) + ")";
    throw std::runtime_error(msg);
}

namespace {

// the context of rank r of a sharded run (one per rank, the same for every chromosome: asking for the last sequence passes the
// feeding-order check whatever was fed)
bdx_ctx* rank_context(const RunContexts& rc, size_t r) { return bdx_dist_chromosome(rc.ranks[r], (int)rc.rank_of.size() - 1); }

// Counts over the resident records, one item per query: on the single context all at once, or -- a sharded run -- item i on the rank that
// holds chromosome item_tid[i], every rank on its own context and on a thread of its own.  count(context, the items' indices, their
// counts [items][ns]) returns a bdx status.
template <class T, class F>
void count_on_ranks(const RunContexts& rc, const std::vector<int32_t>& item_tid, size_t ns, const char* what, std::vector<T>& counts, F count) {
    const size_t nq = item_tid.size();
    counts.assign(nq * ns, T{});
    if (!nq) return;
    if (rc.ranks.empty()) {
        std::vector<size_t> all(nq);
        for (size_t i = 0; i < nq; ++i) all[i] = i;
        check(rc.ctx, count(rc.ctx, all, counts.data()), what);
        return;
    }
    const size_t world = rc.ranks.size();
    std::vector<std::vector<size_t>> mine(world);
    for (size_t i = 0; i < nq; ++i) mine[(size_t)rc.rank_of[item_tid[i]]].push_back(i);
    std::vector<std::string> errs(world);
    std::vector<std::thread> th;
    for (size_t r = 0; r < world; ++r) {
        if (mine[r].empty()) continue;
        th.emplace_back([&, r] {
            const std::vector<size_t>& m = mine[r];
            std::vector<T> c(m.size() * ns);
            bdx_ctx* rctx = rank_context(rc, r);
            const int st = rctx ? count(rctx, m, c.data()) : BDX_EINTERNAL;
            if (st != BDX_OK) {
                errs[r] = std::string(what) + " on rank " + std::to_string(r) + ": " + bdx_strerror(st) + (rctx ? std::string(" (") + bdx_last_error(rctx) + ")" : "");
                return;
            }
            for (size_t j = 0; j < m.size(); ++j) std::copy(c.begin() + j * ns, c.begin() + (j + 1) * ns, counts.begin() + m[j] * ns);
        });
    }
    for (auto& t : th) t.join();
    for (auto const& e : errs)
        if (!e.empty()) throw std::runtime_error(e);
}

// DR of --vcf and --sites-vcf records: the normal pairs covering the record's junctions, counted on the GPU over the records the run holds
// (K8).  A same-chromosome record is one query over both junctions (a pair counts once); a CTX record two, added.  DR is unknown with -t
// (no read carries the normal-pair bit) and for a junction on a chromosome the run did not read (the -o chromosome only).
void fill_dr(const Options& opts, const RunContexts& rc, size_t ns, std::vector<VcfRecord>& out) {
    const bool by_lib = opts.o.cn_lib != 0;
    std::vector<int32_t> q_tid, q_a, q_b;
    std::vector<size_t> q_row;
    for (size_t k = 0; k < out.size(); ++k) {
        VcfRecord& r = out[k];
        r.dr.assign(ns, -1);
        if (opts.o.transchr_rearrange || !rc.held(r.chr1) || !rc.held(r.chr2) || r.pos1 < 1 || r.pos2 < 1) continue;
        r.dr.assign(ns, 0);
        if (r.chr1 == r.chr2) {
            q_tid.push_back(r.chr1); q_a.push_back(std::min(r.pos1, r.pos2)); q_b.push_back(std::max(r.pos1, r.pos2)); q_row.push_back(k);
        } else {
            q_tid.push_back(r.chr1); q_a.push_back(r.pos1); q_b.push_back(r.pos1); q_row.push_back(k);
            q_tid.push_back(r.chr2); q_a.push_back(r.pos2); q_b.push_back(r.pos2); q_row.push_back(k);
        }
    }
    std::vector<uint32_t> counts;
    count_on_ranks(rc, q_tid, ns, "bdx_count_junction_pairs", counts, [&](bdx_ctx* c, const std::vector<size_t>& m, uint32_t* cnt) {
        std::vector<int32_t> t(m.size()), a(m.size()), b(m.size());
        for (size_t j = 0; j < m.size(); ++j) { t[j] = q_tid[m[j]]; a[j] = q_a[m[j]]; b[j] = q_b[m[j]]; }
        return bdx_count_junction_pairs(c, t.data(), a.data(), b.data(), m.size(), by_lib ? 1 : 0, cnt);
    });
    for (size_t i = 0; i < q_tid.size(); ++i)
        for (size_t k = 0; k < ns; ++k) out[q_row[i]].dr[k] += counts[i * ns + k];
}

}  // namespace

// DV: the dominant type's pairs of the sample (library with -a, else BAM file); DR: fill_dr.
std::vector<VcfRecord> vcf_records(const Options& opts, const BamConfig& cfg, const std::vector<bdx_sv>& svs, const std::vector<size_t>& rows,
                                   const std::vector<int32_t>& li, const std::vector<int32_t>& lp, const RunContexts& rc) {
    const bool by_lib = opts.o.cn_lib != 0;
    const size_t ns = sample_names(opts, cfg).size();
    std::vector<VcfRecord> out(rows.size());
    for (size_t k = 0; k < rows.size(); ++k) {
        const bdx_sv& s = svs[rows[k]];
        VcfRecord& r = out[k];
        r.row = k + 1;
        r.chr1 = s.chr[0]; r.pos1 = s.pos[0]; r.chr2 = s.chr[1]; r.pos2 = s.pos[1];
        r.ori1 = std::to_string(s.fwd[0]) + "+" + std::to_string(s.rev[0]) + "-";
        r.ori2 = std::to_string(s.fwd[1]) + "+" + std::to_string(s.rev[1]) + "-";
        r.type = opts.sv_type(s.flag);
        r.size = s.size; r.score = s.score; r.nreads = s.num_reads; r.af = s.allele_frequency;
        r.dv.assign(ns, 0);
        for (int i = 0; i < s.lib_count; ++i) {
            const size_t lib = (size_t)li[s.lib_begin + i];
            const size_t key = by_lib ? lib : cfg.library_config(lib).bam_file_index;
            if (key < ns) r.dv[key] += lp[s.lib_begin + i];
        }
    }
    fill_dr(opts, rc, ns, out);
    return out;
}

// DV: the pairs of the site's type with a mate starting within `window` of each end, counted on the GPU over the records the run holds
// (KS, bdx_count_site_pairs) -- a sharded run's sites on the rank that holds tid1, where a pair's lower mate lives, CTX included; DR:
// fill_dr.  Both are unknown for a site with an end on a chromosome the run did not read.
std::vector<VcfRecord> site_records(const Options& opts, const BamConfig& cfg, const SiteTable& table, int32_t window, const RunContexts& rc) {
    const bool by_lib = opts.o.cn_lib != 0;
    const size_t ns = sample_names(opts, cfg).size();
    std::vector<VcfRecord> out(table.sites.size());
    std::vector<bdx_site> q;
    std::vector<int32_t> q_tid;
    std::vector<size_t> q_row;
    for (size_t k = 0; k < table.sites.size(); ++k) {
        const SiteLine& s = table.sites[k];
        VcfRecord& r = out[k];
        r.row = k + 1;
        r.chr1 = s.chr1; r.pos1 = s.pos1; r.chr2 = s.chr2; r.pos2 = s.pos2;
        r.type = s.type;
        r.has_size = s.has_size;
        r.size = (int)std::max<long long>(-0x7FFFFFFF, std::min<long long>(s.size, 0x7FFFFFFF));
        r.dv.assign(ns, -1);
        if (!rc.held(s.chr1) || !rc.held(s.chr2)) continue;
        r.dv.assign(ns, 0);
        q.push_back(s.site); q_tid.push_back(s.site.tid1); q_row.push_back(k);
    }
    std::vector<uint32_t> counts;
    count_on_ranks(rc, q_tid, ns, "bdx_count_site_pairs", counts, [&](bdx_ctx* c, const std::vector<size_t>& m, uint32_t* cnt) {
        std::vector<bdx_site> mine(m.size());
        for (size_t j = 0; j < m.size(); ++j) mine[j] = q[m[j]];
        return bdx_count_site_pairs(c, mine.data(), m.size(), window, by_lib ? 1 : 0, cnt);
    });
    for (size_t i = 0; i < q.size(); ++i)
        for (size_t k = 0; k < ns; ++k) out[q_row[i]].dv[k] = counts[i * ns + k];
    fill_dr(opts, rc, ns, out);
    return out;
}

// Each record becomes a site -- its two ends put into order, its mask the read classes that print as its type (Options::sv_flag_mask,
// the mapping --sites uses) -- whose supporting pairs bound the breakpoint at either end (KI, bdx_site_breakpoint_bounds; a sharded
// run's sites on the rank that holds tid1, as for KS).  An end that was swapped for normalisation is swapped back.  No CI for a record
// with an end on a chromosome the run did not read, a position below 1, a type no read class maps to, or no supporting pair.
void fill_ci(const Options& opts, const RunContexts& rc, int32_t window, std::vector<VcfRecord>& out) {
    constexpr size_t kWords = sizeof(bdx_site_bounds) / 4;   // (count_on_ranks moves rows of 32-bit words: a site's bounds are five)
    static_assert(sizeof(bdx_site_bounds) == 20 && alignof(bdx_site_bounds) == 4, "bdx_site_bounds is five 32-bit words");
    std::vector<bdx_site> q;
    std::vector<int32_t> q_tid;
    std::vector<size_t> q_row;
    std::vector<char> q_swapped;
    for (size_t k = 0; k < out.size(); ++k) {
        const VcfRecord& r = out[k];
        const uint32_t mask = opts.sv_flag_mask(r.type);
        if (!rc.held(r.chr1) || !rc.held(r.chr2) || r.pos1 < 1 || r.pos2 < 1 || mask == 0) continue;
        const bool swapped = r.chr1 > r.chr2 || (r.chr1 == r.chr2 && r.pos1 > r.pos2);
        q.push_back(swapped ? bdx_site{r.chr2, r.pos2, r.chr1, r.pos1, mask} : bdx_site{r.chr1, r.pos1, r.chr2, r.pos2, mask});
        q_tid.push_back(q.back().tid1); q_row.push_back(k); q_swapped.push_back(swapped ? 1 : 0);
    }
    std::vector<uint32_t> words;
    count_on_ranks(rc, q_tid, kWords, "bdx_site_breakpoint_bounds", words, [&](bdx_ctx* c, const std::vector<size_t>& m, uint32_t* w) {
        std::vector<bdx_site> mine(m.size());
        for (size_t j = 0; j < m.size(); ++j) mine[j] = q[m[j]];
        std::vector<bdx_site_bounds> b(m.size());
        const int st = bdx_site_breakpoint_bounds(c, mine.data(), m.size(), window, b.data());
        if (st == BDX_OK) memcpy(w, b.data(), b.size() * sizeof(bdx_site_bounds));
        return st;
    });
    for (size_t i = 0; i < q.size(); ++i) {
        bdx_site_bounds b;
        memcpy(&b, words.data() + i * kWords, sizeof b);
        if (b.n == 0) continue;
        VcfRecord& r = out[q_row[i]];
        r.has_ci = true;
        r.ci_n = b.n;
        r.ci_lo1 = q_swapped[i] ? b.lo2 : b.lo1; r.ci_hi1 = q_swapped[i] ? b.hi2 : b.hi1;
        r.ci_lo2 = q_swapped[i] ? b.lo1 : b.lo2; r.ci_hi2 = q_swapped[i] ? b.hi1 : b.hi2;
    }
}

// Each record becomes a site exactly as in fill_ci -- its ends put into order, its mask Options::sv_flag_mask -- and every end of it that
// lies on a chromosome the run read is one query (KM, bdx_site_end_quality): up to two per record, all of an output's in one call, a
// sharded run's on the rank that holds the ASKED end's chromosome -- every record that can count for an end lives there, so a CTX record's
// two ends go to two ranks.  The ends stay in the site's order and the record notes that its own is the reverse (the writer swaps them
// back).  A record takes part when both positions are >= 1, a read class maps to its type and at least one end is held.
void fill_quality(const Options& opts, const RunContexts& rc, int32_t window, std::vector<VcfRecord>& out) {
    constexpr size_t kWords = sizeof(bdx_site_quality) / 4;   // (count_on_ranks moves rows of 32-bit words: an end's summary is four)
    static_assert(sizeof(bdx_site_quality) == 16 && alignof(bdx_site_quality) == 4, "bdx_site_quality is four 32-bit words");
    std::vector<bdx_site> q;
    std::vector<uint8_t> q_end;
    std::vector<int32_t> q_tid;
    std::vector<size_t> q_row;
    for (size_t k = 0; k < out.size(); ++k) {
        VcfRecord& r = out[k];
        const uint32_t mask = opts.sv_flag_mask(r.type);
        if ((!rc.held(r.chr1) && !rc.held(r.chr2)) || r.pos1 < 1 || r.pos2 < 1 || mask == 0) continue;
        const bool swapped = r.chr1 > r.chr2 || (r.chr1 == r.chr2 && r.pos1 > r.pos2);
        const bdx_site s = swapped ? bdx_site{r.chr2, r.pos2, r.chr1, r.pos1, mask} : bdx_site{r.chr1, r.pos1, r.chr2, r.pos2, mask};
        r.has_mapq = true;
        r.mq_swapped = swapped;
        for (int e = 0; e < 2; ++e) {
            const int32_t t = e ? s.tid2 : s.tid1;
            r.mq[e] = EndQuality{};
            if (!rc.held(t)) continue;
            r.mq[e].held = true;
            q.push_back(s); q_end.push_back((uint8_t)(e + 1)); q_tid.push_back(t); q_row.push_back(k);
        }
    }
    std::vector<uint32_t> words;
    count_on_ranks(rc, q_tid, kWords, "bdx_site_end_quality", words, [&](bdx_ctx* c, const std::vector<size_t>& m, uint32_t* w) {
        std::vector<bdx_site> mine(m.size());
        std::vector<uint8_t> ends(m.size());
        for (size_t j = 0; j < m.size(); ++j) { mine[j] = q[m[j]]; ends[j] = q_end[m[j]]; }
        std::vector<bdx_site_quality> b(m.size());
        const int st = bdx_site_end_quality(c, mine.data(), ends.data(), m.size(), window, b.data());
        if (st == BDX_OK) memcpy(w, b.data(), b.size() * sizeof(bdx_site_quality));
        return st;
    });
    for (size_t i = 0; i < q.size(); ++i) {
        bdx_site_quality b;
        memcpy(&b, words.data() + i * kWords, sizeof b);
        EndQuality& e = out[q_row[i]].mq[q_end[i] - 1];
        e.n = b.n; e.n_all = b.n_all; e.n_low = b.n_low;
        e.qmin = b.qmin; e.q1 = b.q1; e.median = b.median; e.qmax = b.qmax;
    }
}

// As fill_quality, query for query: KP (bdx_site_clip_peaks) instead of KM, on the rank that holds the asked end's chromosome.
uint64_t fill_clips(const Options& opts, const RunContexts& rc, int32_t window, int32_t min_clip, std::vector<VcfRecord>& out) {
    constexpr size_t kWords = sizeof(bdx_clip_peaks) / 4;   // (count_on_ranks moves rows of 32-bit words: an end's piles are six)
    static_assert(sizeof(bdx_clip_peaks) == 24 && alignof(bdx_clip_peaks) == 4, "bdx_clip_peaks is six 32-bit words");
    std::vector<bdx_site> q;
    std::vector<uint8_t> q_end;
    std::vector<int32_t> q_tid;
    std::vector<size_t> q_row;
    for (size_t k = 0; k < out.size(); ++k) {
        VcfRecord& r = out[k];
        const uint32_t mask = opts.sv_flag_mask(r.type);
        if ((!rc.held(r.chr1) && !rc.held(r.chr2)) || r.pos1 < 1 || r.pos2 < 1 || mask == 0) continue;
        const bool swapped = r.chr1 > r.chr2 || (r.chr1 == r.chr2 && r.pos1 > r.pos2);
        const bdx_site s = swapped ? bdx_site{r.chr2, r.pos2, r.chr1, r.pos1, mask} : bdx_site{r.chr1, r.pos1, r.chr2, r.pos2, mask};
        r.has_clip = true;
        r.cl_swapped = swapped;
        for (int e = 0; e < 2; ++e) {
            const int32_t t = e ? s.tid2 : s.tid1;
            r.cl[e] = EndClips{};
            r.cl[e].pos = e ? s.pos2 : s.pos1;
            if (!rc.held(t)) continue;
            r.cl[e].held = true;
            q.push_back(s); q_end.push_back((uint8_t)(e + 1)); q_tid.push_back(t); q_row.push_back(k);
        }
    }
    std::vector<uint32_t> words;
    count_on_ranks(rc, q_tid, kWords, "bdx_site_clip_peaks", words, [&](bdx_ctx* c, const std::vector<size_t>& m, uint32_t* w) {
        std::vector<bdx_site> mine(m.size());
        std::vector<uint8_t> ends(m.size());
        for (size_t j = 0; j < m.size(); ++j) { mine[j] = q[m[j]]; ends[j] = q_end[m[j]]; }
        std::vector<bdx_clip_peaks> b(m.size());
        const int st = bdx_site_clip_peaks(c, mine.data(), ends.data(), m.size(), window, min_clip, b.data());
        if (st == BDX_OK) memcpy(w, b.data(), b.size() * sizeof(bdx_clip_peaks));
        return st;
    });
    uint64_t observations = 0;
    for (size_t i = 0; i < q.size(); ++i) {
        bdx_clip_peaks b;
        memcpy(&b, words.data() + i * kWords, sizeof b);
        EndClips& e = out[q_row[i]].cl[q_end[i] - 1];
        e.n_left = b.n_left; e.n_right = b.n_right; e.pos_left = b.pos_left; e.pos_right = b.pos_right; e.peak_left = b.peak_left; e.peak_right = b.peak_right;
        observations += (uint64_t)b.n_left + b.n_right;
    }
    return observations;
}

// Every record with both ends on one sequence the run read and pos1 != pos2 gives three intervals of read starts -- its inside and its two
// flanks (vcf.h depth_spans), clamped to the sequence -- and all of them go to the GPU in one call (KR, bdx_count_interval_reads; a sharded
// run's on the rank that holds the sequence).  RCI is the inside's count per sample, RCF the two flanks' together.
void fill_depth(const Options& opts, const RunContexts& rc, int32_t flank, const std::vector<uint32_t>& lengths, size_t ns, std::vector<VcfRecord>& out) {
    const bool by_lib = opts.o.cn_lib != 0;
    std::vector<bdx_interval> q;
    std::vector<int32_t> q_tid;
    std::vector<size_t> q_row;
    for (size_t k = 0; k < out.size(); ++k) {
        VcfRecord& r = out[k];
        if (r.chr1 != r.chr2 || r.pos1 == r.pos2 || !rc.held(r.chr1) || (size_t)r.chr1 >= lengths.size()) continue;
        r.has_depth = true;
        r.spans = depth_spans(r.pos1, r.pos2, flank, std::min<int64_t>(lengths[r.chr1], 2147483646));
        r.rci.assign(ns, 0); r.rcf.assign(ns, 0);
        const DepthSpans& s = r.spans;
        for (const bdx_interval& iv : {bdx_interval{r.chr1, (int32_t)s.in_beg, (int32_t)s.in_end}, bdx_interval{r.chr1, (int32_t)s.left_beg, (int32_t)s.left_end},
                                       bdx_interval{r.chr1, (int32_t)s.right_beg, (int32_t)s.right_end}}) {
            q.push_back(iv); q_tid.push_back(r.chr1); q_row.push_back(k);
        }
    }
    std::vector<uint32_t> counts;
    count_on_ranks(rc, q_tid, ns, "bdx_count_interval_reads", counts, [&](bdx_ctx* c, const std::vector<size_t>& m, uint32_t* cnt) {
        std::vector<bdx_interval> mine(m.size());
        for (size_t j = 0; j < m.size(); ++j) mine[j] = q[m[j]];
        return bdx_count_interval_reads(c, mine.data(), m.size(), by_lib ? 1 : 0, cnt);
    });
    for (size_t i = 0; i < q.size(); ++i)
        for (size_t k = 0; k < ns; ++k) (i % 3 == 0 ? out[q_row[i]].rci : out[q_row[i]].rcf)[k] += counts[i * ns + k];
}

int32_t cutoff_window(const BamConfig& cfg, const char* option) {
    double ub = -1.0;
    for (size_t i = 0; i < cfg.num_libs(); ++i) {
        const double u = cfg.library_config(i).uppercutoff;
        if (std::isfinite(u)) ub = std::max(ub, std::ceil(u));
    }
    if (ub < 0) throw std::runtime_error(std::string(option) + ": no library has a finite uppercutoff, give " + option + "-window");
    return (int32_t)std::min(ub, 1073741824.0);
}

int32_t clip_default_window(const BamConfig& cfg) {
    double ub = -1.0;
    for (size_t i = 0; i < cfg.num_libs(); ++i) {
        const double u = cfg.library_config(i).uppercutoff;
        if (std::isfinite(u)) ub = std::max(ub, std::ceil(u));
    }
    return ub < 0 ? BDX_CLIP_WINDOW_MAX : (int32_t)std::min(ub, (double)BDX_CLIP_WINDOW_MAX);
}

// --mini: the store's insert-size histogram after the run (--mark-dup's marks are in the flag column), summed over the ranks
void store_insert_histogram(const RunContexts& rc, size_t nlibs, std::vector<uint64_t>& hist) {
    hist.assign(nlibs * (size_t)BDX_ISIZE_BINS, 0);
    std::vector<uint64_t> over(nlibs);
    if (rc.ranks.empty()) {
        check(rc.ctx, bdx_insert_size_histogram(rc.ctx, hist.data(), over.data()), "bdx_insert_size_histogram");
        return;
    }
    std::vector<uint64_t> h(hist.size());
    for (bdx_dist* r : rc.ranks) {
        if (bdx_dist_insert_size_histogram(r, h.data(), over.data()) != BDX_OK)
            throw std::runtime_error(std::string("bdx_dist_insert_size_histogram: ") + bdx_dist_last_error(r));
        for (size_t i = 0; i < hist.size(); ++i) hist[i] += h[i];
    }
}

void set_insert_null(const RunContexts& rc, const uint64_t* hist) {
    if (rc.ranks.empty()) {
        check(rc.ctx, bdx_set_insert_null(rc.ctx, hist), "bdx_set_insert_null");
        return;
    }
    for (size_t r = 0; r < rc.ranks.size(); ++r) {
        bdx_ctx* c = rank_context(rc, r);
        if (!c) throw std::runtime_error(std::string("bdx_dist_chromosome: ") + bdx_dist_last_error(rc.ranks[r]));
        check(c, bdx_set_insert_null(c, hist), "bdx_set_insert_null");
    }
}

void window_insert_shift(const RunContexts& rc, const std::vector<bdx_interval>& iv, size_t nlibs, std::vector<bdx_insert_shift>& rows) {
    std::vector<int32_t> q_tid(iv.size());
    for (size_t i = 0; i < iv.size(); ++i) q_tid[i] = iv[i].tid;
    count_on_ranks(rc, q_tid, nlibs, "bdx_window_insert_shift", rows, [&](bdx_ctx* c, const std::vector<size_t>& m, bdx_insert_shift* out) {
        if (m.size() == iv.size()) return bdx_window_insert_shift(c, iv.data(), iv.size(), out);   // (the single context: all of them, in order)
        std::vector<bdx_interval> mine(m.size());
        for (size_t j = 0; j < m.size(); ++j) mine[j] = iv[m[j]];
        return bdx_window_insert_shift(c, mine.data(), m.size(), out);
    });
}

void window_anchor_split(const RunContexts& rc, const std::vector<bdx_interval>& iv, int32_t min_qual, std::vector<bdx_anchor_split>& rows) {
    if (iv.size() > ((size_t)1 << 22)) throw std::runtime_error("window_anchor_split: more than 2^22 windows in one call");
    std::vector<int32_t> q_tid(iv.size());
    for (size_t i = 0; i < iv.size(); ++i) q_tid[i] = iv[i].tid;
    count_on_ranks(rc, q_tid, 1, "bdx_window_anchor_split", rows, [&](bdx_ctx* c, const std::vector<size_t>& m, bdx_anchor_split* out) {
        if (m.size() == iv.size()) return bdx_window_anchor_split(c, iv.data(), iv.size(), min_qual, out);   // (the single context: all of them, in order)
        std::vector<bdx_interval> mine(m.size());
        for (size_t j = 0; j < m.size(); ++j) mine[j] = iv[m[j]];
        return bdx_window_anchor_split(c, mine.data(), m.size(), min_qual, out);
    });
}

}  // namespace bdhost
