// --vcf / --sites / --ci / --depth / --mapq / --mini / --anchor: the counts over the records a finished run holds on the GPU (K8, KS, KI, KR, KM, KW, KA of include/bdx.h), turned into the
// records VcfWriter prints (vcf.h).
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "bdx.h"
#include "config.h"
#include "options.h"
#include "sites.h"
#include "vcf.h"

namespace bdhost {

// throws std::runtime_error naming `what`, the status and the context's last error unless rc is BDX_OK (ctx may be null)
void check(bdx_ctx* ctx, int rc, const char* what);

// The contexts a finished run left behind: the single context, or the ranks of a sharded run (each holds its chromosomes' records).
struct RunContexts {
    bdx_ctx* ctx;
    const std::vector<bdx_dist*>& ranks;
    const std::vector<int>& rank_of;   // (sharded runs) chromosome -> rank
    int only_tid;                      // >= 0: the -o chromosome, the only one the run read
    bool held(int t) const { return t >= 0 && (only_tid < 0 || t == only_tid) && (ranks.empty() || (size_t)t < rank_of.size()); }
};

// --vcf: one record per printed row (svs[rows[k]] is row k + 1 of the table).  DV: the dominant type's pairs of the sample (library with
// -a, else BAM file); DR: the normal pairs covering the record's junctions, counted on the GPU.
std::vector<VcfRecord> vcf_records(const Options& opts, const BamConfig& cfg, const std::vector<bdx_sv>& svs, const std::vector<size_t>& rows,
                                   const std::vector<int32_t>& li, const std::vector<int32_t>& lp, const RunContexts& rc);

// --sites-vcf: one record per kept line of the --sites table, as the file gave it, DV and DR counted on the GPU.
std::vector<VcfRecord> site_records(const Options& opts, const BamConfig& cfg, const SiteTable& table, int32_t window, const RunContexts& rc);

// --ci: CIPOS / CIEND of --vcf and --sites-vcf records from the breakpoint bounds their supporting pairs give.
void fill_ci(const Options& opts, const RunContexts& rc, int32_t window, std::vector<VcfRecord>& out);

// --mapq: SQ* / LQ* of --vcf and --sites-vcf records from the mapping qualities of the reads that support either end and of those around it.
void fill_quality(const Options& opts, const RunContexts& rc, int32_t window, std::vector<VcfRecord>& out);

// --clip: CL* of --vcf and --sites-vcf records from the piles of clipped reads at either end (KP, bdx_site_clip_peaks); which records take
// part, and where an end is asked, as in fill_quality.  Returns the observations of all ends together.
uint64_t fill_clips(const Options& opts, const RunContexts& rc, int32_t window, int32_t min_clip, std::vector<VcfRecord>& out);

// --depth: RCI / RCF of --vcf and --sites-vcf records from the passing read starts inside and beside them; lengths: the sequences' (the
// flanks are clamped to them), ns: the samples.
void fill_depth(const Options& opts, const RunContexts& rc, int32_t flank, const std::vector<uint32_t>& lengths, size_t ns, std::vector<VcfRecord>& out);

// --mini: the store's insert-size histogram after the run, summed over the ranks (hist[nlibs][BDX_ISIZE_BINS]); that histogram as the null of
// every context of the run; and the rows [windows][nlibs] of bdx_window_insert_shift, each window answered by the rank that holds its sequence
// (every iv[i].tid is a sequence the run holds).
void store_insert_histogram(const RunContexts& rc, size_t nlibs, std::vector<uint64_t>& hist);
void set_insert_null(const RunContexts& rc, const uint64_t* hist);
void window_insert_shift(const RunContexts& rc, const std::vector<bdx_interval>& iv, size_t nlibs, std::vector<bdx_insert_shift>& rows);

// --anchor: the rows [windows] of bdx_window_anchor_split (KA), each window answered by the rank that holds its sequence (every iv[i].tid is
// a sequence the run holds); at most 2^22 windows per call (160 MiB of rows)
void window_anchor_split(const RunContexts& rc, const std::vector<bdx_interval>& iv, int32_t min_qual, std::vector<bdx_anchor_split>& rows);

// How far a supporting mate can start from a breakpoint it brackets: the ceiling of the largest finite library uppercutoff, the window
// of --sites, --ci and --mapq when theirs is not given.
int32_t cutoff_window(const BamConfig& cfg, const char* option);
// --clip's: the same ceiling, at most BDX_CLIP_WINDOW_MAX; that when no cutoff is finite
int32_t clip_default_window(const BamConfig& cfg);

}  // namespace bdhost
