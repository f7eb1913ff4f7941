// Command line of breakdancer-max: same getopt string, defaults and usage text as the reference
// (common/Options.cpp:27-122), -C / -R (the pass-1 cache, cache.h) included, plus the long options --vcf, --exclude, --sites / --sites-vcf /
// --sites-window, --mark-dup, --ci / --ci-window, --depth / --depth-flank, --mapq / --mapq-window, --clip / --clip-window / --clip-min / --clip-support, --estimate / --estimate-config, --mini / --mini-window / --mini-step / --mini-min-pairs / --mini-score and
// --anchor / --anchor-window / --anchor-step / --anchor-min / --anchor-mapq.
#pragma once
#include <string>
#include <vector>

#include "bdx.h"

namespace bdhost {

struct Options {
    std::string chr;             // -o
    std::string cache_file;      // -C: write the pass-1 cache
    std::string restore_file;    // -R: run from a pass-1 cache (no other argument allowed)
    std::string bam_config_path;
    std::string prefix_fastq;    // -d
    std::string dump_BED;        // -g
    std::string vcf;             // --vcf: the printed calls as VCF with per-sample genotypes (vcf.h)
    std::string exclude;         // --exclude: a BED file of regions whose read pairs the readers drop (exclude.h)
    std::string sites;           // --sites: a table of SV sites to genotype over the records the run holds (sites.h) ...
    std::string sites_vcf;       // --sites-vcf: ... and the VCF they are written to (one needs the other)
    bool mark_dup = false;       // --mark-dup: duplicate read pairs get SAM flag 0x400 on the GPU before pass 1 (bdx_set_mark_duplicates)
    int sites_window = -1;       // --sites-window: how far from a breakpoint a supporting read may start (-1: from the libraries' cutoffs)
    bool ci = false;             // --ci: CIPOS / CIEND / CIN of every --vcf / --sites-vcf record from its supporting pairs (bdx_site_breakpoint_bounds)
    int ci_window = -1;          // --ci-window: how far from a breakpoint such a pair's read may start (-1: from the libraries' cutoffs)
    bool depth = false;          // --depth: RCI / RCF / RDR of every --vcf / --sites-vcf record: passing read starts inside and beside it (bdx_count_interval_reads)
    int depth_flank = -1;        // --depth-flank: the width of either flank (-1: kDepthFlankDefault)
    bool mapq = false;           // --mapq: SQ* / LQ* of every --vcf / --sites-vcf record: mapping quality at either end (bdx_site_end_quality)
    int mapq_window = -1;        // --mapq-window: how far from a breakpoint a read of --mapq may start (-1: from the libraries' cutoffs)
    bool estimate = false;       // --estimate: mean, std and cutoffs of every library from all pairs the run holds (bdx_insert_size_histogram, estimate.h)
    std::string estimate_config; // --estimate-config: the configuration with the estimated values, written for later runs (needs --estimate)
    std::string mini;            // --mini: small insertions and deletions from windowed insert-size Kolmogorov-Smirnov tests, written to this file (mini.h)
    int mini_window = -1;        // --mini-window: the window's width (-1: the ceiling of the largest library mean insert size)
    int mini_step = -1;          // --mini-step: the distance between two windows' starts (-1: half the window)
    int mini_min_pairs = -1;     // --mini-min-pairs: the pairs of one library a window needs for its row to score (-1: kMiniMinPairsDefault)
    int mini_score = -1;         // --mini-score: the score a window must reach (-1: from the number of scoring windows)
    static constexpr int kMiniMinPairsDefault = 20;
    std::string anchor;          // --anchor: insertion sites from clusters of reads whose mate is unmapped, written to this file (anchor.h)
    int anchor_window = -1;      // --anchor-window: the window's width (-1: twice the ceiling of the largest finite library uppercutoff)
    int anchor_step = -1;        // --anchor-step: the distance between two windows' starts (-1: half the window)
    int anchor_min = -1;         // --anchor-min: the distinct starts a call needs on either side (-1: kAnchorMinDefault)
    int anchor_mapq = -1;        // --anchor-mapq: bdx_window_anchor_split's min_qual, 0 .. 255 (-1: the libraries' own minima)
    static constexpr int kAnchorMinDefault = 3;
    static constexpr int kDepthFlankDefault = 1000;
    bool clip = false;           // --clip: CLN / CLPOS / CLSUP / CLSIDE of every --vcf / --sites-vcf record: the piles of clipped reads at either end (bdx_site_clip_peaks)
    int clip_window = -1;        // --clip-window: how far from a breakpoint a clip may stand, 0 .. BDX_CLIP_WINDOW_MAX (-1: from the libraries' cutoffs, at most that)
    int clip_min = -1;           // --clip-min: the clipped bases a read needs to count, 1 .. 255 (-1: kClipMinDefault)
    int clip_support = -1;       // --clip-support: the reads a pile needs to be reported (-1: kClipSupportDefault)
    static constexpr int kClipMinDefault = 10, kClipSupportDefault = 2;
    int min_clip() const { return clip_min > 0 ? clip_min : kClipMinDefault; }
    int clip_needed() const { return clip_support > 0 ? clip_support : kClipSupportDefault; }
    int flank() const { return depth_flank > 0 ? depth_flank : kDepthFlankDefault; }
    bdx_opts o;                  // numeric options in the C-ABI layout
    std::vector<std::string> orig_argv;
    int device = 0;              // env BDX_DEVICE

    // parses argv; prints usage to stderr and exits 1 like the reference when no config is given
    Options(int argc, char** argv);
    std::string sv_type(int flag) const;  // Options.cpp:105-119
    // the inverse of sv_type: bit f set when ReadFlag f (an anomalous class) prints as `type`; 0: none does under this run's -l
    uint32_t sv_flag_mask(const std::string& type) const;
};

}  // namespace bdhost
