#include "options.h"

#include <getopt.h>

#include <cstdio>
#include <cstdlib>
#include <stdexcept>
#include <string>

namespace bdhost {

namespace {

// One row per command-line option: where its value goes and what the usage text says about it.  The getopt string and the
// usage block are generated from this table (letters, argument kinds, defaults and wording as the reference documents them,
// common/Options.cpp:27-122; -C / -R are accepted without being listed, as there).
enum Kind { kInt, kFlag, kString };
struct Row {
    char letter;
    Kind kind;
    int32_t bdx_opts::*num;        // kInt / kFlag
    std::string Options::*str;     // kString
    const char* help;              // nullptr: not listed in the usage text
    bool show_default;
};
const Row kRows[] = {
    {'o', kString, nullptr, &Options::chr, "operate on a single chromosome [all chromosome]", false},
    {'s', kInt, &bdx_opts::min_len, nullptr, "minimum length of a region", true},
    {'c', kInt, &bdx_opts::cut_sd, nullptr, "cutoff in unit of standard deviation", true},
    {'m', kInt, &bdx_opts::max_sd, nullptr, "maximum SV size", true},
    {'q', kInt, &bdx_opts::min_map_qual, nullptr, "minimum alternative mapping quality", true},
    {'r', kInt, &bdx_opts::min_read_pair, nullptr, "minimum number of read pairs required to establish a connection", true},
    {'x', kInt, &bdx_opts::seq_coverage_lim, nullptr, "maximum threshold of haploid sequence coverage for regions to be ignored", true},
    {'b', kInt, &bdx_opts::buffer_size, nullptr, "buffer size for building connection", true},
    {'t', kFlag, &bdx_opts::transchr_rearrange, nullptr, "only detect transchromosomal rearrangement, by default off", false},
    {'f', kFlag, &bdx_opts::fisher, nullptr, nullptr, false},
    {'d', kString, nullptr, &Options::prefix_fastq, "prefix of fastq files that SV supporting reads will be saved by library", false},
    {'g', kString, nullptr, &Options::dump_BED, "dump SVs and supporting reads in BED format for GBrowse", false},
    {'l', kFlag, &bdx_opts::illumina_long_insert, nullptr, "analyze Illumina long insert (mate-pair) library", false},
    {'a', kFlag, &bdx_opts::cn_lib, nullptr, "print out copy number and support reads per library rather than per bam, by default off", false},
    {'h', kFlag, &bdx_opts::print_af, nullptr, "print out Allele Frequency column, by default off", false},
    {'y', kInt, &bdx_opts::score_threshold, nullptr, "output score filter", true},
    {'C', kString, nullptr, &Options::cache_file, nullptr, false},
    {'R', kString, nullptr, &Options::restore_file, nullptr, false},
};

std::string getopt_string() {
    std::string g;
    for (const Row& r : kRows) {
        g += r.letter;
        if (r.kind != kFlag) g += ':';
    }
    return g;
}

void print_usage(const bdx_opts& o) {
    fprintf(stderr, "\nbreakdancer-max (MI355X-native clustering path, libbdx)\n\nUsage: breakdancer-max <analysis.config>\n\nOptions: \n");
    for (const Row& r : kRows) {
        if (!r.help) continue;
        const char* arg = r.kind == kInt ? "INT   " : r.kind == kString ? "STRING" : "      ";
        if (r.show_default) fprintf(stderr, "       -%c %s       %s [%d]\n", r.letter, arg, r.help, o.*(r.num));
        else fprintf(stderr, "       -%c %s       %s\n", r.letter, arg, r.help);
    }
    fprintf(stderr, "       --vcf FILE     write the printed calls as VCF with per-sample genotypes (GT:GQ:PL:DR:DV)\n");
    fprintf(stderr, "       --exclude FILE drop read pairs with a mate starting in a region of this BED file (centromeres, gaps, pile-ups)\n");
    fprintf(stderr, "       --sites FILE   genotype the SV sites of this table (the tool's own output columns) over the records the run holds\n");
    fprintf(stderr, "       --sites-vcf FILE   the VCF the --sites genotypes are written to (GT:GQ:PL:DR:DV; required with --sites)\n");
    fprintf(stderr, "       --sites-window INT how far from a breakpoint a supporting read may start [the largest library uppercutoff]\n");
    fprintf(stderr, "       --ci           add CIPOS / CIEND (and CIN) to every --vcf / --sites-vcf record: the breakpoint intervals its supporting pairs allow\n");
    fprintf(stderr, "       --ci-window INT    how far from a breakpoint a supporting read of --ci may start [the largest library uppercutoff]\n");
    fprintf(stderr, "       --mapq         add SQN / SQMIN / SQQ1 / SQMED / SQMAX and LQA / LQN / LQF to every --vcf / --sites-vcf record: the mapping quality of the reads that support either end, and the share of low-quality reads around it\n");
    fprintf(stderr, "       --mapq-window INT  how far from a breakpoint a read of --mapq may start [the largest library uppercutoff]\n");
    fprintf(stderr, "       --clip         add CLN / CLPOS / CLSUP / CLSIDE to every --vcf / --sites-vcf record: where the soft-clipped reads around either end pile up, the breakpoint to the base\n");
    fprintf(stderr, "       --clip-window INT  how far from a breakpoint a clipped read's clip may stand, 0 to %d [the largest library uppercutoff, at most %d]\n", BDX_CLIP_WINDOW_MAX, BDX_CLIP_WINDOW_MAX);
    fprintf(stderr, "       --clip-min INT     the clipped bases a read needs to count, 1 to 255 [%d]\n", Options::kClipMinDefault);
    fprintf(stderr, "       --clip-support INT the reads a pile needs to be reported, 1 to 2^30 [%d]\n", Options::kClipSupportDefault);
    fprintf(stderr, "       --depth        add RCI / RCF / RDR to every sample of a --vcf / --sites-vcf record: passing read starts inside the record, in its flanks, and their ratio\n");
    fprintf(stderr, "       --depth-flank INT  the width of either flank of --depth [%d]\n", Options::kDepthFlankDefault);
    fprintf(stderr, "       --mark-dup     flag duplicate read pairs (same library, positions and strands of both mates) on the GPU; they are ignored like reads with SAM flag 0x400\n");
    fprintf(stderr, "       --estimate     take mean, std and the cutoffs of every library from all read pairs the run holds (on the GPU), not from the configuration\n");
    fprintf(stderr, "       --estimate-config FILE write the configuration with the estimated values to FILE (with --estimate)\n");
    fprintf(stderr, "       --mini FILE    small insertions and deletions: windows whose pairs' insert sizes differ from their library's distribution (Kolmogorov-Smirnov), written to FILE\n");
    fprintf(stderr, "       --mini-window INT  the window's width [the largest library mean insert size]\n");
    fprintf(stderr, "       --mini-step INT    the distance between the starts of two windows [half the window]\n");
    fprintf(stderr, "       --mini-min-pairs INT   the pairs of one library a window needs to be tested [%d]\n", Options::kMiniMinPairsDefault);
    fprintf(stderr, "       --mini-score INT   the score a window must reach [20 + 10 log10 of the number of tested windows]\n");
    fprintf(stderr, "       --anchor FILE  insertions longer than the fragment: windows where reads whose mate is unmapped pile up on both sides of a position, written to FILE\n");
    fprintf(stderr, "       --anchor-window INT  the window's width, 1 to 2^30 [twice the largest library uppercutoff]\n");
    fprintf(stderr, "       --anchor-step INT    the distance between the starts of two windows, 1 to 2^30 [half the window]\n");
    fprintf(stderr, "       --anchor-min INT     the distinct read starts a call needs on either side, 1 to 2^30 [%d]\n", Options::kAnchorMinDefault);
    fprintf(stderr, "       --anchor-mapq INT    the quality an anchoring read needs, 0 to 255 [above its library's minimum]\n");
    fprintf(stderr, "\n");
}

// (a stated limit: the cache's pass-1 statistics belong to cutoffs the -R run would have to estimate again)
[[noreturn]] void estimate_with_cache() {
    fprintf(stderr, "--estimate does not go with -C or -R: the cache's pass-1 statistics belong to the cutoffs of the run that wrote it.\n");
    exit(1);
}

}  // namespace

Options::Options(int argc, char** argv) : orig_argv(argv, argv + argc) {
    bdx_opts_default(&o);
    const std::string spec = getopt_string();
    // (the reference's letters parse exactly as with getopt; the long options are this tool's own)
    enum { kVcf = 256, kExclude, kSites, kSitesVcf, kSitesWindow, kMarkDup, kCi, kCiWindow, kDepth, kDepthFlank, kMapq, kMapqWindow, kEstimate, kEstimateConfig, kMini, kMiniWindow, kMiniStep, kMiniMinPairs, kMiniScore, kClip, kClipWindow, kClipMin, kClipSupport, kAnchor, kAnchorWindow, kAnchorStep, kAnchorMin, kAnchorMapq };
    static const struct option kLong[] = {{"vcf", required_argument, nullptr, kVcf}, {"exclude", required_argument, nullptr, kExclude},
                                         {"sites", required_argument, nullptr, kSites}, {"sites-vcf", required_argument, nullptr, kSitesVcf},
                                         {"sites-window", required_argument, nullptr, kSitesWindow}, {"mark-dup", no_argument, nullptr, kMarkDup},
                                         {"ci", no_argument, nullptr, kCi}, {"ci-window", required_argument, nullptr, kCiWindow},
                                         {"depth", no_argument, nullptr, kDepth}, {"depth-flank", required_argument, nullptr, kDepthFlank},
                                         {"mapq", no_argument, nullptr, kMapq}, {"mapq-window", required_argument, nullptr, kMapqWindow},
                                         {"estimate", no_argument, nullptr, kEstimate}, {"estimate-config", required_argument, nullptr, kEstimateConfig},
                                         {"mini", required_argument, nullptr, kMini}, {"mini-window", required_argument, nullptr, kMiniWindow},
                                         {"mini-step", required_argument, nullptr, kMiniStep}, {"mini-min-pairs", required_argument, nullptr, kMiniMinPairs},
                                         {"mini-score", required_argument, nullptr, kMiniScore},
                                         {"clip", no_argument, nullptr, kClip}, {"clip-window", required_argument, nullptr, kClipWindow},
                                         {"clip-min", required_argument, nullptr, kClipMin}, {"clip-support", required_argument, nullptr, kClipSupport},
                                         {"anchor", required_argument, nullptr, kAnchor}, {"anchor-window", required_argument, nullptr, kAnchorWindow},
                                         {"anchor-step", required_argument, nullptr, kAnchorStep}, {"anchor-min", required_argument, nullptr, kAnchorMin},
                                         {"anchor-mapq", required_argument, nullptr, kAnchorMapq},
                                         {nullptr, 0, nullptr, 0}};
    int c;
    while ((c = getopt_long(argc, argv, spec.c_str(), kLong, nullptr)) >= 0) {
        if (c == kVcf) {
            vcf = optarg;
            continue;
        }
        if (c == kExclude) {
            exclude = optarg;
            continue;
        }
        if (c == kMarkDup) {
            mark_dup = true;
            continue;
        }
        if (c == kSites) {
            sites = optarg;
            continue;
        }
        if (c == kSitesVcf) {
            sites_vcf = optarg;
            continue;
        }
        if (c == kCi) {
            ci = true;
            continue;
        }
        if (c == kDepth) {
            depth = true;
            continue;
        }
        if (c == kMapq) {
            mapq = true;
            continue;
        }
        if (c == kEstimate) {
            estimate = true;
            continue;
        }
        if (c == kClip) {
            clip = true;
            continue;
        }
        if (c == kClipWindow || c == kClipMin || c == kClipSupport) {
            const long lo = c == kClipWindow ? 0 : 1, hi = c == kClipWindow ? BDX_CLIP_WINDOW_MAX : c == kClipMin ? 255 : (1L << 30);
            char* end = nullptr;
            const long v = strtol(optarg, &end, 10);
            if (end == optarg || *end || v < lo || v > hi) {
                fprintf(stderr, "--clip-%s takes an integer from %ld to %ld, not '%s'.\n", c == kClipWindow ? "window" : c == kClipMin ? "min" : "support", lo, hi, optarg);
                exit(1);
            }
            (c == kClipWindow ? clip_window : c == kClipMin ? clip_min : clip_support) = (int)v;
            continue;
        }
        if (c == kEstimateConfig) {
            estimate_config = optarg;
            continue;
        }
        if (c == kMini) {
            mini = optarg;
            continue;
        }
        if (c == kMiniWindow || c == kMiniStep || c == kMiniMinPairs || c == kMiniScore) {
            const bool width = c == kMiniWindow || c == kMiniStep;
            const long lo = width ? 1 : c == kMiniMinPairs ? 2 : 0, hi = width ? (1L << 30) : c == kMiniMinPairs ? BDX_MINI_CAP : 99999;
            const char* name = c == kMiniWindow ? "window" : c == kMiniStep ? "step" : c == kMiniMinPairs ? "min-pairs" : "score";
            char* end = nullptr;
            const long v = strtol(optarg, &end, 10);
            if (end == optarg || *end || v < lo || v > hi) {
                fprintf(stderr, "--mini-%s takes an integer from %ld to %ld, not '%s'.\n", name, lo, hi, optarg);
                exit(1);
            }
            (c == kMiniWindow ? mini_window : c == kMiniStep ? mini_step : c == kMiniMinPairs ? mini_min_pairs : mini_score) = (int)v;
            continue;
        }
        if (c == kAnchor) {
            anchor = optarg;
            continue;
        }
        if (c == kAnchorWindow || c == kAnchorStep || c == kAnchorMin || c == kAnchorMapq) {
            const long lo = c == kAnchorMapq ? 0 : 1, hi = c == kAnchorMapq ? 255 : (1L << 30);
            const char* name = c == kAnchorWindow ? "window" : c == kAnchorStep ? "step" : c == kAnchorMin ? "min" : "mapq";
            char* end = nullptr;
            const long v = strtol(optarg, &end, 10);
            if (end == optarg || *end || v < lo || v > hi) {
                fprintf(stderr, "--anchor-%s takes an integer from %ld to %ld, not '%s'.\n", name, lo, hi, optarg);
                exit(1);
            }
            (c == kAnchorWindow ? anchor_window : c == kAnchorStep ? anchor_step : c == kAnchorMin ? anchor_min : anchor_mapq) = (int)v;
            continue;
        }
        if (c == kDepthFlank) {
            char* end = nullptr;
            const long v = strtol(optarg, &end, 10);
            if (end == optarg || *end || v < 1 || v > (1L << 30)) {
                fprintf(stderr, "--depth-flank takes an integer from 1 to 2^30, not '%s'.\n", optarg);
                exit(1);
            }
            depth_flank = (int)v;
            continue;
        }
        if (c == kSitesWindow || c == kCiWindow || c == kMapqWindow) {
            char* end = nullptr;
            const long v = strtol(optarg, &end, 10);
            if (end == optarg || *end || v < 0 || v > (1L << 30)) {
                fprintf(stderr, "--%s-window takes an integer from 0 to 2^30, not '%s'.\n", c == kCiWindow ? "ci" : c == kMapqWindow ? "mapq" : "sites", optarg);
                exit(1);
            }
            (c == kCiWindow ? ci_window : c == kMapqWindow ? mapq_window : sites_window) = (int)v;
            continue;
        }
        const Row* row = nullptr;
        for (const Row& r : kRows)
            if (r.letter == c) row = &r;
        if (!row) {
            fprintf(stderr, "Unrecognized option '-%c'.\n", c);
            exit(1);
        }
        switch (row->kind) {
            case kInt: o.*(row->num) = atoi(optarg); break;
            case kFlag: o.*(row->num) = 1; break;
            case kString: this->*(row->str) = optarg; break;
        }
        if (c == 'R') {  // a run from a pass-1 cache takes its options from the cache (ConfigLoader.cpp:19-23)
            if (argc == 3) return;
            // other options beside -R: an error either way.  The same parser goes on over the rest of the line, quietly, only to see
            // whether --estimate is among them: it has a message of its own
            opterr = 0;
            while ((c = getopt_long(argc, argv, spec.c_str(), kLong, nullptr)) >= 0)
                if (c == kEstimate || c == kEstimateConfig) estimate = true;
            if (estimate) estimate_with_cache();
            throw std::runtime_error("When using -R, no other options are allowed");
        }
    }
    if (sites.empty() != sites_vcf.empty() || (sites.empty() && sites_window >= 0)) {
        fprintf(stderr, "--sites FILE and --sites-vcf FILE go together (and --sites-window with them).\n");
        exit(1);
    }
    if ((ci && vcf.empty() && sites_vcf.empty()) || (!ci && ci_window >= 0)) {
        fprintf(stderr, "--ci needs --vcf FILE or --sites-vcf FILE to write to (and --ci-window goes with --ci).\n");
        exit(1);
    }
    if ((depth && vcf.empty() && sites_vcf.empty()) || (!depth && depth_flank >= 0)) {
        fprintf(stderr, "--depth needs --vcf FILE or --sites-vcf FILE to write to (and --depth-flank goes with --depth).\n");
        exit(1);
    }
    if ((mapq && vcf.empty() && sites_vcf.empty()) || (!mapq && mapq_window >= 0)) {
        fprintf(stderr, "--mapq needs --vcf FILE or --sites-vcf FILE to write to (and --mapq-window goes with --mapq).\n");
        exit(1);
    }
    if ((clip && vcf.empty() && sites_vcf.empty()) || (!clip && (clip_window >= 0 || clip_min >= 0 || clip_support >= 0))) {
        fprintf(stderr, "--clip needs --vcf FILE or --sites-vcf FILE to write to (and --clip-window, --clip-min and --clip-support go with --clip).\n");
        exit(1);
    }
    if (mini.empty() && (mini_window >= 0 || mini_step >= 0 || mini_min_pairs >= 0 || mini_score >= 0)) {
        fprintf(stderr, "--mini-window, --mini-step, --mini-min-pairs and --mini-score go with --mini FILE.\n");
        exit(1);
    }
    if (anchor.empty() && (anchor_window >= 0 || anchor_step >= 0 || anchor_min >= 0 || anchor_mapq >= 0)) {
        fprintf(stderr, "--anchor-window, --anchor-step, --anchor-min and --anchor-mapq go with --anchor FILE.\n");
        exit(1);
    }
    if (!estimate && !estimate_config.empty()) {
        fprintf(stderr, "--estimate-config FILE goes with --estimate.\n");
        exit(1);
    }
    if (estimate && !cache_file.empty()) estimate_with_cache();
    o.chr_restricted = chr.empty() ? 0 : 1;
    if (optind == argc) {
        print_usage(o);
        exit(1);
    }
    bam_config_path = argv[optind];
    if (const char* d = getenv("BDX_DEVICE")) device = atoi(d);
}

std::string Options::sv_type(int flag) const {
    if (o.illumina_long_insert) {
        switch (flag) {
            case BDX_ARP_FF: return "INV";
            case BDX_ARP_SMALL_INSERT: return "INS";
            case BDX_ARP_RF: return "DEL";
            case BDX_ARP_RR: return "INV";
            case BDX_ARP_CTX: return "CTX";
            default: return "";
        }
    }
    switch (flag) {
        case BDX_ARP_FF: return "INV";
        case BDX_ARP_LARGE_INSERT: return "DEL";
        case BDX_ARP_SMALL_INSERT: return "INS";
        case BDX_ARP_RF: return "ITX";
        case BDX_ARP_RR: return "INV";
        case BDX_ARP_CTX: return "CTX";
        default: return "";
    }
}

// (the inverse of sv_type by construction: the two cannot drift)
uint32_t Options::sv_flag_mask(const std::string& type) const {
    uint32_t mask = 0;
    for (int f = 0; f < BDX_NUM_FLAGS; ++f)
        if (((BDX_SITE_FLAGS >> f) & 1u) && !type.empty() && sv_type(f) == type) mask |= 1u << f;
    return mask;
}

}  // namespace bdhost
