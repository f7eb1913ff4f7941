// --vcf: the printed calls as VCFv4.2 with per-sample genotypes (GT:GQ:PL:DR:DV).  No counterpart in the reference, whose table
// carries the supporting pairs of a call (DV) but not the normal pairs that cover its breakpoints (DR): those are counted on the GPU
// over the run's resident records (bdx_count_junction_pairs).
// --sites-vcf: the same writer for given sites (sites.h) -- there DV is counted on the GPU as well (bdx_count_site_pairs), a record has
// no score, orientation counts, NREADS or BDAF, and its ID is SITE<k>.
// --ci: either output's records gain CIPOS / CIEND (CIPOS2 where the record prints no END) and CIN from the breakpoint bounds their
// supporting pairs give (bdx_site_breakpoint_bounds).
// --depth: either output's samples gain RCI / RCF / RDR behind DV: the passing read starts inside the record and in its two flanks,
// counted on the GPU (bdx_count_interval_reads), and the ratio of the two densities.
// --mapq: either output's records gain eight Number=2 INFO keys, one entry per printed end: SQN / SQMIN / SQQ1 / SQMED / SQMAX, the number
// and the mapping qualities of the reads that support the end, and LQA / LQN / LQF, the reads around it, the low-quality ones among them and
// their share (bdx_site_end_quality).  All samples pooled; FORMAT and the samples do not change.
#pragma once
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

namespace bdhost {

// Biallelic binomial model, alt-read probability 0.01 / 0.5 / 0.99 for 0/0, 0/1, 1/1:
//   log10 L(g) = dv log10(p_g) + dr log10(1 - p_g);  PL_g = round(-10 (log10 L(g) - max log10 L))  (halves away from zero);
//   GT = the smallest PL (ties: the lower genotype), GQ = min(99, second-smallest PL).  dr < 0 (unknown) or dr + dv == 0: no call.
struct Genotype {
    bool called = false;
    int gt = 0;        // 0 = 0/0, 1 = 0/1, 2 = 1/1
    int gq = 0;
    int64_t pl[3] = {0, 0, 0};
};
Genotype call_genotype(int64_t dr, int64_t dv);

// --ci: the confidence interval around an end printed at P whose supporting pairs bound the breakpoint below by lo and above by hi
// (1-based; lo > hi: the pairs contradict each other), as offsets from P: a = min(lo, hi, P) - P, b = max(lo, hi, P) - P.  So a <= 0 <= b
// always, and a contradictory cluster shows as the span of its contradiction.
struct CiOffsets {
    int64_t a = 0, b = 0;
};
CiOffsets ci_offsets(int64_t lo, int64_t hi, int64_t P);

// --depth: the three intervals of read starts a record with both ends on one sequence is counted over, 0-based and half-open as
// bdx_count_interval_reads takes them.  With lo = min(pos1, pos2), hi = max(pos1, pos2) (1-based, as printed) and flank F the record's
// inside is the starts P = pos + 1 with lo <= P < hi, its flanks lo - F <= P < lo and hi <= P < hi + F; every bound is clamped to
// [1, contig_len + 1] first, so that no interval leaves the sequence (and none is negative when a position lies outside it).
struct DepthSpans {
    int64_t in_beg = 0, in_end = 0, left_beg = 0, left_end = 0, right_beg = 0, right_end = 0;
    int64_t len_in() const { return in_end - in_beg; }
    int64_t len_flank() const { return (left_end - left_beg) + (right_end - right_beg); }
};
DepthSpans depth_spans(int64_t pos1, int64_t pos2, int64_t flank, int64_t contig_len);
// RDR as printed: (rci / len_in) / (rcf / len_flank) with three decimals (printf's rounding of the double rci * len_flank / (len_in * rcf));
// "." when rcf == 0 or either length is 0 (or below), or a count is unknown (< 0)
std::string depth_ratio(int64_t rci, int64_t rcf, int64_t len_in, int64_t len_flank);

// --mapq: what bdx_site_end_quality says about one end of a record; held: the end lies on a chromosome the run read (otherwise every
// entry of the end is '.')
struct EndQuality {
    bool held = false;
    uint32_t n = 0, n_all = 0, n_low = 0;
    unsigned qmin = 0, q1 = 0, median = 0, qmax = 0;
};
// The INFO fragment of --mapq, ";SQN=a,b;SQMIN=a,b;SQQ1=a,b;SQMED=a,b;SQMAX=a,b;LQA=a,b;LQN=a,b;LQF=a,b": e1 / e2 are the ends of the site
// the record was counted as ((tid1, pos1) <= (tid2, pos2)), swapped: the record prints them the other way round, so e2's entry comes first.
// An entry is '.' for an end that is not held (every key), with n == 0 (SQMIN, SQQ1, SQMED, SQMAX; SQN prints 0) and with n_all == 0 (LQF);
// LQF is n_low / n_all with three decimals (printf's rounding of the double quotient).
std::string mapq_info(const EndQuality& e1, const EndQuality& e2, bool swapped);

// --clip: what bdx_site_clip_peaks says about one end of a record; held as in EndQuality; pos: the end's own position P
struct EndClips {
    bool held = false;
    int64_t pos = 0;
    uint32_t n_left = 0, n_right = 0;
    int32_t pos_left = 0, pos_right = 0;
    uint32_t peak_left = 0, peak_right = 0;
};
// The winning pile of an end: the side with the larger peak, then the one nearer to P, then the left one.  side 'L' / 'R'; 0: the end has no
// observation at all.
struct ClipWinner { char side = 0; int32_t pos = 0; uint32_t peak = 0; };
ClipWinner clip_winner(const EndClips& e);
// The INFO fragment of --clip, ";CLN=a,b;CLPOS=a,b;CLSUP=a,b;CLSIDE=a,b": e1 / e2 and swapped as in mapq_info.  CLN is n_left + n_right;
// CLPOS / CLSUP / CLSIDE are the winning pile's X, its reads and L or R, all three '.' when the winner's peak is below `support` (none is
// below any support); every entry is '.' for an end that is not held.
std::string clip_info(const EndClips& e1, const EndClips& e2, bool swapped, uint32_t support);

// one printed row of the table
struct VcfRecord {
    size_t row = 0;                  // 1-based row number among the printed rows (ID = BDX<row>)
    int chr1 = 0, pos1 = 0, chr2 = 0, pos2 = 0;
    std::string ori1, ori2, type;
    int size = 0, score = 0, nreads = 0;
    float af = 0;
    std::vector<int64_t> dr, dv;     // per sample; < 0: unknown ('.')
    bool has_size = true;            // (a site: the table it came from had a numeric Size column; no SVLEN without)
    bool has_ci = false;             // --ci: the record's supporting pairs bound its breakpoints (none do: no CI keys) ...
    uint32_t ci_n = 0;               // ... their number (CIN) ...
    int ci_lo1 = 0, ci_hi1 = 0, ci_lo2 = 0, ci_hi2 = 0;   // ... and the bounds at (chr1, pos1) and at (chr2, pos2), as the record prints its ends
    bool has_depth = false;          // --depth: both ends on one sequence the run read, pos1 != pos2 (otherwise '.' in all three fields) ...
    DepthSpans spans;                // ... what was counted over ...
    std::vector<int64_t> rci, rcf;   // ... and the counts per sample: inside, and in the two flanks together
    bool has_mapq = false;           // --mapq: the record took part (both positions >= 1, a read class maps to its type, an end the run read) ...
    EndQuality mq[2];                // ... the two ends of the site it was counted as, in the site's order ...
    bool mq_swapped = false;         // ... which is the reverse of the record's own
    bool has_clip = false;           // --clip: the record took part (--mapq's conditions) ...
    EndClips cl[2];                  // ... the two ends of the site it was asked as, in the site's order ...
    bool cl_swapped = false;         // ... which is the reverse of the record's own
};

// what makes an output a --sites-vcf one: the records are given sites (ID SITE<row>, QUAL '.', INFO without ORI1 / ORI2 / NREADS / BDAF)
struct VcfSites {
    std::string file;                // --sites, for the ##sites= line
    int32_t window = 0;              // the window the pairs were counted with, for ##sites_window=
};

// what makes an output a --ci one: the ##ci_window= line and the CIPOS / CIEND / CIPOS2 / CIN header lines
struct VcfCi {
    int32_t window = 0;              // the window the supporting pairs were looked for with
};

// what makes an output a --depth one: the ##depth_flank= line, the RCI / RCF / RDR header lines and the three FORMAT fields
struct VcfDepth {
    int32_t flank = 0;               // the width of either flank
};

// what makes an output a --mapq one: the ##mapq_window= line and the eight SQ* / LQ* header lines
struct VcfMapq {
    int32_t window = 0;              // the window the reads were looked for with
};

// what makes an output a --clip one: the ##clip_window= / ##clip_min= / ##clip_support= lines and the four CL* header lines
struct VcfClip {
    int32_t window = 0, min_clip = 0, support = 0;
};

class VcfWriter {
public:
    // opens (truncates) the file at once: an unwritable path fails before any work is done
    explicit VcfWriter(const std::string& path);
    ~VcfWriter();
    VcfWriter(const VcfWriter&) = delete;
    VcfWriter& operator=(const VcfWriter&) = delete;
    // header + records, sorted by (chr1, pos1) with ties in row order; `contigs` are the reference sequences (names are also the
    // records' CHROM / CHR2 values); exclude: the --exclude file of the run ("": none) for the ##exclude= line; sites: non-null for a
    // --sites-vcf output; mark_dup: the run marked duplicates (--mark-dup), for the ##mark_dup=1 line; ci: non-null for a run
    // with --ci, depth: for a run with --depth, mapq: for a run with --mapq; estimate: the run took its
    // libraries from its own pairs (--estimate), for the ##estimate=1 line; clip: non-null for a run with --clip; the file is closed afterwards
    void write(const std::vector<std::string>& argv, const std::vector<std::string>& contigs, const std::vector<uint32_t>& lengths,
               const std::vector<std::string>& samples, std::vector<VcfRecord> records, const std::string& exclude = "",
               const VcfSites* sites = nullptr, bool mark_dup = false, const VcfCi* ci = nullptr,
               const VcfDepth* depth = nullptr, const VcfMapq* mapq = nullptr, bool estimate = false, const VcfClip* clip = nullptr);

private:
    std::string path_;
    FILE* f_ = nullptr;
};

}  // namespace bdhost
