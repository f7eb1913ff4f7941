/* bdx.h -- C ABI of libbdx, the MI355X-native anomalous read-pair clustering path of BreakDancerMax.
 *
 * This is the drop-in boundary: plain pointers and sizes, no C++ or torch types.  The reference has no
 * FFI for this path; what it has are C++ seams, and each entry point below names the one it replaces
 * (file:line under the reference's src/).  A maintainer's binding is shown in INTEGRATION.md.
 *
 * Data contract: the caller (the BAM producer) hands over the *merged, position-sorted* stream of
 * records that survive the reference's reader filter (primary, tid >= 0; io/AlignmentFilter.hpp:24-34,
 * io/BamIo.cpp:11-18), as structure-of-arrays batches.  With "-o <chr>" the stream is the records of
 * that tid only (io/RegionLimitedBamReader.hpp:63-71) and opts.chr_restricted is 1.
 */
#ifndef BDX_H
#define BDX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct bdx_ctx bdx_ctx;

/* status codes (the reference throws C++ exceptions caught in main(), BreakDancerMax.cpp:157-160) */
enum {
    BDX_OK = 0,
    BDX_EINVAL = 1,    /* bad argument */
    BDX_ENOMEM = 2,    /* host or device allocation failed */
    BDX_EHIP = 3,      /* HIP runtime error (no device, launch failure ...) */
    BDX_ESTATE = 4,    /* call out of order (e.g. results before bdx_run) */
    BDX_ELIMIT = 5,    /* input exceeds a documented limit */
    BDX_EINTERNAL = 6
};

/* ReadFlag, common/ReadFlags.hpp:14-27 (values are part of the output contract) */
enum {
    BDX_NA = 0, BDX_ARP_FF = 1, BDX_ARP_LARGE_INSERT = 2, BDX_ARP_SMALL_INSERT = 3, BDX_ARP_RF = 4, BDX_ARP_RR = 5,
    BDX_NORMAL_FR = 6, BDX_NORMAL_RF = 7, BDX_ARP_CTX = 8, BDX_MATE_UNMAPPED = 9, BDX_UNMAPPED = 10, BDX_NUM_FLAGS = 11
};

/* per-read class byte written by the classifier kernel (bdx_get_read_class / bdx_classify):
 *   bits 0-3  ReadFlag after the pass-2 remaps (-l, RR->FF) when the read passes the filters,
 *             the raw classifier flag otherwise
 *   bit 4     read passes the pass-2 filter chain (breakdancer/BreakDancer.cpp:159-167)
 *   bit 5     pass && Alignment::proper_pair() (io/Alignment.hpp:144-148)
 *   bit 6     pass && NORMAL_* && Alignment::leftmost() (counted as a normal read pair, BreakDancer.cpp:202-206) */
#define BDX_CLS_FLAG(c) ((c) & 15)
#define BDX_CLS_PASS 0x10
#define BDX_CLS_PROPER 0x20
#define BDX_CLS_NORMAL_LEFT 0x40

/* Options, common/Options.hpp:24-45 / defaults Options.cpp:27-41 */
typedef struct bdx_opts {
    int32_t min_len;               /* -s */
    int32_t cut_sd;                /* -c (consumed by the config parser) */
    int32_t max_sd;                /* -m */
    int32_t min_map_qual;          /* -q */
    int32_t min_read_pair;         /* -r */
    int32_t seq_coverage_lim;      /* -x */
    int32_t buffer_size;           /* -b */
    int32_t transchr_rearrange;    /* -t */
    int32_t fisher;                /* -f */
    int32_t illumina_long_insert;  /* -l */
    int32_t cn_lib;                /* -a */
    int32_t print_af;              /* -h */
    int32_t score_threshold;       /* -y */
    int32_t chr_restricted;        /* 1 when -o was given (opts.chr non-empty) */
} bdx_opts;

void bdx_opts_default(bdx_opts* o);

/* LibraryConfig, io/LibraryConfig.hpp:11-24; libraries are indexed in sorted-name order
 * (io/BamConfig.cpp:97-101); bam_index indexes the sorted BAM path list (:103-119). */
typedef struct bdx_lib {
    float mean_insertsize, std_insertsize, uppercutoff, lowercutoff, readlens;
    int32_t min_mapping_quality; /* -1: use opts.min_map_qual */
    int32_t bam_index;
} bdx_lib;

/* One batch of records (what io/AlignmentSource.hpp:48-65 + io/Alignment.cpp:45-64 produce per read).
 *   isize     raw BAM isize (the kernels take |isize|)
 *   flag      SAM flag bits
 *   qlen      l_qseq
 *   mapq      "bdqual": AM aux tag if present else MAPQ, as uint8 (io/Alignment.cpp:12-23)
 *   lib       library index resolved from the RG tag (io/BamConfig.hpp:62-72 fallback included)
 *   bam       index of the physical file the record came from (pass-1 counters are per file,
 *             io/BamSummary.cpp:123,135-138)
 *             (an index out of range counts as 0; a context with one library / one file therefore never looks at the
 *             respective array -- it still has to be there)
 *   name_key  64-bit key of the read name; mates share it (ReadRegionData.cpp:109 joins on qname)
 *   name_check a second, independent 64-bit hash of the read name (after bdx_use_name_check; ignored and may be NULL otherwise):
 *             two reads are taken for one name only if key and check both agree, so that two names whose keys collide are
 *             not joined (the reference compares the names themselves, ReadRegionData.cpp:109, SvBuilder.cpp:101-118) */
typedef struct bdx_batch {
    const int32_t *tid, *pos, *mtid, *mpos, *isize;
    const uint16_t *flag, *qlen;
    const uint8_t *mapq, *lib, *bam;
    const uint64_t* name_key;
    size_t n;
    const uint64_t* name_check;
} bdx_batch;

/* Replaces: ConfigLoader + BreakDancer construction (io/ConfigLoader.cpp:18-44, BreakDancer.cpp:87-128).
 * max_read_window_size0 is BamConfig::max_read_window_size() (io/BamConfig.cpp:92-93,121). */
int bdx_create(bdx_ctx** out, const bdx_opts* opts, const bdx_lib* libs, int nlibs, int nbams, int ntids,
               int max_read_window_size0, int device);
void bdx_destroy(bdx_ctx* ctx);
const char* bdx_strerror(int code);
const char* bdx_last_error(const bdx_ctx* ctx);

/* Replaces: AlignmentSource::next feeding BamSummary::_analyze_bam and BreakDancer::push_read
 * (io/AlignmentSource.hpp:48-65: one record stream, consumed as it is produced).  Three ways in:
 *
 *   bdx_acquire_batch / bdx_submit_batch   the streaming producer's path.  acquire hands out the columns of a pinned staging
 *       buffer owned by the context (a ring of four; it blocks only while all four are still being copied), the producer
 *       fills the first n records and submits them: the H2D copies run on the context's copy stream and the classifier
 *       (K1) follows on the tiles the batch completed, so decode, PCIe and pass 1 overlap and host memory stays bounded
 *       by the ring.  The buffer belongs to the context again as soon as bdx_submit_batch returns.
 *   bdx_push             a batch in the caller's own memory.  The copies are asynchronous: every array of the batch must
 *       stay valid and unchanged until the next bdx_run on this context has returned.  Arrays in pinned (page-locked)
 *       memory are copied at PCIe speed; pinned name_key and qlen arrays are not copied at all -- only the anomalous reads
 *       (about 1 %) need them and the compaction kernel fetches those straight from the caller's arrays (25 instead
 *       of 35 bytes per read cross the bus; 23 with one library and one BAM, whose index columns are not copied).
 *   bdx_set_device_reads adopts arrays that already live in HBM (no copy; must stay valid until bdx_destroy or
 *       bdx_reset_reads; every array base 16-byte aligned).
 *
 * bdx_reserve sizes the resident store up front (growing it later re-lays the per-tile tables: the classifier then starts
 * over in bdx_run) and, from 2^20 reads on, the buffers of the later stages for the prior a first run goes by (1/32 of the reads
 * anomalous): a context's ~60 device and pinned allocations then happen here, while the caller still decodes or copies, and not
 * inside its first bdx_run.  bdx_reset_reads empties the store (capacity is kept) so that one context can take the next
 * chromosome.  One context holds at most 2^32 - 1 reads. */
typedef struct bdx_batch_buf {
    int32_t *tid, *pos, *mtid, *mpos, *isize;
    uint16_t *flag, *qlen;
    uint8_t *mapq, *lib, *bam;
    uint64_t* name_key;
    size_t capacity;   /* records the buffer holds (>= the capacity asked for) */
    uint64_t* name_check;   /* read by bdx_submit_batch after bdx_use_name_check(ctx, 1) only */
} bdx_batch_buf;
/* Declares that every batch of this context (pushed, staged, adopted, or decoded by a bdx_bamdec) carries name_check.  Only the
 * anomalous reads' values are ever looked at: the mate join compares them on every key match, across GPUs as well (bdx_dist), and
 * the read-level replay tells names apart by the pair.  To be called while the context holds no reads; default off. */
int bdx_use_name_check(bdx_ctx* ctx, int on);

/* The clip word of a record: no counterpart in the reference, which never looks at a CIGAR beyond bam_calend.  What a record's CIGAR
 * says about clips at its ends and about the reference it covers, the evidence bdx_site_clip_peaks piles up.  The rule, written down
 * here once (one function for every reader: csrc/bdx_clip.h):
 *   INPUT   the CIGAR as n_cigar little-endian words (len << 4 | op; M0 I1 D2 N3 S4 H5 P6 =7 X8), l_seq and the SAM flag.
 *   WORD    left | right << 8 | span << 16.
 *   left    the summed length of the leading run of S / H operations, capped at 255.
 *   right   the summed length of the trailing run of S / H operations, capped at 255 -- counted only if at least one other operation
 *           stands in front of that run: a CIGAR of clips alone has left only, right = 0.
 *   span    the reference bases consumed (M D N = X, as bam_calend), capped at 65535.  When the cap takes effect (more than 65535)
 *           right is 0, because its position is unknown.
 *   ZERO    the word is 0 when n_cigar == 0, when the record is unmapped (flag 0x4), and for htslib's long-CIGAR placeholder (two
 *           operations: S of length l_seq, then N; the real CIGAR is in the CG tag, which is not read).
 * bdx_clip_word is a host function and touches no GPU; cigar may be NULL with n_cigar == 0. */
uint32_t bdx_clip_word(const uint32_t* cigar, uint32_t n_cigar, int32_t l_seq, uint32_t flag);
#define BDX_CLIP_LEFT(w) ((w) & 255u)
#define BDX_CLIP_RIGHT(w) (((w) >> 8) & 255u)
#define BDX_CLIP_SPAN(w) ((w) >> 16)
/* An optional column of the store beside bdx_batch's: one clip word per record, 4 bytes.  bdx_use_clips switches it on or off while the
 * context holds no reads (BDX_ESTATE otherwise); default off, and then nothing is allocated and nothing below may be called
 * (BDX_ESTATE).  With it on the store grows a zero-filled column that growth carries over and bdx_reset_reads empties; a store adopted
 * with bdx_set_device_reads cannot carry one (BDX_ESTATE).  bdx_put_clips copies n host words into rows [first, first + n) of records
 * the context already holds (bdx_push, bdx_acquire_batch / bdx_submit_batch: the batch structs are unchanged, the words come behind
 * them); rows never put stay 0; first + n beyond the records held is BDX_EINVAL.  The words are copied into a pinned buffer of the context's
 * (a ring of four) and go to the device behind the batches' own copies: `clip` may be reused when the call returns, the call does not wait
 * for the copy (only for the one four calls back), and the copy is ordered before any later run or query on the context.
 * bdx_reset_reads zeroes the whole column.  bdx_get_clips reads the first min(cap, records held) words back. */
int bdx_use_clips(bdx_ctx* ctx, int on);
int bdx_put_clips(bdx_ctx* ctx, size_t first, const uint32_t* clip, size_t n);
int bdx_get_clips(bdx_ctx* ctx, uint32_t* out, size_t cap);
int bdx_reserve(bdx_ctx* ctx, size_t n_reads);
int bdx_push(bdx_ctx* ctx, const bdx_batch* host_batch);
int bdx_acquire_batch(bdx_ctx* ctx, size_t capacity, bdx_batch_buf* out);
int bdx_submit_batch(bdx_ctx* ctx, size_t n);
int bdx_set_device_reads(bdx_ctx* ctx, const bdx_batch* device_batch);
int bdx_reset_reads(bdx_ctx* ctx);

/* Replaces: BamSummary::_analyze_bams (io/BamSummary.cpp:129-150), main()'s density/window block
 * (BreakDancerMax.cpp:83-116) and BreakDancer::run (BreakDancer.cpp:131-144) up to the scored SV list. */
int bdx_run(bdx_ctx* ctx);

/* Replaces: a restored BamSummary (io/ConfigLoader.cpp:19-23, the -R cache).  counters = [nlibs*11 flag histogram |
 * nlibs library read counts | nbams file read counts] in bdx_get_counters' layout, e.g. those of an earlier run over the
 * whole genome; the following bdx_run calls derive window, read densities, lambda and the reported statistics from them
 * instead of from their own reads.  NULL switches back to the run's own statistics. */
int bdx_set_pass1_statistics(bdx_ctx* ctx, const uint32_t* counters, uint32_t covered_ref_len);

/* Replaces: the reference run once per chromosome (`-o <chr>`, README:73; one process each) when the caller holds one context per
 * chromosome on one GPU: bdx_run on every context of the list, at most in_flight of them at a time -- one host thread per context
 * in flight, each context on its own streams, so that one context's latency-bound tail (region cut, join, walk) runs beside
 * another's classifier.  The contexts must be distinct; results through each context's getters.  Returns the first error. */
int bdx_run_many(bdx_ctx* const* ctxs, size_t n, int in_flight);

typedef struct bdx_summary {
    uint64_t n_reads;
    uint64_t n_anomalous;        /* reads entering the region accumulator */
    uint32_t covered_ref_len;    /* BamSummary::covered_reference_length() */
    int32_t window;              /* final max_read_window_size (BreakDancerMax.cpp:109-116) */
    uint32_t n_candidates;       /* candidate regions cut by the sliding window */
    uint32_t n_regions;          /* accepted regions (ReadRegionData::add_region calls) */
    uint32_t n_pairs;            /* mate pairs with both reads in accepted regions */
    uint32_t n_groups;           /* distinct region x region connections */
    uint32_t n_svs;              /* SV candidates that reached scoring */
    uint32_t n_svs_printed;      /* ... with score > opts.score_threshold */
} bdx_summary;
int bdx_get_summary(const bdx_ctx* ctx, bdx_summary* out);

/* pass-1 counters: lib_read_count[nlibs], bam_read_count[nbams], flag_hist[nlibs*11] (BamSummary /
 * LibraryFlagDistribution), seqcov[nlibs] (BamSummary.cpp:140-149), density[nlibs] (read density of the
 * library's key, BreakDancerMax.cpp:94-107).  Any pointer may be NULL. */
int bdx_get_counters(const bdx_ctx* ctx, uint32_t* lib_read_count, uint32_t* bam_read_count, uint32_t* flag_hist,
                     float* seqcov, float* density);

/* BasicRegion (breakdancer/BasicRegion.hpp:24-46) as created by add_region */
typedef struct bdx_region {
    int32_t tid, start, end, normal_read_pairs, fwd_read_count, rev_read_count;
    int32_t n_reads;  /* anomalous reads in the region */
    int32_t stored;   /* reads kept for SV building (ReadRegionData.cpp:118-121) */
    int32_t max_qlen; /* BreakDancer::_max_readlen when the region closed */
} bdx_region;
int bdx_get_regions(const bdx_ctx* ctx, bdx_region* out, size_t cap);

/* One SV candidate = one process_sv call that reached the score (BreakDancer.cpp:348-497).
 * pos[] are 1-based as printed.  lib_* / cn_* index the flat lists below. */
typedef struct bdx_sv {
    int32_t chr[2], pos[2], fwd[2], rev[2];
    int32_t flag;       /* dominant ReadFlag (SvBuilder::choose_sv_flag) */
    int32_t size;       /* diffspan */
    int32_t score;      /* PhredQ */
    int32_t num_reads;  /* flag_counts[flag] */
    int32_t printed;    /* score > opts.score_threshold */
    int32_t region[2];  /* region ids; region[1] = -1 for a single-region SV */
    int32_t lib_begin, lib_count; /* (library, pairs) of the dominant flag, ascending library index */
    int32_t cn_begin, cn_count;   /* (key, copy number); key = library index with -a else BAM index */
    float allele_frequency;
    double logp;        /* ComputeProbScore result (BreakDancer.cpp:44-84) */
} bdx_sv;
int bdx_get_svs(const bdx_ctx* ctx, bdx_sv* out, size_t cap);
int bdx_get_sv_lists(const bdx_ctx* ctx, int32_t* lib_index, int32_t* lib_pairs, size_t lib_cap, int32_t* cn_key,
                     float* cn_value, size_t cn_cap);

/* Supporting reads of every SV candidate (SvBuilder::support_reads, SvBuilder.cpp:101-118), for the -g BED and
 * -d FASTQ dumps (BedWriter.cpp:21-56, BreakDancer.cpp:514-534).  Call bdx_set_collect_support(ctx, 1) before
 * bdx_run; afterwards sv_offsets[i]..sv_offsets[i+1] delimit SV i's reads in read_index (index into the pushed
 * stream) / read_flag (the read's ReadFlag after the pass-2 remaps), in the reference's order: per pair the
 * second-observed mate, then its mate; pairs in observation order.  Single-context runs only. */
int bdx_set_collect_support(bdx_ctx* ctx, int on);
int bdx_get_sv_support(const bdx_ctx* ctx, uint32_t* sv_offsets, uint64_t* read_index, uint8_t* read_flag, size_t cap,
                       size_t* n_total);

/* debug / parity: per-read class byte of the last bdx_run (n_reads bytes) */
int bdx_get_read_class(const bdx_ctx* ctx, uint8_t* out, size_t cap);

/* stage timings of the last bdx_run in milliseconds (HIP events on the context's stream):
 * [0] classify kernel (its own begin-to-end time from kernel-level start/stop events, taken on every 4th run, or every run with
 *     stage timing on; the latest measurement), [1] compaction, [2] region cut, [3] mate join + grouping + SV assembly + scores on the device,
 * [4] host: wait for the host's share of the groups, [5] host walk of that share, [6] host: final wait, merge, score
 * combination, [7] whole run; [8]-[10] split [6] into the final wait, the merge of the device's and the host's SV lists,
 * and the score combination.  Returns the number written. */
int bdx_get_timings(const bdx_ctx* ctx, float* ms, int cap);
/* [1]-[3] need HIP events between the stages, which idle the GPU for a few microseconds each: off by default */
int bdx_set_stage_timing(bdx_ctx* ctx, int on);
/* Enqueue-ahead: the stages behind pass 1 are launched before the pass-1 record is back on the host (which would leave
 * the GPU idle for a host round trip), sized by a guess of the number of anomalous reads; if the guess was too small the
 * device skips them and the host runs them again with the true count.
 *   2 (default)  the guess is the previous run's count where this context has just run an input of the same size,
 *                otherwise a prior of 1/32 of the reads (inputs of a million reads or more)
 *   1            always the prior: every bdx_run behaves like a first run of its input (what bench.py times)
 *   0            off: wait for pass 1's exact count of anomalous reads, then size and launch (the count reaches the host
 *                ahead of the rest of the pass-1 record, which the host takes behind the launches) */
int bdx_set_enqueue_ahead(bdx_ctx* ctx, int on);

/* Where the SV candidates of the last bdx_run were assembled.  Components of the region graph that are one region, or
 * two regions of one flush window joined by one connection, are walked on the device (build_connection /
 * process_sv, BreakDancer.cpp:266-497); every other component goes through the host walk.  bdx_set_host_walk(ctx, 1)
 * sends everything through the host walk (same results; used by the parity tests).  Any pointer may be NULL. */
int bdx_set_host_walk(bdx_ctx* ctx, int on);
/* Test switches, by name.  Each forces a route the product takes by itself on some input, so that the tests reach it at any size;
 * every route gives the same results, and none is needed in production.  Value 0 restores the default (big_walk: -1).
 *   "no_stash"       K2 gathers every record from the columns (the route of more counter keys than K1's stash holds)
 *   "max_chunks"     n: the tile scan in at most n chunks (the chunked scan of large inputs)
 *   "spec_test"      enqueue-ahead guesses deliberately short (the rerun when more reads are anomalous than guessed)
 *   "big_walk"       1 / 0: components of 5..64 regions always / never walked on the device (-1: by the host's share)
 *   "bucketed_join"  the partitioned join at every size (the route of more than kDirectJoinMax entries)
 *   "no_poll"        blocking waits instead of polled ready words (the fall-back when a stream write-value command fails)
 *   "ins_plain"      1: the insertion list ranked by the rank-sort launch, 2: by the bitonic fall-back (chosen by the list's length)
 *   "regions_copy"   1: the host copies the region table before its share of the walk (small tables), 2: never (large ones)
 *   "asm_plain"      the walk's candidate assembly merges its parts by the three-way merge (the route of one library, or of many)
 *   "gather_walk"    sharded runs: 1 = rank 0 walks the gathered components on its device, 2 = on its host (by their number otherwise)
 *   "depth_plain"    bdx_count_interval_reads walks every interval record by record, without the chunk table (the route of an interval that holds no whole chunk)
 *   "mini_staged"    bdx_window_insert_shift ranks every window's observations by the all-pairs passes over its LDS slice (the route of a window with more than 64)
 * BDX_EINVAL for any other name. */
int bdx_set_debug(bdx_ctx* ctx, const char* name, int value);
int bdx_get_walk_split(const bdx_ctx* ctx, uint32_t* n_sv_device, uint32_t* n_sv_host, uint32_t* n_groups_host);
/* After a run, once the caller has what it wants: the result tables are copied out of the pinned host buffers the device assembled them
 * in (every getter keeps working, from the copies) and those buffers -- sized for the worst case of a prior, hundreds of MB for a genome --
 * are handed back.  A process pays for pinned memory when it ends (0.15 s per GB on this platform: tools/exit_cost_probe.hip); the CLI calls
 * this on a thread of its own while it prints the table.  The reference's counterpart is the end of BreakDancer::run (BreakDancer.cpp:131-144):
 * nothing is kept.  A later bdx_run allocates them again. */
int bdx_trim_results(bdx_ctx* ctx);
/* Of the device-assembled candidates, those whose traversal started from a region of an earlier flush window (the
 * reference's flush cadence, BreakDancer.cpp:254-264; they are placed in the output by order key, not by position). */
int bdx_get_cross_window_svs(const bdx_ctx* ctx, uint32_t* n_sv_device);
/* 1 if the last bdx_run met a read name more than twice among the anomalous reads (e.g. merged BAMs with clashing read
 * names) and therefore replayed everything behind the region cut one read at a time on the host, with the reference's
 * semantics for such names (ReadRegionData.cpp:108-113,152-175, SvBuilder.cpp:101-118, BreakDancer.cpp:357-368); 0 otherwise. */
int bdx_was_replayed(const bdx_ctx* ctx);

/* The HIP runtime loads a translation unit's device code at the first launch of one of its kernels (0.4-0.8 ms each, inside whatever
 * run comes first in the process).  bdx_warm_up launches one no-op kernel per translation unit of the library and waits: a process
 * that calls it while it still reads its input has its first run at the speed of the later ones.  bdx_dist_prepare calls it. */
int bdx_warm_up(int device);
/* Process-wide test / measurement switches (the library reads no environment variable for a behaviour switch; BDX_*_TRACE / BDX_*_PROF
 * variables only add output).  "pin_malloc" 1: every pinned buffer comes from hipHostMalloc (default: large ones are registered
 * huge pages).  Takes effect for buffers allocated afterwards.  BDX_EINVAL for an unknown name. */
int bdx_set_process_option(const char* name, int value);

/* Kernel-level entry points for parity tests.
 * bdx_classify replaces IAlignmentClassifier::classify (io/IlluminaPEReadClassifier.cpp:59-101) plus the
 * filter/remap half of push_read: host arrays in, class bytes out.
 * bdx_poisson_log_upper_tail replaces log(cdf(complement(poisson(lambda), k))) (BreakDancer.cpp:64-65). */
int bdx_classify(const bdx_opts* opts, const bdx_lib* libs, int nlibs, const bdx_batch* host_batch, uint8_t* cls_out,
                 int device);
int bdx_poisson_log_upper_tail(const double* lambda, const int32_t* k, double* out, size_t n, int device);

/* ---- chromosome-sharded runs on several GPUs: ONE whole-genome result (what a single `breakdancer-max cfg` run prints,
 * -t included) with the chromosomes spread over ranks, one rank per GPU.  Regions never span chromosomes
 * (breakdancer/BreakDancer.cpp:216), so every rank runs classify / compact / region cut / mate join on its own chromosomes;
 * the ranks exchange the global pass-1 statistics and per-chromosome totals (all-reduces of a few KB), the inter-chromosomal
 * (ARP_CTX) join records in ONE all-to-all to owner(name key) -- pairs with both mates on one chromosome never leave their
 * GPU --, and finally gather region tables and pair groups on rank 0, which walks the region graph and holds the result.
 * The collectives run on device buffers over RCCL (xGMI inside a node).
 *
 *   bdx_dist_unique_id       rank 0 obtains the communicator id (ncclGetUniqueId); the caller hands the 128 bytes to every
 *                            rank by whatever means it has (torch.distributed, MPI, a file)
 *   bdx_dist_create          one per process: joins the communicator (ncclCommInitRank) -- collective
 *   bdx_dist_create_threads  the same ranks as threads of ONE process (out[world], one per device in `devices`, which may
 *                            repeat a device); every out[r] is then driven by its own thread.  Collectives are
 *                            device-to-device copies around a barrier
 *   bdx_dist_chromosome      the context that takes chromosome `tid`'s records: ONE context per rank holds all of the rank's
 *                            chromosomes (the same handle for every tid), fed with bdx_push / bdx_acquire_batch as usual -- a rank's
 *                            chromosomes in ASCENDING order, each chromosome's records together --; do NOT call bdx_run on it.
 *                            ntids = number of reference sequences; every chromosome that has reads is fed to exactly one rank
 *   bdx_dist_prepare         optional, after the chromosomes are loaded: sizes the buffers of the later stages for the prior a
 *                            first run goes by (what bdx_reserve does for a single context), outside the run
 *   bdx_dist_run             collective: all ranks call it once their chromosomes are loaded
 *   bdx_dist_result          rank 0 after bdx_dist_run: a context whose getters (bdx_get_summary, bdx_get_counters,
 *                            bdx_get_regions, bdx_get_svs, bdx_get_sv_lists) return the whole-genome result; NULL on other ranks
 *   bdx_dist_owner           the rank that takes the census of a name key (the routing rule of the name census; the inter-chromosomal
 *                            join records travel to the rank that holds the LATER of their two chromosomes)
 *   bdx_dist_plan            chromosomes -> ranks by longest-processing-time packing on `weight` (reads or length)
 * The -g/-d support lists (bdx_dist_set_collect_support), read names that occur more than twice and a negative -s (the read-less region 0
 * of BreakDancer.cpp:244-264, registered once for the genome) are served by the read-level walk: the compact records are gathered and
 * rank 0 walks them read by read. */
typedef struct bdx_dist bdx_dist;
typedef struct bdx_unique_id { char internal[128]; } bdx_unique_id;
int bdx_dist_unique_id(bdx_unique_id* out);
int bdx_dist_create(bdx_dist** out, const bdx_opts* opts, const bdx_lib* libs, int nlibs, int nbams, int ntids,
                    int max_read_window_size0, int device, int rank, int world, const bdx_unique_id* id);
int bdx_dist_create_threads(bdx_dist** out, const bdx_opts* opts, const bdx_lib* libs, int nlibs, int nbams, int ntids,
                            int max_read_window_size0, const int* devices, int world);
void bdx_dist_destroy(bdx_dist* d);
const char* bdx_dist_last_error(const bdx_dist* d);
int bdx_dist_rank(const bdx_dist* d);
int bdx_dist_world(const bdx_dist* d);
bdx_ctx* bdx_dist_chromosome(bdx_dist* d, int tid);
int bdx_dist_prepare(bdx_dist* d);
int bdx_dist_reset_reads(bdx_dist* d);   /* empties the rank's store (capacity kept): the chromosomes are fed again */
int bdx_dist_run(bdx_dist* d);
bdx_ctx* bdx_dist_result(bdx_dist* d);
/* before bdx_dist_run, on every rank alike: the result context also holds the supporting reads of every SV (bdx_get_sv_support on
 * bdx_dist_result; read_index = position in the merged stream of the whole run, chromosomes ascending) -- the input of the
 * reference's -g / -d dumps (BreakDancer.cpp:514-534).  The compact records of all chromosomes are then gathered and rank 0 walks
 * them read by read, as for read names seen more than twice. */
int bdx_dist_set_collect_support(bdx_dist* d, int on);
/* after bdx_dist_run: CTX join records this rank sent / received in the all-to-all, bytes gathered on rank 0, wall time
 * of the whole run and of the exchange + CTX join (ms).  Any pointer may be NULL. */
int bdx_dist_get_exchange(const bdx_dist* d, uint64_t* ctx_records_sent, uint64_t* ctx_records_received, uint64_t* gathered_bytes,
                          float* ms_total, float* ms_exchange);
/* collectives this rank entered in the last bdx_dist_run: out[0] all-reduces, out[1] all-to-alls, out[2] gathers; the library that
 * carried them ("threads" for the in-process backend, else the path of the librccl that was loaded) and its ncclGetVersion code (0: none) */
int bdx_dist_get_collectives(const bdx_dist* d, uint32_t out[3], const char** backend, int* rccl_version);
/* bdx_set_debug for this rank's contexts -- its own and, on rank 0, the result context ("gather_walk": 1 = rank 0 walks the gathered
 * components on its device whatever their number, 2 = on its host; 0 = by their number).  Routes to the same results; tests force each */
int bdx_dist_set_debug(bdx_dist* d, const char* name, int value);
/* this rank's milliseconds of the last bdx_dist_run, phase by phase: local phases and the collectives behind them alternate
 * (bdx_dist_phase_name(i) names entry i; a collective's figure includes waiting for the slowest rank), then what only rank 0 does:
 * the merge of the ranks' tables, its walk of the gathered components on the device (K6 on the result context) and what of it its host takes. */
int bdx_dist_get_phase_ms(const bdx_dist* d, float* out, int n);
const char* bdx_dist_phase_name(int i);
int bdx_dist_owner(uint64_t name_key, int world);
int bdx_dist_plan(const uint64_t* weight, int ntids, int world, int* rank_of_tid);

/* ---- BAM decode on the device: BGZF inflate + record fields in HBM ----
 * Replaces, for one BAM file, what the host producer does per byte and per record: bgzf inflate (samtools bgzf.c behind
 * io/BamReader.hpp:62-70), bam_read1, Alignment's constructor (io/Alignment.cpp:12-29,45-64: core fields, bdqual from the AM tag,
 * RG), the RG -> library lookup with its fallback (io/BamConfig.hpp:62-72, io/AlignmentSource.hpp:57-62) and the reader filter
 * (primary, placed: io/AlignmentFilter.hpp:24-34, io/BamIo.cpp:11-18; -o region: io/RegionLimitedBamReader.hpp:63-71).  The caller
 * reads the file, finds the BGZF members (18-byte headers, 8-byte footers) and hands the bytes over as they are, in pieces of whole
 * members; everything else happens on the GPU, and the file crosses PCIe compressed.
 * Integrity: the inflate kernel rejects what zlib rejects (invalid codes, distances before the window, a member that does not end
 * at its ISIZE) and the record stage rejects chains that do not add up; the members' CRC-32 words are NOT checked on the device --
 * the host reader (host/column_reader.cpp, BDX_DECODE=host) checks every member's, as htslib does.
 *
 *   bdx_bamdec_create    sink != NULL: the decoded records are appended to that context's resident store (one file: the stream
 *                        IS the file's record order) and the classifier follows them; bdx_run afterwards as usual.  sink == NULL:
 *                        the decoder keeps the columns in HBM and bdx_bamdec_fetch copies them out (tests; callers that merge
 *                        several files themselves).  first_record_offset: offset of the first record in the inflated stream,
 *                        counted from the first member that will be submitted (the caller has parsed the BAM header).
 *   bdx_bamdec_acquire   a pinned staging buffer for `bytes` of file and a table of max_blocks members, both owned by the decoder
 *                        (a ring of six; blocks only while the next one's copy is in flight).  A caller may acquire several before it
 *                        submits -- reading the file ahead of the piece it is cutting into members -- up to all six; bdx_bamdec_submit
 *                        takes them in the order they were acquired, bdx_bamdec_finish drops what was acquired and never submitted
 *   bdx_bamdec_submit    the first `bytes` of the buffer are whole members, described by the first nblocks table entries
 *                        (offset = start of the member's deflate payload in the buffer); last != 0 with the file's final piece.
 *                        Asynchronous: the copy is enqueued at once; inflate and record kernels run per BATCH of pieces (one member is
 *                        one wavefront, so a launch wants thousands of them), the record kernels one batch behind
 *   bdx_bamdec_progress  non-blocking: records appended so far, records seen, whether a record behind the -o region was met
 *                        (a caller that seeked through the index may stop there), device-side error code
 *   bdx_bamdec_finish    waits for everything; errors of the decode (corrupt block, corrupt or truncated record chain, a record
 *                        beyond the device path's 4 MiB) surface here.  Without a `last` piece it ends the stream where it is
 *   bdx_inflate_blocks   kernel-level entry point for parity tests: members inflated by the GPU, host buffers in and out;
 *                        status[i] != 0: member i was rejected (the caller lets zlib judge it) */
typedef struct bdx_bamdec bdx_bamdec;
typedef struct bdx_bgzf_block {
    uint64_t offset;        /* of the member's deflate payload within the submitted bytes */
    uint32_t payload_len;   /* BSIZE + 1 - XLEN - 20 */
    uint32_t inflated_len;  /* ISIZE, at most 65536 */
} bdx_bgzf_block;
typedef struct bdx_bamdec_params {
    int32_t device;               /* used when there is no sink */
    int32_t n_targets;            /* reference sequences of the file's header */
    int32_t bam_index;            /* index of the file among the configuration's BAMs (the records' `bam` column) */
    int32_t only_tid, region_beg, region_end;  /* -o region; only_tid < 0: every placed record */
    uint32_t n_read_groups;       /* read-group ids of the configuration and their library indices */
    const char* const* rg_ids;
    const uint8_t* rg_lib;
    uint8_t fallback_lib;         /* library of records without (or with an unknown) read group */
    uint64_t first_record_offset;
    size_t ring_bytes;            /* inflated bytes kept in flight (at least four batches' worth), 0: 3 GiB */
    size_t batch_bytes;           /* compressed bytes and members after which the pieces gathered so far are launched as one batch */
    size_t batch_blocks;          /* (0: 256 MiB / 8192 members -- more members than the GPU has wave slots for the inflate kernel) */
    size_t expected_bytes;        /* compressed bytes the caller is going to submit (the file's size), 0: unknown.  With a sink whose
                                     store is still empty the decoder sizes the store from it, and once the first batch has shown how
                                     many records the bytes hold, the buffers of the stages behind pass 1 (what bdx_reserve does up
                                     front) -- while the GPU inflates, not in front of it */
    size_t piece_bytes, piece_blocks;  /* the sizes bdx_bamdec_acquire will be called with, 0: unknown.  Known: the staging buffers are
                                     pinned by threads of their own while the caller reads its first piece (pinning costs ~0.2 ms per
                                     MiB, and the first pieces would otherwise wait for it one after the other) */
    int32_t batch_rounds;         /* rounds of the GPU's wave slots an inflate launch takes (7,680 members each), 1..16; 0: from expected_bytes
                                     (one round per 2.5 GB, at most four).  Ignored when batch_blocks is given */
    int32_t record_mode;          /* bits: 1 = no reader filter (secondary / supplementary / unplaced records are kept too), 2 = the quality column is
                                     MAPQ whether or not a record carries an AM tag.  0 for breakdancer-max's reader; bam2cfg sets them.
                                     4 = a decoder WITHOUT a sink keeps the records' clip words (bdx_clip_word) beside its columns, for a
                                     gather target with bdx_use_clips on (bdx_merge_decoded / bdx_append_decoded refuse a decoder without
                                     them then: BDX_EINVAL); with a sink the sink's own switch decides and the bit is ignored */
    int32_t missing_lib_plus1;    /* library of records WITHOUT a read-group tag, plus one; 0: fallback_lib, like an unknown read group */
    int32_t time_kernels;         /* != 0: a HIP event pair around every inflate launch; bdx_bamdec_host_ms [12] = their sum in ms, [13] = launches
                                     (a measurement: each pair idles the GPU for a few microseconds) */
} bdx_bamdec_params;
int bdx_bamdec_create(bdx_bamdec** out, bdx_ctx* sink, const bdx_bamdec_params* p);
/* the clip words of records [first, first + n) of a finished decoder that keeps its own columns and clip words (for tests) */
int bdx_bamdec_fetch_clips(bdx_bamdec* d, uint64_t first, uint64_t n, uint32_t* out);
void bdx_bamdec_destroy(bdx_bamdec* d);
const char* bdx_bamdec_last_error(const bdx_bamdec* d);
int bdx_bamdec_acquire(bdx_bamdec* d, size_t bytes, size_t max_blocks, void** buf, bdx_bgzf_block** blocks);
int bdx_bamdec_submit(bdx_bamdec* d, size_t bytes, size_t nblocks, int last);
int bdx_bamdec_progress(bdx_bamdec* d, uint64_t* n_records, uint64_t* n_raw, int* past_region, uint32_t* error);
int bdx_bamdec_finish(bdx_bamdec* d, uint64_t* n_records);
/* a finished decoder takes another stretch of the same file (another sequence's range, found through the index): buffers, streams and
 * events are kept, the region filter and the record chain start over; with a sink the records go behind what its store holds */
int bdx_bamdec_rearm(bdx_bamdec* d, int32_t only_tid, int32_t region_beg, int32_t region_end, uint64_t first_record_offset, size_t expected_bytes);
int bdx_bamdec_fetch(bdx_bamdec* d, uint64_t first, uint64_t n, const bdx_batch_buf* out);
int bdx_bamdec_stats(const bdx_bamdec* d, uint64_t* compressed_bytes, uint64_t* inflated_bytes, uint64_t* pieces, uint64_t* blocks_walked_twice);
/* Several BAMs decoded on the GPU, each by a decoder of its own (no sink: the records stay in the decoder's columns, bdx_bamdec_fetch
 * returns the columns the caller gives room for -- tid, pos and flag are what BamMerger's order looks at, io/BamMerger.cpp:40-61).  The
 * caller works out the merged order and hands it over as a permutation: record i of the context's store = record src_index[i] of
 * decoder src_file[i].  The gather runs in HBM; the context must hold no reads yet and then stands as after bdx_push of the merged stream. */
int bdx_merge_decoded(bdx_ctx* ctx, bdx_bamdec* const* decs, int k, const uint8_t* src_file, const uint32_t* src_index, uint64_t n);
/* The same gather BEHIND what the context's store holds (a rank of a sharded run takes its chromosomes one after the other: every chromosome
 * of a several-BAM configuration is decoded per file through the files' indexes, io/RegionLimitedBamReader.hpp:43-71, and merged in
 * BamMerger's order, io/BamMerger.cpp:40-126).  The store keeps its records; it must not hold batches whose name keys are still the caller's. */
int bdx_append_decoded(bdx_ctx* ctx, bdx_bamdec* const* decs, int k, const uint8_t* src_file, const uint32_t* src_index, uint64_t n);
/* milliseconds the feeding thread spent inside the decoder so far, by cause: [0] waiting for a staging buffer's copy, [1] pinning
 * staging memory, [2] waiting for a batch slot, [3] sizing a slot's buffers, [4] the pieces' copy calls, [5] launching batches
 * (includes [6]), [6] launching record stages, [7] feeding the classifier; and two marks, ms after the decoder's creation (or its last
 * bdx_bamdec_rearm): [8] the first inflate launch, [9] bdx_bamdec_finish's return; [10] / [11] of [7]: sizing the later stages' buffers,
 * classifier launches; [12] / [13] the inflate kernel's own milliseconds by HIP events and its launches (bdx_bamdec_params::time_kernels) */
int bdx_bamdec_host_ms(const bdx_bamdec* d, float* out, int n);
int bdx_inflate_blocks(int device, const void* compressed, size_t bytes, const bdx_bgzf_block* blocks, size_t nblocks, void* out,
                       size_t out_bytes, uint32_t* status, float* kernel_ms);

/* --exclude: a region mask inside the decoder's reader filter.  No counterpart in the reference (its -x drops a REGION after its reads
 * have been counted).  The mask is a set of half-open, 0-based intervals [beg, end) per reference sequence (BED coordinates).  A record
 * that passed the reader filter (primary, placed, the -o region) is dropped when tid >= 0 and pos lies in an interval of tid, or
 * mtid >= 0 and mpos lies in an interval of mtid: only the start coordinates the record itself carries, so both mates of a consistent
 * pair go together.  A dropped record does not exist for anything downstream; n_records of bdx_bamdec_progress / bdx_bamdec_finish keeps
 * meaning kept records.  A tid / mtid beyond the mask's sequences, or with no interval, is never dropped.
 *   bdx_bamdec_set_exclude  before the decoder's first submit; intervals in any order, they may overlap or touch (they are sorted and
 *                           merged, touching ones too; beg == end is empty and ignored); the table is uploaded once and kept across
 *                           bdx_bamdec_rearm; n == 0 removes the mask.  BDX_EINVAL: a null array with n > 0, tid < 0, beg < 0 or
 *                           end < beg; BDX_ESTATE: after the first submit; BDX_ELIMIT: more than 2^24 merged intervals (a 128 MiB
 *                           table) or a tid of 2^24 and beyond
 *   bdx_bamdec_excluded     after bdx_bamdec_finish: records the mask dropped since the decoder's creation or its last bdx_bamdec_rearm
 *   bdx_exclude_mask        kernel-level entry point for parity tests, and for callers of bdx_push / bdx_set_device_reads that filter
 *                           their own columns: host arrays in, mask[i] = 1 where the rule drops record i; same argument errors */
typedef struct bdx_interval { int32_t tid, beg, end; } bdx_interval;   /* 0-based, half-open */
int bdx_bamdec_set_exclude(bdx_bamdec* d, const bdx_interval* iv, size_t n);
int bdx_bamdec_excluded(const bdx_bamdec* d, uint64_t* n);
int bdx_exclude_mask(int device, const int32_t* tid, const int32_t* pos, const int32_t* mtid, const int32_t* mpos, size_t n,
                     const bdx_interval* iv, size_t niv, uint8_t* mask);

/* bam2cfg's insert-size statistics of nlibs libraries on the GPU (perl/bam2cfg.pl:153-197; `bam2cfg --device`): library i's observations
 * are x[offsets[i] .. offsets[i + 1]).  mean_all / sd_all over all of them (n - 1); mean / sd over the n_kept that are not more than five
 * standard deviations above mean_all; sd_minus / sd_plus the one-sided deviations around mean (n_minus observations <= mean, n_plus above,
 * each with n - 1).  Summed in the script's order with round-to-nearest operations: the figures equal the CPU tool's bit for bit. */
typedef struct bdx_insert_stats {
    double mean_all, sd_all, mean, sd, sd_minus, sd_plus;
    uint64_t n_kept, n_minus, n_plus;
} bdx_insert_stats;
int bdx_insert_size_stats(int device, const double* x, const uint32_t* offsets, int nlibs, bdx_insert_stats* out);

/* Reference-supporting read pairs at SV junctions: no counterpart in the reference (the input of --vcf's DR / GT).
 * Query i: chromosome tid[i], junctions pos_a[i] <= pos_b[i] (1-based; pos_a == pos_b: one junction).
 * counts[i * nkeys + k]: pairs of key k (library with by_library, else BAM file; nkeys = nlibs / nbams) that the last run counted as
 * normal pairs (BDX_CLS_NORMAL_LEFT, each pair once by its leftmost mate) whose fragment [pos+1, pos+|isize|] covers base p and p+1
 * of at least one junction p of the query.  After bdx_run, or on a rank's context (bdx_dist_chromosome) after bdx_dist_run: that
 * rank's chromosomes.  A chromosome the context holds no reads of counts 0.
 * BDX_ESTATE before a run has classified the reads the context holds (or while a sizing pass is in flight); BDX_EINVAL for a null
 * array with n > 0, tid < 0, pos_a < 1 or pos_a > pos_b.  Not beside another call on the same context (bdx_trim_results included). */
int bdx_count_junction_pairs(bdx_ctx* ctx, const int32_t* tid, const int32_t* pos_a, const int32_t* pos_b, size_t n,
                             int by_library, uint32_t* counts);

/* Alternate-supporting read pairs at GIVEN SV sites: no counterpart in the reference (the DV / GT input of --sites; the run's own calls
 * get their supporting pairs from the region walk).  The rule, written down here once:
 *   A site is (tid1, pos1, tid2, pos2, flag_mask): positions 1-based as the table prints them, (tid1, pos1) <= (tid2, pos2)
 *   lexicographically; bit f of flag_mask is set when ReadFlag f supports the site's type -- only the anomalous classes BDX_ARP_FF,
 *   BDX_ARP_LARGE_INSERT, BDX_ARP_SMALL_INSERT, BDX_ARP_RF, BDX_ARP_RR, BDX_ARP_CTX (BDX_SITE_FLAGS), at least one.
 *   A record is NEAR P on T when tid == T and |pos + 1 - P| <= window; its mate when mtid == T and |mpos + 1 - P| <= window (64-bit
 *   arithmetic).  Record i of the resident store counts for a site when
 *     1. cls[i] & BDX_CLS_PASS and bit BDX_CLS_FLAG(cls[i]) of flag_mask is set (the flag after the pass-2 remaps -l and RR->FF, as the
 *        walk sees it);
 *     2. it is its pair's lower mate, so that each pair counts once: (tid, pos) < (mtid, mpos) lexicographically, or the two are equal
 *        and SAM flag bit 0x40 (first in pair) is set;
 *     3. forward: it is near pos1 on tid1 and its mate near pos2 on tid2; or reverse: it is near pos2 on tid2 and its mate near pos1 on
 *        tid1 (possible only when the windows overlap: tid1 == tid2 and pos2 - pos1 <= 2 window).  A record matching both ways counts once.
 *   Only what the record itself carries is looked at (as in --exclude's rule): not the mate's own record, its quality, or whether it
 *   survived a filter.  The count is therefore NOT the walk's num_Reads, which also wants both mates inside accepted regions.
 * counts[i * nkeys + k]: the records of key k (library with by_library, else BAM file; nkeys = nlibs / nbams; a key index out of range
 * counts as 0) that count for site i.  After bdx_run, or on a rank's context (bdx_dist_chromosome) after bdx_dist_run: that rank's
 * chromosomes -- a pair's lower mate lives on tid1.  A chromosome the context holds no reads of, or beyond the header, counts 0.
 * BDX_ESTATE before a run has classified the reads the context holds (or while a sizing pass is in flight); n == 0 is BDX_OK even with
 * null pointers; BDX_EINVAL for a null array with n > 0, tid1 < 0 or tid2 < 0, pos1 < 1 or pos2 < 1, a site that is not normalised,
 * flag_mask 0 or with a bit outside BDX_SITE_FLAGS, window < 0 or window > 2^30; BDX_ELIMIT above 2^31 sites.  Not beside another call
 * on the same context (bdx_trim_results included). */
#define BDX_SITE_FLAGS ((1u << BDX_ARP_FF) | (1u << BDX_ARP_LARGE_INSERT) | (1u << BDX_ARP_SMALL_INSERT) | (1u << BDX_ARP_RF) | (1u << BDX_ARP_RR) | (1u << BDX_ARP_CTX))
typedef struct bdx_site { int32_t tid1, pos1, tid2, pos2; uint32_t flag_mask; } bdx_site;
int bdx_count_site_pairs(bdx_ctx* ctx, const bdx_site* sites, size_t n, int32_t window, int by_library, uint32_t* counts); /* [n][nkeys] */

/* Breakpoint intervals of GIVEN SV sites from their supporting pairs: no counterpart in the reference (CIPOS / CIEND of the CLI's --ci).
 * A read of a supporting pair lies wholly on one side of the breakpoint its fragment crosses, and the fragment reaches no further than
 * its library's uppercutoff from the read's start; intersecting those one-read intervals over a site's supporting pairs is the classical
 * paired-end breakpoint interval.  The rule, written down here once:
 *   WHICH RECORDS   sites, window, the context's state and every argument error are those of bdx_count_site_pairs, checked in the same
 *                   order.  The records that count for site i are exactly the records bdx_count_site_pairs counts for it, all keys pooled;
 *                   out[i].n is their number (the row sum of bdx_count_site_pairs for either key choice).
 *   OBSERVATIONS    a counting record gives one observation (x, reverse, U) to each end of the site.  By the forward route (it is near pos1,
 *                   its mate near pos2): end 1 gets (pos, flag & 0x10, U), end 2 gets (mpos, flag & 0x20, U).  By the reverse route only:
 *                   end 1 gets (mpos, flag & 0x20, U), end 2 gets (pos, flag & 0x10, U).  A record that matches both routes is taken by
 *                   the forward route, once.  U belongs to the record's library (lib; an index out of range is library 0): ceil(uppercutoff),
 *                   0 when that is negative, 2^30 when the cutoff is NaN, infinite or above 2^30.  With opts.illumina_long_insert (-l) reads
 *                   point away from their fragment: `reverse` is inverted.
 *   INTERVALS       with P = x + 1 (64-bit arithmetic) a forward read bounds the breakpoint to [P, P + U], a reverse read to [P - U, P].
 *   BOUNDS          lo_e is the maximum of the lower bounds of end e's observations, hi_e the minimum of their upper bounds; both are
 *                   clamped to [1, 2^31 - 1] at the end.  With n == 0 all four are 0.  lo_e > hi_e is a legitimate result -- the pairs
 *                   contradict each other, as when an aligner lets a read overhang the junction -- and is reported as it is.
 * Only what the record itself carries is looked at (as in the other rules): qlen is not used -- it is not resident for pinned pushes and
 * the mate's is unknown anyway -- which loosens each bound by at most one read length.
 * After bdx_run, or on a rank's context (bdx_dist_chromosome) after bdx_dist_run: that rank's chromosomes -- a site is answered by the
 * rank that holds tid1.  A chromosome the context holds no reads of, or beyond the header, gives n == 0.  Not beside another call on the
 * same context (bdx_trim_results included). */
typedef struct bdx_site_bounds { uint32_t n; int32_t lo1, hi1, lo2, hi2; } bdx_site_bounds;   /* 20 bytes */
int bdx_site_breakpoint_bounds(bdx_ctx* ctx, const bdx_site* sites, size_t n, int32_t window, bdx_site_bounds* out);

/* Mapping quality at ONE END of given SV sites: no counterpart in the reference (the SQ* / LQ* keys of the CLI's --mapq).  How good are the
 * reads that support the end, and how large a share of the reads around it did -q turn away -- the classic sign of a repeat.  The rule,
 * written down here once:
 *   A QUERY    is (site, end): site a bdx_site exactly as bdx_count_site_pairs takes it (1-based, normalised, flag_mask), end 1 or 2.
 *              (T, P) is the asked end -- (tid1, pos1) for end 1, (tid2, pos2) for end 2 --, (T', P') the other one.  NEAR is that of
 *              bdx_count_site_pairs: 64-bit arithmetic, window 0 to 2^30.
 *   SUPPORT    record i supports the end when cls[i] & BDX_CLS_PASS, bit BDX_CLS_FLAG(cls[i]) of flag_mask is set, it is near P on T and
 *              its mate (mtid, mpos) is near P' on T'.  There is NO lower-mate condition: both mates of a pair are records and each
 *              counts at its own end, which is what brings the upper mate's quality in.  When the two windows overlap one record may
 *              support both ends; that is the rule, not an accident.  Only what the record itself carries is looked at.
 *   AROUND     record i is around the end when tid == T, |pos + 1 - P| <= window and SAM flag 0x4 is clear.  It is LOW when its quality
 *              (the mapq column: the AM tag if present, else MAPQ) is <= its library's minimum mapping quality, resolved as K1 resolves
 *              it: bdx_lib.min_mapping_quality, or opts.min_map_qual when that is negative; a library index out of range is library 0.
 *              The comparison is made in int, so a minimum below 0 or above 255 behaves as in K1 (which lets quality > minimum pass).
 *   RESULT     n: the supporters; n_all: the records around, supporters or not; n_low: the low ones among them.  Over the supporters'
 *              qualities: qmin and qmax the extremes, median the smallest q with #(quality <= q) >= ceil(n / 2) (the lower median),
 *              q1 the smallest q with #(quality <= q) >= ceil(n / 4); the ranks in 64-bit.  With n == 0 the four bytes are 0.
 * State, errors and their order are those of bdx_count_site_pairs; besides BDX_EINVAL for a null `end` with n > 0 and, behind the sites'
 * own checks, for an end[i] outside {1, 2}; BDX_ELIMIT above 2^31 queries.  After bdx_run, or on a rank's context (bdx_dist_chromosome)
 * after bdx_dist_run: a query is answered by the rank that holds T, since every record that can count for it has tid == T (the routing of
 * bdx_count_interval_reads, not that of bdx_count_site_pairs).  A chromosome the context holds no reads of, or beyond the header, gives
 * all zeros.  Not beside another call on the same context (bdx_trim_results included). */
typedef struct bdx_site_quality { uint32_t n, n_all, n_low; uint8_t qmin, q1, median, qmax; } bdx_site_quality;   /* 16 bytes */
int bdx_site_end_quality(bdx_ctx* ctx, const bdx_site* sites, const uint8_t* end, size_t n, int32_t window, bdx_site_quality* out);

/* Where the clipped reads pile up around ONE END of given SV sites: no counterpart in the reference, whose calls are all imprecise.  A read
 * that crosses a junction is aligned up to it and clipped behind it, so the clips of one breakpoint stand on one base.  The rule, written
 * down here once (KP, csrc/kp_clip.hip):
 *   A QUERY       is (site, end) as bdx_site_end_quality takes it; (T, P) is the asked end.  The site's flag_mask is checked like there
 *                 but NOT used: a clipped read says where a junction is whatever its pair looks like.
 *   OBSERVATIONS  record i with clip word w (bdx_clip_word) gives up to two:
 *                   a LEFT one at  X = pos + 1     when BDX_CLIP_LEFT(w) >= min_clip  (its first aligned base: the junction lies
 *                                                  between X - 1 and X);
 *                   a RIGHT one at X = pos + span  when BDX_CLIP_RIGHT(w) >= min_clip and 1 <= span <= BDX_CLIP_SPAN_MAX (its last
 *                                                  aligned base: the junction lies between X and X + 1).
 *                 pos is the 0-based column, X 1-based, the arithmetic 64-bit; an X outside [1, 2^31 - 1] is no position and gives no
 *                 observation.
 *   COUNTS        an observation counts when cls[i] & BDX_CLS_PASS (so -q, 0x400 and bdx_set_mark_duplicates' marks are honoured),
 *                 tid[i] == T and |X - P| <= window.
 *   RESULT        per side: n the observations that count, pos the X that most of them share and peak that number.  Ties go to the
 *                 smaller |X - P|, then to the smaller X.  With n == 0, pos and peak are 0.  All integers: the result is exact.
 * window in [0, BDX_CLIP_WINDOW_MAX] and min_clip in [1, 255], else BDX_EINVAL.  BDX_ESTATE without bdx_use_clips, and before a run has
 * classified the reads the context holds; otherwise state, errors and their order are those of bdx_site_end_quality.  A query is
 * answered by the context that holds T; a chromosome it holds no reads of gives all zeros.  Not beside another call on the same context. */
#define BDX_CLIP_SPAN_MAX 4096     /* a right clip further than this behind its read's start is not looked for (published for the tests) */
#define BDX_CLIP_WINDOW_MAX 1023
typedef struct bdx_clip_peaks { uint32_t n_left, n_right; int32_t pos_left, pos_right; uint32_t peak_left, peak_right; } bdx_clip_peaks;   /* 24 bytes */
int bdx_site_clip_peaks(bdx_ctx* ctx, const bdx_site* sites, const uint8_t* end, size_t n, int32_t window, int32_t min_clip, bdx_clip_peaks* out);

/* Passing read starts inside given intervals: no counterpart in the reference, which says nothing about read depth (the input of --depth's
 * RCI / RCF / RDR).  The rule, written down here once:
 *   Record i of the resident store counts for interval (tid, [beg, end)) -- 0-based, half-open, as in --exclude's mask -- when
 *   tid[i] == tid, beg <= pos[i] < end and cls[i] & BDX_CLS_PASS: the records K1 let pass the pass-2 filter chain, the reads the caller
 *   itself works with (paired, both ends mapped, not a duplicate -- SAM flag 0x400, bdx_set_mark_duplicates' marks included --, mapping
 *   quality above the library's minimum, |isize| <= -m or CTX), normal and anomalous alike.
 * Only what the record itself carries is looked at (as in the other rules): qlen is not used -- it is not resident for pinned pushes -- and
 * no CIGAR.  The count is a density of READ STARTS, NOT a per-base pileup of the kind samtools depth or mosdepth give: a read that starts
 * in front of beg and reaches into the interval does not count, one that starts inside and reaches out of it does.
 * counts[i * nkeys + k]: the records of key k (library with by_library, else BAM file; nkeys = nlibs / nbams; a key index out of range
 * counts as 0; a context with one key never reads the key column) that count for interval i.  beg == end counts 0; a tid the context
 * holds no reads of, or beyond the header, counts 0.  After bdx_run, or on a rank's context (bdx_dist_chromosome) after bdx_dist_run: that
 * rank's chromosomes.  With opts.transchr_rearrange (-t) no same-chromosome read passes; the call is legal and says so.
 * The cost per interval does not grow with the interval: every call first counts the passing records per chunk of BDX_DEPTH_CHUNK
 * consecutive records and key (KR, csrc/kr_depth.hip; about a byte per record and key column), and an interval takes its whole chunks from
 * that table and walks only its two edges.  Nothing is kept between calls.
 * BDX_ESTATE before a run has classified the reads the context holds (or while a sizing pass is in flight); n == 0 is BDX_OK even with
 * null pointers; BDX_EINVAL for a null array with n > 0, tid < 0, beg < 0 or end < beg; BDX_ELIMIT above 2^31 intervals.  Not beside
 * another call on the same context (bdx_trim_results included). */
#define BDX_DEPTH_CHUNK 2048   /* an implementation constant, published for the tests (they place intervals on and around chunk boundaries) */
int bdx_count_interval_reads(bdx_ctx* ctx, const bdx_interval* iv, size_t n, int by_library, uint32_t* counts); /* [n][nkeys] */

/* Duplicate marking: no counterpart in the reference, which only ignores reads that already carry SAM flag 0x400
 * (io/IlluminaPEReadClassifier.cpp:66-74; K1 restates that).  The rule, written down here once:
 *   RUNS        the store is cut into runs: maximal stretches of consecutive records with equal (tid, pos).  For coordinate-sorted input a
 *               run is all records that start at one position; the rule is defined for any input this way (no sortedness is asked for).
 *   CANDIDATES  a record with flag & 0x1, none of 0x4, 0x8, 0x100, 0x400, 0x800, tid >= 0 and mtid >= 0.  A record that already carries
 *               0x400 stays as it is and competes with nobody.
 *   KEY         K = (lib, tid, pos, flag & 0x10, mtid, mpos, flag & 0x20, flag & 0x40): the library, not the file (one library spread over
 *               two BAMs is one library); the first-in-pair bit keeps the two mates of a pair that start at one place with one strand apart.
 *   GROUPS      the candidates of one run with equal K.  In a group of two or more the record with the smallest (name_key, store index)
 *               survives and every other record gets 0x400.  Groups of one, and non-candidates, are untouched.
 * Only what the record itself carries is looked at (as in --exclude's and --sites' rules): not CIGAR or unclipped ends, base qualities, or
 * the mate's own record -- position-and-strand marking in the manner of samtools rmdup.  Both mates of a pair carry one name_key and the
 * group seen from the mate's end mirrors the group seen from this end (mates in the store and consistent), so both ends keep the same pair.
 * Two different pairs whose name keys collide inside one group fall to the index and may keep different pairs at the two ends.
 *   bdx_set_mark_duplicates  while the context holds no reads (BDX_ESTATE otherwise); default off.  With it on, pass 1 does not start
 *                            behind arriving batches: the marking kernel (KD, csrc/kd_markdup.hip) runs over the whole store at the head
 *                            of pass 1, once per load -- a repeated bdx_run gives the same table and counts --, and everything downstream
 *                            sees the marked flag column.  The marks are defined per load: once a run has marked it, bdx_push,
 *                            bdx_submit_batch, a decoder and bdx_append_decoded refuse to append (BDX_ESTATE) until bdx_reset_reads.  Reads adopted with bdx_set_device_reads stay unchanged: the context marks a
 *                            private copy of their flag column (2 B per read)
 *   bdx_get_duplicates       after a run (BDX_ESTATE before): records that got 0x400, and groups of two or more.  Either pointer may be NULL
 *   bdx_dist_*               the same for a rank's reads (a chromosome lives whole on one rank, so every run does); the getter returns this
 *                            rank's sums, after bdx_dist_run
 *   bdx_mark_duplicates      kernel-level entry point on host arrays (parity tests; callers that filter their own columns): mask[i] = 1
 *                            where the rule marks record i, *n_groups (may be NULL) = groups of two or more.  n == 0 is BDX_OK; a null
 *                            array with n > 0 is BDX_EINVAL; BDX_ELIMIT from 2^32 records */
int bdx_set_mark_duplicates(bdx_ctx* ctx, int on);
int bdx_get_duplicates(const bdx_ctx* ctx, uint64_t* n_marked, uint64_t* n_groups);
int bdx_dist_set_mark_duplicates(bdx_dist* d, int on);
int bdx_dist_get_duplicates(const bdx_dist* d, uint64_t* n_marked, uint64_t* n_groups);
int bdx_mark_duplicates(int device, const int32_t* tid, const int32_t* pos, const int32_t* mtid, const int32_t* mpos, const uint16_t* flag,
                        const uint8_t* lib, const uint64_t* name_key, size_t n, uint8_t* mask, uint64_t* n_groups);

/* Insert-size cutoffs from ALL pairs the store holds: no counterpart in the reference, whose bam2cfg takes them from the first ~10,000
 * pairs of a file (perl/bam2cfg.pl:153-197) and whose breakdancer-max only ever reads them from the configuration (the CLI's --estimate).
 * The rule, written down here once:
 *   OBSERVATION  record i of the resident store is an observation x = isize[i] of its library (lib; an index out of range is library 0; a
 *                context with one library never reads the column) when flag & 0x1 (paired) is set, flag & 0x400, 0x4 and 0x8 are clear (not
 *                a duplicate, both ends mapped), mtid == tid, flag & 0x2 (proper pair) is set, isize >= 0 -- zero counts; the upper mate's
 *                negative isize does not, so each pair is counted once -- and its quality (the mapq column) is GREATER than the library's
 *                minimum, resolved as K1 resolves it (bdx_lib.min_mapping_quality, or opts.min_map_qual when that is negative) and compared
 *                in int.  This is bam2cfg's "flag 18 or 20 and isize >= 0", restated on what the record itself carries.
 *   ROUTING      x < BDX_ISIZE_BINS is counted in hist[lib][x]; x >= BDX_ISIZE_BINS only in n_over[lib].
 *   ESTIMATE     of one library from its histogram, bam2cfg's arithmetic: n, mean_all, sd_all over all observations (n - 1); every x with
 *                !(x > mean_all + 5 sd_all) is kept; n_kept, mean, sd over the kept ones; sd_minus the deviation around mean over the kept
 *                x <= mean (n_minus of them, divided by n_minus - 1), sd_plus over the kept x > mean (n_plus).  All sums in double, bin by
 *                bin in ascending x, as count * x and count * (x - mean)^2; a deviation over fewer than two observations is 0.
 *                valid = n_kept >= 100 && n_minus >= 2 && n_plus >= 2 (100 is bam2cfg's own figure).
 *   bdx_insert_size_histogram  KH (csrc/kh_insert_hist.hip) over the records the store holds by whatever way they came in (pushed, staged,
 *                adopted, decoded, merged), on the context's stream and behind pending batch copies; before or after a run (it needs no
 *                class bytes; after a run with bdx_set_mark_duplicates the marks are in the flag column and count).  All counts are integers:
 *                the result is exact.  hist[nlibs][BDX_ISIZE_BINS] and n_over[nlibs] are overwritten.  BDX_EINVAL for a null pointer,
 *                BDX_ESTATE while a sizing pass is in flight
 *   bdx_dist_insert_size_histogram  the same over the rank's own store; the caller sums the ranks
 *   bdx_estimate_insert_size   host only, no GPU: the ESTIMATE of one library's hist[BDX_ISIZE_BINS].  BDX_EINVAL for a null pointer
 *   bdx_set_libs   replaces the context's libraries and max_read_window_size0 (what bdx_create was given) for the runs that follow: the
 *                host copy and the device tables in stream order; a live or finished pass 1 is invalidated, so the next bdx_run classifies
 *                from the first tile (the route a grown store takes), and the query calls refuse until then.  The store, and the marks
 *                bdx_set_mark_duplicates made on it, stay.  nlibs must be the context's and every bam_index the one given at creation (the
 *                counter keys cannot move): BDX_EINVAL otherwise; BDX_ESTATE while a sizing pass is in flight
 *   bdx_dist_set_libs   the same for the rank's contexts; on every rank alike, before bdx_dist_run */
#define BDX_ISIZE_BINS 32768   /* published for the tests (they aim at its edges) */
typedef struct bdx_insert_estimate {
    double mean_all, sd_all, mean, sd, sd_minus, sd_plus;
    uint64_t n, n_kept, n_minus, n_plus;
    int32_t valid;
} bdx_insert_estimate;
int bdx_insert_size_histogram(bdx_ctx* ctx, uint64_t* hist /*[nlibs][BDX_ISIZE_BINS]*/, uint64_t* n_over /*[nlibs]*/);
int bdx_dist_insert_size_histogram(bdx_dist* d, uint64_t* hist, uint64_t* n_over);
int bdx_estimate_insert_size(const uint64_t* hist /*[BDX_ISIZE_BINS]*/, bdx_insert_estimate* out);
int bdx_set_libs(bdx_ctx* ctx, const bdx_lib* libs, int nlibs, int max_read_window_size0);
int bdx_dist_set_libs(bdx_dist* d, const bdx_lib* libs, int nlibs, int max_read_window_size0);

/* Insert-size shift of the pairs that start inside given windows: no counterpart in the C++ reference, whose calls need -r pairs beyond a
 * hard cutoff; the original distribution's BreakDancerMini slid a window over the normally mapped pairs and tested their insert sizes
 * against the library's distribution with Kolmogorov-Smirnov (the CLI's --mini).  The rule, written down here once:
 *   NULL         bdx_set_insert_null takes hist[nlibs][BDX_ISIZE_BINS] exactly as bdx_insert_size_histogram writes it (the caller may sum
 *                ranks first) and keeps, per library, the cumulative table C_L(x) = sum over y <= x of hist[L][y] on the device, with
 *                N_L = C_L(BDX_ISIZE_BINS - 1).  The next call replaces the table; NULL, or bdx_destroy, frees it.  BDX_ELIMIT when some
 *                N_L >= 2^51: with BDX_MINI_CAP that keeps every product below in int64.  BDX_ESTATE while a sizing pass is in flight.
 *   OBSERVATION  record i of the resident store is an observation x = |isize[i]| of its library for interval (tid, [beg, end)) -- 0-based,
 *                half-open, bdx_interval as everywhere -- when tid[i] == tid and beg <= pos[i] < end; cls[i] & BDX_CLS_PASS;
 *                BDX_CLS_FLAG(cls[i]) is one of BDX_NORMAL_FR, BDX_NORMAL_RF, BDX_ARP_LARGE_INSERT, BDX_ARP_SMALL_INSERT (the same-chromosome
 *                classes whose only possible anomaly is the insert size); mtid[i] == tid[i]; and it is its pair's lower mate exactly as
 *                bdx_count_site_pairs decides it: pos < mpos, or the two are equal and the record is first in pair (flag & 0x40).  The
 *                library index resolves as everywhere (out of range: library 0; a context with one library never reads the column).
 *                x >= BDX_ISIZE_BINS counts only in n_over and is otherwise no observation.
 *                A window is selected by the read's START, not by what its fragment spans: every pair has one lower mate with one start,
 *                whatever its insert size, so the window's sample is drawn without regard to x and the null needs no length-bias correction.
 *   ROW          out[q * nlibs + L], for the observations x_1 .. x_n of library L in interval q:
 *                  n, n_over; sum = x_1 + .. + x_n;
 *                  t_plus  = max(0, max over i of ( #{j: x_j <= x_i} N_L - C_L(x_i) n ));
 *                  t_minus = max(0, max over i of ( C_L(x_i - 1) n - #{j: x_j < x_i} N_L )), with C_L(-1) = 0.
 *                These are n N_L times the one-sided Kolmogorov-Smirnov distances D+ and D- between the window's empirical distribution
 *                function and the null's: both are right-continuous steps on the integers, so the suprema are attained at x_i and x_i - 1.
 *                Everything is an integer: the result is exact and does not depend on the order of evaluation.  N_L == 0 or n == 0: both
 *                t's are 0.  A library absent from a window gets an all-zero row.
 *   CAP          when the observations of a window, all libraries together, exceed BDX_MINI_CAP, every row of that window has
 *                saturated = 1 and t_plus = t_minus = 0; n, n_over and sum stay exact.  This covers pile-ups; nothing is silent.
 *   SCORE        bdx_insert_shift_score, host only, no GPU (csrc/bdx_mini.h): D = max(t_plus, t_minus) / ((double)n (double)N),
 *                lambda = (sqrt(n) + 0.12 + 0.11 / sqrt(n)) D; score = 0 for lambda < 0.4; otherwise
 *                ln p = ln 2 - 2 lambda^2 + ln( sum over j >= 1 of (-1)^(j-1) exp(-2 (j^2 - 1) lambda^2) ), terms added until one is below 1e-17,
 *                and score = -10 ln p / ln 10: the asymptotic Kolmogorov tail, written so that it never underflows.  score and D are 0 for
 *                n == 0, N == 0 or a saturated row.  Either result pointer may be NULL; BDX_EINVAL for a null row.
 * bdx_window_insert_shift (KW, csrc/km_mini.hip): state, errors and their order are those of bdx_count_interval_reads -- BDX_ESTATE before a
 * run has classified the reads the context holds, while a sizing pass is in flight, or with no null set; n == 0 is BDX_OK; BDX_EINVAL for a
 * null array with n > 0, tid < 0, beg < 0 or end < beg; BDX_ELIMIT above 2^31 intervals.  After bdx_run, or on a rank's context
 * (bdx_dist_chromosome) after bdx_dist_run; a tid the context holds nothing of gives zero rows.  Not beside another call on the same context. */
#define BDX_MINI_CAP 4096   /* published for the tests */
typedef struct bdx_insert_shift {     /* 40 bytes */
    uint32_t n, n_over, saturated, pad;   /* pad = 0 */
    uint64_t sum;
    int64_t  t_plus, t_minus;
} bdx_insert_shift;
int bdx_set_insert_null(bdx_ctx* ctx, const uint64_t* hist /*[nlibs][BDX_ISIZE_BINS], NULL frees*/);
int bdx_window_insert_shift(bdx_ctx* ctx, const bdx_interval* iv, size_t n, bdx_insert_shift* out /*[n][nlibs]*/);
int bdx_insert_shift_score(const bdx_insert_shift* row, uint64_t N, double* score, double* D);

/* One-end-anchored reads inside given windows and the position that best splits them: no counterpart in the C++ reference.  An insertion
 * longer than the fragment (novel sequence, a mobile element, a viral integration) leaves no anomalous pair: its only trace is reads whose
 * mates fell into the inserted sequence and did not map -- those on the forward strand pile up left of the junction, those on the reverse
 * strand right of it (the anchor step of NovelSeq, MELT and Pindel; the CLI's --anchor).  The rule, written down here once:
 *   CANDIDATE    record i of the resident store is a candidate for interval (tid, [beg, end)) -- 0-based, half-open, bdx_interval as
 *                everywhere -- when tid[i] == tid, beg <= pos[i] < end and cls[i] == BDX_MATE_UNMAPPED, the whole byte: the classifier
 *                writes 9 exactly for a paired record without 0x400, itself mapped (0x4 clear) with its mate unmapped (0x8 set), and such
 *                a record never carries BDX_CLS_PASS.  A duplicate flag the BAM carries is honoured that way; bdx_set_mark_duplicates never
 *                marks these records (its candidates need a mapped mate), which is why the row reports distinct starts.  The unmapped mate's
 *                own record is class BDX_UNMAPPED and no candidate.
 *   ANCHOR       a candidate whose quality (the store's one quality per record: the AM tag where the aligner wrote one, else MAPQ) passes:
 *                min_qual < 0: quality > its library's minimum as the classifier resolved it (bdx_site_end_quality's test; the library
 *                index resolves as everywhere: out of range is library 0); min_qual >= 0: quality >= min_qual, for every library.  A
 *                candidate that fails counts in n_low and nowhere else.
 *   DIRECTION    an anchor points right when flag & 0x10 is clear, left when it is set; with opts.illumina_long_insert (-l) the other way
 *                round, exactly as bdx_site_breakpoint_bounds inverts strands.
 *   SPLIT        for an integer S in [beg, end]: A(S) = the right-pointing anchors with pos < S, B(S) = the left-pointing anchors with
 *                pos >= S.  split = the smallest S that maximises A(S) + B(S); n_left = A(split), n_right = B(split); u_left / u_right =
 *                the distinct pos among those; last_left = the largest pos of a right-pointing anchor with pos < split, first_right = the
 *                smallest pos of a left-pointing anchor with pos >= split, -1 where there is none.  n_fwd / n_rev = all anchors of the
 *                window by direction.  So: no anchor, or n_left == 0, gives split == beg; n_left > 0 gives split == last_left + 1.  The rule
 *                speaks of positions, never of indices: records of equal pos give the same row in any store order.  Everything is an exact
 *                integer, positions in 64-bit arithmetic (end may be 2^31 - 1).  An empty interval (end == beg) gives zeros, split = beg,
 *                last_left = first_right = -1, as does a tid the context holds nothing of.
 * bdx_window_anchor_split (KA, csrc/ka_anchor.hip): state, errors and their order are those of bdx_window_insert_shift without its null --
 * BDX_ESTATE before a run has classified the reads the context holds or while a sizing pass is in flight; n == 0 is BDX_OK; BDX_EINVAL for
 * a null array with n > 0, min_qual outside -1..255, tid < 0, beg < 0 or end < beg; BDX_ELIMIT above 2^31 intervals.  After bdx_run, or
 * on a rank's context (bdx_dist_chromosome) after bdx_dist_run.  Not beside another call on the same context. */
typedef struct bdx_anchor_split {
    uint32_t n_fwd, n_rev;      /* anchors in the window pointing right / pointing left */
    uint32_t n_low;             /* class-9 records in the window that fail the quality test */
    uint32_t n_left, n_right;   /* A(split), B(split) */
    uint32_t u_left, u_right;   /* distinct pos among those */
    int32_t  split;             /* 0-based: the first position right of the split */
    int32_t  last_left;         /* largest pos of a right-pointing anchor with pos < split; -1: none */
    int32_t  first_right;       /* smallest pos of a left-pointing anchor with pos >= split; -1: none */
} bdx_anchor_split;             /* 40 bytes, 4-aligned */
int bdx_window_anchor_split(bdx_ctx* ctx, const bdx_interval* iv, size_t n, int32_t min_qual, bdx_anchor_split* out /*[n]*/);

/* device the context is bound to and the HIP stream it launches on (as void*), for callers that time it */
int bdx_device(const bdx_ctx* ctx);
void* bdx_stream(const bdx_ctx* ctx);

#ifdef __cplusplus
}
#endif
#endif /* BDX_H */
