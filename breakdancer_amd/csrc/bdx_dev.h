// Shared device-side declarations of libbdx (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace bdx {

constexpr int kTile = 256;      // reads per tile = one wave64 x 4 consecutive reads per lane (no workgroup barrier per tile)
constexpr int kBlock = 256;     // threads per workgroup (4 wave64)
constexpr int kWaves = kBlock / 64;
constexpr int kNumFlags = 11;
constexpr int kK2TilesPerWave = 4; // K2 compacts four of K1's tiles per wave and needs the prefixes at those boundaries only
constexpr int kCntCopies = 64;   // replication factor of the global pass-1 counters (power of two)
constexpr int kMaxChunks = 64;   // chunks a tile-total column is scanned in (one workgroup of finalize_kernel each)
constexpr int kKhMaxGrid = 1024; // KH's persistent workgroups: 256 CUs x 4, what its 35 KiB of LDS per workgroup lets a CU hold (K1's cap, kK1MaxGrid in
                                 // bdx_api.hip, is a measured optimum of a kernel without such a limit; this one is the residency bound, so that the
                                 // number of flushes stays the number of workgroups that can run at once)
constexpr int kStashCap = 16;    // anomalous reads per tile that K1 leaves ready-made for K2 (a tile with more is compacted from the columns)
constexpr int kStashKeys = 2;    // ... when there are at most this many normal-read counter keys (K2's fast path holds their totals in 16 lanes)

// What K1 leaves for K2 about an anomalous read (slot `rank in tile` of the tile's kStashCap slots): everything K2 would
// otherwise gather from seven columns -- K1 has it in registers anyway -- plus the read's in-tile prefix counts, so that K2
// needs neither the class bytes nor the columns of a tile whose anomalous reads fit (name key and read length are fetched by
// K2: K1 does not load those columns).  Only tiles whose reads share one library and source file are served (their normal
// reads count for one key); the slots K2 would read of any other tile with anomalous reads say so: where == 0xFFFFFFFF.
struct StashRec {
    int32_t tid, pos, isize;   // isize = |isize|
    uint32_t meta;             // flag | rev << 4 | lib << 8 (read length: K2)
    uint32_t where;            // offset in tile (8 bits) | normal-leftmost reads before it in the tile << 8 | the tile's counter key << 20
    uint32_t proper;           // proper reads (of that key) up to and including it in the tile
    uint32_t pad[2];
};
static_assert(sizeof(StashRec) == 32, "two 16-byte stores");

enum : int { F_NA = 0, F_FF = 1, F_LARGE = 2, F_SMALL = 3, F_RF = 4, F_RR = 5, F_NORMAL_FR = 6, F_NORMAL_RF = 7,
             F_CTX = 8, F_MATE_UNMAPPED = 9, F_UNMAPPED = 10 };

struct DevLib {
    float upper, lower;
    int32_t min_mapq;  // already resolved against opts.min_map_qual
    int32_t key;       // normal-read counter key: library index (-a) or the library's BAM index
};

struct ReadsSoA {
    const int32_t *tid, *pos, *mtid, *mpos, *isize;
    const uint16_t *flag, *qlen;
    const uint8_t *mapq, *lib, *bam;
    const uint64_t* key;
    const uint64_t* check;   // second, independent hash of the read name (nullptr: names are compared by key alone)
};

// reference-length monoid of one (tile, source file): BamSummary.cpp:70-74 adds pos - last_pos for consecutive
// same-tid records of a file; (first, last, interior sum) composes associatively across tiles
struct MonoRec {
    int32_t ft, fp, lt, lp;
    long long sum;
};

// tile-total columns: 0 anomalous, 1 normal leftmost, 2.. per normal-read key
constexpr int kColAnom = 0, kColNormal = 1, kColKey0 = 2;

struct K1Params {
    ReadsSoA r;
    uint64_t n;
    uint32_t ntiles, tstride;  // tstride = padded row length of the per-tile tables
    uint32_t tile0;            // first tile of this launch (streamed input: tiles are classified as their reads arrive)
    int nlibs, nbams, nkeys;
    int max_sd, opt_t, opt_l;
    const DevLib* libs;
    uint8_t* cls;              // [n]
    uint32_t* tile_tot;        // [2+nkeys][tstride]
    MonoRec* tile_mono;        // [nbams][tstride], pre-set to 0xFF (ft == -1: file absent from the tile)
    uint32_t* blk_cnt;         // [kCntCopies][ncnt] zero-filled, ncnt = nlibs*11 + nlibs + nbams
    StashRec* stash;           // [tiles][kStashCap]; null: more than kStashKeys counter keys (K2 gathers everything itself)
};

// results of pass 1, produced on the device and mirrored to the host
struct Pass1 {
    uint32_t covered_ref_len;
    int32_t window;
    uint32_t n_anom;      // total anomalous reads
    uint32_t n_normal;    // total normal-leftmost reads
    uint32_t key_tot[60]; // proper read totals per key
    unsigned long long ref_len[256];  // per source file: sum of pos - last_pos (BamSummary.cpp:70-74)
};

struct FinalizeParams {
    uint32_t ntiles, tstride, nblk;
    uint32_t nfold;             // workgroups folding the monoid table (first level)
    MonoRec* fold_part;         // [nbams][nfold]
    int nlibs, nbams, nkeys, ncols, ncnt;
    int w0;
    const uint32_t* tile_tot;
    uint32_t* tile_pre;         // [ncols][tstride]: exclusive scan of tile_tot per column at every kK2TilesPerWave-th tile (entry tile /
                                // kK2TilesPerWave), restarting at every chunk of chunk_super such entries ...
    uint32_t* chunk_tot;        // [ncols][kMaxChunks]: ... whose totals are here ...
    uint32_t* chunk_base;       // [ncols][kMaxChunks]: ... and, from the second level, the totals of the chunks before each
    uint32_t chunk_super, nchunk;
    const MonoRec* tile_mono;
    const uint32_t* blk_cnt;
    uint32_t* cnt;              // [ncnt] reduced counters
    Pass1* p1;
    uint32_t* cnt_host;         // pinned host mirrors written by the last kernel (no copy command on the stream); may be null
    Pass1* p1_host;
    const DevLib* libs;         // for the read densities per counter key (BreakDancerMax.cpp:94-107)
    int cn_lib;
    float* key_density;         // [nkeys]; may be null
    uint32_t* flag_host;        // pinned word set to flag_value once the mirrors are written (the host polls it); may be null
    uint32_t flag_value;
    uint64_t* count_host;       // pinned [kMaxChunks], may be null: the workgroup that scans chunk g of column kColAnom stores
                                // (count_stamp << 32 | the chunk's total) to word g as soon as it knows it -- one plain aligned 8-byte
                                // store, value and stamp in one word -- so that the host can size and launch the later stages while
                                // the second level still runs
    uint32_t count_stamp;
    uint32_t na_cap;            // 0, or the capacity the later stages were already enqueued with: if there are more anomalous
                                // reads, the device copy of n_anom is zeroed (they then do nothing) and the host, which still
                                // gets the true count, runs them again
};

// one launch that sets several scratch buffers to their start values (replaces a chain of small fill commands)
struct InitList {
    uint32_t* ptr[6];
    uint32_t words[6];
    uint32_t value[6];
    int n;
};
void launch_init(const InitList& l, hipStream_t s);

// compact anomalous-read records (one per read entering the region accumulator)
struct Compact {
    int32_t* tid;
    int32_t* pos;
    int32_t* isize;     // |isize|
    uint32_t* meta;     // flag (4) | rev<<4 | lib<<8 | qlen<<16
    uint64_t* key;
    uint64_t* check;    // nullptr: the stream has no second name hash
    uint32_t* idx;      // index of the read in the resident stream
    uint32_t* nn;       // normal-leftmost reads seen before this read (stream order)
    uint32_t* pk;       // [nkeys][cap]: proper reads of key k seen up to and including this read
    uint32_t cap;
};

struct K2Params {
    ReadsSoA r;
    uint64_t n;
    uint32_t ntiles, tstride;
    int nkeys, nlibs;
    const DevLib* libs;
    const uint8_t* cls;
    const uint32_t* tile_pre;  // chunk-local prefixes and the chunks' totals (FinalizeParams)
    const uint32_t* chunk_tot;  // (K2 adds up the chunks before its own when it runs beside the second level ...
    const uint32_t* chunk_base; // ... and reads the sum otherwise)
    uint32_t chunk_super;
    const uint32_t* tile_tot;  // K1's per-tile totals and its ready-made records (stash null: not available)
    const StashRec* stash;
    Compact c;
    // initialisation of later stages' scratch folded into this launch (its grid is large and mostly idle)
    uint32_t* fill_ptr[4];
    uint32_t fill_words[4];
    uint32_t fill_value[4];
    // name keys and read lengths left in the caller's pinned host memory (bdx_push): read i's key is seg_ptr[s][i], its
    // length seg_qlen[s][i], for the segment s with seg_begin[s] <= i < seg_begin[s+1]; only the ~1 % anomalous reads ever
    // fetch theirs (over PCIe).  nseg = 0: r.key / r.qlen
    int nseg;
    const uint64_t* seg_begin;          // [nseg + 1]
    const uint64_t* const* seg_ptr;     // [nseg] device-visible, biased by -seg_begin[s]
    const uint16_t* const* seg_qlen;    // [nseg] likewise
    const uint64_t* const* seg_check;   // [nseg] likewise (only read when c.check is set)
};

__device__ __forceinline__ uint32_t meta_pack(int flag, int rev, int lib, int qlen) {
    return (uint32_t)flag | ((uint32_t)rev << 4) | ((uint32_t)lib << 8) | ((uint32_t)qlen << 16);
}
__host__ __device__ __forceinline__ int meta_flag(uint32_t m) { return m & 15; }
__host__ __device__ __forceinline__ int meta_rev(uint32_t m) { return (m >> 4) & 1; }
__host__ __device__ __forceinline__ int meta_lib(uint32_t m) { return (m >> 8) & 255; }
__host__ __device__ __forceinline__ int meta_qlen(uint32_t m) { return m >> 16; }

// ---- wave helpers (wave64) ----------------------------------------------------------------------
__device__ __forceinline__ int lane_id() { return threadIdx.x & 63; }
__device__ __forceinline__ int wave_id() { return threadIdx.x >> 6; }
// (the builtin keeps the condition a lane mask; __ballot() goes through a 0/1 integer per lane and a second compare)
__device__ __forceinline__ uint64_t ballot64(bool p) { return __builtin_amdgcn_ballot_w64(p); }
__device__ __forceinline__ int popc64(uint64_t m) { return __popcll(m); }

// inclusive wave scan of a u32 (6 shuffle steps)
__device__ __forceinline__ uint32_t wave_incl_scan(uint32_t v) {
    const int l = lane_id();
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        uint32_t t = __shfl_up(v, o);
        if (l >= o) v += t;
    }
    return v;
}

// The resident store as the kernels that answer queries over it see it (K8, KS, KI, KM: kq_queries.hip; their shared pieces: bdx_window.h)
struct StoreView {
    const int32_t *tid, *pos, *mtid, *mpos, *isize;   // sorted by (tid, pos)
    const uint16_t* flag;               // SAM flags
    const uint8_t* cls;                 // K1's class bytes
    uint64_t n;
};

// K8: normal pairs covering SV junctions, per query and key (bdx_count_junction_pairs)
struct K8Params {
    StoreView st;
    const uint8_t* key;                 // library or source-file column; read only when nkeys > 1
    const int32_t *q_tid, *q_a, *q_b;   // queries: chromosome, junctions a <= b (1-based)
    uint32_t nq;
    int nkeys;                          // 1..255
    int32_t lmax;                       // no normal pair's |isize| exceeds it
    uint32_t* counts;                   // [nq][nkeys]
};

// KS: alternate-supporting pairs at given SV sites, per site and key (bdx_count_site_pairs)
struct KsSite {                         // = bdx_site (include/bdx.h)
    int32_t tid1, pos1, tid2, pos2;     // 1-based positions, (tid1, pos1) <= (tid2, pos2)
    uint32_t flag_mask;                 // bit f: ReadFlag f supports the site
};
struct KsParams {
    StoreView st;
    const uint8_t* key;                 // library or source-file column; read only when nkeys > 1
    const KsSite* sites;
    uint32_t nq;
    int nkeys;                          // 1..255
    int32_t window;                     // 0..2^30
    uint32_t* counts;                   // [nq][nkeys]
};

// KI: breakpoint intervals of given SV sites from the records KS counts, keys pooled (bdx_site_breakpoint_bounds)
struct KiBounds {                       // = bdx_site_bounds (include/bdx.h)
    uint32_t n;                         // the records that count for the site
    int32_t lo1, hi1, lo2, hi2;         // per end: the largest lower and the smallest upper bound, 1-based; all 0 with n == 0
};
struct KiParams {
    StoreView st;
    const uint8_t* lib;                 // library column; read only when nlibs > 1
    const KsSite* sites;
    uint32_t nq;
    int nlibs;                          // 1..255
    int32_t window;                     // 0..2^30
    int32_t long_insert;                // -l: reads point away from their fragment
    uint32_t u0;                        // library 0's insert-size bound U (0..2^30) ...
    const uint32_t* utab;               // ... and every library's [nlibs]; read only when nlibs > 1
    KiBounds* out;                      // [nq]
};

// KM: mapping quality of the supporters of one end of given SV sites and of the records around it (bdx_site_end_quality)
struct KmQuality {                      // = bdx_site_quality (include/bdx.h)
    uint32_t n, n_all, n_low;           // supporters; records around the end; the low ones among them
    uint8_t qmin, q1, median, qmax;     // over the supporters' qualities; all 0 with n == 0
};
struct KmParams {
    StoreView st;
    const uint8_t* mapq;                // quality column (AM tag if present, else MAPQ)
    const uint8_t* lib;                 // library column; read only when nlibs > 1
    int nlibs;                          // 1..255
    int32_t q0;                         // library 0's minimum mapping quality, resolved as for K1 ...
    const int32_t* qtab;                // ... and every library's [nlibs]; read only when nlibs > 1
    const KsSite* sites;
    const uint8_t* end;                 // [nq] 1 or 2: the end of sites[q] that is asked
    uint32_t nq;
    int32_t window;                     // 0..2^30
    KmQuality* out;                     // [nq]
};

// KP (kp_clip.hip): the piles of clipped reads around one end of given SV sites (bdx_site_clip_peaks)
struct KpPeaks {                        // = bdx_clip_peaks (include/bdx.h)
    uint32_t n_left, n_right;           // observations per side
    int32_t pos_left, pos_right;        // the X most of them share (1-based) ...
    uint32_t peak_left, peak_right;     // ... and how many do; both 0 with n == 0
};
struct KpParams {
    StoreView st;
    const uint32_t* clip;               // the clip words (bdx_use_clips); read only for records that pass
    const KsSite* sites;
    const uint8_t* end;                 // [nq] 1 or 2: the end of sites[q] that is asked
    uint32_t nq;
    int32_t window;                     // 0..BDX_CLIP_WINDOW_MAX: sizes the launch's LDS
    int32_t min_clip;                   // 1..255
    KpPeaks* out;                       // [nq]
};
void launch_kp(const KpParams& p, hipStream_t s);

// KR (kr_depth.hip): passing read starts inside given intervals, per interval and key (bdx_count_interval_reads)
struct KrInterval {                     // = bdx_interval (include/bdx.h)
    int32_t tid, beg, end;              // 0-based, half-open
};
struct KrParams {
    StoreView st;
    const uint8_t* key;                 // library or source-file column; read only when nkeys > 1
    const KrInterval* iv;
    uint32_t nq;
    int nkeys;                          // 1..255
    uint32_t nchunks;                   // chunks of BDX_DEPTH_CHUNK records the store is cut into (the last one partial)
    uint32_t* table;                    // [nkeys][nchunks + 1]: passing records of the key in front of each chunk; null: every interval is walked
    uint32_t* counts;                   // [nq][nkeys]
};

// KH (kh_insert_hist.hip): insert-size histogram per library over the resident store (bdx_insert_size_histogram)
struct KhParams {
    const int32_t *tid, *mtid, *isize;
    const uint16_t* flag;
    const uint8_t* mapq;
    const uint8_t* lib;                 // null: one library (the column is not resident)
    uint64_t n;
    int nlibs;                          // 1..255
    const DevLib* libs;                 // [nlibs]: min_mapq, resolved as for K1
    const float* lib_mean;              // [nlibs]: the libraries' mean insert sizes (where a library's LDS window sits; never the result)
    unsigned long long* hist;           // [nlibs][BDX_ISIZE_BINS], zeroed by the caller
    unsigned long long* n_over;         // [nlibs], likewise
};
void launch_kh(const KhParams& p, hipStream_t s);

// KW (km_mini.hip): insert-size shift of the pairs that start inside given windows, per window and library (bdx_window_insert_shift)
struct KwShift {                        // = bdx_insert_shift (include/bdx.h)
    uint32_t n, n_over, saturated, pad;
    uint64_t sum;
    int64_t t_plus, t_minus;
};
struct KwParams {
    StoreView st;
    const uint8_t* lib;                 // library column; read only when nlibs > 1
    const KrInterval* iv;
    uint32_t nq;
    int nlibs;                          // 1..255
    const uint64_t* ctab;               // [nlibs][BDX_ISIZE_BINS]: the null's cumulative counts C_L(x); N_L is the row's last entry (< 2^51)
    int staged;                         // "mini_staged": the all-pairs route at every size
    KwShift* out;                       // [nq][nlibs]
};
void launch_kw(const KwParams& p, hipStream_t s);

// KA (ka_anchor.hip): the one-end-anchored reads that start inside given windows and their best split (bdx_window_anchor_split)
struct KaSplit {                        // = bdx_anchor_split (include/bdx.h)
    uint32_t n_fwd, n_rev, n_low;
    uint32_t n_left, n_right, u_left, u_right;
    int32_t split, last_left, first_right;
};
struct KaParams {
    StoreView st;
    const uint8_t* mapq;                // quality column (AM tag if present, else MAPQ); read only for class-9 records
    const uint8_t* lib;                 // library column; read only when qtab is given
    const KrInterval* iv;
    uint64_t nq;                        // up to 2^31: the grid strides over them
    int nlibs;                          // 1..255
    int32_t long_insert;                // -l: reads point away from their fragment
    int32_t q0;                         // a candidate is an anchor when its quality is ABOVE this (min_qual - 1, or library 0's minimum) ...
    const int32_t* qtab;                // ... or above its library's [nlibs]; null: q0 for every record (one library, or min_qual >= 0)
    KaSplit* out;                       // [nq]
};
void launch_ka(const KaParams& p, hipStream_t s);

// KD (kd_markdup.hip): duplicate marking over the resident store (bdx_set_mark_duplicates, bdx_mark_duplicates)
constexpr int kDupT = 64;               // neighbours a record looks at each way; runs of more records go through the table
struct KdCounts {
    unsigned long long marked, groups;  // records that got 0x400; groups of two or more
    uint32_t nwork, nlist;              // candidates of runs longer than kDupT (counted by kd_scan); work-list entries appended so far
};
struct KdParams {
    const int32_t *tid, *pos, *mtid, *mpos;
    const uint16_t* flag;
    const uint8_t* lib;                 // null: one library
    const uint64_t* key;                // name keys (nseg == 0) ...
    int nseg;                           // ... or K2Params' segments: keys the caller's pinned batches still hold
    const uint64_t* seg_begin;
    const uint64_t* const* seg_ptr;
    uint64_t n;
    uint64_t* bits;                     // [(n + 63) / 64] one bit per record: it is marked
    uint64_t* longbits;                 // likewise: it is a candidate of a run longer than kDupT
    KdCounts* cnt;                      // zeroed by the caller
    // only for a count of long-run candidates that is not zero, sized from it:
    uint32_t *work, *wrun;              // [nwork] the work list (record indices) and the entries' run ids
    uint64_t* starts;                   // [(n + 63) / 64] one bit per record: it starts a run
    uint32_t *pre, *cbase;              // [(n + 63) / 64], [kd_chunks(n)]: run starts before each word in its chunk, before each chunk
    uint32_t *table, *multi;            // [tmask + 1] each: the table (work-list indices) and its "group has a loser" words
    uint64_t tmask;
};
uint32_t kd_chunks(uint64_t n);
void launch_kd_scan(const KdParams& p, hipStream_t s);
void launch_kd_long(const KdParams& p, uint32_t nwork, hipStream_t s);
void launch_kd_apply(const KdParams& p, uint16_t* flag, uint8_t* mask, hipStream_t s);

// launchers (host side, defined in the .hip files)
void launch_k8(const K8Params& p, hipStream_t s);
void launch_ks(const KsParams& p, hipStream_t s);
void launch_ki(const KiParams& p, hipStream_t s);
void launch_km(const KmParams& p, hipStream_t s);
void launch_kr_table(const KrParams& p, hipStream_t s);   // chunk counts and their prefix per key: before launch_kr_query when p.table
void launch_kr_query(const KrParams& p, hipStream_t s);
void launch_k1(const K1Params& p, int grid, size_t lds, hipStream_t s, hipEvent_t start = nullptr, hipEvent_t stop = nullptr);
size_t k1_lds_bytes(int nlibs, int nbams, int nkeys);
void launch_finalize(const FinalizeParams& p, hipStream_t s, bool second_level = true);
void launch_finalize2_only(const FinalizeParams& p, hipStream_t s);
void launch_k2(const K2Params& p, size_t lds, hipStream_t s, const FinalizeParams* side = nullptr);  // side: finalize2_body as an extra workgroup
size_t k2_lds_bytes(int nkeys);

}  // namespace bdx
