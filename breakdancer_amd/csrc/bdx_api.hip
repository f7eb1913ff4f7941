// libbdx: context, HBM-resident read store, stage orchestration and the extern "C" boundary (include/bdx.h).
//
// One context = one GPU = one HIP stream.  The whole record stream stays resident in HBM (a 30x human
// genome is ~33 GB of SoA, well inside 288 GB), so pass 1 and pass 2 of the reference collapse into one
// read of the data: K1 -> finalize -> K2 -> K3 -> K4 on the device, one small readback, the host walk,
// K5 for the scores.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <functional>
#include <memory>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstddef>
#include <cstring>
#include <string>
#include <thread>
#include <unordered_map>
#include <utility>
#include <vector>

#include "../../include/bdx.h"
#include "bdx_buf.h"
#include "bdx_dev.h"
#include "bdx_k3.h"
#include "bdx_shard.h"
#include "bdx_scan.h"
#include "bdx_walk.h"
#include "bdx_bam_dev.h"
#include "bdx_clip.h"
#include "bdx_estimate.h"
#include "bdx_mini.h"

using namespace bdx;

namespace {

// KD's scratch: the mark bits, the long-run bits and the counters (1/4 B per read, kept); what only runs longer than kDupT need is
// allocated from their candidates' count and handed back when the marks are made
struct KdScratch {
    DevBuf bits, longbits, cnt;
    DevBuf work, wrun, starts, pre, cbase, table, multi;
    void release_long() { work.release(); wrun.release(); starts.release(); pre.release(); cbase.release(); table.release(); multi.release(); }
};

// The buffers of the stages behind pass 1 (K2 compaction, K3 region cut, K4 join, K6 up to the table), apart from the context so that the
// functions which size them (size_compact .. size_k6) can be handed these and nothing else of a context.  One DevBuf / PinBuf per array.
struct StageBufs {
    DevBuf b_c_tid, b_c_pos, b_c_isize, b_c_meta, b_c_key, b_c_check, b_c_idx, b_c_nn, b_c_pk;
    DevBuf b_cand, b_pre_q, b_pre_rev, b_pre_nonctx, b_c_first, b_c_maxq, b_c_rid, b_region_of, b_lb;
    DevBuf b_bcnt, b_boff, b_bcur, b_e_key, b_e_idx, b_partner, b_t_key, b_t_idx, b_pair_lo;
    DevBuf b_groups;                  // (sharded runs) the join's pair groups, where they stay in HBM instead of pinned host memory
    DevBuf b_r_rec, b_r_pk, b_out_deg, b_parts, b_rs, b_slot, b_members, b_own, b_lib_stage, b_cn_stage, b_t_lambda, b_t_k, b_ws6;
    DevBuf b_sv_src, b_dlists, b_ltail, b_ins, b_member_ids;
    DevBuf b_sv_out, b_lib_index_out, b_lib_pairs_out, b_cn_key_out, b_cn_value_out, b_ltail_out, b_sv_key;   // the final table where it stays in HBM
    PinBuf h_regs, h_pk, h_groups, h_counts0, h_counts2, h_sv_out, h_lib_index, h_lib_pairs, h_cn_key, h_cn_value, h_ltail_dev;
};

constexpr int kNumStages = 12;
// bdx_ctx::stage_ms, in the order bdx_get_timings hands them out (include/bdx.h)
enum StageMs { kMsClassify, kMsCompact, kMsCut, kMsJoinAssemble, kMsGroupsWait, kMsHostWalk, kMsFinish, kMsRun, kMsTableWait, kMsMerge, kMsScores };
// the words of bdx_ctx::h_flags: a kernel (or a stream write) sets each to the run's sequence number once what it names is complete
enum ReadyWord { kPass1Ready, kGroupsReady, kTableReady, kRegionsReady };
constexpr int kK1MaxGrid = 8192;  // measured best on MI355X (tools/k1_probe.hip; again at the end of round 2: 2048 74.6 us, 4096 70.9,
                                  // 8192 69.9, 12288 72.5, 16384 73.4): 256 CUs x 32 workgroups queued, 4 independent waves each
constexpr uint32_t kK1EventPeriod = 4;  // K1 is bracketed by HIP events on every n-th run (an event pair idles the GPU ~10 us)

}  // namespace

struct bdx_ctx {
    // Order of release: members go in reverse order of declaration, so the two streams are declared FIRST and destroyed LAST, behind
    // every buffer and event that is used on them (bdx_destroy synchronises both before anything goes).
    int device = 0;
    Stream stream;
    Stream copy_stream;                 // H2D copies of the batches; the classifier follows each batch on `stream` behind ev_copy
    bdx_opts opts{};
    std::vector<bdx_lib> libs;
    int nlibs = 0, nbams = 0, ntids = 0, nkeys = 0, w0 = 0;
    std::string err;

    // resident reads
    ReadsSoA d{};
    size_t n = 0, cap = 0;
    bool adopted = false;
    DevBuf b_tid, b_pos, b_mtid, b_mpos, b_isize, b_flag, b_qlen, b_mapq, b_lib, b_bam, b_key, b_check;
    bool groups_in_hbm = false;       // (sharded runs) the join's pair groups stay in HBM instead of pinned host memory
    bool use_check = false;           // bdx_use_name_check: every batch carries a second hash of the read name, mates must agree in it too
    bool use_clips = false;           // bdx_use_clips: the store has a column of clip words (b_clip: [cap], zero where nothing was put)
    DevBuf b_clip;
    // bdx_put_clips: the caller's words go through pinned buffers of the context's own, so that the call returns without waiting for the copy
    struct ClipStage { PinBuf buf; Event done; bool busy = false; };
    ClipStage clip_ring[4];
    int clip_next = 0;

    // stage buffers
    DevBuf b_libs, b_cls, b_tile_tot, b_tile_pre, b_tile_mono, b_blk_cnt, b_cnt, b_p1, b_fold, b_stash, b_chunk_tot, b_counts;
    DevBuf b_lib_mean, b_kdens;
    PinBuf h_p1, h_cnt, h_counts, h_terms;
    PinBuf h_hs_rec, h_hs_aux, h_hs_lists, h_printed;
    StageBufs sb;                     // K2 .. K6: what a sizing pass grows
    PinBuf h_flags;                   // one word per ReadyWord: pass 1, the host's groups, the final table, the region table (= run sequence number)
    PinBuf h_count;                   // [kMaxChunks] 64-bit words: finalize_kernel's chunk totals of anomalous reads, each stamped with the run sequence number
                                      // in its high half (FinalizeParams::count_host; read by wait_count)
    uint32_t seq = 0;
    // test / measurement switches (bdx_set_debug): all off by default
    int dbg_no_stash = 0, dbg_max_chunks = 0, dbg_ins_plain = 0, dbg_gather_walk = 0, dbg_regions_copy = 0, dbg_asm_plain = 0, dbg_depth_plain = 0, dbg_mini_staged = 0;
    uint32_t lb_seq = 0;              // launches of look-back scans so far: every launch stamps its words with its own number (bdx_scan.h)
    float k1_ms_last = 0;
    bool k1_timed = false;
    bool stage_timing = false;        // HIP events around K2 / K3 / K4+K6 (each costs a few microseconds of idle GPU)
    bool poll = true;                 // BDX_NO_POLL=1: wait with stream / event synchronisation only
    bool materialized = true;         // c->walk holds the final table (false: it still sits in the pinned buffers only)
    bool rows_packed = false;         // ... as SvWire rows (48 bytes: what a single-context run's table kernel writes over PCIe), not SvOut
    uint32_t n_sv_total = 0, n_groups_total = 0, n_terms_total = 0, n_cn_total = 0;
    Event ev_groups, ev_regions;
    int big_walk_mode = -1;           // BDX_BIG_WALK=1 / 0: components of 5..64 regions always / never walked on the device; default: when
                                      // the host's share is large enough to matter (StageDims::walks_big)
    int64_t last_big_groups = -1;     // groups of such components in the previous run of this context (device + host share)
    FinalizeParams fp_deferred{};     // second level of the pass-1 finalisation, to be run by K2's launch (enqueue-ahead runs)
    bool finalize2_deferred = false;
    bool bucketed_join = false;       // BDX_BUCKETED_JOIN=1: use the partitioned LDS join at every size (it is the path for > 4 M entries)
    bool host_walk_only = false;      // BDX_HOST_WALK=1: every component goes through the host walk (A/B testing of K6)
    K6Arrays k6{};
    const GroupRec* k6_in_groups = nullptr;  // (a caller that holds pair groups as aggregates: K6 takes them instead of counting pairs)
    const uint32_t* k6_in_goff = nullptr;
    // sharded runs (bdx_dist_*): this context holds several chromosomes of a genome, in ascending order (bdx_shard.h)
    bool force_direct_join = false;   // the join takes foreign entries: the direct table at every size
    uint32_t k6_cap = 0;              // capacity of K6's per-region arrays: the GENOME's regions (0: this context's anomalous reads)
    const RegionRec* k6_r_rec = nullptr;   // the region table laid out by genome-wide id (this rank's regions, n == 0 elsewhere)
    const uint32_t* k6_r_pk = nullptr;
    uint8_t* k6_taint = nullptr;
    bool table_in_hbm = false;        // the final table stays in HBM (with its order keys): rank 0 merges the ranks' tables

    // results
    bool ran = false;
    Pass1 p1{};
    StageCounts counts{};
    std::vector<uint32_t> cnt;        // adopted counters: hist[nlibs*11], lib_cnt[nlibs], bam_cnt[nbams]
    std::vector<uint32_t> cnt_local;  // this context's own counters
    uint32_t g_covered = 0;
    int32_t g_window = 0;
    uint32_t ntiles = 0, tstride = 0;
    Compact cp{};
    K3Arrays k3{};
    K4Arrays k4{};
    std::vector<double> log_tail;
    bool collect_support = false;
    std::vector<uint32_t> ov_cnt;     // bdx_set_pass1_statistics: restored pass-1 counters that replace the run's own
    uint32_t ov_covered = 0;
    bool replayed = false;            // the last run went through the read-level host replay (a read name seen more than twice)
    bool use_stash = false;           // K1 leaves ready-made records of the anomalous reads for K2 (at most kStashKeys counter keys)
    // The sizing passes (bdx_reserve, the BAM decoder's sizing thread; presize_stages): the size functions of the stages behind pass 1 are
    // handed `sb` and a description by value, not the context, so they cannot reach its run state (no flag on the context says "sizing":
    // round 5's did, and a run beside the sizing thread saw it and launched nothing).  While one is in flight the entry points that
    // launch those stages refuse with BDX_ESTATE; its error text goes to sizing_err (the feeding thread owns `err`).
    std::atomic<int> sizing{0};
    std::string sizing_err;
    std::vector<uint32_t> sup_off;    // [n_svs + 1]
    std::vector<uint64_t> sup_idx;
    std::vector<uint8_t> sup_flag;
    std::vector<float> seqcov, lib_density, key_density;
    std::vector<HostRegion> regions;  // owned copies (small tables, phantom shift, own_borrowed_regions); otherwise reg/rpk point into pinned memory
    std::vector<uint32_t> r_pk;
    const HostRegion* reg = nullptr;
    size_t nreg = 0;
    const uint32_t* rpk = nullptr;
    std::vector<GroupPart> parts;
    WalkResult walk;
    std::unique_ptr<WalkScratch, void (*)(WalkScratch*)> walk_scratch{nullptr, walk_scratch_free};
    uint32_t n_printed = 0;
    uint32_t n_sv_host = 0;
    // enqueue-ahead: a context that has just run an input of the same size sizes the later stages from that run's count of
    // anomalous reads (+12 %) and enqueues them before the pass-1 record is back, so the device does not idle at the
    // host's decision; finalize2_kernel neutralises them if the guess was too small and the host runs them again
    int speculate = 2;                // enqueue-ahead: 0 off (BDX_NO_SPECULATE=1), 1 sized from a prior on the read count only, 2 (default)
                                      // from the previous run of the same input where there is one, else from the prior
    int spec_test = 0;                // BDX_SPEC_TEST=1: guess half of the last count (forces the retry path)
    uint32_t last_na = 0;
    size_t last_n = 0;
    uint32_t count_chunks = 0;        // words of h_count the pass 1 in flight posts (0: none, the count comes with the record)
    uint32_t na_alloc = 0;            // the count the later stages are sized and launched with
    bool region_of_fused = false;
    uint32_t join_table_clean = 0;    // slots of the direct join table already set to -1 (by K2), 0 = none
    float stage_ms[kNumStages] = {0};
    Event ev[8];

    // ---- streamed input (bdx_push / bdx_acquire_batch + bdx_submit_batch) ----
    Event ev_copy;
    bool copy_pending = false;          // copies enqueued since the last run: `stream` has to wait for ev_copy
    // pass 1 as the reads arrive: the tile tables are laid out for k1_cap_tiles tiles and tiles [0, k1_done) are classified
    bool k1_live = false;
    uint32_t k1_done = 0, k1_cap_tiles = 0;
    struct Stage {                      // one pinned staging buffer of the ring
        PinBuf buf;
        size_t cap = 0;
        Event done;
        bool busy = false;
    };
    Stage ring[4];
    int ring_next = 0, ring_cur = -1;
    // name keys that stay in the caller's pinned memory (bdx_push): one segment per batch; host == nullptr: that range of
    // keys was copied into the resident column
    struct KeySeg { uint64_t begin; const uint64_t* host; const uint16_t* host_qlen; const uint64_t* host_check; };
    std::vector<KeySeg> key_segs;
    DevBuf b_seg;

    // ---- bdx_count_junction_pairs, bdx_count_site_pairs, bdx_site_breakpoint_bounds, bdx_site_end_quality (run_query) ----
    size_t cls_n = (size_t)-1;        // reads the class bytes in b_cls describe (set by a completed pass 1; -1: none)
    DevBuf b_qtab;                    // bdx_count_interval_reads' table of one call (scratch: rebuilt by every call)
    DevBuf b_hist;                    // bdx_insert_size_histogram's table of one call: [nlibs][BDX_ISIZE_BINS] counts and behind them n_over[nlibs]
    DevBuf b_null;                    // bdx_set_insert_null's cumulative table [nlibs][BDX_ISIZE_BINS], kept until it is replaced or freed
    bool null_set = false;
    DevBuf b_qin, b_qout;             // a call's uploads (queries or sites, and behind them KI's table of the libraries' U, or KM's of their minima and its ends) and its results.
                                      // One pair serves the three: every call ends with hipStreamSynchronize, so none can see another's data
    // ---- bdx_set_mark_duplicates ----
    bool mark_dup = false;            // KD marks duplicates in the flag column at the head of pass 1; pass 1 then does not start behind arriving batches
    bool dup_done = false;            // KD has run over this load (nothing can be appended to it any more)
    uint64_t dup_marked = 0, dup_groups = 0;
    KdScratch kd;
};

namespace {

int fail(bdx_ctx* c, int code, const std::string& msg) {
    if (c) c->err = msg;
    return code;
}
// entry points that launch the stages behind pass 1: not while their buffers are being sized on another thread
#define NOT_WHILE_SIZING(c)                                                                                                              \
    do {                                                                                                                                 \
        if ((c)->sizing.load(std::memory_order_acquire))                                                                                 \
            return fail(c, BDX_ESTATE, "the buffers of the later stages are being sized on another thread (bdx_bamdec_finish has not returned)"); \
    } while (0)
int hipfail(bdx_ctx* c, hipError_t e, const char* what) {
    return fail(c, BDX_EHIP, std::string(what) + ": " + hipGetErrorString(e));
}
#define HIPCHK(ctx, expr)                                   \
    do {                                                    \
        hipError_t _e = (expr);                             \
        if (_e != hipSuccess) return hipfail(ctx, _e, #expr); \
    } while (0)
// the same for a call that returns a BDX_* status
#define BDX_TRY(expr)                      \
    do {                                   \
        const int _rc = (expr);            \
        if (_rc != BDX_OK) return _rc;     \
    } while (0)

size_t round_up(size_t x, size_t m) { return (x + m - 1) / m * m; }

// a library's minimum mapping quality as K1 compares against it (quality > minimum passes) and as bdx_site_end_quality calls a record low
int32_t resolved_min_mapq(const bdx_opts& o, const bdx_lib& l) { return l.min_mapping_quality < 0 ? o.min_map_qual : l.min_mapping_quality; }

// The stamp of the next look-back launch on this context.  A state array may see a given stamp only once (a word of an
// earlier launch with the same stamp would read as already published), so the stamp counts LAUNCHES, not runs -- the cut and
// the table stage can be launched again without a new pass 1 -- and when the 30-bit counter comes round the arrays start
// from zero again.
hipError_t next_lb_stamp(bdx_ctx* c, uint32_t* out) {
    if (((++c->lb_seq) & 0x3FFFFFFFu) == 0) {
        if (c->sb.b_lb.p) { const hipError_t e = hipMemsetAsync(c->sb.b_lb.p, 0, c->sb.b_lb.bytes, c->stream); if (e != hipSuccess) return e; }
        if (c->sb.b_ws6.p) { const hipError_t e = hipMemsetAsync(c->sb.b_ws6.p, 0, c->sb.b_ws6.bytes, c->stream); if (e != hipSuccess) return e; }
        ++c->lb_seq;
    }
    *out = c->lb_seq & 0x3FFFFFFFu;
    return hipSuccess;
}

int alloc_reads(bdx_ctx* c, size_t cap) {
    cap = round_up(std::max<size_t>(cap, 1), 1024);
    if (cap <= c->cap) return BDX_OK;
    if (c->copy_stream) HIPCHK(c, hipStreamSynchronize(c->copy_stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->k1_live = false;  // the tile tables were laid out for the old capacity: bdx_run classifies from the first tile again
    struct Col { DevBuf* b; size_t esz; const void** slot; };
    Col cols[] = {{&c->b_tid, 4, (const void**)&c->d.tid},     {&c->b_pos, 4, (const void**)&c->d.pos},
                  {&c->b_mtid, 4, (const void**)&c->d.mtid},   {&c->b_mpos, 4, (const void**)&c->d.mpos},
                  {&c->b_isize, 4, (const void**)&c->d.isize}, {&c->b_flag, 2, (const void**)&c->d.flag},
                  {&c->b_qlen, 2, (const void**)&c->d.qlen},   {&c->b_mapq, 1, (const void**)&c->d.mapq},
                  {&c->b_lib, 1, (const void**)&c->d.lib},     {&c->b_bam, 1, (const void**)&c->d.bam},
                  {&c->b_key, 8, (const void**)&c->d.key},     {&c->b_check, 8, (const void**)&c->d.check}};
    for (Col& col : cols) {
        if (col.b == &c->b_check && !c->use_check) continue;
        DevBuf nb;
        HIPCHK(c, nb.ensure(cap * col.esz));
        if (c->n) HIPCHK(c, hipMemcpyAsync(nb.p, col.b->p, c->n * col.esz, hipMemcpyDeviceToDevice, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        col.b->release();
        *col.b = std::move(nb);
        *col.slot = col.b->p;
    }
    if (c->use_clips) {   // the clip words: rows nobody has put stay 0
        DevBuf nb;
        HIPCHK(c, nb.ensure(cap * 4));
        HIPCHK(c, hipMemsetAsync(nb.p, 0, cap * 4, c->stream));
        if (c->n) HIPCHK(c, hipMemcpyAsync(nb.p, c->b_clip.p, c->n * 4, hipMemcpyDeviceToDevice, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        c->b_clip.release();
        c->b_clip = std::move(nb);
    }
    c->cap = cap;
    return BDX_OK;
}

// columns of a staging buffer: every column starts 8-byte aligned (the stride is a multiple of 64 records)
void stage_view(const bdx_ctx::Stage& st, bdx_batch_buf* out) {
    char* p = (char*)st.buf.p;
    const size_t K = st.cap;
    out->name_key = (uint64_t*)p; p += K * 8;
    out->name_check = (uint64_t*)p; p += K * 8;
    out->tid = (int32_t*)p; p += K * 4;
    out->pos = (int32_t*)p; p += K * 4;
    out->mtid = (int32_t*)p; p += K * 4;
    out->mpos = (int32_t*)p; p += K * 4;
    out->isize = (int32_t*)p; p += K * 4;
    out->flag = (uint16_t*)p; p += K * 2;
    out->qlen = (uint16_t*)p; p += K * 2;
    out->mapq = (uint8_t*)p; p += K;
    out->lib = (uint8_t*)p; p += K;
    out->bam = (uint8_t*)p;
    out->capacity = K;
}

// What decides the sizes of the buffers of the stages behind pass 1, by value.  The size functions (size_compact .. size_k6, in front of the
// stages) get this, the buffers, the stream (two arrays are zeroed when they are allocated) and a place for an error text -- NOT a context:
// a stage calls its size function at its head, and a sizing pass (presize_stages) calls all four, possibly on a thread beside the one
// that feeds the context.
enum class RegionDst { HostAndHbm, Hbm };   // K3's region table: pinned host memory and a copy in HBM for K6 (bdx_run);
                                            // HBM only (sharded runs: a chromosome's table is sent on from there, nobody reads it on this host)
struct StageDims {
    uint32_t na = 0;                  // anomalous reads the stages are sized for
    int nkeys = 0, nlibs = 0;
    bool use_check = false;
    bool k2_clears_join = false;      // the context joins its own reads through the direct table: K2's launch presets it (table, partner[], pair_lo[])
    RegionDst regions = RegionDst::HostAndHbm;
    bool groups_in_hbm = false, table_in_hbm = false;
    uint32_t k6_cap = 0;              // K6's per-region arrays hold at least this many regions (sharded runs: the genome's)
    int big_walk = -1;                // components of 5..64 regions walked on the device: 1 / 0 (test switch, the previous run's groups), -1: the size decides
    // the join: its entries; those with a partner[] / pair_lo[] word (the context's own reads); the direct table's slots (0: the bucketed
    // join, which sizes its tables when it runs); whether pair_lo[] is wanted where K2 has not preset it
    uint32_t join_n = 0, join_own = 0, join_slots = 0;
    bool join_pair_lo = false;

    uint32_t join_groups() const { return join_n / 2 + 1; }
    uint32_t k6_regions() const { return std::max(na, k6_cap); }   // (sharded runs: K6's arrays are indexed by genome-wide region id)
    // Components of 5..64 regions cost one more launch (k6_walk_big_kernel) and a member table of 256 B per label.  Few of
    // them are walked by the host behind the device's own walk for free; many (dense data) make the host walk the longest
    // stage.  Without a previous run to go by, the number of anomalous reads decides.
    int walks_big() const { return big_walk >= 0 ? big_walk : (k6_regions() > 500000u ? 1 : 0); }
};

// a join of `n` entries on this context takes the direct table (else the partitioned LDS join)
bool joins_direct(const bdx_ctx* c, uint32_t n) { return c->force_direct_join || (!c->bucketed_join && n <= kDirectJoinMax); }

// Capacity of the later stages for `count` anomalous reads: the count plus the headroom an enqueue-ahead run of the same input asks for,
// so that its buffers are the buffers of the run before it.  Not clamped: each caller has its own answer beyond kMaxAnomalous.
uint64_t with_headroom(uint64_t count) { return count + count / 8 + 1024; }
// The prior a first run of `n_reads` reads sizes the later stages by, where it takes one (plan_sizing has the measurements), and
// what bdx_reserve and the BAM decoder's sizing thread therefore allocate: if they disagreed, the first run would reallocate inside the
// timed step.  divisor: 32; BDX_SPEC_TEST's 4096 makes it too small on purpose.
uint64_t prior_anomalous(uint64_t n_reads, uint32_t divisor = 32) { return n_reads / divisor + 4096; }

// ... of a context that takes `na` anomalous reads of its own through all four stages (bdx_run, the sizing passes)
StageDims stage_dims(const bdx_ctx* c, uint32_t na) {
    StageDims d;
    d.na = na; d.nkeys = c->nkeys; d.nlibs = c->nlibs; d.use_check = c->use_check;
    d.k2_clears_join = joins_direct(c, na);
    d.groups_in_hbm = c->groups_in_hbm; d.table_in_hbm = c->table_in_hbm; d.k6_cap = c->k6_cap;
    d.big_walk = c->big_walk_mode >= 0 ? c->big_walk_mode : (c->last_big_groups >= 0 ? (c->last_big_groups > 2000 ? 1 : 0) : -1);
    d.join_n = d.join_own = na; d.join_slots = d.k2_clears_join ? direct_join_slots(na) : 0;
    return d;
}

int pass1_prepare(bdx_ctx* c, uint32_t tiles_cap);
int presize_stages_here(bdx_ctx* c, const StageDims& dm);
int pass1_classify(bdx_ctx* c, uint32_t upto, bool timed);

constexpr uint32_t kStreamTilesMin = 4096;  // classify behind a batch only once this many new tiles (1 M reads) are complete

// One batch of host records into the resident store: H2D copies on the copy stream, then -- for a store that is being
// filled from empty -- the classifier over the tiles the batch completed, on the compute stream behind the copies.
// lazy_keys: the batch is the caller's own memory and stays valid until bdx_run returns, so pinned name keys need not
// travel: K2 fetches the keys of the anomalous reads (about 1 %) straight from there.
int enqueue_batch(bdx_ctx* c, const bdx_batch& b, bool lazy_keys) {
    if (c->n + b.n > c->cap) {
        BDX_TRY(alloc_reads(c, std::max(c->n + b.n, c->cap * 2)));
    }
    const size_t o = c->n, n = b.n;
    if (c->mark_dup && c->dup_done && o)
        return fail(c, BDX_ESTATE, "duplicates of this load are marked already: reads cannot be appended behind a run (bdx_reset_reads starts the next load)");
    hipStream_t s = c->copy_stream;
    if (o == 0) {  // a fresh store: pass 1 runs as the reads arrive
        c->key_segs.clear();
        const uint64_t tiles = (c->cap + kTile - 1) / kTile;
        if (tiles <= 0xFFFFFFFFull) {
            BDX_TRY(pass1_prepare(c, (uint32_t)tiles));
            c->k1_live = !c->mark_dup;   // (duplicates are marked over the whole store before K1 reads a flag)
        }
    }
    // (one stream: splitting the columns over two copy streams measured 10.8 ms against 9.1 ms for 15 M records)
    hipStream_t s2 = s;
    HIPCHK(c, hipMemcpyAsync((void*)(c->d.tid + o), b.tid, n * 4, hipMemcpyHostToDevice, s));
    HIPCHK(c, hipMemcpyAsync((void*)(c->d.pos + o), b.pos, n * 4, hipMemcpyHostToDevice, s2));
    HIPCHK(c, hipMemcpyAsync((void*)(c->d.mtid + o), b.mtid, n * 4, hipMemcpyHostToDevice, s));
    HIPCHK(c, hipMemcpyAsync((void*)(c->d.mpos + o), b.mpos, n * 4, hipMemcpyHostToDevice, s2));
    HIPCHK(c, hipMemcpyAsync((void*)(c->d.isize + o), b.isize, n * 4, hipMemcpyHostToDevice, s));
    HIPCHK(c, hipMemcpyAsync((void*)(c->d.flag + o), b.flag, n * 2, hipMemcpyHostToDevice, s2));
    HIPCHK(c, hipMemcpyAsync((void*)(c->d.mapq + o), b.mapq, n, hipMemcpyHostToDevice, s2));
    // (with one library / one source file the kernels take every index as 0 and do not read the column)
    if (c->nlibs > 1) HIPCHK(c, hipMemcpyAsync((void*)(c->d.lib + o), b.lib, n, hipMemcpyHostToDevice, s2));
    if (c->nbams > 1) HIPCHK(c, hipMemcpyAsync((void*)(c->d.bam + o), b.bam, n, hipMemcpyHostToDevice, s2));
    // name keys and read lengths are only needed for the anomalous reads (about 1 %): pinned ones stay where they are
    const uint64_t* dev_view = nullptr;
    const uint16_t* dev_qlen = nullptr;
    const uint64_t* dev_check = nullptr;
    if (lazy_keys && c->key_segs.size() < 64) {
        auto device_view = [](const void* hp) -> void* {
            hipPointerAttribute_t attr{};
            void* dp = nullptr;
            if (hipPointerGetAttributes(&attr, hp) == hipSuccess && attr.type == hipMemoryTypeHost &&
                hipHostGetDevicePointer(&dp, (void*)hp, 0) == hipSuccess)
                return dp;
            (void)hipGetLastError();  // ordinary pageable memory: not an error
            return nullptr;
        };
        dev_view = (const uint64_t*)device_view(b.name_key);
        dev_qlen = dev_view ? (const uint16_t*)device_view(b.qlen) : nullptr;
        if (dev_qlen && c->use_check) dev_check = (const uint64_t*)device_view(b.name_check);
        if (!dev_qlen || (c->use_check && !dev_check)) dev_view = nullptr;
    }
    if (!dev_view) {
        HIPCHK(c, hipMemcpyAsync((void*)(c->d.key + o), b.name_key, n * 8, hipMemcpyHostToDevice, s2));
        HIPCHK(c, hipMemcpyAsync((void*)(c->d.qlen + o), b.qlen, n * 2, hipMemcpyHostToDevice, s));
        if (c->use_check) HIPCHK(c, hipMemcpyAsync((void*)(c->d.check + o), b.name_check, n * 8, hipMemcpyHostToDevice, s2));
    }
    if (c->key_segs.empty() || dev_view || c->key_segs.back().host)
        c->key_segs.push_back(bdx_ctx::KeySeg{(uint64_t)o, dev_view, dev_qlen, dev_check});
    HIPCHK(c, hipEventRecord(c->ev_copy, s));
    c->copy_pending = true;
    c->n += n;
    c->ran = false;
    if (o == 0) c->dup_done = false;
    if (c->k1_live) {
        const uint32_t full = (uint32_t)(c->n / kTile);
        if (full >= c->k1_done + kStreamTilesMin) {
            HIPCHK(c, hipStreamWaitEvent(c->stream, c->ev_copy, 0));
            c->copy_pending = false;
            BDX_TRY(pass1_classify(c, full, false));
        }
    }
    return BDX_OK;
}

}  // namespace

extern "C" {

void bdx_opts_default(bdx_opts* o) {  // common/Options.cpp:27-41
    if (!o) return;
    o->min_len = 7; o->cut_sd = 3; o->max_sd = 1000000000; o->min_map_qual = 35; o->min_read_pair = 2;
    o->seq_coverage_lim = 1000; o->buffer_size = 100; o->transchr_rearrange = 0; o->fisher = 0;
    o->illumina_long_insert = 0; o->cn_lib = 0; o->print_af = 0; o->score_threshold = 30; o->chr_restricted = 0;
}

const char* bdx_strerror(int code) {
    switch (code) {
        case BDX_OK: return "ok";
        case BDX_EINVAL: return "invalid argument";
        case BDX_ENOMEM: return "out of memory";
        case BDX_EHIP: return "HIP runtime error";
        case BDX_ESTATE: return "call out of order";
        case BDX_ELIMIT: return "limit exceeded";
        default: return "internal error";
    }
}
const char* bdx_last_error(const bdx_ctx* ctx) { return ctx ? ctx->err.c_str() : ""; }
int bdx_device(const bdx_ctx* ctx) { return ctx ? ctx->device : -1; }
void* bdx_stream(const bdx_ctx* ctx) { return ctx ? (void*)ctx->stream : nullptr; }

int bdx_create(bdx_ctx** out, const bdx_opts* opts, const bdx_lib* libs, int nlibs, int nbams, int ntids,
               int max_read_window_size0, int device) {
    if (!out || !opts || !libs || nlibs < 1 || nbams < 1) return BDX_EINVAL;
    if (nlibs > 255 || nbams > 254) return BDX_ELIMIT;
    const int nkeys = opts->cn_lib ? nlibs : nbams;
    if (nkeys > 60) return BDX_ELIMIT;
    for (int i = 0; i < nlibs; ++i)
        if (libs[i].bam_index < 0 || libs[i].bam_index >= nbams) return BDX_EINVAL;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device < 0 || device >= ndev) return BDX_EHIP;
    if (hipSetDevice(device) != hipSuccess) return BDX_EHIP;
    std::unique_ptr<bdx_ctx> c(new (std::nothrow) bdx_ctx);   // (a failure below frees what the context holds by then)
    if (!c) return BDX_ENOMEM;
    c->device = device;
    c->opts = *opts;
    c->libs.assign(libs, libs + nlibs);
    c->nlibs = nlibs; c->nbams = nbams; c->ntids = ntids; c->nkeys = nkeys; c->w0 = max_read_window_size0;
    if (c->stream.create(hipStreamNonBlocking) != hipSuccess) return BDX_EHIP;
    for (auto& e : c->ev)
        if (e.create() != hipSuccess) return BDX_EHIP;
    if (c->copy_stream.create(hipStreamNonBlocking) != hipSuccess) return BDX_EHIP;
    if (c->ev_copy.create(hipEventDisableTiming) != hipSuccess) return BDX_EHIP;
    for (auto& st : c->ring)
        if (st.done.create(hipEventDisableTiming) != hipSuccess) return BDX_EHIP;
    if (c->ev_groups.create(hipEventDisableTiming) != hipSuccess) return BDX_EHIP;
    if (c->ev_regions.create(hipEventDisableTiming) != hipSuccess) return BDX_EHIP;
    std::vector<DevLib> dl(nlibs);
    for (int i = 0; i < nlibs; ++i) {
        dl[i].upper = libs[i].uppercutoff;
        dl[i].lower = libs[i].lowercutoff;
        dl[i].min_mapq = resolved_min_mapq(*opts, libs[i]);
        dl[i].key = opts->cn_lib ? i : libs[i].bam_index;
    }
    std::vector<float> means(nlibs);
    for (int i = 0; i < nlibs; ++i) means[i] = libs[i].mean_insertsize;
    if (c->b_libs.ensure(nlibs * sizeof(DevLib)) != hipSuccess ||
        hipMemcpy(c->b_libs.p, dl.data(), nlibs * sizeof(DevLib), hipMemcpyHostToDevice) != hipSuccess ||
        c->b_lib_mean.ensure(nlibs * 4) != hipSuccess ||
        hipMemcpy(c->b_lib_mean.p, means.data(), nlibs * 4, hipMemcpyHostToDevice) != hipSuccess)
        return BDX_EHIP;
    *out = c.release();
    return BDX_OK;
}

// What is about ORDER; the buffers, events and streams themselves go with the context's members (see the head of bdx_ctx).
void bdx_destroy(bdx_ctx* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->copy_stream) (void)hipStreamSynchronize(c->copy_stream);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    delete c;
}

int bdx_reserve(bdx_ctx* c, size_t n_reads) {
    if (!c) return BDX_EINVAL;
    if (c->adopted) return fail(c, BDX_ESTATE, "reads were adopted from the caller");
    NOT_WHILE_SIZING(c);
    HIPCHK(c, hipSetDevice(c->device));
    BDX_TRY(alloc_reads(c, n_reads));
    // The buffers of the stages behind pass 1 as well, for the prior a first run sizes them by (1/32 of the reads anomalous, see
    // plan_sizing): ~60 device and pinned allocations, 3-4 ms at 15 M reads, most of it page pinning -- here they happen while the
    // caller still decodes or copies, not inside its first bdx_run.  Small inputs size theirs exactly, when they run.
    if (n_reads >= (1u << 20) && !c->ran) {
        const uint64_t prior = prior_anomalous(n_reads);
        if (prior <= kMaxAnomalous) return presize_stages_here(c, stage_dims(c, (uint32_t)prior));
    }
    return BDX_OK;
}

int bdx_push(bdx_ctx* c, const bdx_batch* b) {
    if (!c || !b) return BDX_EINVAL;
    if (c->adopted) return fail(c, BDX_ESTATE, "reads were adopted from the caller");
    if (b->n == 0) return BDX_OK;
    if (!b->tid || !b->pos || !b->mtid || !b->mpos || !b->isize || !b->flag || !b->qlen || !b->mapq || !b->lib || !b->bam ||
        !b->name_key || (c->use_check && !b->name_check))
        return fail(c, BDX_EINVAL, "null array in batch");
    HIPCHK(c, hipSetDevice(c->device));
    return enqueue_batch(c, *b, true);
}

int bdx_acquire_batch(bdx_ctx* c, size_t capacity, bdx_batch_buf* out) {
    if (!c || !out || capacity == 0) return BDX_EINVAL;
    if (c->adopted) return fail(c, BDX_ESTATE, "reads were adopted from the caller");
    if (c->ring_cur >= 0) return fail(c, BDX_ESTATE, "the previous batch was not submitted");
    HIPCHK(c, hipSetDevice(c->device));
    bdx_ctx::Stage& st = c->ring[c->ring_next];
    if (st.busy) {  // all staging buffers are in flight: wait for the oldest copy
        HIPCHK(c, hipEventSynchronize(st.done));
        st.busy = false;
    }
    st.cap = round_up(capacity, 64);
    HIPCHK(c, st.buf.ensure(st.cap * 43 + 64));
    stage_view(st, out);
    c->ring_cur = c->ring_next;
    c->ring_next = (c->ring_next + 1) % 4;
    return BDX_OK;
}

int bdx_submit_batch(bdx_ctx* c, size_t n) {
    if (!c) return BDX_EINVAL;
    if (c->ring_cur < 0) return fail(c, BDX_ESTATE, "no batch was acquired");
    bdx_ctx::Stage& st = c->ring[c->ring_cur];
    c->ring_cur = -1;
    if (n == 0) return BDX_OK;
    HIPCHK(c, hipSetDevice(c->device));
    bdx_batch_buf v{};
    stage_view(st, &v);  // the layout bdx_acquire_batch handed out
    if (n > v.capacity) return fail(c, BDX_EINVAL, "more records than the acquired batch holds");
    bdx_batch b{v.tid, v.pos, v.mtid, v.mpos, v.isize, v.flag, v.qlen, v.mapq, v.lib, v.bam, v.name_key, n, v.name_check};
    BDX_TRY(enqueue_batch(c, b, false));  // (the buffer is recycled: its name keys travel with the other columns)
    HIPCHK(c, hipEventRecord(st.done, c->copy_stream));
    st.busy = true;
    return BDX_OK;
}

int bdx_reset_reads(bdx_ctx* c) {
    if (!c) return BDX_EINVAL;
    HIPCHK(c, hipSetDevice(c->device));
    if (c->copy_stream) HIPCHK(c, hipStreamSynchronize(c->copy_stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (c->adopted) {
        c->d = ReadsSoA{};
        c->cap = 0;
        c->adopted = false;
    }
    if (c->use_clips && c->b_clip.p) {   // the next load's rows start from 0 again: all of them (a decoder that gave up may have written beyond n)
        HIPCHK(c, hipMemsetAsync(c->b_clip.p, 0, c->cap * 4, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    c->n = 0;
    c->ran = false;
    c->dup_done = false;
    c->cls_n = (size_t)-1;
    c->k1_live = false;
    c->k1_done = 0;
    c->copy_pending = false;
    c->key_segs.clear();
    c->ring_cur = -1;
    for (auto& st : c->ring) st.busy = false;
    return BDX_OK;
}

int bdx_set_device_reads(bdx_ctx* c, const bdx_batch* b) {
    if (!c || !b) return BDX_EINVAL;
    if (c->n && !c->adopted) return fail(c, BDX_ESTATE, "context already holds pushed reads");
    if (c->use_clips) return fail(c, BDX_ESTATE, "an adopted store cannot carry clip words (bdx_use_clips is on)");
    const void* ptrs[] = {b->tid, b->pos, b->mtid, b->mpos, b->isize, b->flag, b->qlen, b->mapq, b->lib, b->bam, b->name_key,
                          c->use_check ? (const void*)b->name_check : (const void*)b->name_key};
    for (const void* p : ptrs)
        if (b->n && (!p || ((uintptr_t)p & 15))) return fail(c, BDX_EINVAL, "device arrays must be non-null and 16-byte aligned");
    c->d.tid = b->tid; c->d.pos = b->pos; c->d.mtid = b->mtid; c->d.mpos = b->mpos; c->d.isize = b->isize;
    c->d.flag = b->flag; c->d.qlen = b->qlen; c->d.mapq = b->mapq; c->d.lib = b->lib; c->d.bam = b->bam; c->d.key = b->name_key;
    c->d.check = c->use_check ? b->name_check : nullptr;
    c->n = b->n;
    c->cap = b->n;
    c->adopted = true;
    c->ran = false;
    c->dup_done = false;
    c->cls_n = (size_t)-1;
    c->k1_live = false;
    c->key_segs.clear();
    return BDX_OK;
}

// ---------------------------------------------------------------------------------------------------------
// Stages.  bdx_run chains them on one context; a sharded run (bdx_dist_impl.h) runs the same stages per rank and
// exchanges the few global quantities between them.
// ---------------------------------------------------------------------------------------------------------
}  // extern "C"

namespace {

// Spin on a word of pinned host memory that a kernel sets once its results are written there.  Much shorter than the
// wake-up of a blocking stream / event wait; falls back to the caller's blocking wait if the word does not show up.
bool wait_flag(const bdx_ctx* c, ReadyWord w, uint32_t value) {
    if (!c->poll || !c->h_flags.p) return false;
    volatile uint32_t* f = (volatile uint32_t*)c->h_flags.p + w;
    const auto t0 = std::chrono::steady_clock::now();
    for (uint32_t spin = 0;; ++spin) {
        if (*f == value) { std::atomic_thread_fence(std::memory_order_acquire); return true; }
        __builtin_ia32_pause();
        if ((spin & 1023u) == 1023u && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(200)) return false;
    }
}

// The count of anomalous reads, ahead of the pass-1 record: finalize_kernel's chunk totals, posted while finalize2_kernel has yet to
// run.  Every word carries the run's sequence number in its high half, so a word of an earlier run (or of the launch a too-small guess
// repeated) does not pass for this one's.  false: not posted, polling off or not there in time -- the caller waits for the record.
bool wait_count(const bdx_ctx* c, uint64_t* n_anom) {
    if (!c->poll || !c->h_count.p || !c->count_chunks) return false;
    const volatile uint64_t* w = (const volatile uint64_t*)c->h_count.p;
    const uint32_t nchunk = c->count_chunks;
    const auto t0 = std::chrono::steady_clock::now();
    uint64_t sum = 0;
    uint32_t g = 0;
    for (uint32_t spin = 0; g < nchunk; ++spin) {
        const uint64_t v = w[g];   // (one aligned 8-byte load: value and stamp together)
        if ((uint32_t)(v >> 32) == c->seq) { sum += (uint32_t)v; ++g; continue; }
        __builtin_ia32_pause();
        if ((spin & 1023u) == 1023u && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(200)) return false;
    }
    std::atomic_thread_fence(std::memory_order_acquire);
    *n_anom = sum;
    return true;
}

// behind a poll that timed out and a stream that has drained: was the word written at all?  (A kernel that was never launched -- a
// launch that failed, a stage that returned early -- leaves zeros where its results should be; they must not pass for an empty input.)
// always_set: the word is written whether or not the host polls for it, so it is looked at without polling too (the pass-1 record's)
bool flag_arrived(const bdx_ctx* c, ReadyWord w, bool always_set = false) {
    return (!c->poll && !always_set) || !c->h_flags.p || ((volatile uint32_t*)c->h_flags.p)[w] == c->seq;
}

// The wait for a ready word of this run: poll; failing that, wait for `ev` (polling off, and the caller recorded one in the word's place:
// signal_ready) or else for the stream; then the word must be there, or the run fails with `missing`.
int await_ready(bdx_ctx* c, ReadyWord w, hipEvent_t ev, const char* missing, bool always_set = false) {
    if (wait_flag(c, w, c->seq)) return BDX_OK;
    hipStream_t s = c->stream;
    if (!c->poll && ev) HIPCHK(c, hipEventSynchronize(ev)); else HIPCHK(c, hipStreamSynchronize(s));
    return flag_arrived(c, w, always_set) ? BDX_OK : fail(c, BDX_EINTERNAL, missing);
}

// Tell the host that everything enqueued so far has completed: a stream write-value into a polled pinned word, or (polling
// off / the stream operation unavailable) an event.  The word must be written AFTER a kernel boundary behind the kernels
// whose results it announces (their stores to host memory come from several compute dies; only the end of the kernel
// orders them).  On this runtime the write-value command is itself a one-thread kernel (__amd_rocclr_streamOpsWrite in
// the kernel trace, ~4 us on the stream), so where another kernel follows anyway its first thread sets the word instead
// (K6Arrays::flag_regions / flag_groups); the command remains for the end of the run.
int signal_ready(bdx_ctx* c, ReadyWord w, hipEvent_t ev) {
    if (c->poll) {
        if (hipStreamWriteValue32(c->stream, c->h_flags.as<uint32_t>() + w, c->seq, 0) == hipSuccess) return BDX_OK;
        (void)hipGetLastError();
        c->poll = false;  // not supported here: blocking waits from now on
    }
    if (ev) {
        hipError_t e = hipEventRecord(ev, c->stream);
        if (e != hipSuccess) return hipfail(c, e, "hipEventRecord");
    }
    return BDX_OK;
}

float ms_between(std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) {
    return std::chrono::duration<float, std::milli>(b - a).count();
}


// The segment table of the name keys (read lengths, second hashes) that the caller's pinned batches still hold (bdx_push), in b_seg:
// [ns + 1] segment begins | [ns] key pointers | [ns] read-length pointers | [ns] second-hash pointers, each biased by -begin; a segment
// that was copied points into the resident column.  *ns = 0: every key is in the resident column.
int upload_key_segs(bdx_ctx* c, size_t* ns_out) {
    *ns_out = 0;
    bool any_host = false;
    for (auto const& sg : c->key_segs) any_host |= sg.host != nullptr;
    if (!any_host || c->adopted) return BDX_OK;
    const size_t ns = c->key_segs.size();
    std::vector<uint64_t> tab(4 * ns + 1);
    for (size_t i = 0; i < ns; ++i) {
        const bdx_ctx::KeySeg& sg = c->key_segs[i];
        tab[i] = sg.begin;
        tab[ns + 1 + i] = (uint64_t)(uintptr_t)(sg.host ? sg.host - sg.begin : c->d.key);
        tab[2 * ns + 1 + i] = (uint64_t)(uintptr_t)(sg.host ? sg.host_qlen - sg.begin : c->d.qlen);
        tab[3 * ns + 1 + i] = (uint64_t)(uintptr_t)(sg.host ? sg.host_check - sg.begin : c->d.check);
    }
    tab[ns] = c->n;
    HIPCHK(c, c->b_seg.ensure(tab.size() * 8));
    HIPCHK(c, hipMemcpyAsync(c->b_seg.p, tab.data(), tab.size() * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));  // (tab is a local; this path is PCIe-bound anyway)
    *ns_out = ns;
    return BDX_OK;
}

// KD over columns in HBM: scan, the table for the runs longer than kDupT (sized from the work list's count, which the host reads), then
// the marks into `flag` (the words that change) and / or `mask` (a byte per record).  The counts are added to *marked / *groups.
int kd_run(bdx_ctx* c, KdParams p, KdScratch& k, uint16_t* flag, uint8_t* mask, hipStream_t s, uint64_t* marked, uint64_t* groups) {
    if (!p.n) return BDX_OK;
    const size_t nwords = (p.n + 63) / 64;
    HIPCHK(c, k.bits.ensure(nwords * 8));
    HIPCHK(c, k.longbits.ensure(nwords * 8));
    HIPCHK(c, k.cnt.ensure(sizeof(KdCounts)));
    p.bits = k.bits.as<uint64_t>(); p.longbits = k.longbits.as<uint64_t>(); p.cnt = k.cnt.as<KdCounts>();
    HIPCHK(c, hipMemsetAsync(p.cnt, 0, sizeof(KdCounts), s));
    launch_kd_scan(p, s);
    HIPCHK(c, hipGetLastError());
    KdCounts h{};
    HIPCHK(c, hipMemcpyAsync(&h, p.cnt, sizeof(h), hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    if (h.nwork) {
        if (h.nwork > (1u << 30)) return fail(c, BDX_ELIMIT, "more than 2^30 duplicate candidates in runs too long for direct comparison");
        uint64_t slots = 1024;
        while (slots < 2 * (uint64_t)h.nwork) slots <<= 1;
        HIPCHK(c, k.work.ensure((size_t)h.nwork * 4));
        HIPCHK(c, k.wrun.ensure((size_t)h.nwork * 4));
        HIPCHK(c, k.starts.ensure(nwords * 8));
        HIPCHK(c, k.pre.ensure(nwords * 4));
        HIPCHK(c, k.cbase.ensure((size_t)kd_chunks(p.n) * 4));
        HIPCHK(c, k.table.ensure(slots * 4));
        HIPCHK(c, k.multi.ensure(slots * 4));
        p.work = k.work.as<uint32_t>(); p.wrun = k.wrun.as<uint32_t>(); p.starts = k.starts.as<uint64_t>();
        p.pre = k.pre.as<uint32_t>(); p.cbase = k.cbase.as<uint32_t>();
        p.table = k.table.as<uint32_t>(); p.multi = k.multi.as<uint32_t>(); p.tmask = slots - 1;
        launch_kd_long(p, h.nwork, s);
        HIPCHK(c, hipGetLastError());
    }
    launch_kd_apply(p, flag, mask, s);
    HIPCHK(c, hipGetLastError());
    if (h.nwork) {
        HIPCHK(c, hipMemcpyAsync(&h, p.cnt, sizeof(h), hipMemcpyDeviceToHost, s));
        HIPCHK(c, hipStreamSynchronize(s));
        if (h.nlist != h.nwork) return fail(c, BDX_EINTERNAL, "duplicate marking: the work list does not hold the candidates that were counted");
        k.release_long();   // (the stream has drained)
    }
    *marked += h.marked; *groups += h.groups;
    return BDX_OK;
}

// bdx_set_mark_duplicates: KD over the store at the head of a pass 1 that starts from tile 0, once per load
int mark_duplicates(bdx_ctx* c) {
    if (c->dup_done) return BDX_OK;   // (nothing was appended since: enqueue_batch and the gathers refuse that)
    c->dup_marked = 0; c->dup_groups = 0;
    hipStream_t s = c->stream;
    if (c->adopted && (const void*)c->d.flag != c->b_flag.p) {   // the caller's arrays are const: a private copy of the flag column takes the marks
        HIPCHK(c, c->b_flag.ensure(c->n * 2));
        HIPCHK(c, hipMemcpyAsync(c->b_flag.p, c->d.flag, c->n * 2, hipMemcpyDeviceToDevice, s));
        c->d.flag = c->b_flag.as<uint16_t>();
    }
    KdParams p{};
    p.tid = c->d.tid; p.pos = c->d.pos; p.mtid = c->d.mtid; p.mpos = c->d.mpos; p.flag = c->d.flag;
    p.lib = c->nlibs > 1 ? c->d.lib : nullptr;   // (with one library the column is not copied)
    p.key = c->d.key; p.n = c->n;
    size_t ns = 0;
    BDX_TRY(upload_key_segs(c, &ns));
    if (ns) {
        p.nseg = (int)ns;
        p.seg_begin = c->b_seg.as<uint64_t>();
        p.seg_ptr = (const uint64_t* const*)(c->b_seg.as<uint64_t>() + ns + 1);
    }
    BDX_TRY(kd_run(c, p, c->kd, (uint16_t*)c->d.flag, nullptr, s, &c->dup_marked, &c->dup_groups));
    c->dup_done = true;
    return BDX_OK;
}

// Start of a pass 1: per-tile tables laid out for tiles_cap tiles, counters and tables at their start values.
int pass1_prepare(bdx_ctx* c, uint32_t tiles_cap) {
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t s = c->stream;
    const int nlibs = c->nlibs, nbams = c->nbams, nkeys = c->nkeys;
    const int ncols = 2 + nkeys, ncnt = nlibs * kNumFlags + nlibs + nbams;
    const uint32_t tstride = (uint32_t)round_up(std::max<uint32_t>(tiles_cap, 16), 16);
    c->tstride = tstride;
    c->k1_cap_tiles = tiles_cap;
    c->k1_done = 0;
    HIPCHK(c, c->b_cls.ensure(std::max<size_t>((size_t)tiles_cap * kTile, 16)));
    // K1's ready-made records for K2: 2 B per read of address space, written (and later read) only where reads are anomalous
    c->use_stash = !c->dbg_no_stash && nkeys <= kStashKeys;   // (no_stash: K2 gathers everything from the columns)
    if (c->use_stash) HIPCHK(c, c->b_stash.ensure(std::max<size_t>((size_t)tiles_cap * kStashCap * sizeof(StashRec), 64)));
    HIPCHK(c, c->b_tile_tot.ensure((size_t)ncols * tstride * 4));
    HIPCHK(c, c->b_tile_pre.ensure((size_t)ncols * tstride * 4));
    HIPCHK(c, c->b_tile_mono.ensure((size_t)nbams * tstride * sizeof(MonoRec)));
    HIPCHK(c, c->b_blk_cnt.ensure((size_t)kCntCopies * ncnt * 4));
    HIPCHK(c, c->b_cnt.ensure((size_t)ncnt * 4));
    HIPCHK(c, c->b_p1.ensure(sizeof(Pass1)));
    HIPCHK(c, c->h_p1.ensure(sizeof(Pass1)));
    HIPCHK(c, c->h_cnt.ensure((size_t)ncnt * 4));
    HIPCHK(c, c->h_counts.ensure(sizeof(StageCounts)));
    HIPCHK(c, c->b_counts.ensure(sizeof(StageCounts)));
    HIPCHK(c, c->h_count.ensure((size_t)kMaxChunks * 8));
    const size_t w_tot = (size_t)ncols * tstride, w_mono = (size_t)nbams * tstride * sizeof(MonoRec) / 4;
    if (w_tot > 0xFFFFFFFFull || w_mono > 0xFFFFFFFFull) {  // beyond the init kernel's 32-bit word counts
        HIPCHK(c, hipMemsetAsync(c->b_tile_tot.p, 0, w_tot * 4, s));
        HIPCHK(c, hipMemsetAsync(c->b_tile_mono.p, 0xFF, w_mono * 4, s));
    }
    InitList il{};
    int k = 0;
    auto add = [&](void* p, size_t words, uint32_t value) { il.ptr[k] = (uint32_t*)p; il.words[k] = (uint32_t)words; il.value[k] = value; ++k; };
    if (w_tot <= 0xFFFFFFFFull && w_mono <= 0xFFFFFFFFull) { add(c->b_tile_tot.p, w_tot, 0u); add(c->b_tile_mono.p, w_mono, 0xFFFFFFFFu); }
    add(c->b_blk_cnt.p, (size_t)kCntCopies * ncnt, 0u);
    add(c->b_p1.p, sizeof(Pass1) / 4, 0u);
    add(c->b_counts.p, sizeof(StageCounts) / 4, 0u);
    il.n = k;
    launch_init(il, s);
    return BDX_OK;
}

// K1 over the tiles [k1_done, upto) of the c->n reads that are (or, behind ev_copy, will be) in HBM
int pass1_classify(bdx_ctx* c, uint32_t upto, bool timed) {
    hipStream_t s = c->stream;
    if (upto <= c->k1_done) return BDX_OK;
    K1Params k1{};
    k1.r = c->d; k1.n = c->n; k1.ntiles = upto; k1.tstride = c->tstride; k1.tile0 = c->k1_done;
    k1.nlibs = c->nlibs; k1.nbams = c->nbams; k1.nkeys = c->nkeys;
    k1.max_sd = c->opts.max_sd; k1.opt_t = c->opts.transchr_rearrange; k1.opt_l = c->opts.illumina_long_insert;
    k1.libs = c->b_libs.as<DevLib>(); k1.cls = c->b_cls.as<uint8_t>(); k1.tile_tot = c->b_tile_tot.as<uint32_t>();
    k1.tile_mono = c->b_tile_mono.as<MonoRec>();
    k1.blk_cnt = c->b_blk_cnt.as<uint32_t>();
    k1.stash = c->use_stash ? c->b_stash.as<StashRec>() : nullptr;
    const uint32_t span = upto - c->k1_done;
    const int grid1 = (int)std::min<uint32_t>((span + kWaves - 1) / kWaves, (uint32_t)kK1MaxGrid);
    launch_k1(k1, grid1, k1_lds_bytes(c->nlibs, c->nbams, c->nkeys), s, timed ? c->ev[0] : nullptr, timed ? c->ev[1] : nullptr);
    c->k1_done = upto;
    return BDX_OK;
}

// K1 + finalize: class bytes, per-tile tables, *local* pass-1 counters.  Enqueues only: wait_pass1 receives the record.
struct Pass1Launch {
    uint32_t na_cap = 0;        // enqueue-ahead: the count the later stages behind this launch were sized for (finalize2_kernel neutralises them beyond it)
    bool defer_second = false;  // ... and K2's launch takes the second level of the finalisation along
    bool post_count = false;    // finalize_kernel also posts the chunk totals of anomalous reads to h_count (the caller reads them with wait_count)
};
// the finalisation behind K1 over c->ntiles tiles: a new run sequence number, the scan of the tile totals, the record and the counters
int pass1_finalize(bdx_ctx* c, const Pass1Launch& opt) {
    const int nlibs = c->nlibs, nbams = c->nbams, nkeys = c->nkeys;
    const int ncols = 2 + nkeys, ncnt = nlibs * kNumFlags + nlibs + nbams;
    const uint32_t ntiles = c->ntiles;
    FinalizeParams fp{};
    fp.ntiles = ntiles; fp.tstride = c->tstride; fp.nblk = 0;
    fp.nfold = std::max<uint32_t>(1, std::min<uint32_t>(64, (ntiles + 1023) / 1024));
    HIPCHK(c, c->b_fold.ensure((size_t)nbams * fp.nfold * sizeof(MonoRec)));
    fp.fold_part = c->b_fold.as<MonoRec>();
    fp.nlibs = nlibs; fp.nbams = nbams; fp.nkeys = nkeys; fp.ncols = ncols; fp.ncnt = ncnt; fp.w0 = c->w0;
    fp.tile_tot = c->b_tile_tot.as<uint32_t>(); fp.tile_pre = c->b_tile_pre.as<uint32_t>(); fp.tile_mono = c->b_tile_mono.as<MonoRec>();
    {   // the tile-total columns are scanned in chunks of whole rounds of a workgroup (4096 super tiles), at most kMaxChunks of them
        const uint32_t nsuper = (ntiles + kK2TilesPerWave - 1) / kK2TilesPerWave;
        const uint32_t round = 4096;
        const uint32_t rounds = std::max<uint32_t>(1, (nsuper + round - 1) / round);
        // (tests: chunks of several rounds at small sizes)
        const uint32_t max_chunks = c->dbg_max_chunks > 0 ? (uint32_t)std::min(c->dbg_max_chunks, (int)kMaxChunks) : (uint32_t)kMaxChunks;
        fp.chunk_super = round * ((rounds + max_chunks - 1) / max_chunks);
        fp.nchunk = std::max<uint32_t>(1, (nsuper + fp.chunk_super - 1) / fp.chunk_super);
        HIPCHK(c, c->b_chunk_tot.ensure((size_t)ncols * kMaxChunks * 8));
        fp.chunk_tot = c->b_chunk_tot.as<uint32_t>();
        fp.chunk_base = fp.chunk_tot + (size_t)ncols * kMaxChunks;
    }
    fp.blk_cnt = c->b_blk_cnt.as<uint32_t>(); fp.cnt = c->b_cnt.as<uint32_t>(); fp.p1 = c->b_p1.as<Pass1>();
    HIPCHK(c, c->b_kdens.ensure(64 * 4));
    fp.libs = c->b_libs.as<DevLib>(); fp.cn_lib = c->opts.cn_lib; fp.key_density = c->b_kdens.as<float>();
    fp.cnt_host = c->h_cnt.as<uint32_t>(); fp.p1_host = c->h_p1.as<Pass1>();  // written by the kernel: no copy commands
    memset(c->h_p1.p, 0, sizeof(Pass1));
    HIPCHK(c, c->h_flags.ensure(64));
    ++c->seq;
    fp.flag_host = c->h_flags.as<uint32_t>(); fp.flag_value = c->seq;
    fp.na_cap = opt.na_cap;
    fp.count_host = opt.post_count && c->poll ? c->h_count.as<uint64_t>() : nullptr; fp.count_stamp = c->seq;
    c->count_chunks = fp.count_host ? fp.nchunk : 0;
    // enqueue-ahead: K2 follows without a host decision in between, so its launch takes the one-workgroup second level along
    c->fp_deferred = fp;
    c->finalize2_deferred = opt.defer_second;
    launch_finalize(fp, c->stream, !opt.defer_second);
    return BDX_OK;
}

int do_pass1(bdx_ctx* c, const Pass1Launch& opt) {
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t s = c->stream;
    if (c->n >= ((size_t)1 << 32)) return fail(c, BDX_ELIMIT, "more than 2^32 - 1 reads in one context (read indices and the prefix counters are 32-bit)");
    const uint32_t ntiles = (uint32_t)((c->n + kTile - 1) / kTile);
    c->ntiles = ntiles;
    c->ran = false; c->replayed = false;
    c->cls_n = (size_t)-1;
    c->na_alloc = 0;
    c->regions.clear(); c->r_pk.clear(); c->parts.clear();
    c->reg = nullptr; c->nreg = 0; c->rpk = nullptr;
    c->walk.clear();
    if (!c->walk_scratch) c->walk_scratch.reset(walk_scratch_new());
    c->n_printed = 0;
    memset(&c->counts, 0, sizeof(c->counts));
    for (float& m : c->stage_ms) m = 0;

    if (c->copy_pending) {  // batches pushed since the last classifier launch
        HIPCHK(c, hipStreamWaitEvent(s, c->ev_copy, 0));
        c->copy_pending = false;
    }
    // a store that was filled from empty has its first tiles classified already; anything else starts from tile 0
    if (!(c->k1_live && c->k1_cap_tiles >= ntiles)) {
        BDX_TRY(pass1_prepare(c, ntiles));
    }
    c->k1_live = false;  // (consumed: a repeated run classifies everything again)
    if (c->mark_dup && c->k1_done == 0) {   // classification starts from tile 0: the marks are in the flag column before K1 reads it
        BDX_TRY(mark_duplicates(c));
    }
    const bool time_k1 = (c->stage_timing || c->seq % kK1EventPeriod == 0) && c->k1_done == 0 && ntiles > 0;
    BDX_TRY(pass1_classify(c, ntiles, time_k1));
    BDX_TRY(pass1_finalize(c, opt));
    c->k1_timed = time_k1;
    return BDX_OK;
}

// the pass-1 record and counters, written into pinned memory by finalize2_kernel
int wait_pass1(bdx_ctx* c) {
    const int ncnt = c->nlibs * kNumFlags + c->nlibs + c->nbams;
    // (always_set: the word is set by the kernel that writes the record, whether or not the host polls for it: a stream that has drained
    // without it means that kernel was never launched -- an empty pass-1 record must not pass for a BAM without reads)
    BDX_TRY(await_ready(c, kPass1Ready, nullptr, "the pass-1 record did not arrive: its kernel was not launched", /*always_set=*/true));
    c->p1 = *c->h_p1.as<Pass1>();
    c->cnt_local.assign(c->h_cnt.as<uint32_t>(), c->h_cnt.as<uint32_t>() + ncnt);
    if (c->k1_timed) {
        float ms = 0;
        if (hipEventElapsedTime(&ms, c->ev[0], c->ev[1]) == hipSuccess) c->k1_ms_last = ms;
    }
    c->stage_ms[kMsClassify] = c->k1_ms_last;  // the latest measured launch
    if (c->p1.n_anom > kMaxAnomalous) return fail(c, BDX_ELIMIT, "more than 2^31 anomalous reads in one context");
    // capacity of the later stages (an enqueue-ahead run has set its guess already)
    if (!c->na_alloc && c->p1.n_anom) c->na_alloc = (uint32_t)std::min<uint64_t>(with_headroom(c->p1.n_anom), kMaxAnomalous);
    c->cls_n = c->n;
    return BDX_OK;
}

// final window from the (global) counters: BreakDancerMax.cpp:109-116
int32_t window_from(const bdx_ctx* c, const uint32_t* cnt, uint32_t covered) {
    int W = c->w0;
    for (int i = 0; i < c->nlibs; ++i) {
        const int nd = (int)(cnt[i * kNumFlags + F_LARGE] + cnt[i * kNumFlags + F_SMALL]);
        const int tmp = nd > 0 ? (int)((float)covered / (float)nd) : 50;
        W = std::min(W, tmp);
    }
    return W;
}

// adopt the pass-1 statistics the rest of the path runs with (the context's own, or all-reduced ones)
int set_pass1(bdx_ctx* c, const uint32_t* cnt, uint32_t covered, int32_t window, bool upload) {
    const int nlibs = c->nlibs, nkeys = c->nkeys;
    const int ncnt = nlibs * kNumFlags + nlibs + c->nbams;
    c->cnt.assign(cnt, cnt + ncnt);
    c->g_covered = covered;
    c->g_window = window;
    // host-side scalars of main() (BreakDancerMax.cpp:88-107, BamSummary.cpp:140-149), float32 like the reference
    const uint32_t* lib_cnt = c->cnt.data() + nlibs * kNumFlags;
    const uint32_t* bam_cnt = lib_cnt + nlibs;
    c->seqcov.assign(nlibs, 0.f);
    c->lib_density.assign(nlibs, 0.f);
    c->key_density.assign(nkeys, 0.000001f);
    for (int i = 0; i < nlibs; ++i) {
        float covg = 0;
        if (lib_cnt[i] != 0 && covered != 0) covg = float(lib_cnt[i]) * c->libs[i].readlens / covered;
        c->seqcov[i] = covg;
        float dens = 0.000001f;
        if (c->opts.cn_lib) {
            if (lib_cnt[i] != 0) dens = float(lib_cnt[i]) / covered;
        } else {
            dens = float(bam_cnt[c->libs[i].bam_index]) / covered;
        }
        c->lib_density[i] = dens;
        c->key_density[c->opts.cn_lib ? i : c->libs[i].bam_index] = dens;
    }
    // the region cut reads the window from the device copy of Pass1
    struct { uint32_t covered; int32_t window; } hdr{covered, window};
    static_assert(offsetof(Pass1, covered_ref_len) == 0 && offsetof(Pass1, window) == 4, "Pass1 header layout");
    if (upload) {  // a single-context run adopts its own statistics: the device copy already holds them
        HIPCHK(c, hipMemcpyAsync(c->b_p1.p, &hdr, sizeof(hdr), hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    return BDX_OK;
}

// ---- the size functions: every capacity expression of the later stages' buffers stands here, once ----
#define SZCHK(expr)                                                                                       \
    do {                                                                                                  \
        const hipError_t _e = (expr);                                                                     \
        if (_e != hipSuccess) { *err = std::string(#expr) + ": " + hipGetErrorString(_e); return BDX_EHIP; } \
    } while (0)

// arrays that two stages size (K2 clears what K3 and K4 fill; K3 and the sharded run use K6's scratch): one expression each
hipError_t size_c_maxq(StageBufs& b, size_t cap) { return b.b_c_maxq.ensure(cap * 4); }
hipError_t size_out_deg(StageBufs& b, size_t cap) { return b.b_out_deg.ensure(cap * 6 * 4); }
hipError_t size_join_words(StageBufs& b, size_t n_own, bool pair_lo) {
    const hipError_t e = b.b_partner.ensure(n_own * 4);
    return e == hipSuccess && pair_lo ? b.b_pair_lo.ensure(n_own * 4) : e;
}
// look-back words of a scan (bdx_scan.h): they must start out zero once; afterwards every launch brings its own stamp (next_lb_stamp)
hipError_t size_zero_once(DevBuf& b, size_t bytes, hipStream_t s) {
    if (b.bytes >= bytes) return hipSuccess;
    const hipError_t e = b.ensure(bytes);
    return e == hipSuccess ? hipMemsetAsync(b.p, 0, b.bytes, s) : e;
}

int size_compact(StageBufs& b, const StageDims& d, std::string* err) {
    if (!d.na) return BDX_OK;
    if (d.na > kMaxAnomalous) { *err = "more than 2^31 anomalous reads in one context"; return BDX_ELIMIT; }
    const size_t cap = d.na;
    SZCHK(b.b_c_tid.ensure(cap * 4)); SZCHK(b.b_c_pos.ensure(cap * 4)); SZCHK(b.b_c_isize.ensure(cap * 4));
    SZCHK(b.b_c_meta.ensure(cap * 4)); SZCHK(b.b_c_key.ensure(cap * 8)); SZCHK(b.b_c_nn.ensure(cap * 4));
    SZCHK(b.b_c_idx.ensure(cap * 4));
    if (d.use_check) SZCHK(b.b_c_check.ensure(cap * 8));
    SZCHK(b.b_c_pk.ensure(cap * 4 * d.nkeys));
    SZCHK(size_c_maxq(b, cap));
    if (d.k2_clears_join) {
        SZCHK(b.b_t_key.ensure((size_t)direct_join_slots(d.na) * 8));
        SZCHK(size_join_words(b, cap, true));
    }
    return BDX_OK;
}

int size_cut(StageBufs& b, const StageDims& d, hipStream_t s, std::string* err) {
    if (!d.na) return BDX_OK;
    const size_t cap = d.na;
    for (DevBuf* u : {&b.b_cand, &b.b_pre_q, &b.b_pre_rev, &b.b_pre_nonctx, &b.b_c_first, &b.b_c_rid, &b.b_region_of}) SZCHK(u->ensure(cap * 4));
    SZCHK(size_c_maxq(b, cap));
    // the region table and the group list are written by the kernels straight into pinned host memory: they are write-once,
    // read-never on the device, so the PCIe writes overlap the kernels and no D2H copy is needed
    // (HBM only: no pinned mirror -- pinning 24 chromosomes' tables cost a sharded run tens of milliseconds)
    if (d.regions != RegionDst::Hbm) {
        SZCHK(b.h_regs.ensure(cap * sizeof(RegionRec)));
        SZCHK(b.h_pk.ensure(cap * 2 * d.nkeys * 4));
    }
    SZCHK(b.b_r_rec.ensure(cap * sizeof(RegionRec)));
    SZCHK(b.b_r_pk.ensure(cap * 2 * d.nkeys * 4));
    if (d.regions == RegionDst::HostAndHbm) {   // the device-side SV assembly follows
        SZCHK(size_out_deg(b, cap));
        SZCHK(b.h_counts0.ensure(sizeof(StageCounts)));
    }
    // the two scans' look-back words, for one element per thread (the finest split they use)
    SZCHK(size_zero_once(b.b_lb, 5 * (scan_grid(d.na, 1) + 1) * 8, s));
    return BDX_OK;
}

int size_join(StageBufs& b, const StageDims& d, std::string* err) {
    if (!d.join_n) return BDX_OK;
    if (d.groups_in_hbm) SZCHK(b.b_groups.ensure((size_t)d.join_groups() * sizeof(GroupRec)));   // sharded runs: the groups are packaged for rank 0 from HBM
    else SZCHK(b.h_groups.ensure((size_t)d.join_groups() * sizeof(GroupRec)));
    // (foreign entries of a sharded run have no partner[] / pair_lo[] entry: sized for the context's own reads, as K2 cleared them)
    SZCHK(size_join_words(b, d.join_own, d.join_slots && d.join_pair_lo));
    if (d.join_slots) SZCHK(b.b_t_key.ensure((size_t)d.join_slots * 8));
    return BDX_OK;
}

K6Caps k6_caps(const StageDims& d) { return k6_caps_of(d.k6_regions(), d.nkeys, d.nlibs); }

int size_k6(StageBufs& b, const StageDims& d, hipStream_t s, std::string* err) {
    const size_t cap = d.k6_regions();
    if (!cap) return BDX_OK;
    const K6Caps k = k6_caps(d);
    SZCHK(size_out_deg(b, cap));
    SZCHK(b.b_parts.ensure(cap * sizeof(PartRec)));
    SZCHK(b.b_rs.ensure(cap * sizeof(RegSum)));
    SZCHK(b.b_members.ensure(cap * kK6MaxMembers * sizeof(MemberInfo)));
    SZCHK(b.b_own.ensure(cap * 7 * 4 + 64 * 4 * 4));
    if (d.walks_big()) SZCHK(b.b_member_ids.ensure(cap * kK6BigMembers * 4));
    SZCHK(b.b_slot.ensure(cap * sizeof(SvOut)));
    SZCHK(b.b_lib_stage.ensure(cap * k.lib_stride * sizeof(LibStage)));
    SZCHK(b.b_cn_stage.ensure(cap * (size_t)d.nkeys * sizeof(CnStage) + 16));
    SZCHK(b.b_t_lambda.ensure((size_t)k.term * 8)); SZCHK(b.b_t_k.ensure((size_t)k.term * 4));
    if (d.table_in_hbm) {   // (rank 0 of a sharded run merges the ranks' tables: this one goes there from HBM)
        SZCHK(b.b_sv_out.ensure((size_t)k.sv * sizeof(SvOut))); SZCHK(b.b_sv_key.ensure((size_t)k.sv * 8));
        SZCHK(b.b_lib_index_out.ensure((size_t)k.term * 4)); SZCHK(b.b_lib_pairs_out.ensure((size_t)k.term * 4));
        SZCHK(b.b_cn_key_out.ensure((size_t)k.cn * 4 + 16)); SZCHK(b.b_cn_value_out.ensure((size_t)k.cn * 4 + 16));
        SZCHK(b.b_ltail_out.ensure((size_t)k.term * 8));
    } else {
        SZCHK(b.h_sv_out.ensure((size_t)k.sv * sizeof(SvOut)));
        SZCHK(b.h_lib_index.ensure((size_t)k.term * 4)); SZCHK(b.h_lib_pairs.ensure((size_t)k.term * 4));
        SZCHK(b.h_cn_key.ensure((size_t)k.cn * 4 + 16)); SZCHK(b.h_cn_value.ensure((size_t)k.cn * 4 + 16));
        SZCHK(b.h_ltail_dev.ensure((size_t)k.term * 8));
    }
    SZCHK(b.h_counts2.ensure(sizeof(StageCounts)));
    SZCHK(b.b_sv_src.ensure((size_t)k.sv * 16)); SZCHK(b.b_ltail.ensure((size_t)k.term * 8));
    SZCHK(b.b_dlists.ensure((size_t)k.term * 4 + (size_t)k.cn * 8 + 64));
    // old_key [p2] u64 | hs_key_dev [sv] u64 | old_slot [p2] | ins_T, ins_src, ins_pre_l, ins_pre_c [sv + 1] each | sorted_key [nsort] u64 | sorted_slot [nsort] | rank_part
    SZCHK(b.b_ins.ensure(k.p2 * 12 + (size_t)k.sv * 8 + ((size_t)k.sv + 1) * 16 + k.nsort * 12 + k.nsort * 4 * kK6RankSlices + 64));
    SZCHK(size_zero_once(b.b_ws6, 4 * (scan_grid((uint32_t)cap, 1) + 1) * 8, s));   // look-back words of the table scan
    return BDX_OK;
}

// K2: compact anomalous reads
int do_compact(bdx_ctx* c) {
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t s = c->stream;
    const int nkeys = c->nkeys;
    const uint32_t na = c->na_alloc;
    if (c->stage_timing) HIPCHK(c, hipEventRecord(c->ev[2], s));
    Compact& cp = c->cp;
    cp = Compact{};
    c->k3 = K3Arrays{};
    if (na) {
        const StageDims dm = stage_dims(c, na);
        BDX_TRY(size_compact(c->sb, dm, &c->err));
        const StageBufs& b = c->sb;
        cp.tid = b.b_c_tid.as<int32_t>(); cp.pos = b.b_c_pos.as<int32_t>(); cp.isize = b.b_c_isize.as<int32_t>();
        cp.meta = b.b_c_meta.as<uint32_t>(); cp.key = b.b_c_key.as<uint64_t>(); cp.nn = b.b_c_nn.as<uint32_t>();
        cp.idx = b.b_c_idx.as<uint32_t>();
        cp.check = c->use_check ? b.b_c_check.as<uint64_t>() : nullptr;
        cp.pk = b.b_c_pk.as<uint32_t>(); cp.cap = na;
        K2Params k2{};
        k2.r = c->d; k2.n = c->n; k2.ntiles = c->ntiles; k2.tstride = c->tstride; k2.nkeys = nkeys; k2.nlibs = c->nlibs; k2.libs = c->b_libs.as<DevLib>();
        k2.cls = c->b_cls.as<uint8_t>(); k2.tile_pre = c->b_tile_pre.as<uint32_t>(); k2.c = cp;
        k2.tile_tot = c->b_tile_tot.as<uint32_t>(); k2.stash = c->use_stash ? c->b_stash.as<StashRec>() : nullptr;
        k2.chunk_tot = c->fp_deferred.chunk_tot; k2.chunk_base = c->fp_deferred.chunk_base; k2.chunk_super = c->fp_deferred.chunk_super;
        // scratch of the later stages cleared by this launch: the per-candidate max read length of K3, and (when this
        // context joins its own reads) the slot indices of K4's direct table
        k2.fill_ptr[0] = b.b_c_maxq.as<uint32_t>(); k2.fill_words[0] = na; k2.fill_value[0] = 0u;
        c->join_table_clean = 0;
        if (dm.k2_clears_join) {
            const uint32_t slots = dm.join_slots;
            k2.fill_ptr[1] = b.b_t_key.as<uint32_t>(); k2.fill_words[1] = 2 * slots; k2.fill_value[1] = 0xFFFFFFFFu;
            k2.fill_ptr[2] = b.b_partner.as<uint32_t>(); k2.fill_words[2] = na; k2.fill_value[2] = 0xFFFFFFFFu;
            k2.fill_ptr[3] = b.b_pair_lo.as<uint32_t>(); k2.fill_words[3] = na; k2.fill_value[3] = 0xFFFFFFFFu;
            c->join_table_clean = slots;
        }
        {   // name keys the caller's pinned batches still hold (bdx_push): one segment per batch
            size_t ns = 0;
            BDX_TRY(upload_key_segs(c, &ns));
            if (ns) {
                k2.nseg = (int)ns;
                k2.seg_begin = c->b_seg.as<uint64_t>();
                k2.seg_ptr = (const uint64_t* const*)(c->b_seg.as<uint64_t>() + ns + 1);
                k2.seg_qlen = (const uint16_t* const*)(c->b_seg.as<uint64_t>() + 2 * ns + 1);
                k2.seg_check = (const uint64_t* const*)(c->b_seg.as<uint64_t>() + 3 * ns + 1);
            }
        }
        launch_k2(k2, k2_lds_bytes(nkeys), s, c->finalize2_deferred ? &c->fp_deferred : nullptr);
        c->finalize2_deferred = false;
    }
    if (c->finalize2_deferred) {  // (no K2 launch to ride on)
        launch_finalize2_only(c->fp_deferred, s);
        c->finalize2_deferred = false;
    }
    if (c->stage_timing) HIPCHK(c, hipEventRecord(c->ev[3], s));
    return BDX_OK;
}

// a result whose region table is read where the device left it (c->reg == h_regs.p: bdx_run on a large table, sharded runs) gets its own copy:
// called before the pinned buffers may be reallocated under it (a sizing pass for a larger input) or handed back (bdx_trim_results)
void own_borrowed_regions(bdx_ctx* c) {
    if (!c->reg || (const void*)c->reg != c->sb.h_regs.p) return;
    const HostRegion* r = c->reg;
    const uint32_t* pk = c->rpk;
    const size_t n = c->nreg;
    std::vector<HostRegion> keep(r, r + n);
    std::vector<uint32_t> keep_pk;
    if (pk) keep_pk.assign(pk, pk + n * 2 * (size_t)c->nkeys);
    c->regions.swap(keep); c->r_pk.swap(keep_pk);
    c->reg = c->regions.data(); c->rpk = c->r_pk.data();
}

// K3: cut regions.  tid_tail: see launch_k3 (null: a single-context run)
int do_cut(bdx_ctx* c, const uint32_t* tid_tail, RegionDst dst) {
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t s = c->stream;
    const uint32_t na = c->na_alloc;
    if (na) {
        StageDims dm = stage_dims(c, na);
        dm.regions = dst;
        BDX_TRY(size_cut(c->sb, dm, s, &c->err));
        const StageBufs& b = c->sb;
        K3Arrays& k3 = c->k3;
        const bool for_k6 = dst == RegionDst::HostAndHbm;
        k3.cap = na;
        k3.cand = b.b_cand.as<int32_t>(); k3.pre_q = b.b_pre_q.as<uint32_t>(); k3.pre_rev = b.b_pre_rev.as<uint32_t>();
        k3.pre_nonctx = b.b_pre_nonctx.as<uint32_t>(); k3.c_first = b.b_c_first.as<uint32_t>();
        k3.c_maxq = b.b_c_maxq.as<int32_t>(); k3.c_rid = b.b_c_rid.as<int32_t>(); k3.region_of = b.b_region_of.as<int32_t>();
        k3.r_rec = for_k6 ? b.h_regs.as<RegionRec>() : b.b_r_rec.as<RegionRec>();
        k3.r_pk = for_k6 ? b.h_pk.as<uint32_t>() : b.b_r_pk.as<uint32_t>();
        if (for_k6) {  // the device-side SV assembly reads the region table back: a copy in HBM
            k3.r_rec_dev = b.b_r_rec.as<RegionRec>(); k3.r_pk_dev = b.b_r_pk.as<uint32_t>(); k3.out_deg = b.b_out_deg.as<uint32_t>();
            // with the direct join right behind K3, that kernel forwards the table to the host
            k3.host_copy_later = joins_direct(c, na) ? 1 : 0;
            memset(b.h_counts0.p, 0, sizeof(StageCounts));
            k3.counts_host = b.h_counts0.as<StageCounts>();
        } else {
            k3.r_rec_dev = nullptr; k3.r_pk_dev = nullptr; k3.host_copy_later = 0;
        }
        k3.lb_state = b.b_lb.as<unsigned long long>();
        HIPCHK(c, next_lb_stamp(c, &k3.lb_stamp));
        k3.counts = c->b_counts.as<StageCounts>();
        // single-context runs that take the direct join let that kernel do k3_region_of_kernel's work
        c->region_of_fused = for_k6 && joins_direct(c, na);
        launch_k3(k3, c->cp, c->b_p1.as<Pass1>(), na, c->opts.min_len, c->opts.seq_coverage_lim, c->nkeys, tid_tail, !c->region_of_fused, s);
        if (for_k6 && !k3.host_copy_later) {  // the region table is in pinned memory
            BDX_TRY(signal_ready(c, kRegionsReady, c->ev_regions));
        }
    }
    if (c->stage_timing) HIPCHK(c, hipEventRecord(c->ev[4], s));
    return BDX_OK;
}

// K4 on the context's own reads (single-context run), with the foreign entries of a sharded run behind them
int do_join_local(bdx_ctx* c, uint32_t n, const Entries& en, const uint32_t* n_ptr) {
    hipStream_t s = c->stream;
    K4Arrays& k4 = c->k4;
    k4 = K4Arrays{};
    if (!n) return BDX_OK;
    const bool direct = joins_direct(c, n);
    StageDims dm = stage_dims(c, c->na_alloc);
    dm.join_n = n;
    dm.join_own = en.n_local ? std::min<uint32_t>(n, std::max<uint32_t>(c->na_alloc, 1u)) : n;
    // (the foreign entries of a sharded run come on top of the reads K2 sized the table for: it still has room at half its load)
    dm.join_slots = !direct ? 0u : (c->join_table_clean && (uint64_t)n * 2 <= c->join_table_clean) ? c->join_table_clean : direct_join_slots(n);
    dm.join_pair_lo = en.want_pair_lo != 0;
    BDX_TRY(size_join(c->sb, dm, &c->err));
    StageBufs& b = c->sb;
    k4.g_cap = dm.join_groups();
    k4.g_rec = c->groups_in_hbm ? b.b_groups.as<GroupRec>() : b.h_groups.as<GroupRec>();
    k4.partner = b.b_partner.as<int32_t>();
    if (direct) {
        const uint32_t slots = dm.join_slots;
        const size_t n_own = dm.join_own;
        const bool want_lo = en.c_rid || en.want_pair_lo;
        if (c->join_table_clean != slots) {   // (K2 has not preset the table)
            HIPCHK(c, hipMemsetAsync(b.b_t_key.p, 0xFF, (size_t)slots * 8, s));
            HIPCHK(c, hipMemsetAsync(b.b_partner.p, 0xFF, n_own * 4, s));
            if (en.want_pair_lo) HIPCHK(c, hipMemsetAsync(b.b_pair_lo.p, 0xFF, n_own * 4, s));
        }
        k4.pair_lo = ((c->join_table_clean == slots && want_lo) || en.want_pair_lo) ? b.b_pair_lo.as<int32_t>() : nullptr;  // preset to -1 by K2
        c->join_table_clean = 0;
        k4.direct = 1; k4.t_mask = slots - 1;
        k4.t_key = b.b_t_key.as<uint64_t>(); k4.t_idx = b.b_t_idx.as<int32_t>();
        launch_k4_join_only(k4, en, n_ptr, n, c->b_counts.as<StageCounts>(), s);
        return BDX_OK;
    }
    // the partitioned join: its tables go by the entries that have arrived, sized here
    uint32_t nb = 1, lg = 0;
    while (nb < (uint32_t)kMaxBuckets && (size_t)nb * 384 < n) { nb <<= 1; ++lg; }  // ~256-512 entries per bucket: >= 1 workgroup per CU early
    k4.nbuckets = nb; k4.log2b = lg;
    if ((size_t)nb * 4 > b.b_bcnt.bytes) {  // (re)allocated: the partition histogram has to start from zero once
        HIPCHK(c, b.b_bcnt.ensure((size_t)kMaxBuckets * 4));
        HIPCHK(c, hipMemsetAsync(b.b_bcnt.p, 0, b.b_bcnt.bytes, s));
    }
    HIPCHK(c, b.b_boff.ensure((nb + 1) * 4)); HIPCHK(c, b.b_bcur.ensure(nb * 4));
    HIPCHK(c, b.b_e_key.ensure((size_t)n * 8)); HIPCHK(c, b.b_e_idx.ensure((size_t)n * 4));
    HIPCHK(c, b.b_t_key.ensure((size_t)n * 16)); HIPCHK(c, b.b_t_idx.ensure((size_t)n * 8));
    k4.bcnt = b.b_bcnt.as<uint32_t>(); k4.boff = b.b_boff.as<uint32_t>(); k4.bcur = b.b_bcur.as<uint32_t>();
    k4.e_key = b.b_e_key.as<uint64_t>(); k4.e_idx = b.b_e_idx.as<uint32_t>();
    k4.t_key = b.b_t_key.as<uint64_t>(); k4.t_idx = b.b_t_idx.as<int32_t>();
    launch_k4_join_only(k4, en, n_ptr, n, c->b_counts.as<StageCounts>(), s);
    return BDX_OK;
}

// region table for the host side.  borrow: rr / pk stay valid (the context's pinned buffers) and no id shift is
// needed, so the walk and the getters read them in place.
constexpr uint32_t kBorrowRegionsMin = 32768;   // regions from which on the host's share of the walk may read the table in pinned memory (bdx_run)
void decode_regions(bdx_ctx* c, const RegionRec* rr, const uint32_t* pk, uint32_t nr, uint32_t ph, bool borrow) {
    static_assert(sizeof(HostRegion) == sizeof(RegionRec) && offsetof(HostRegion, first) == offsetof(RegionRec, first), "region layout");
    const int nkeys = c->nkeys;
    if (borrow && !ph) {
        c->reg = (const HostRegion*)rr; c->nreg = nr; c->rpk = pk;
        return;
    }
    c->regions.resize(nr + ph);
    if (ph) c->regions[0] = HostRegion{-1, -1, -1, 0, 0, 0, 0, 0, 0};
    if (nr) memcpy(c->regions.data() + ph, rr, (size_t)nr * sizeof(RegionRec));
    c->r_pk.assign((size_t)ph * 2 * nkeys, 0u);
    c->r_pk.insert(c->r_pk.end(), pk, pk + (size_t)nr * 2 * nkeys);
    c->reg = c->regions.data(); c->nreg = c->regions.size(); c->rpk = c->r_pk.data();
}

void decode_groups(bdx_ctx* c, const GroupRec* gr, uint32_t ng, uint32_t ph) {
    c->parts.resize(ng);
    for (uint32_t i = 0; i < ng; ++i) {
        const uint64_t k = gr[i].key;
        c->parts[i] = GroupPart{(uint32_t)(k >> 38) + ph, (uint32_t)((k >> 12) & ((1u << 26) - 1)) + ph, (uint8_t)(k & 15),
                                (uint8_t)((k >> 4) & 255), gr[i].pairs, gr[i].sum_isize};
    }
}

// K6's arrays for `na` regions, in the buffers size_k6 has sized: capacities, the carved-up scratch, inputs from K3 / K4, outputs
void k6_layout(const bdx_ctx* c, K6Arrays& a, const StageDims& dm, uint32_t na) {
    const StageBufs& b = c->sb;
    const K6Caps k = k6_caps(dm);
    const size_t cap = na, p2 = k.p2, svc = k.sv, nsort = k.nsort;
    a.sv_cap = k.sv; a.term_cap = k.term; a.cn_cap = k.cn; a.lib_stride = k.lib_stride;
    a.old_key = b.b_ins.as<uint64_t>(); a.hs_key_dev = a.old_key + p2;
    a.old_slot = (uint32_t*)(a.hs_key_dev + svc); a.ins_T = a.old_slot + p2; a.ins_src = a.ins_T + svc + 1;
    a.ins_pre_l = a.ins_src + svc + 1; a.ins_pre_c = a.ins_pre_l + svc + 1;
    a.sorted_key = (uint64_t*)(((uintptr_t)(a.ins_pre_c + svc + 1) + 7) & ~(uintptr_t)7); a.sorted_slot = (uint32_t*)(a.sorted_key + nsort);
    // (k6_ranksort_kernel is launched, and its ranks are read, where the list of candidates placed by key CAN outgrow what k6_insert_kernel's
    // one workgroup sorts in LDS (2,048 entries) -- a -t run's candidates are all of that kind: 5-10 k of them at a genome share took that
    // workgroup's bitonic sort in HBM half a millisecond.  Smaller inputs do without the launch)
    a.rank_part = a.sv_cap > 2048u ? a.sorted_slot + nsort : nullptr;
    a.sv_begin = b.b_sv_src.as<uint2>(); a.sv_src = (uint32_t*)(a.sv_begin + a.sv_cap); a.ltail = b.b_ltail.as<double>();
    a.d_lib_index = b.b_dlists.as<int32_t>(); a.d_cn_key = a.d_lib_index + a.term_cap; a.d_cn_value = (float*)(a.d_cn_key + a.cn_cap);
    a.cap = na;
    a.r_rec = c->k6_r_rec ? c->k6_r_rec : b.b_r_rec.as<RegionRec>(); a.r_pk = c->k6_r_pk ? c->k6_r_pk : b.b_r_pk.as<uint32_t>();
    a.taint = c->k6_taint;
    a.region_of = c->k3.region_of; a.partner = c->k4.partner; a.pair_lo = c->k4.pair_lo; a.meta = c->cp.meta; a.isize = c->cp.isize;
    a.in_groups = c->k6_in_groups; a.in_goff = c->k6_in_goff; a.first_of = c->k6_in_groups ? c->k6_in_goff : nullptr;
    a.parts = b.b_parts.as<PartRec>();
    a.rs = b.b_rs.as<RegSum>();
    a.out_deg = b.b_out_deg.as<uint32_t>(); a.label = a.out_deg + cap; a.bad_v = a.out_deg + 2 * cap; a.bad = a.out_deg + 3 * cap;
    a.mcount = a.out_deg + 4 * cap; a.pcount = a.out_deg + 5 * cap;
    a.members = b.b_members.as<MemberInfo>();
    a.own_nsv = b.b_own.as<uint32_t>(); a.own_nacc = a.own_nsv + cap; a.own_ncn = a.own_nsv + 2 * cap; a.own_first = a.own_nsv + 3 * cap; a.slot_next = a.own_nsv + 4 * cap; a.owners = a.own_nsv + 5 * cap; a.owners_big = a.own_nsv + 6 * cap; a.emit_part = a.own_nsv + 7 * cap;
    a.big_walk = dm.walks_big();
    a.member_ids = a.big_walk ? b.b_member_ids.as<uint32_t>() : nullptr;
    a.sv_stage = b.b_slot.as<SvOut>(); a.lib_stage = b.b_lib_stage.as<LibStage>(); a.cn_stage = b.b_cn_stage.as<CnStage>();
    if (c->table_in_hbm) {
        a.sv_out = b.b_sv_out.as<SvOut>(); a.lib_index = b.b_lib_index_out.as<int32_t>(); a.lib_pairs = b.b_lib_pairs_out.as<int32_t>();
        a.cn_key = b.b_cn_key_out.as<int32_t>(); a.cn_value = b.b_cn_value_out.as<float>();
        a.sv_key = b.b_sv_key.as<unsigned long long>();
    } else {
        a.sv_out = b.h_sv_out.as<SvOut>(); a.lib_index = b.h_lib_index.as<int32_t>(); a.lib_pairs = b.h_lib_pairs.as<int32_t>();
        a.cn_key = b.h_cn_key.as<int32_t>(); a.cn_value = b.h_cn_value.as<float>();
    }
    a.sv_vx = a.sv_key ? a.sv_src + a.sv_cap : nullptr;
    a.t_lambda = b.b_t_lambda.as<double>(); a.t_k = b.b_t_k.as<int32_t>();
    a.g_rec = c->k4.g_rec; a.g_cap = c->k4.g_cap;
    a.lb_state = b.b_ws6.as<unsigned long long>();
    a.counts_host2 = b.h_counts2.as<StageCounts>();
}

// K6 on the context's own regions: pair groups per region, SV assembly of the components that need no traversal, everything else listed
// for the host walk; then (do_k6_table) the dense results and K5 for the device-assembled SVs.  k6_prepare lays out K6's arrays and run
// constants and launches nothing; the callers then launch what they mean (k6_pairs, k6_then_walk below).
// rounds: min-label propagation rounds (0: kK6LabelRounds, or kK6LabelRoundsBig with the general walk)
int k6_prepare(bdx_ctx* c, bool force_host, int rounds) {
    K6Arrays& a = c->k6;
    a = K6Arrays{};
    const StageDims dm = stage_dims(c, c->na_alloc);
    const uint32_t na = dm.k6_regions();
    if (!na) return BDX_OK;
    BDX_TRY(size_k6(c->sb, dm, c->stream, &c->err));
    k6_layout(c, a, dm, na);
    HIPCHK(c, next_lb_stamp(c, &a.lb_stamp));
    a.counts = c->b_counts.as<StageCounts>();
    // run constants: the flag histogram is the device's own reduced counter table (a single-context run adopts its own
    // statistics), the read densities per counter key travel in the kernel arguments
    a.hist = c->b_cnt.as<uint32_t>();
    a.key_density = c->b_kdens.as<float>();
    a.lib_mean = c->b_lib_mean.as<float>();
    a.counts_host = c->h_counts.as<StageCounts>();
    memset(c->h_counts.p, 0, sizeof(StageCounts));
    memset(a.counts_host2, 0, sizeof(StageCounts));
    a.p1 = c->b_p1.as<Pass1>();
    a.nlibs = c->nlibs; a.nkeys = c->nkeys; a.min_read_pair = c->opts.min_read_pair; a.chr_restricted = c->opts.chr_restricted;
    a.period = std::max(1, c->opts.buffer_size + 1);
    a.force_host = force_host ? 1 : 0;
    a.ins_plain = c->dbg_ins_plain;
    a.asm_plain = c->dbg_asm_plain;
    // (long chains need more rounds to agree on one label; with the general walk on, the step is long enough not to care)
    a.propagation_rounds = rounds ? rounds : (a.big_walk ? kK6LabelRoundsBig : kK6LabelRounds);
    if (c->poll) {  // ready words set by the kernels themselves (first thread of k6_pairs_kernel / first wave of k6_walk_kernel)
        a.flag_value = c->seq;
        a.flag_groups = c->h_flags.as<uint32_t>() + kGroupsReady;
        if (c->k3.host_copy_later) a.flag_regions = c->h_flags.as<uint32_t>() + kRegionsReady;
        a.mirror_in_walk = force_host ? 0 : 1;  // (k6_walk_kernel follows k6_emit_kernel unless everything goes to the host)
    }
    return BDX_OK;
}

// the launches behind k6_prepare (none where it found nothing to do): k6_pairs_kernel alone, and `first` (launch_k6_groups: pairs and
// components in one go; launch_k6_components) with the device's walk behind it.  A context that does not poll gets the event that says
// the host's share of the groups is complete in between; one that polls has the word set by k6_pairs_kernel's first thread
void k6_pairs(bdx_ctx* c) {
    if (c->k6.cap) launch_k6_pairs(c->k6, c->k6.cap, c->stream);
}
int k6_then_walk(bdx_ctx* c, void (*first)(const K6Arrays&, uint32_t, hipStream_t)) {
    const K6Arrays& a = c->k6;
    if (!a.cap) return BDX_OK;
    first(a, a.cap, c->stream);
    if (!c->poll) BDX_TRY(signal_ready(c, kGroupsReady, c->ev_groups));
    launch_k6_walk(a, a.cap, c->stream);
    return BDX_OK;
}

// A sizing pass (bdx_reserve, bdx_dist_prepare, the BAM decoder's sizing thread): the four size functions and no launch.  It may run on a
// thread of its own beside the thread that feeds the context: the size functions see the later stages' buffers and `dm`, nothing else of
// the context (bdx_ctx::sizing), and the message of a failure goes to sizing_err, not to the feeding thread's `err`.
int presize_stages(bdx_ctx* c, const StageDims& dm) {
    struct Guard {
        bdx_ctx* c;
        explicit Guard(bdx_ctx* c_) : c(c_) { c->sizing.fetch_add(1, std::memory_order_acq_rel); c->sizing_err.clear(); }
        ~Guard() { c->sizing.fetch_sub(1, std::memory_order_acq_rel); }
    } guard(c);
    std::string* err = &c->sizing_err;
    SZCHK(hipSetDevice(c->device));
    own_borrowed_regions(c);   // (the pinned region table may grow below.  bdx_reserve sizes nothing once the context has run, and the decoder's
                               // pass follows a reset -- no live result should read it in place; if one does, it keeps a copy)
    BDX_TRY(size_compact(c->sb, dm, err));
    BDX_TRY(size_cut(c->sb, dm, c->stream, err));
    BDX_TRY(size_join(c->sb, dm, err));
    return size_k6(c->sb, dm, c->stream, err);
}

// a sizing pass on the caller's own thread: its message is the context's
int presize_stages_here(bdx_ctx* c, const StageDims& dm) {
    const int r = presize_stages(c, dm);
    if (r != BDX_OK) c->err = c->sizing_err;
    return r;
}

// the host walk's SV candidates with their order keys and lists, in pinned memory for the table stage (a.hs_*)
int stage_host_svs(bdx_ctx* c, K6Arrays& a) {
    const WalkResult& H = c->walk;
    const uint32_t nh = (uint32_t)H.svs.size(), nt = (uint32_t)H.terms.size(), nc = (uint32_t)H.cn_key.size();
    a.nh = nh;
    if (nh) {
        const uint64_t period = (uint64_t)std::max(1, c->opts.buffer_size + 1);
        HIPCHK(c, c->h_hs_rec.ensure((size_t)nh * sizeof(SvOut)));
        HIPCHK(c, c->h_hs_aux.ensure((size_t)nh * 12 + 16));
        HIPCHK(c, c->h_hs_lists.ensure((size_t)nt * 16 + (size_t)nc * 8 + 16));
        memcpy(c->h_hs_rec.p, H.svs.data(), (size_t)nh * sizeof(HostSv));
        uint64_t* hkey = c->h_hs_aux.as<uint64_t>();
        uint32_t* hcnt = (uint32_t*)(hkey + nh);
        for (uint32_t j = 0; j < nh; ++j) {
            hkey[j] = host_order_key(H.sv_key[j], period);
            if (a.force_host) hkey[j] = 0;  // no device candidates to interleave with (and the ids may carry the phantom shift)
            hcnt[j] = (uint32_t)H.svs[j].sv.lib_count | ((uint32_t)H.svs[j].sv.cn_count << 16);
        }
        double* lam = c->h_hs_lists.as<double>();
        int32_t* li = (int32_t*)(lam + nt);
        int32_t* lp = li + nt;
        int32_t* ck = lp + nt;
        float* cv = (float*)(ck + nc);
        for (uint32_t i = 0; i < nt; ++i) { lam[i] = H.terms[i].lambda; li[i] = H.lib_index[i]; lp[i] = H.lib_pairs[i]; }
        for (uint32_t i = 0; i < nc; ++i) { ck[i] = H.cn_key[i]; cv[i] = H.cn_value[i]; }
        a.hs_rec = c->h_hs_rec.as<SvOut>(); a.hs_key = hkey; a.hs_cnt = hcnt;
        a.hs_lambda = lam; a.hs_lib_index = li; a.hs_lib_pairs = lp; a.hs_cn_key = ck; a.hs_cn_value = cv;
    }
    return BDX_OK;
}

// second half of K6, enqueued once the host walk has produced its share: the host's SV candidates (pinned memory) are
// interleaved with the device's by the compaction, K5 scores every term, the score kernel finishes every candidate --
// the final table is assembled by the device in pinned host memory, in the reference's output order.
int do_k6_table(bdx_ctx* c) {
    hipStream_t s = c->stream;
    K6Arrays& a = c->k6;
    const uint32_t na = a.cap;
    if (!na) return BDX_OK;
    BDX_TRY(stage_host_svs(c, a));
    // (K5 runs inside the table kernel.  The terms' log tails go to the host for Fisher's combination only -- BreakDancer.cpp:71-81 uses the
    // host's exp / log --; otherwise they are 8 bytes per term over PCIe that nobody reads)
    a.ltail_host = c->table_in_hbm ? c->sb.b_ltail_out.as<double>() : (c->opts.fisher ? c->sb.h_ltail_dev.as<double>() : nullptr);
    // (the table kernel's launch: for the regions the pair groups' report named -- the host has read it by now -- not for their upper bound)
    a.fin_regions = (c->counts.n_regions && c->counts.n_regions <= na) ? c->counts.n_regions : na;
    HIPCHK(c, c->h_printed.ensure((size_t)k6_score_grid(a) * 4));
    a.printed_host = c->h_printed.as<uint32_t>();
    // The word the host polls for the end of the run is set by a one-thread kernel behind the table kernel (a kernel boundary
    // orders it behind that kernel's stores to host memory).  A stream write-value command does the same as a one-thread kernel of
    // the runtime's own, but starts 5 us after the kernel before it has ended; back-to-back launches follow each other at once.
    if (c->poll) { a.flag_done = c->h_flags.as<uint32_t>() + kTableReady; a.flag_value = c->seq; }
    a.wire_rows = c->table_in_hbm ? 0 : 1;   // (a table that stays in HBM for rank 0's merge keeps its full rows)
    c->rows_packed = a.wire_rows != 0;
    launch_k6_table(a, na, std::log(10), c->opts.score_threshold, c->opts.fisher ? 0 : 1, s);
    if (!a.flag_done) {  // (without polling: finish_table waits for the stream)
        BDX_TRY(signal_ready(c, kTableReady, nullptr));
    }
    return BDX_OK;
}

// copy the final table out of the pinned buffers the device assembled it in (getters, support lists, Fisher scores)
int materialize(bdx_ctx* c) {
    if (c->materialized) return BDX_OK;
    WalkResult& M = c->walk;
    M.clear();
    const uint32_t n = c->n_sv_total, nt = c->n_terms_total, nc = c->n_cn_total;
    if (c->rows_packed) {
        // the rows crossed the link as SvWire: chromosomes and strand counts are the regions' (SvBuilder.cpp:18-99 takes them from there too),
        // the list offsets the running sums of the counts in table order
        const SvWire* w = c->sb.h_sv_out.as<SvWire>();
        M.svs.resize(n);
        int32_t lb = 0, cb = 0;
        for (uint32_t i = 0; i < n; ++i) {
            const SvWire& r = w[i];
            HostSv& o = M.svs[i];
            bdx_sv& v = o.sv;
            const HostRegion& ra = c->reg[r.region[0]];
            const HostRegion& rb = r.region[1] >= 0 ? c->reg[r.region[1]] : ra;
            v.chr[0] = ra.tid; v.chr[1] = rb.tid;
            v.pos[0] = r.pos[0]; v.pos[1] = r.pos[1];
            v.fwd[0] = (int32_t)(ra.n - ra.rev); v.rev[0] = (int32_t)ra.rev;
            v.fwd[1] = (int32_t)(rb.n - rb.rev); v.rev[1] = (int32_t)rb.rev;
            v.flag = (int32_t)((r.bits >> 16) & 15u); v.size = r.size; v.score = r.score; v.num_reads = r.num_reads; v.printed = (int32_t)((r.bits >> 23) & 1u);
            v.region[0] = r.region[0]; v.region[1] = r.region[1];
            v.lib_begin = lb; v.lib_count = (int32_t)(r.bits & 255u); lb += v.lib_count;
            v.cn_begin = cb; v.cn_count = (int32_t)((r.bits >> 8) & 255u); cb += v.cn_count;
            v.allele_frequency = r.allele_frequency; v.logp = r.logp;
            o.grp_mask = (r.bits >> 20) & 7u; o.start = r.start;
        }
    } else {
        const HostSv* d = c->sb.h_sv_out.as<HostSv>();
        M.svs.assign(d, d + n);
    }
    M.lib_index.assign(c->sb.h_lib_index.as<int32_t>(), c->sb.h_lib_index.as<int32_t>() + nt);
    M.lib_pairs.assign(c->sb.h_lib_pairs.as<int32_t>(), c->sb.h_lib_pairs.as<int32_t>() + nt);
    M.cn_key.assign(c->sb.h_cn_key.as<int32_t>(), c->sb.h_cn_key.as<int32_t>() + nc);
    M.cn_value.assign(c->sb.h_cn_value.as<float>(), c->sb.h_cn_value.as<float>() + nc);
    if (c->opts.fisher) c->log_tail.assign(c->sb.h_ltail_dev.as<double>(), c->sb.h_ltail_dev.as<double>() + nt); else c->log_tail.clear();
    M.n_groups = c->n_groups_total;
    c->materialized = true;
    return BDX_OK;
}

// end of a single-context run: wait for the device's table
int finish_table(bdx_ctx* c) {
    const auto tf0 = std::chrono::steady_clock::now();
    BDX_TRY(await_ready(c, kTableReady, nullptr, "the SV table did not arrive: its kernels were not launched"));
    const auto tf1 = std::chrono::steady_clock::now();
    static_assert(sizeof(HostSv) == sizeof(SvOut) && offsetof(HostSv, grp_mask) == offsetof(SvOut, grp_mask) &&
                      offsetof(HostSv, start) == offsetof(SvOut, start), "SV record layout");
    c->n_sv_host = (uint32_t)c->walk.svs.size();
    c->n_groups_total = c->walk.n_groups + c->counts.n_groups_dev;
    const StageCounts c2 = *c->sb.h_counts2.as<StageCounts>();
    if (c2.overflow) return fail(c, BDX_EINTERNAL, "SV list overflow");
    c->n_sv_total = c2.n_sv_dev; c->n_terms_total = c2.n_terms_dev; c->n_cn_total = c2.n_cn_dev;
    c->counts.n_sv_dev = c2.n_sv_dev - c->n_sv_host;
    {
        // printed candidates: every workgroup of the score kernel left its count (no run: none)
        const uint32_t g = c->k6.printed_host ? k6_score_grid(c->k6) : 0u;
        const uint32_t* pb = c->k6.printed_host;
        uint32_t np = 0;
        for (uint32_t i = 0; i < g; ++i) np += pb[i];
        c->n_printed = np;
    }
    c->counts.n_old = c2.n_old;
    c->materialized = false;
    if (c->opts.fisher && !c->table_in_hbm) {  // Fisher's combination (BreakDancer.cpp:71-81) uses the host's exp / log (sharded: after the merge)
        materialize(c);
        finish_scores(c->opts, c->log_tail.data(), c->walk.svs.data(), c->walk.svs.size(), &c->n_printed);
    }
    const auto tf2 = std::chrono::steady_clock::now();
    c->stage_ms[kMsTableWait] = ms_between(tf0, tf1);
    c->stage_ms[kMsMerge] = ms_between(tf1, tf2);
    c->stage_ms[kMsScores] = 0;
    c->ran = true;
    return BDX_OK;
}

// H1 walk over c->regions / c->r_pk / c->parts with the adopted pass-1 statistics
int host_walk(bdx_ctx* c, int32_t last_maxq, bool any_anomalous) {
    HIPCHK(c, hipSetDevice(c->device));
    WalkInput wi{};
    wi.opts = c->opts; wi.libs = c->libs.data(); wi.nlibs = c->nlibs; wi.nbams = c->nbams; wi.nkeys = c->nkeys;
    wi.hist = c->cnt.data(); wi.covered_ref_len = c->g_covered; wi.key_density = c->key_density.data();
    wi.regions = c->reg; wi.nregions = c->nreg; wi.r_pk = c->rpk; wi.parts = &c->parts; wi.last_maxq = last_maxq;
    wi.any_anomalous = any_anomalous;
    c->walk.clear();
    if (!c->parts.empty()) greedy_walk(wi, c->walk_scratch.get(), c->walk);
    return BDX_OK;
}

// h_terms for `nt` terms: [nt] lambda (double) | [nt] k (int32) | the log tails K5 writes back, on the next 8-byte boundary
double* terms_log_tail(const bdx_ctx* c, size_t nt) { return (double*)((char*)c->h_terms.p + ((nt * 12 + 7) & ~(size_t)7)); }

// K5 for the host walk's terms (the read-level replay: the whole walk is the host's)
int score_host_terms(bdx_ctx* c) {
    hipStream_t s = c->stream;
    const uint32_t nt = (uint32_t)c->walk.terms.size();
    if (nt) {
        // zero-copy: the kernel reads lambda / k from pinned host memory and writes the log tails back into it (a few
        // tens of KB; the PCIe traffic overlaps the kernel and no copy engine round trips are paid)
        HIPCHK(c, c->h_terms.ensure((size_t)nt * 20 + 16));
        double* hl = c->h_terms.as<double>();
        int32_t* hk = (int32_t*)(hl + nt);
        for (uint32_t i = 0; i < nt; ++i) { hl[i] = c->walk.terms[i].lambda; hk[i] = c->walk.terms[i].k; }
        launch_k5(hl, hk, terms_log_tail(c, nt), nt, s);
    }
    return BDX_OK;
}

// the read-level replay, a run without anomalous reads: the walk, the list and the score combination are the host's
int finish_host_walk(bdx_ctx* c) {
    hipStream_t s = c->stream;
    HIPCHK(c, hipStreamSynchronize(s));
    HIPCHK(c, hipGetLastError());
    const uint32_t nt = (uint32_t)c->walk.terms.size();
    const double* host_tail = nt ? terms_log_tail(c, nt) : nullptr;
    c->log_tail.assign(host_tail, host_tail + nt);
    finish_scores(c->opts, c->log_tail.data(), c->walk.svs.data(), c->walk.svs.size(), &c->n_printed);
    c->n_sv_host = c->n_sv_total = (uint32_t)c->walk.svs.size();
    c->n_terms_total = nt; c->n_cn_total = (uint32_t)c->walk.cn_key.size();
    c->n_groups_total = c->walk.n_groups;
    c->counts.n_sv_dev = 0;
    c->materialized = true;
    c->ran = true;
    return BDX_OK;
}

// Supporting reads per SV, in SvBuilder's observation order (SvBuilder.cpp:101-118): reads of region A then region B
// are visited in stream order and a pair is recorded when its second mate shows up, second mate first.
int collect_support(bdx_ctx* c, uint32_t ph) {
    c->sup_off.assign(1, 0);
    c->sup_idx.clear();
    c->sup_flag.clear();
    const uint32_t na = c->p1.n_anom;
    std::vector<int32_t> partner(na), region_of(na);
    std::vector<uint32_t> idx(na), meta(na);
    if (na) {
        HIPCHK(c, hipMemcpy(partner.data(), c->k4.partner, (size_t)na * 4, hipMemcpyDeviceToHost));
        HIPCHK(c, hipMemcpy(region_of.data(), c->k3.region_of, (size_t)na * 4, hipMemcpyDeviceToHost));
        HIPCHK(c, hipMemcpy(idx.data(), c->cp.idx, (size_t)na * 4, hipMemcpyDeviceToHost));
        HIPCHK(c, hipMemcpy(meta.data(), c->cp.meta, (size_t)na * 4, hipMemcpyDeviceToHost));
    }
    std::vector<std::pair<uint32_t, uint32_t>> pairs;  // (second-observed j, its mate p)
    for (const HostSv& hs : c->walk.svs) {
        pairs.clear();
        const uint32_t rA = (uint32_t)hs.sv.region[0], rB = (uint32_t)hs.sv.region[1];
        const uint32_t glo[3] = {rA, rA, rB}, ghi_[3] = {rA, rB, rB};
        for (uint32_t g = 0; g < 3; ++g) {
            if (!(hs.grp_mask & (1u << g))) continue;
            const uint32_t lo = glo[g], hi = ghi_[g];
            const uint32_t f = c->reg[hi].first, n = c->reg[hi].n;
            for (uint32_t j = f; j < f + n; ++j) {
                const int32_t p = partner[j];
                if (p < 0 || (uint32_t)p >= j) continue;
                if ((uint32_t)(region_of[p] + (int32_t)ph) != lo) continue;
                pairs.emplace_back(j, (uint32_t)p);
            }
        }
        std::sort(pairs.begin(), pairs.end());
        for (auto const& pr : pairs) {
            c->sup_idx.push_back(idx[pr.first]); c->sup_flag.push_back((uint8_t)meta_flag(meta[pr.first]));
            c->sup_idx.push_back(idx[pr.second]); c->sup_flag.push_back((uint8_t)meta_flag(meta[pr.second]));
        }
        c->sup_off.push_back((uint32_t)c->sup_idx.size());
    }
    return BDX_OK;
}

// The read-level replay (H2) over compact records in stream order -- name key, accepted region id (or -1), meta, |isize| -- on the
// context's region table (c->reg / c->rpk) and pass-1 statistics; scores from K5.  Shared by the single-context replay below and
// by rank 0 of a sharded run, which gathers the records of all chromosomes first.
int replay_arrays(bdx_ctx* c, uint32_t na, const uint64_t* key, const int32_t* region_of, const uint32_t* meta, const int32_t* isize, uint32_t ph,
                  std::vector<uint32_t>* sup) {
    ReadWalkInput ri{};
    WalkInput& wi = ri.base;
    wi.opts = c->opts; wi.libs = c->libs.data(); wi.nlibs = c->nlibs; wi.nbams = c->nbams; wi.nkeys = c->nkeys;
    wi.hist = c->cnt.data(); wi.covered_ref_len = c->g_covered; wi.key_density = c->key_density.data();
    wi.regions = c->reg; wi.nregions = c->nreg; wi.r_pk = c->rpk; wi.parts = nullptr; wi.last_maxq = c->counts.last_maxq;
    wi.any_anomalous = na != 0;
    ri.n_reads = na; ri.key = key; ri.region_of = region_of; ri.meta = meta; ri.isize = isize;
    ri.phantom = ph;
    if (sup) { ri.support_off = &c->sup_off; ri.support = sup; }
    c->walk.clear();
    read_level_walk(ri, c->walk);
    c->counts.n_groups = 0; c->counts.n_pairs = 0;
    int rc = score_host_terms(c);
    if (rc == BDX_OK) rc = finish_host_walk(c);
    if (rc != BDX_OK) return rc;
    c->replayed = true;
    return BDX_OK;
}

// The read-level replay tells names apart by one 64-bit word.  With a second name hash in the stream, two reads are the same
// name only if both words agree: every (key, check) pair gets a number of its own, which then serves as the key.
void unify_names(uint64_t* key, const uint64_t* check, size_t n) {
    struct PairHash {
        size_t operator()(const std::pair<uint64_t, uint64_t>& p) const { return (size_t)(p.first ^ (p.second * 0x9E3779B97F4A7C15ull)); }
    };
    std::unordered_map<std::pair<uint64_t, uint64_t>, uint64_t, PairHash> ids;
    ids.reserve(n);
    for (size_t i = 0; i < n; ++i) key[i] = ids.emplace(std::make_pair(key[i], check[i]), (uint64_t)ids.size()).first->second;
}

// A read name occurs more than twice (StageCounts::irregular): everything behind the region cut is replayed one read at a
// time on the host (H2), from the compact records; the scores still come from K5.  Names clashing across merged BAMs are the
// usual cause -- the reference keeps running on them (ReadRegionData.cpp:108-113), so does this.
int replay_reads(bdx_ctx* c, uint32_t ph) {
    hipStream_t s = c->stream;
    HIPCHK(c, hipStreamSynchronize(s));  // K6's kernels were enqueued on the pair model: let them finish, their results are dropped
    const uint32_t na = c->p1.n_anom;
    std::vector<uint64_t> key(na);
    std::vector<int32_t> region_of(na), isize(na);
    std::vector<uint32_t> meta(na);
    HIPCHK(c, hipMemcpy(key.data(), c->cp.key, (size_t)na * 8, hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(region_of.data(), c->k3.region_of, (size_t)na * 4, hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(meta.data(), c->cp.meta, (size_t)na * 4, hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(isize.data(), c->cp.isize, (size_t)na * 4, hipMemcpyDeviceToHost));
    if (c->cp.check && na) {
        std::vector<uint64_t> check(na);
        HIPCHK(c, hipMemcpy(check.data(), c->cp.check, (size_t)na * 8, hipMemcpyDeviceToHost));
        unify_names(key.data(), check.data(), na);
    }
    if (ph)
        for (int32_t& r : region_of)
            if (r >= 0) r += (int32_t)ph;
    std::vector<uint32_t> sup;
    BDX_TRY(replay_arrays(c, na, key.data(), region_of.data(), meta.data(), isize.data(), ph, c->collect_support ? &sup : nullptr));
    if (c->collect_support) {  // compact indices -> stream indices and flags
        std::vector<uint32_t> idx(na);
        HIPCHK(c, hipMemcpy(idx.data(), c->cp.idx, (size_t)na * 4, hipMemcpyDeviceToHost));
        c->sup_idx.resize(sup.size());
        c->sup_flag.resize(sup.size());
        for (size_t i = 0; i < sup.size(); ++i) { c->sup_idx[i] = idx[sup[i]]; c->sup_flag[i] = (uint8_t)meta_flag(meta[sup[i]]); }
    }
    return BDX_OK;
}

// ---- bdx_run's phases: the sizing plan, one function per route, the hand-over to the host, the end of the run ----

// The very first anomalous read "breaks" an empty accumulator (start = end = -1, no reads).  With a negative
// -s that empty candidate passes process_breakpoint's test (0 > min_len, coverage 0) and the reference
// registers a read-less region 0 (BreakDancer.cpp:216-231, 244-252); every real region id shifts by one.
bool phantom_region_opt(const bdx_ctx* c) { return 0 > c->opts.min_len && 0.0f < (float)c->opts.seq_coverage_lim; }
// shifted region ids and a non-positive -r are left to the host walk entirely
bool host_walks_all(const bdx_ctx* c) { return c->host_walk_only || phantom_region_opt(c) || c->opts.min_read_pair < 1; }

// K2 .. K6 (first half) for c->na_alloc anomalous reads
int enqueue_middle(bdx_ctx* c, bool force_host) {
    BDX_TRY(do_compact(c));
    BDX_TRY(do_cut(c, nullptr, RegionDst::HostAndHbm));
    if (!c->na_alloc) return BDX_OK;
    // the region table is final after K3: the host takes its copy while the device joins the mates
    Entries en{};
    en.key = c->cp.key; en.check = c->cp.check; en.region = c->k3.region_of; en.meta = c->cp.meta; en.isize = c->cp.isize;
    if (c->region_of_fused) {
        en.cand = c->k3.cand; en.c_rid = c->k3.c_rid; en.region_out = c->k3.region_of;
        en.k6_scratch = c->k3.out_deg; en.scratch_cap = c->k3.cap;
        // (the join kernel forwards the region table to pinned host memory.  A kernel of its own on the copy stream, beside the join, was
        // measured in round 6: 1.525 against 1.530 ms at a genome share -- the join does not wait for those 5.7 MB; profiles/r06_genome_ab.txt)
        if (c->k3.host_copy_later) {
            en.r_rec_dev = c->k3.r_rec_dev; en.r_pk_dev = c->k3.r_pk_dev; en.r_rec_host = c->k3.r_rec; en.r_pk_host = c->k3.r_pk;
            en.counts = c->b_counts.as<StageCounts>(); en.nkeys2 = 2 * c->nkeys;
        }
    }
    BDX_TRY(do_join_local(c, c->na_alloc, en, &c->b_p1.as<Pass1>()->n_anom));
    if (c->k3.host_copy_later && !c->poll) {  // the join kernel has forwarded the region table to pinned memory
        BDX_TRY(signal_ready(c, kRegionsReady, c->ev_regions));  // (polling: the next kernel, k6_pairs_kernel, sets the ready word itself)
    }
    BDX_TRY(k6_prepare(c, force_host, 0));
    return k6_then_walk(c, launch_k6_groups);
}

// How a run sizes the stages behind pass 1.  Restored: pass-1 statistics were restored, which are adopted between pass 1 and the rest --
// nothing ahead.  Ahead: sized by `guess` and enqueued before the pass-1 record is back.  Exact: from the count pass 1 delivers.
enum class Sizing { Restored, Ahead, Exact };
struct SizingPlan { Sizing route; uint32_t guess; };

// ... decided from the context's state alone; launches nothing, changes nothing
SizingPlan plan_sizing(const bdx_ctx* c) {
    if (!c->ov_cnt.empty()) return {Sizing::Restored, 0};
    uint64_t guess = 0;
    if (c->speculate == 2 && c->ran && c->last_n == c->n && c->last_na) {
        // this context has just run an input of the same size
        guess = c->spec_test ? std::max(1u, c->last_na / 2) : with_headroom(c->last_na);
    } else if (c->speculate && c->n >= (1u << 20) && (c->speculate == 1 || c->n < (1u << 25))) {
        // no history: a prior.  Anomalous reads are a few percent of a sorted BAM at most (1 % at configs[1]); 1/32 of the
        // reads covers that with room, costs a few microseconds of oversized grids when it is generous, and one more pass
        // over the (short) later stages when it is not.  Small inputs are not worth it: their whole run is launch latency.
        // (measured at configs[1], 1.1 % anomalous: prior n/32 0.309 ms per step, n/64 0.300 ms, exact sizing after the read-back
        // 0.307 ms, sizing from the previous run 0.295 ms -- an oversized launch grid costs about what the host round trip does)
        // (a GPU's share of a genome -- 2^25 reads and more -- does not take the prior by itself: K1's half millisecond covers the launches either way,
        // and a prior twice the truth, eighteen times with -t, costs its oversized grids and tables: 1.534 against 1.514 ms, 0.92 against 0.83 with -t.
        // The compaction ALONE ahead under the prior, the rest sized exactly, was built too: 1.656 against 1.612 ms, 0.90 against 0.83 -- the tables K2
        // clears for K3 and K4 are sized by the guess.  profiles/r06_genome_ab.txt)
        guess = prior_anomalous(c->n, c->spec_test ? 4096 : 32);
    }
    if (!guess || guess > kMaxAnomalous) return {Sizing::Exact, 0};
    return {Sizing::Ahead, (uint32_t)guess};
}

// the run adopts the statistics of its own pass 1 (the device copy already holds them)
int adopt_own_pass1(bdx_ctx* c) { return set_pass1(c, c->cnt_local.data(), c->p1.covered_ref_len, c->p1.window, false); }

// Restored pass-1 statistics (a cache written by an earlier run: ConfigLoader.cpp:19-23): the classifier still runs --
// pass 2 needs its class bytes -- but window, densities, lambda and the printed counters come from the cache
int run_restored(bdx_ctx* c, bool force_host) {
    hipStream_t s = c->stream;
    BDX_TRY(do_pass1(c, {}));
    BDX_TRY(wait_pass1(c));
    BDX_TRY(set_pass1(c, c->ov_cnt.data(), c->ov_covered, window_from(c, c->ov_cnt.data(), c->ov_covered), true));
    HIPCHK(c, hipMemcpyAsync(c->b_cnt.p, c->ov_cnt.data(), c->ov_cnt.size() * 4, hipMemcpyHostToDevice, s));
    HIPCHK(c, hipMemcpyAsync(c->b_kdens.p, c->key_density.data(), c->key_density.size() * 4, hipMemcpyHostToDevice, s));
    HIPCHK(c, hipStreamSynchronize(s));
    return enqueue_middle(c, force_host);
}

// Enqueue-ahead: the later stages go out behind pass 1, sized by `guess`, and the record is received behind them
int run_ahead(bdx_ctx* c, uint32_t guess, bool force_host) {
    hipStream_t s = c->stream;
    BDX_TRY(do_pass1(c, {.na_cap = guess, .defer_second = true}));
    c->na_alloc = guess;
    BDX_TRY(enqueue_middle(c, force_host));
    BDX_TRY(wait_pass1(c));
    BDX_TRY(adopt_own_pass1(c));
    if (c->p1.n_anom <= guess) return BDX_OK;
    // more anomalous reads than guessed: the enqueued stages saw none; run them properly
    HIPCHK(c, hipStreamSynchronize(s));
    HIPCHK(c, hipMemcpy(&c->b_p1.as<Pass1>()->n_anom, &c->p1.n_anom, 4, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemset(c->b_counts.p, 0, sizeof(StageCounts)));
    ++c->seq;  // fresh ready-words: the ones of the neutralised launches are already set
    c->na_alloc = c->p1.n_anom;
    return enqueue_middle(c, force_host);
}

// Exact sizing: the later stages are sized and launched from the count finalize_kernel posts, while finalize2_kernel still runs;
// the record and what the host derives from it come behind the launches
int run_exact(bdx_ctx* c, bool force_host) {
    hipStream_t s = c->stream;
    BDX_TRY(do_pass1(c, {.post_count = true}));
    uint64_t count = 0;
    if (!wait_count(c, &count)) {  // (polling off, or the words did not arrive in time: the record first)
        BDX_TRY(wait_pass1(c));
        BDX_TRY(adopt_own_pass1(c));
        return enqueue_middle(c, force_host);
    }
    if (count > kMaxAnomalous) {
        HIPCHK(c, hipStreamSynchronize(s));
        return fail(c, BDX_ELIMIT, "more than 2^31 anomalous reads in one context");
    }
    if (count) c->na_alloc = (uint32_t)std::min<uint64_t>(with_headroom(count), kMaxAnomalous);
    BDX_TRY(enqueue_middle(c, force_host));
    BDX_TRY(wait_pass1(c));
    if (c->p1.n_anom != count) {
        HIPCHK(c, hipStreamSynchronize(s));
        return fail(c, BDX_EINTERNAL, "the count of anomalous reads posted ahead of the pass-1 record differs from the record's");
    }
    return adopt_own_pass1(c);
}

// K1 .. K6 (first half) by the plan's route; what the next run of the same input is sized from
int enqueue_device_half(bdx_ctx* c, const SizingPlan& plan, bool force_host) {
    hipStream_t s = c->stream;
    switch (plan.route) {
        case Sizing::Restored: BDX_TRY(run_restored(c, force_host)); break;
        case Sizing::Ahead: BDX_TRY(run_ahead(c, plan.guess, force_host)); break;
        case Sizing::Exact: BDX_TRY(run_exact(c, force_host)); break;
    }
    c->last_n = c->n;
    c->last_na = c->p1.n_anom;
    if (c->stage_timing) HIPCHK(c, hipEventRecord(c->ev[5], s));
    return BDX_OK;
}

// The region table and the host's share of the pair groups, as the device completes them: c->reg / c->rpk, c->counts and -- unless a
// read name was seen more than twice (c->counts.irregular: the caller replays) -- c->parts.  ph: 1 with the phantom region 0
int receive_regions_and_groups(bdx_ctx* c, uint32_t ph) {
    hipStream_t s = c->stream;
    BDX_TRY(await_ready(c, kRegionsReady, c->ev_regions, "the region table did not arrive: its kernels were not launched"));
    const uint32_t nr_host = c->sb.h_counts0.as<StageCounts>()->n_regions;
    if ((uint64_t)nr_host + ph > kMaxRegions) {   // (region ids are 26-bit fields of the packed group key)
        HIPCHK(c, hipStreamSynchronize(s));
        return fail(c, BDX_ELIMIT, "more than 2^26 - 2 accepted regions in one context");
    }
    // The host's share of the walk reads the table where the device left it, in pinned memory.  (Until round 6 the table was copied into
    // ordinary memory first -- "one streaming copy is cheaper than the walk's scattered reads", true when the host walked every component:
    // 5.7 MB at a genome share, 0.28 ms of this thread between the join kernel's end and the pair groups' arrival 0.14 ms later; the
    // host's walk of its ~1,200 groups then started late and the device stood idle in front of the table stage.)  A large share
    // (debug "regions_copy" = 1: always) still gets its copy, once the groups have said how large it is.
    // (a small table is copied at once, as ever: its copy fits between the join kernel's end and the groups' arrival -- 32 k regions are 70 us)
    const bool copy_first = c->dbg_regions_copy == 1 || (c->dbg_regions_copy == 0 && nr_host < kBorrowRegionsMin);
    if (copy_first) decode_regions(c, c->sb.h_regs.as<RegionRec>(), c->sb.h_pk.as<uint32_t>(), nr_host, ph, false);
    BDX_TRY(await_ready(c, kGroupsReady, c->ev_groups, "the pair groups did not arrive: their kernels were not launched"));
    c->counts = *c->h_counts.as<StageCounts>();
    if (!copy_first) decode_regions(c, c->sb.h_regs.as<RegionRec>(), c->sb.h_pk.as<uint32_t>(), nr_host, ph,
                                    c->dbg_regions_copy == 2 || (uint64_t)c->counts.n_groups * 8 < nr_host);   // (borrowed while the walk touches a fraction of the table:
                                    // a walk of 20 k groups over 15 k regions was 46 us faster on its copy)
    if (c->counts.irregular) return BDX_OK;
    if (c->counts.overflow) return fail(c, BDX_EINTERNAL, "group list overflow");
    decode_groups(c, c->sb.h_groups.as<GroupRec>(), c->counts.n_groups, ph);
    c->last_big_groups = (int64_t)c->counts.n_groups + c->counts.n_groups_big;  // (the host's share: mostly such components)
    return BDX_OK;
}

// host-side time stamps of a run: its begin, the hand-over to the host, the start and the end of the host walk (bdx_get_timings [4] .. [7])
using RunTime = std::chrono::steady_clock::time_point;
struct RunClock { RunTime begin, h0, h1, h2; };
RunTime run_now() { return std::chrono::steady_clock::now(); }

// a read name seen more than twice: the pair model does not hold (see bdx_walk_reads.cpp) and the run ends through the read-level replay
int finish_by_replay(bdx_ctx* c, uint32_t ph, const RunClock& t) {
    BDX_TRY(replay_reads(c, ph));
    const RunTime t_r = run_now();
    c->stage_ms[kMsGroupsWait] = ms_between(t.h0, t.h1); c->stage_ms[kMsHostWalk] = ms_between(t.h1, t_r); c->stage_ms[kMsRun] = ms_between(t.begin, t_r);
    return BDX_OK;
}

void record_timings(bdx_ctx* c, const RunClock& t) {
    const RunTime t_end = run_now();
    if (c->stage_timing) {
        (void)hipEventSynchronize(c->ev[5]);  // (complete by now; makes the elapsed-time queries valid)
        auto evms = [&](int a, int b) { float ms = 0; (void)hipEventElapsedTime(&ms, c->ev[a], c->ev[b]); return ms; };
        c->stage_ms[kMsCompact] = evms(2, 3);
        c->stage_ms[kMsCut] = evms(3, 4);
        c->stage_ms[kMsJoinAssemble] = evms(4, 5);
    }
    c->stage_ms[kMsGroupsWait] = ms_between(t.h0, t.h1);
    c->stage_ms[kMsHostWalk] = ms_between(t.h1, t.h2);
    c->stage_ms[kMsFinish] = ms_between(t.h2, t_end);
    c->stage_ms[kMsRun] = ms_between(t.begin, t_end);
}

}  // namespace

extern "C" {

// plan, route, receive, host walk, table or host finish, support, timings
int bdx_run(bdx_ctx* c) {
    if (!c) return BDX_EINVAL;
    NOT_WHILE_SIZING(c);
    RunClock t;
    t.begin = run_now();
    BDX_TRY(enqueue_device_half(c, plan_sizing(c), host_walks_all(c)));
    const uint32_t na = c->p1.n_anom;
    const uint32_t ph = (na && phantom_region_opt(c)) ? 1u : 0u;
    t.h0 = run_now();
    if (na) BDX_TRY(receive_regions_and_groups(c, ph));
    t.h1 = run_now();
    if (na && c->counts.irregular) return finish_by_replay(c, ph, t);
    BDX_TRY(host_walk(c, c->counts.last_maxq, na != 0));
    t.h2 = run_now();
    if (na) {
        BDX_TRY(do_k6_table(c));
        BDX_TRY(finish_table(c));
    } else {
        BDX_TRY(finish_host_walk(c));
    }
    if (c->collect_support) {
        materialize(c);
        BDX_TRY(collect_support(c, ph));
    }
    record_timings(c, t);
    return BDX_OK;
}

int bdx_get_summary(const bdx_ctx* c, bdx_summary* o) {
    if (!c || !o) return BDX_EINVAL;
    if (!c->ran) return BDX_ESTATE;
    o->n_reads = c->n; o->n_anomalous = c->p1.n_anom; o->covered_ref_len = c->g_covered; o->window = c->g_window;
    o->n_candidates = c->counts.n_cand; o->n_regions = (uint32_t)c->nreg; o->n_pairs = c->counts.n_pairs;
    o->n_groups = c->n_groups_total; o->n_svs = c->n_sv_total; o->n_svs_printed = c->n_printed;
    return BDX_OK;
}

int bdx_get_counters(const bdx_ctx* c, uint32_t* lib_read_count, uint32_t* bam_read_count, uint32_t* flag_hist, float* seqcov,
                     float* density) {
    if (!c) return BDX_EINVAL;
    if (!c->ran) return BDX_ESTATE;
    const uint32_t* hist = c->cnt.data();
    const uint32_t* lib_cnt = hist + c->nlibs * kNumFlags;
    const uint32_t* bam_cnt = lib_cnt + c->nlibs;
    if (flag_hist) memcpy(flag_hist, hist, (size_t)c->nlibs * kNumFlags * 4);
    if (lib_read_count) memcpy(lib_read_count, lib_cnt, (size_t)c->nlibs * 4);
    if (bam_read_count) memcpy(bam_read_count, bam_cnt, (size_t)c->nbams * 4);
    if (seqcov) memcpy(seqcov, c->seqcov.data(), (size_t)c->nlibs * 4);
    if (density) memcpy(density, c->lib_density.data(), (size_t)c->nlibs * 4);
    return BDX_OK;
}

int bdx_get_regions(const bdx_ctx* c, bdx_region* out, size_t cap) {
    if (!c || (!out && cap)) return BDX_EINVAL;
    if (!c->ran) return BDX_ESTATE;
    const size_t n = std::min(cap, c->nreg);
    for (size_t i = 0; i < n; ++i) {
        const HostRegion& r = c->reg[i];
        const int valid = c->opts.chr_restricted ? (int)r.nonctx : (int)r.n;
        out[i] = bdx_region{r.tid, r.start, r.end, (int32_t)r.nnormal, (int32_t)(r.n - r.rev), (int32_t)r.rev, (int32_t)r.n,
                            valid >= c->opts.min_read_pair ? 1 : 0, r.maxq};
    }
    return BDX_OK;
}

int bdx_get_svs(const bdx_ctx* c, bdx_sv* out, size_t cap) {
    if (!c || (!out && cap)) return BDX_EINVAL;
    if (!c->ran) return BDX_ESTATE;
    materialize(const_cast<bdx_ctx*>(c));
    const size_t n = std::min(cap, c->walk.svs.size());
    for (size_t i = 0; i < n; ++i) out[i] = c->walk.svs[i].sv;
    return BDX_OK;
}

int bdx_trim_results(bdx_ctx* c) {
    if (!c) return BDX_EINVAL;
    if (!c->ran) return BDX_ESTATE;
    NOT_WHILE_SIZING(c);
    HIPCHK(c, hipSetDevice(c->device));
    materialize(c);
    own_borrowed_regions(c);   // (a region table read where the device left it: the getters go on from a copy)
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (PinBuf* b : {&c->sb.h_regs, &c->sb.h_pk, &c->sb.h_groups, &c->sb.h_sv_out, &c->sb.h_lib_index, &c->sb.h_lib_pairs, &c->sb.h_cn_key, &c->sb.h_cn_value, &c->sb.h_ltail_dev}) b->release();
    return BDX_OK;
}

int bdx_get_sv_lists(const bdx_ctx* c, int32_t* lib_index, int32_t* lib_pairs, size_t lib_cap, int32_t* cn_key, float* cn_value,
                     size_t cn_cap) {
    if (!c) return BDX_EINVAL;
    if (!c->ran) return BDX_ESTATE;
    materialize(const_cast<bdx_ctx*>(c));
    const size_t nl = std::min(lib_cap, c->walk.lib_index.size());
    if (lib_index) memcpy(lib_index, c->walk.lib_index.data(), nl * 4);
    if (lib_pairs) memcpy(lib_pairs, c->walk.lib_pairs.data(), nl * 4);
    const size_t nc = std::min(cn_cap, c->walk.cn_key.size());
    if (cn_key) memcpy(cn_key, c->walk.cn_key.data(), nc * 4);
    if (cn_value) memcpy(cn_value, c->walk.cn_value.data(), nc * 4);
    return BDX_OK;
}

int bdx_set_collect_support(bdx_ctx* c, int on) {
    if (!c) return BDX_EINVAL;
    c->collect_support = on != 0;
    return BDX_OK;
}

int bdx_get_sv_support(const bdx_ctx* c, uint32_t* sv_offsets, uint64_t* read_index, uint8_t* read_flag, size_t cap, size_t* n_total) {
    if (!c) return BDX_EINVAL;
    if (!c->ran || !c->collect_support || c->sup_off.size() != c->walk.svs.size() + 1) return BDX_ESTATE;
    if (n_total) *n_total = c->sup_idx.size();
    if (sv_offsets) memcpy(sv_offsets, c->sup_off.data(), c->sup_off.size() * 4);
    const size_t n = std::min(cap, c->sup_idx.size());
    if (read_index && n) memcpy(read_index, c->sup_idx.data(), n * 8);
    if (read_flag && n) memcpy(read_flag, c->sup_flag.data(), n);
    return BDX_OK;
}

int bdx_get_read_class(const bdx_ctx* c, uint8_t* out, size_t cap) {
    if (!c || !out) return BDX_EINVAL;
    if (!c->ran) return BDX_ESTATE;
    const size_t n = std::min(cap, c->n);
    if (n && hipMemcpy(out, c->b_cls.p, n, hipMemcpyDeviceToHost) != hipSuccess) return BDX_EHIP;
    return BDX_OK;
}

int bdx_set_stage_timing(bdx_ctx* c, int on) {
    if (!c) return BDX_EINVAL;
    c->stage_timing = on != 0;
    return BDX_OK;
}

int bdx_set_enqueue_ahead(bdx_ctx* c, int on) {
    if (!c) return BDX_EINVAL;
    c->speculate = on < 0 ? 0 : (on > 2 ? 2 : on);
    return BDX_OK;
}

int bdx_run_many(bdx_ctx* const* ctxs, size_t n, int in_flight) {
    if (!ctxs && n) return BDX_EINVAL;
    for (size_t i = 0; i < n; ++i) {
        if (!ctxs[i]) return BDX_EINVAL;
        for (size_t k = 0; k < i; ++k)
            if (ctxs[k] == ctxs[i]) return BDX_EINVAL;   // (one context cannot run twice at a time)
    }
    const size_t workers = std::min<size_t>(n, (size_t)std::max(1, in_flight));
    if (workers <= 1) {
        for (size_t i = 0; i < n; ++i) {
            BDX_TRY(bdx_run(ctxs[i]));
        }
        return BDX_OK;
    }
    // one host thread per context in flight: a run's waits (pass-1 statistics, the exact sizes of the later stages, the table's
    // arrival) are the thread's own, and the kernels of the contexts overlap on the GPU -- each context has its own streams
    std::atomic<size_t> next{0};
    std::atomic<int> first_error{BDX_OK};
    std::vector<std::thread> pool;
    pool.reserve(workers);
    for (size_t w = 0; w < workers; ++w)
        pool.emplace_back([&] {
            for (;;) {
                const size_t i = next.fetch_add(1);
                if (i >= n || first_error.load() != BDX_OK) return;
                const int rc = bdx_run(ctxs[i]);
                if (rc != BDX_OK) {
                    int ok = BDX_OK;
                    first_error.compare_exchange_strong(ok, rc);
                }
            }
        });
    for (auto& t : pool) t.join();
    return first_error.load();
}

int bdx_use_name_check(bdx_ctx* c, int on) {
    if (!c) return BDX_EINVAL;
    if ((on != 0) == c->use_check) return BDX_OK;
    if (c->n) return fail(c, BDX_ESTATE, "the second name hash is switched while the context holds no reads");
    HIPCHK(c, hipSetDevice(c->device));
    c->use_check = on != 0;
    if (c->use_check && c->cap && !c->adopted) {
        HIPCHK(c, c->b_check.ensure(c->cap * 8));
        c->d.check = c->b_check.as<uint64_t>();
    }
    if (!c->use_check) c->d.check = nullptr;
    return BDX_OK;
}

uint32_t bdx_clip_word(const uint32_t* cigar, uint32_t n_cigar, int32_t l_seq, uint32_t flag) {
    return cigar || !n_cigar ? clip_word((const uint8_t*)cigar, n_cigar, l_seq, flag) : 0u;
}

int bdx_use_clips(bdx_ctx* c, int on) {
    if (!c) return BDX_EINVAL;
    if ((on != 0) == c->use_clips) return BDX_OK;
    if (c->n) return fail(c, BDX_ESTATE, "the clip column is switched while the context holds no reads");
    if (on && c->adopted) return fail(c, BDX_ESTATE, "an adopted store cannot carry clip words");
    HIPCHK(c, hipSetDevice(c->device));
    c->use_clips = on != 0;
    if (c->use_clips && c->cap) {
        HIPCHK(c, c->b_clip.ensure(c->cap * 4));
        HIPCHK(c, hipMemsetAsync(c->b_clip.p, 0, c->cap * 4, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    if (!c->use_clips) c->b_clip.release();
    return BDX_OK;
}

int bdx_put_clips(bdx_ctx* c, size_t first, const uint32_t* clip, size_t n) {
    if (!c) return BDX_EINVAL;
    if (!c->use_clips) return fail(c, BDX_ESTATE, "the context has no clip column (bdx_use_clips)");
    if (first > c->n || n > c->n - first) return fail(c, BDX_EINVAL, "clip words for records the context does not hold");
    if (n == 0) return BDX_OK;
    if (!clip) return fail(c, BDX_EINVAL, "null array");
    HIPCHK(c, hipSetDevice(c->device));
    // Through a pinned buffer of the context's (a ring of four, like the batches'): `clip` is free when the call returns and nobody waits
    // for the copy, which goes on the copy stream behind the batches' own; the compute stream waits for it by an event, so every later
    // run or query sees the rows.
    bdx_ctx::ClipStage& st = c->clip_ring[c->clip_next];
    c->clip_next = (c->clip_next + 1) % 4;
    if (st.busy) {
        HIPCHK(c, hipEventSynchronize(st.done));
        st.busy = false;
    }
    if (!st.done) HIPCHK(c, st.done.create(hipEventDisableTiming));
    HIPCHK(c, st.buf.ensure(n * 4));
    memcpy(st.buf.p, clip, n * 4);
    HIPCHK(c, hipMemcpyAsync(c->b_clip.as<uint32_t>() + first, st.buf.p, n * 4, hipMemcpyHostToDevice, c->copy_stream));
    HIPCHK(c, hipEventRecord(st.done, c->copy_stream));
    st.busy = true;
    HIPCHK(c, hipStreamWaitEvent(c->stream, st.done, 0));
    return BDX_OK;
}

int bdx_get_clips(bdx_ctx* c, uint32_t* out, size_t cap) {
    if (!c) return BDX_EINVAL;
    if (!c->use_clips) return fail(c, BDX_ESTATE, "the context has no clip column (bdx_use_clips)");
    const size_t n = std::min(cap, c->n);
    if (n == 0) return BDX_OK;
    if (!out) return fail(c, BDX_EINVAL, "null array");
    HIPCHK(c, hipSetDevice(c->device));
    if (c->copy_stream) HIPCHK(c, hipStreamSynchronize(c->copy_stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(out, c->b_clip.p, n * 4, hipMemcpyDeviceToHost));
    return BDX_OK;
}

int bdx_set_mark_duplicates(bdx_ctx* c, int on) {
    if (!c) return BDX_EINVAL;
    if ((on != 0) == c->mark_dup) return BDX_OK;
    if (c->n) return fail(c, BDX_ESTATE, "duplicate marking is switched while the context holds no reads");
    c->mark_dup = on != 0;
    c->k1_live = false;
    c->dup_done = false;
    c->dup_marked = 0; c->dup_groups = 0;
    return BDX_OK;
}

int bdx_get_duplicates(const bdx_ctx* c, uint64_t* n_marked, uint64_t* n_groups) {
    if (!c) return BDX_EINVAL;
    if (!c->ran) return BDX_ESTATE;
    const bool have = c->mark_dup && c->dup_done;
    if (n_marked) *n_marked = have ? c->dup_marked : 0;
    if (n_groups) *n_groups = have ? c->dup_groups : 0;
    return BDX_OK;
}

int bdx_mark_duplicates(int device, const int32_t* tid, const int32_t* pos, const int32_t* mtid, const int32_t* mpos, const uint16_t* flag,
                        const uint8_t* lib, const uint64_t* name_key, size_t n, uint8_t* mask, uint64_t* n_groups) {
    if (n_groups) *n_groups = 0;
    if (n == 0) return BDX_OK;
    if (!tid || !pos || !mtid || !mpos || !flag || !lib || !name_key || !mask) return BDX_EINVAL;
    if (n >= ((size_t)1 << 32)) return BDX_ELIMIT;
    if (hipSetDevice(device) != hipSuccess) return BDX_EHIP;
    DevBuf col[7], out;
    KdScratch k;
    const void* src[7] = {tid, pos, mtid, mpos, flag, lib, name_key};
    const size_t esz[7] = {4, 4, 4, 4, 2, 1, 8};
    for (int i = 0; i < 7; ++i) {
        if (col[i].ensure(n * esz[i]) != hipSuccess) return BDX_ENOMEM;
        if (hipMemcpy(col[i].p, src[i], n * esz[i], hipMemcpyHostToDevice) != hipSuccess) return BDX_EHIP;
    }
    if (out.ensure(n) != hipSuccess) return BDX_ENOMEM;
    KdParams p{};
    p.tid = col[0].as<int32_t>(); p.pos = col[1].as<int32_t>(); p.mtid = col[2].as<int32_t>(); p.mpos = col[3].as<int32_t>();
    p.flag = col[4].as<uint16_t>(); p.lib = col[5].as<uint8_t>(); p.key = col[6].as<uint64_t>(); p.n = n;
    uint64_t marked = 0, groups = 0;
    BDX_TRY(kd_run(nullptr, p, k, nullptr, out.as<uint8_t>(), nullptr, &marked, &groups));
    if (hipDeviceSynchronize() != hipSuccess || hipMemcpy(mask, out.p, n, hipMemcpyDeviceToHost) != hipSuccess) return BDX_EHIP;
    if (n_groups) *n_groups = groups;
    return BDX_OK;
}

int bdx_set_debug(bdx_ctx* c, const char* name, int value) {
    if (!c || !name) return BDX_EINVAL;
    struct { const char* n; int* p; } ints[] = {{"no_stash", &c->dbg_no_stash}, {"max_chunks", &c->dbg_max_chunks}, {"spec_test", &c->spec_test},
                                                 {"big_walk", &c->big_walk_mode}, {"ins_plain", &c->dbg_ins_plain}, {"regions_copy", &c->dbg_regions_copy},
                                                 {"asm_plain", &c->dbg_asm_plain}, {"gather_walk", &c->dbg_gather_walk}, {"depth_plain", &c->dbg_depth_plain}, {"mini_staged", &c->dbg_mini_staged}};
    for (auto& e : ints)
        if (!strcmp(name, e.n)) { *e.p = value; return BDX_OK; }
    if (!strcmp(name, "bucketed_join")) { c->bucketed_join = value != 0; return BDX_OK; }
    if (!strcmp(name, "no_poll")) { c->poll = value == 0; return BDX_OK; }
    return fail(c, BDX_EINVAL, std::string("unknown debug switch ") + name);
}

int bdx_set_host_walk(bdx_ctx* c, int on) {
    if (!c) return BDX_EINVAL;
    c->host_walk_only = on != 0;
    return BDX_OK;
}

int bdx_get_walk_split(const bdx_ctx* c, uint32_t* n_sv_device, uint32_t* n_sv_host, uint32_t* n_groups_host) {
    if (!c) return BDX_EINVAL;
    if (!c->ran) return BDX_ESTATE;
    if (n_sv_device) *n_sv_device = c->counts.n_sv_dev;
    if (n_sv_host) *n_sv_host = c->n_sv_host;
    if (n_groups_host) *n_groups_host = c->counts.n_groups;
    return BDX_OK;
}

int bdx_get_cross_window_svs(const bdx_ctx* c, uint32_t* n_sv_device) {
    if (!c || !n_sv_device) return BDX_EINVAL;
    if (!c->ran) return BDX_ESTATE;
    *n_sv_device = c->counts.n_old;
    return BDX_OK;
}

int bdx_set_pass1_statistics(bdx_ctx* c, const uint32_t* counters, uint32_t covered_ref_len) {
    if (!c) return BDX_EINVAL;
    if (!counters) { c->ov_cnt.clear(); return BDX_OK; }
    c->ov_cnt.assign(counters, counters + (size_t)c->nlibs * kNumFlags + c->nlibs + c->nbams);
    c->ov_covered = covered_ref_len;
    c->ran = false;
    return BDX_OK;
}

int bdx_was_replayed(const bdx_ctx* c) { return c && c->ran && c->replayed ? 1 : 0; }

int bdx_get_timings(const bdx_ctx* c, float* ms, int cap) {
    if (!c || !ms) return 0;
    const int n = std::min(cap, kNumStages);
    for (int i = 0; i < n; ++i) ms[i] = c->stage_ms[i];
    return n;
}

int bdx_classify(const bdx_opts* opts, const bdx_lib* libs, int nlibs, const bdx_batch* b, uint8_t* cls_out, int device) {
    if (!opts || !libs || !b || !cls_out) return BDX_EINVAL;
    int nbams = 1;
    for (int i = 0; i < nlibs; ++i) nbams = std::max(nbams, libs[i].bam_index + 1);
    for (size_t i = 0; i < b->n; ++i) nbams = std::max(nbams, (int)b->bam[i] + 1);
    bdx_ctx* c = nullptr;
    BDX_TRY(bdx_create(&c, opts, libs, nlibs, nbams, 0, 100000000, device));
    std::unique_ptr<bdx_ctx, void (*)(bdx_ctx*)> owner(c, bdx_destroy);
    BDX_TRY(bdx_push(c, b));
    BDX_TRY(bdx_run(c));
    return bdx_get_read_class(c, cls_out, b->n);
}

// ---- queries over the resident store: K8, KS, KI, KM (kq_queries.hip) and KR (kr_depth.hip) ----

// What the calls check first, in this order: a context, no sizing pass in flight, a run that classified the store.  *none: n == 0, nothing to do.
static int check_query_state(bdx_ctx* c, size_t n, bool* none) {
    *none = false;
    if (!c) return BDX_EINVAL;
    NOT_WHILE_SIZING(c);
    if (c->cls_n != c->n && !(c->ran && c->n == 0)) return fail(c, BDX_ESTATE, "no run has classified the reads this context holds");
    *none = n == 0;
    return BDX_OK;
}

static StoreView store_view(const bdx_ctx* c) {
    return StoreView{c->d.tid, c->d.pos, c->d.mtid, c->d.mpos, c->d.isize, c->d.flag, c->b_cls.as<uint8_t>(), c->n};
}

// the key column of the counting calls (a context with one library / one file never copies the respective column: every read is key 0 there)
static const uint8_t* key_column(const bdx_ctx* c, int by_library, int nkeys) { return nkeys > 1 ? (by_library ? c->d.lib : c->d.bam) : nullptr; }

// The call sequence the three share: the host arrays of `up` go to the device one behind the other, `launch` gets where they start, where
// the results go and the stream, and the call returns when the results are in `out`.
struct QueryUpload { const void* src; size_t bytes; };
static int run_query(bdx_ctx* c, std::initializer_list<QueryUpload> up, void* out, size_t out_bytes,
                     const std::function<void(const char* in, void* results, hipStream_t s)>& launch) {
    HIPCHK(c, hipSetDevice(c->device));
    size_t in_bytes = 0;
    for (const QueryUpload& u : up) in_bytes += u.bytes;
    HIPCHK(c, c->b_qin.ensure(in_bytes));
    HIPCHK(c, c->b_qout.ensure(out_bytes));
    hipStream_t s = c->stream;
    char* in = c->b_qin.as<char>();
    for (const QueryUpload& u : up) {
        if (u.bytes) HIPCHK(c, hipMemcpyAsync(in, u.src, u.bytes, hipMemcpyHostToDevice, s));
        in += u.bytes;
    }
    launch(c->b_qin.as<char>(), c->b_qout.p, s);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(out, c->b_qout.p, out_bytes, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    return BDX_OK;
}

int bdx_count_junction_pairs(bdx_ctx* c, const int32_t* tid, const int32_t* pos_a, const int32_t* pos_b, size_t n, int by_library,
                             uint32_t* counts) {
    bool none;
    BDX_TRY(check_query_state(c, n, &none));
    if (none) return BDX_OK;
    if (!tid || !pos_a || !pos_b || !counts) return fail(c, BDX_EINVAL, "null array");
    for (size_t i = 0; i < n; ++i)
        if (tid[i] < 0 || pos_a[i] < 1 || pos_a[i] > pos_b[i])
            return fail(c, BDX_EINVAL, "query " + std::to_string(i) + ": tid < 0, pos_a < 1 or pos_a > pos_b");
    if (n > ((size_t)1 << 31)) return fail(c, BDX_ELIMIT, "more than 2^31 queries in one call");
    const int nkeys = by_library ? c->nlibs : c->nbams;
    // K1 calls a pair normal only if (float)|isize| is not above its library's upper cutoff (-l's remaps included: NORMAL_RF needs it
    // below the cutoff) and |isize| <= -m.  Every such integer lies below the float that follows the cutoff (a NaN cutoff bounds nothing).
    double ub = -1.0;
    for (const bdx_lib& l : c->libs) {
        const float u = l.uppercutoff;
        ub = std::max(ub, std::isnan(u) || u == INFINITY ? 2147483647.0 : std::ceil((double)std::nextafter(u, INFINITY)) - 1.0);
    }
    const int32_t lmax = (int32_t)std::max(-1.0, std::min<double>({ub, (double)c->opts.max_sd, 2147483647.0}));
    return run_query(c, {{tid, n * 4}, {pos_a, n * 4}, {pos_b, n * 4}}, counts, n * (size_t)nkeys * 4, [&](const char* in, void* results, hipStream_t s) {
        const int32_t* q = (const int32_t*)in;
        launch_k8(K8Params{store_view(c), key_column(c, by_library, nkeys), q, q + n, q + 2 * n, (uint32_t)n, nkeys, lmax, (uint32_t*)results}, s);
    });
}

// What bdx_count_site_pairs, bdx_site_breakpoint_bounds and bdx_site_end_quality check before they touch the device, in this order.
// *none: n == 0, nothing to do.  others: the call's other arrays (its results; bdx_site_end_quality's ends) are all there.
static int check_site_call(bdx_ctx* c, const bdx_site* sites, size_t n, int32_t window, bool others, bool* none) {
    BDX_TRY(check_query_state(c, n, none));
    if (*none) return BDX_OK;
    if (!sites || !others) return fail(c, BDX_EINVAL, "null array");
    if (window < 0 || window > (1 << 30)) return fail(c, BDX_EINVAL, "window < 0 or window > 2^30");
    if (n > ((size_t)1 << 31)) return fail(c, BDX_ELIMIT, "more than 2^31 sites in one call");
    for (size_t i = 0; i < n; ++i) {
        const bdx_site& s = sites[i];
        if (s.tid1 < 0 || s.tid2 < 0 || s.pos1 < 1 || s.pos2 < 1)
            return fail(c, BDX_EINVAL, "site " + std::to_string(i) + ": tid < 0 or pos < 1");
        if (s.tid1 > s.tid2 || (s.tid1 == s.tid2 && s.pos1 > s.pos2))
            return fail(c, BDX_EINVAL, "site " + std::to_string(i) + ": not normalised, (tid1, pos1) > (tid2, pos2)");
        if (s.flag_mask == 0 || (s.flag_mask & ~BDX_SITE_FLAGS))
            return fail(c, BDX_EINVAL, "site " + std::to_string(i) + ": flag_mask is 0 or has a bit outside the anomalous classes");
    }
    return BDX_OK;
}

int bdx_count_site_pairs(bdx_ctx* c, const bdx_site* sites, size_t n, int32_t window, int by_library, uint32_t* counts) {
    bool none;
    BDX_TRY(check_site_call(c, sites, n, window, counts != nullptr, &none));
    if (none) return BDX_OK;
    const int nkeys = by_library ? c->nlibs : c->nbams;
    return run_query(c, {{sites, n * sizeof(bdx_site)}}, counts, n * (size_t)nkeys * 4, [&](const char* in, void* results, hipStream_t s) {
        launch_ks(KsParams{store_view(c), key_column(c, by_library, nkeys), (const KsSite*)in, (uint32_t)n, nkeys, window, (uint32_t*)results}, s);
    });
}

int bdx_site_breakpoint_bounds(bdx_ctx* c, const bdx_site* sites, size_t n, int32_t window, bdx_site_bounds* out) {
    bool none;
    BDX_TRY(check_site_call(c, sites, n, window, out != nullptr, &none));
    if (none) return BDX_OK;
    // U per library: ceil(uppercutoff); 0 when that is negative; 2^30 when the cutoff is NaN, infinite or above 2^30
    std::vector<uint32_t> u(c->libs.size());
    for (size_t i = 0; i < u.size(); ++i) {
        const double v = (double)c->libs[i].uppercutoff;
        u[i] = !std::isfinite(v) || v > 1073741824.0 ? (1u << 30) : (v < 0 ? 0u : (uint32_t)std::ceil(v));
    }
    const int nlibs = c->nlibs;
    const bool many = nlibs > 1;   // (a context with one library never copies the lib column, and its U travels with the launch: no table)
    const size_t sbytes = n * sizeof(bdx_site);
    return run_query(c, {{sites, sbytes}, {u.data(), many ? u.size() * 4 : 0}}, out, n * sizeof(bdx_site_bounds), [&](const char* in, void* results, hipStream_t s) {
        launch_ki(KiParams{store_view(c), many ? c->d.lib : nullptr, (const KsSite*)in, (uint32_t)n, nlibs, window, c->opts.illumina_long_insert ? 1 : 0,
                           u.empty() ? 0u : u[0], many ? (const uint32_t*)(in + sbytes) : nullptr, (KiBounds*)results}, s);
    });
}

int bdx_site_end_quality(bdx_ctx* c, const bdx_site* sites, const uint8_t* end, size_t n, int32_t window, bdx_site_quality* out) {
    bool none;
    BDX_TRY(check_site_call(c, sites, n, window, end && out, &none));
    if (none) return BDX_OK;
    for (size_t i = 0; i < n; ++i)
        if (end[i] != 1 && end[i] != 2) return fail(c, BDX_EINVAL, "query " + std::to_string(i) + ": end is neither 1 nor 2");
    std::vector<int32_t> least(c->libs.size());
    for (size_t i = 0; i < least.size(); ++i) least[i] = resolved_min_mapq(c->opts, c->libs[i]);
    const int nlibs = c->nlibs;
    const bool many = nlibs > 1;   // (as in bdx_site_breakpoint_bounds: one library's minimum travels with the launch, and its lib column is never read)
    const size_t sbytes = n * sizeof(bdx_site), tbytes = many ? least.size() * 4 : 0;   // (the table in front of the ends: it wants 4-byte alignment)
    return run_query(c, {{sites, sbytes}, {least.data(), tbytes}, {end, n}}, out, n * sizeof(bdx_site_quality), [&](const char* in, void* results, hipStream_t s) {
        launch_km(KmParams{store_view(c), c->d.mapq, many ? c->d.lib : nullptr, nlibs, least.empty() ? 0 : least[0], many ? (const int32_t*)(in + sbytes) : nullptr,
                           (const KsSite*)in, (const uint8_t*)(in + sbytes + tbytes), (uint32_t)n, window, (KmQuality*)results}, s);
    });
}

int bdx_site_clip_peaks(bdx_ctx* c, const bdx_site* sites, const uint8_t* end, size_t n, int32_t window, int32_t min_clip, bdx_clip_peaks* out) {
    if (!c) return BDX_EINVAL;
    if (!c->use_clips) return fail(c, BDX_ESTATE, "the context has no clip column (bdx_use_clips)");
    bool none;
    BDX_TRY(check_site_call(c, sites, n, window, end && out, &none));
    if (none) return BDX_OK;
    if (window > BDX_CLIP_WINDOW_MAX) return fail(c, BDX_EINVAL, "window > " + std::to_string(BDX_CLIP_WINDOW_MAX));
    if (min_clip < 1 || min_clip > 255) return fail(c, BDX_EINVAL, "min_clip < 1 or min_clip > 255");
    for (size_t i = 0; i < n; ++i)
        if (end[i] != 1 && end[i] != 2) return fail(c, BDX_EINVAL, "query " + std::to_string(i) + ": end is neither 1 nor 2");
    const size_t sbytes = n * sizeof(bdx_site);
    return run_query(c, {{sites, sbytes}, {end, n}}, out, n * sizeof(bdx_clip_peaks), [&](const char* in, void* results, hipStream_t s) {
        launch_kp(KpParams{store_view(c), c->b_clip.as<uint32_t>(), (const KsSite*)in, (const uint8_t*)(in + sbytes), (uint32_t)n, window, min_clip, (KpPeaks*)results}, s);
    });
}

// Passing read starts inside given intervals (KR, kr_depth.hip): the table of passing records in front of every chunk of the store is built
// by the call itself, in a scratch buffer, ahead of the queries on the same stream; "depth_plain" answers without one.
int bdx_count_interval_reads(bdx_ctx* c, const bdx_interval* iv, size_t n, int by_library, uint32_t* counts) {
    bool none;
    BDX_TRY(check_query_state(c, n, &none));
    if (none) return BDX_OK;
    if (!iv || !counts) return fail(c, BDX_EINVAL, "null array");
    if (n > ((size_t)1 << 31)) return fail(c, BDX_ELIMIT, "more than 2^31 intervals in one call");
    for (size_t i = 0; i < n; ++i)
        if (iv[i].tid < 0 || iv[i].beg < 0 || iv[i].end < iv[i].beg)
            return fail(c, BDX_EINVAL, "interval " + std::to_string(i) + ": tid < 0, beg < 0 or end < beg");
    const int nkeys = by_library ? c->nlibs : c->nbams;
    const uint32_t nchunks = (uint32_t)((c->n + BDX_DEPTH_CHUNK - 1) / BDX_DEPTH_CHUNK);
    const bool table = !c->dbg_depth_plain && nchunks;
    if (table) {
        HIPCHK(c, hipSetDevice(c->device));
        HIPCHK(c, c->b_qtab.ensure((size_t)nkeys * ((size_t)nchunks + 1) * 4));
    }
    return run_query(c, {{iv, n * sizeof(bdx_interval)}}, counts, n * (size_t)nkeys * 4, [&](const char* in, void* results, hipStream_t s) {
        const KrParams p{store_view(c), key_column(c, by_library, nkeys), (const KrInterval*)in, (uint32_t)n, nkeys, nchunks,
                         table ? c->b_qtab.as<uint32_t>() : nullptr, (uint32_t*)results};
        launch_kr_table(p, s);
        launch_kr_query(p, s);
    });
}

// ---- --estimate: the insert-size histogram of the store (KH, kh_insert_hist.hip), the estimate and the libraries of the runs that follow ----

int bdx_insert_size_histogram(bdx_ctx* c, uint64_t* hist, uint64_t* n_over) {
    if (!c) return BDX_EINVAL;
    if (!hist || !n_over) return fail(c, BDX_EINVAL, "null array");
    NOT_WHILE_SIZING(c);
    static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "the device table is copied out as it is");
    const size_t nh = (size_t)c->nlibs * BDX_ISIZE_BINS, nw = nh + (size_t)c->nlibs;
    if (c->n == 0) {
        memset(hist, 0, nh * 8);
        memset(n_over, 0, (size_t)c->nlibs * 8);
        return BDX_OK;
    }
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t s = c->stream;
    if (c->copy_pending) {  // batches pushed since the last classifier launch
        HIPCHK(c, hipStreamWaitEvent(s, c->ev_copy, 0));
        c->copy_pending = false;
    }
    HIPCHK(c, c->b_hist.ensure(nw * 8));
    HIPCHK(c, hipMemsetAsync(c->b_hist.p, 0, nw * 8, s));
    KhParams p{};
    p.tid = c->d.tid; p.mtid = c->d.mtid; p.isize = c->d.isize; p.flag = c->d.flag; p.mapq = c->d.mapq;
    p.lib = c->nlibs > 1 ? c->d.lib : nullptr;   // (with one library the column is not copied)
    p.n = c->n; p.nlibs = c->nlibs; p.libs = c->b_libs.as<DevLib>(); p.lib_mean = c->b_lib_mean.as<float>();
    p.hist = c->b_hist.as<unsigned long long>(); p.n_over = p.hist + nh;
    launch_kh(p, s);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(hist, p.hist, nh * 8, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipMemcpyAsync(n_over, p.n_over, (size_t)c->nlibs * 8, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    return BDX_OK;
}

int bdx_estimate_insert_size(const uint64_t* hist, bdx_insert_estimate* out) {
    if (!hist || !out) return BDX_EINVAL;
    estimate_insert_size(hist, out);
    return BDX_OK;
}

int bdx_set_libs(bdx_ctx* c, const bdx_lib* libs, int nlibs, int max_read_window_size0) {
    if (!c) return BDX_EINVAL;
    if (!libs) return fail(c, BDX_EINVAL, "null array");
    if (nlibs != c->nlibs) return fail(c, BDX_EINVAL, "the number of libraries is not the context's");
    for (int i = 0; i < nlibs; ++i)
        if (libs[i].bam_index != c->libs[i].bam_index) return fail(c, BDX_EINVAL, "library " + std::to_string(i) + ": bam_index is not the one given at creation");
    NOT_WHILE_SIZING(c);
    HIPCHK(c, hipSetDevice(c->device));
    std::vector<DevLib> dl(nlibs);
    std::vector<float> means(nlibs);
    for (int i = 0; i < nlibs; ++i) {
        dl[i].upper = libs[i].uppercutoff;
        dl[i].lower = libs[i].lowercutoff;
        dl[i].min_mapq = resolved_min_mapq(c->opts, libs[i]);
        dl[i].key = c->opts.cn_lib ? i : libs[i].bam_index;
        means[i] = libs[i].mean_insertsize;
    }
    // in stream order: behind the classifier launches that followed the batches under the old libraries (their results are dropped below)
    HIPCHK(c, hipMemcpyAsync(c->b_libs.p, dl.data(), (size_t)nlibs * sizeof(DevLib), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->b_lib_mean.p, means.data(), (size_t)nlibs * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));   // (the two vectors go with this call)
    c->libs.assign(libs, libs + nlibs);
    c->w0 = max_read_window_size0;
    // a live or finished pass 1 belongs to the old cutoffs: the next run classifies from tile 0 through pass1_prepare
    c->k1_live = false;
    c->k1_done = 0;
    c->ran = false;
    c->cls_n = (size_t)-1;
    return BDX_OK;
}

// ---- --mini: the null's cumulative table and the windows' insert-size shift (KW, km_mini.hip); the score is bdx_mini.h's ----

int bdx_set_insert_null(bdx_ctx* c, const uint64_t* hist) {
    if (!c) return BDX_EINVAL;
    NOT_WHILE_SIZING(c);
    HIPCHK(c, hipSetDevice(c->device));
    if (!hist) {
        HIPCHK(c, hipStreamSynchronize(c->stream));
        c->b_null.release();
        c->null_set = false;
        return BDX_OK;
    }
    const size_t nh = (size_t)c->nlibs * BDX_ISIZE_BINS;
    std::vector<uint64_t> cum(nh);
    for (int l = 0; l < c->nlibs; ++l) {
        uint64_t run = 0;
        for (size_t x = 0; x < BDX_ISIZE_BINS; ++x) {
            const uint64_t h = hist[(size_t)l * BDX_ISIZE_BINS + x];
            if (h >= ((uint64_t)1 << 51) || (run += h) >= ((uint64_t)1 << 51))
                return fail(c, BDX_ELIMIT, "library " + std::to_string(l) + ": the null holds 2^51 observations or more");
            cum[(size_t)l * BDX_ISIZE_BINS + x] = run;
        }
    }
    HIPCHK(c, c->b_null.ensure(nh * 8));
    HIPCHK(c, hipMemcpyAsync(c->b_null.p, cum.data(), nh * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));   // (the vector goes with this call)
    c->null_set = true;
    return BDX_OK;
}

int bdx_window_insert_shift(bdx_ctx* c, const bdx_interval* iv, size_t n, bdx_insert_shift* out) {
    bool none;
    BDX_TRY(check_query_state(c, n, &none));
    if (!c->null_set) return fail(c, BDX_ESTATE, "no null distribution is set (bdx_set_insert_null)");
    if (none) return BDX_OK;
    if (!iv || !out) return fail(c, BDX_EINVAL, "null array");
    if (n > ((size_t)1 << 31)) return fail(c, BDX_ELIMIT, "more than 2^31 intervals in one call");
    for (size_t i = 0; i < n; ++i)
        if (iv[i].tid < 0 || iv[i].beg < 0 || iv[i].end < iv[i].beg)
            return fail(c, BDX_EINVAL, "interval " + std::to_string(i) + ": tid < 0, beg < 0 or end < beg");
    const int nlibs = c->nlibs;
    return run_query(c, {{iv, n * sizeof(bdx_interval)}}, out, n * (size_t)nlibs * sizeof(bdx_insert_shift), [&](const char* in, void* results, hipStream_t s) {
        launch_kw(KwParams{store_view(c), nlibs > 1 ? c->d.lib : nullptr, (const KrInterval*)in, (uint32_t)n, nlibs, c->b_null.as<uint64_t>(),
                           c->dbg_mini_staged ? 1 : 0, (KwShift*)results}, s);
    });
}

int bdx_insert_shift_score(const bdx_insert_shift* row, uint64_t N, double* score, double* D) {
    if (!row) return BDX_EINVAL;
    insert_shift_score(*row, N, score, D);
    return BDX_OK;
}

// ---- --anchor: the one-end-anchored reads of given windows and their best split (KA, ka_anchor.hip) ----

int bdx_window_anchor_split(bdx_ctx* c, const bdx_interval* iv, size_t n, int32_t min_qual, bdx_anchor_split* out) {
    bool none;
    BDX_TRY(check_query_state(c, n, &none));
    if (none) return BDX_OK;
    if (!iv || !out) return fail(c, BDX_EINVAL, "null array");
    if (min_qual < -1 || min_qual > 255) return fail(c, BDX_EINVAL, "min_qual < -1 or min_qual > 255");
    if (n > ((size_t)1 << 31)) return fail(c, BDX_ELIMIT, "more than 2^31 intervals in one call");
    for (size_t i = 0; i < n; ++i)
        if (iv[i].tid < 0 || iv[i].beg < 0 || iv[i].end < iv[i].beg)
            return fail(c, BDX_EINVAL, "interval " + std::to_string(i) + ": tid < 0, beg < 0 or end < beg");
    // quality ABOVE least: the libraries' minima as K1 resolved them, or min_qual - 1 for every library (then no table and no lib column)
    std::vector<int32_t> least(c->libs.size());
    for (size_t i = 0; i < least.size(); ++i) least[i] = min_qual < 0 ? resolved_min_mapq(c->opts, c->libs[i]) : min_qual - 1;
    const int nlibs = c->nlibs;
    const bool many = nlibs > 1 && min_qual < 0;
    const size_t ibytes = n * sizeof(bdx_interval);   // (12 n: the table behind it is 4-aligned)
    return run_query(c, {{iv, ibytes}, {least.data(), many ? least.size() * 4 : 0}}, out, n * sizeof(bdx_anchor_split), [&](const char* in, void* results, hipStream_t s) {
        launch_ka(KaParams{store_view(c), c->d.mapq, many ? c->d.lib : nullptr, (const KrInterval*)in, (uint64_t)n, nlibs, c->opts.illumina_long_insert ? 1 : 0,
                           least.empty() ? 0 : least[0], many ? (const int32_t*)(in + ibytes) : nullptr, (KaSplit*)results}, s);
    });
}

int bdx_set_process_option(const char* name, int value) {
    if (!name) return BDX_EINVAL;
    if (!strcmp(name, "pin_malloc")) { PinBuf::registered_switch().store(value == 0); return BDX_OK; }
    return BDX_EINVAL;
}

int bdx_warm_up(int device) {
    if (hipSetDevice(device) != hipSuccess) return BDX_EHIP;
    warm_k1(nullptr); warm_k2(nullptr); warm_k3(nullptr); warm_k4(nullptr); warm_k5(nullptr); warm_k6(nullptr); warm_k7(nullptr); warm_k9(nullptr);
    warm_kx(nullptr); warm_kq(nullptr); warm_kr(nullptr); warm_kp(nullptr); warm_ka(nullptr);
    return hipDeviceSynchronize() == hipSuccess && hipGetLastError() == hipSuccess ? BDX_OK : BDX_EHIP;
}

int bdx_poisson_log_upper_tail(const double* lambda, const int32_t* k, double* out, size_t n, int device) {
    if (!lambda || !k || !out) return BDX_EINVAL;
    if (n == 0) return BDX_OK;
    if (hipSetDevice(device) != hipSuccess) return BDX_EHIP;
    DevBuf bl, bk, bo;
    if (bl.ensure(n * 8) != hipSuccess || bk.ensure(n * 4) != hipSuccess || bo.ensure(n * 8) != hipSuccess) return BDX_ENOMEM;
    if (hipMemcpy(bl.p, lambda, n * 8, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(bk.p, k, n * 4, hipMemcpyHostToDevice) != hipSuccess)
        return BDX_EHIP;
    launch_k5(bl.as<double>(), bk.as<int32_t>(), bo.as<double>(), (uint32_t)n, nullptr);
    if (hipDeviceSynchronize() != hipSuccess || hipGetLastError() != hipSuccess) return BDX_EHIP;
    if (hipMemcpy(out, bo.p, n * 8, hipMemcpyDeviceToHost) != hipSuccess) return BDX_EHIP;
    return BDX_OK;
}

}  // extern "C"

#include "bdx_dist_impl.h"
#include "bdx_bamdec_impl.h"
