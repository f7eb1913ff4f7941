// Chromosome-sharded runs: one whole-genome result from chromosomes spread over several GPUs (include/bdx.h, bdx_dist_*).
// Included at the end of bdx_api.hip (it drives the stage functions of that translation unit).
//
// The path shards by chromosome -- regions never span tids (BreakDancer.cpp:216) -- and what a single breakdancer-max run
// couples across chromosomes is small: the pass-1 statistics (window, lambda, densities: BamSummary.cpp:129-150,
// BreakDancerMax.cpp:83-116), the running counters sampled at region boundaries, the read that closes a chromosome's
// last candidate region (BreakDancer.cpp:202-231), the region numbering / flush cadence (BreakDancer.cpp:254-259), and the
// inter-chromosomal read pairs (ARP_CTX).  Every rank (one per GPU) holds ALL of its chromosomes in ONE context and runs the
// single-context launch sequence over them -- K1 ... K6 and the table kernel, one launch each whatever the number of
// chromosomes --, with per-chromosome tables (k9_shard.hip) carrying what crosses a chromosome boundary.  Region ids are
// genome-wide on every rank, so flush windows, order keys and the walk itself are the single run's.  FIVE collectives per run
// (round 5: eleven -- six all-reduces, two all-to-alls, three gathers, each behind a host round trip):
//   A   all-reduce (host words): pass-1 counters, per-file reference lengths, per-chromosome totals and owners, every chromosome's
//       first anomalous read, and what the one all-to-all will carry -- inter-chromosomal reads by mate chromosome, census records by
//       owner (the compaction runs in front of it: it needs nothing of the other ranks)
//   B   all-reduce (host words): every chromosome's region count -> genome-wide region ids (every entry has one owner: a sum is a gather)
//   X   ONE all-to-all: per destination the inter-chromosomal join records -- a CTX read whose mate lies on a later chromosome of
//       another rank goes there and joins that rank's reads (k7_exchange.hip) --, the census records of the names it owns, and the read
//       lengths of the flush windows this rank closes.  From here to its finished table a rank waits for nobody: which components span
//       ranks is known without an exchange (a region that sent a join record away, or was joined with a foreign one, is an end of one)
//   S   all-reduce (host words): what every rank will send to rank 0 (pair groups of the components that span ranks or that its device
//       walk leaves, rows and list entries of its table), and whether a read name misbehaved
//   G   ONE gather: every rank's package -- its region records, those pair groups, its finished table (rows sorted by order key) -- to
//       rank 0, which walks the gathered groups in its result context (K6 once more, on the device) and merges the tables by key
// bdx_dist_run reads like this list.  In front of every collective stands a local phase of DistRun whose failure travels with the next
// all-reduce, behind it what every rank derives from the sums (a struct that is const from then on):
//   pass1_and_counts -> A agree_statistics (Stats) -> cut_regions -> B agree_regions (Regions) -> seed_result -> plan_exchange (ExchangePlan),
//   globalize_and_scatter -> X all_to_all -> join_walk_table -> S agree_packages (Summary) -> plan_packages (Packages), pack_and_gather (G) ->
//   rank 0: place_regions, walk_gathered, merge_tables.  Behind S a run may instead take replay_route (a read name seen more than twice, or
//   the supporting reads are wanted: two gathers of their own and rank 0's read-level walk) or, on one rank, adopt_own_table.
// Payloads stay in HBM: the all-to-all and the gather run on device buffers through RCCL (ncclAllToAllv, grouped ncclSend / ncclRecv),
// xGMI between the GPUs of a node; the three all-reduces carry a few KB of host words (staged through device words for RCCL).  A second
// backend runs the ranks as threads of one process (tests on a single GPU; a host program that drives several GPUs itself).
#include <dlfcn.h>

#include <condition_variable>
#include <map>
#include <memory>
#include <mutex>

namespace {

// The timing slots of a run (bdx_dist_get_phase_ms / bdx_dist_phase_name): ONE row gives a slot its enum value and its name.  Up to S a
// local phase and the collective behind it (which includes waiting for the slowest rank) alternate; five slots are spare.
#define BDX_DIST_PHASES(X)                                                         \
    X(kPhPass1, "pass1_compaction_first_reads")                                    \
    X(kPhAllreduceStatistics, "allreduce_statistics_first_reads_exchange_counts") \
    X(kPhSpare2, "")                                                               \
    X(kPhSpare3, "")                                                               \
    X(kPhRegionCut, "rebase_and_region_cut")                                       \
    X(kPhAllreduceRegions, "allreduce_regions")                                    \
    X(kPhGlobalizePack, "globalize_and_pack")                                      \
    X(kPhAlltoall, "alltoall_join_records_census_windows")                         \
    X(kPhSpare8, "")                                                               \
    X(kPhSpare9, "")                                                               \
    X(kPhJoinsWalkTable, "joins_components_walk_table")                            \
    X(kPhAllreducePackages, "allreduce_package_sizes")                             \
    X(kPhSpare12, "")                                                              \
    X(kPhGather, "gather_packages_to_rank0")                                       \
    X(kPhMerge, "rank0_only_merge")                                                \
    X(kPhReplayRoute, "replay_route")                                              \
    X(kPhHostWalk, "rank0_only_host_walk")                                         \
    X(kPhDeviceWalkGathered, "rank0_only_device_walk_of_gathered_groups")
#define BDX_DIST_PHASE_ID(id, name) id,
#define BDX_DIST_PHASE_NAME(id, name) name,
enum DistPhase : int { BDX_DIST_PHASES(BDX_DIST_PHASE_ID) kDistPhases };
constexpr const char* kDistPhaseName[kDistPhases] = {BDX_DIST_PHASES(BDX_DIST_PHASE_NAME)};
static_assert(kDistPhases == 18, "bdx_dist_get_phase_ms: the callers read eighteen slots");
constexpr size_t kGatherHostMax = 2048;   // gathered pair groups up to which rank 0's HOST walks them (more: K6 on the device)

// ------------------------------------------------------------------------------------------------------------------
// communicators
// ------------------------------------------------------------------------------------------------------------------
struct Comm {
    int rank = 0, world = 1;
    std::string err;
    virtual ~Comm() {}
    uint32_t n_allreduce = 0, n_alltoall = 0, n_gather = 0;   // collectives entered since begin_run (bdx_dist_get_collectives)
    virtual void begin_run() {}   // start of a bdx_dist_run (collective)
    virtual void abort() {}       // this rank leaves the run between two collectives: wake whoever waits for it
    // in place sum over the ranks of n 64-bit words in HOST memory, without the device: false = this backend has no such path (the caller
    // stages the words through device memory and calls allreduce_u64)
    virtual bool allreduce_host_u64(uint64_t*, size_t, bool* done) { *done = false; return true; }
    // in place sum over the ranks of n 64-bit words in device memory
    virtual bool allreduce_u64(uint64_t* dev, size_t n, hipStream_t s) = 0;
    // rank r sends scount[d] words from send + sdispl[d] to rank d and receives rcount[d] words from rank d at recv + rdispl[d]
    virtual bool alltoallv_u64(const uint64_t* send, const size_t* scount, const size_t* sdispl, uint64_t* recv, const size_t* rcount,
                               const size_t* rdispl, hipStream_t s) = 0;
    // every rank sends n bytes (n a multiple of 8) to the root, which places rank r's at recv + displ[r] (count[r] bytes)
    virtual bool gatherv_bytes(const void* send, size_t n, void* recv, const size_t* count, const size_t* displ, int root, hipStream_t s) = 0;
};

// ---- RCCL (one process per GPU) -- resolved at run time so that single-GPU users do not depend on librccl ----
struct RcclApi {
    void* lib = nullptr;
    int (*GetUniqueId)(void*) = nullptr;
    int (*CommInitRank)(void**, int, bdx_unique_id, int) = nullptr;
    int (*CommDestroy)(void*) = nullptr;
    int (*AllReduce)(const void*, void*, size_t, int, int, void*, hipStream_t) = nullptr;
    int (*AllToAllv)(const void*, const size_t*, const size_t*, void*, const size_t*, const size_t*, int, void*, hipStream_t) = nullptr;
    int (*Send)(const void*, size_t, int, int, void*, hipStream_t) = nullptr;
    int (*Recv)(void*, size_t, int, int, void*, hipStream_t) = nullptr;
    int (*GroupStart)() = nullptr;
    int (*GroupEnd)() = nullptr;
    const char* (*GetErrorString)(int) = nullptr;
    int (*GetVersion)(int*) = nullptr;
    std::string err, path;
    int version = 0;
    bool load() {
        if (lib) return true;
        for (const char* name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) {
            lib = dlopen(name, RTLD_NOW | RTLD_GLOBAL);
            if (lib) break;
        }
        if (!lib) { err = std::string("librccl not found: ") + dlerror(); return false; }
        auto sym = [&](const char* n) { void* p = dlsym(lib, n); if (!p) err = std::string("librccl lacks ") + n; return p; };
        GetUniqueId = (decltype(GetUniqueId))sym("ncclGetUniqueId");
        CommInitRank = (decltype(CommInitRank))sym("ncclCommInitRank");
        CommDestroy = (decltype(CommDestroy))sym("ncclCommDestroy");
        AllReduce = (decltype(AllReduce))sym("ncclAllReduce");
        AllToAllv = (decltype(AllToAllv))sym("ncclAllToAllv");
        Send = (decltype(Send))sym("ncclSend");
        Recv = (decltype(Recv))sym("ncclRecv");
        GroupStart = (decltype(GroupStart))sym("ncclGroupStart");
        GroupEnd = (decltype(GroupEnd))sym("ncclGroupEnd");
        GetErrorString = (decltype(GetErrorString))sym("ncclGetErrorString");
        GetVersion = (decltype(GetVersion))dlsym(lib, "ncclGetVersion");
        if (GetVersion) (void)GetVersion(&version);
        {   // which file the loader resolved the name to (a process that imported torch first has torch's bundled copy mapped already)
            Dl_info info{};
            if (GetUniqueId && dladdr((void*)GetUniqueId, &info) && info.dli_fname) path = info.dli_fname;
        }
        return err.empty();
    }
};
RcclApi& rccl() { static RcclApi a; return a; }
constexpr int kNcclUint8 = 1, kNcclUint64 = 5, kNcclSum = 0;  // ncclDataType_t / ncclRedOp_t values of rccl.h

struct RcclComm : Comm {
    void* comm = nullptr;
    bool ok(int rc, const char* what) {
        if (rc == 0) return true;
        err = std::string(what) + ": " + (rccl().GetErrorString ? rccl().GetErrorString(rc) : "RCCL error");
        return false;
    }
    ~RcclComm() override { if (comm) (void)rccl().CommDestroy(comm); }
    void begin_run() override { n_allreduce = n_alltoall = n_gather = 0; }
    bool allreduce_u64(uint64_t* dev, size_t n, hipStream_t s) override {
        ++n_allreduce;
        return ok(rccl().AllReduce(dev, dev, n, kNcclUint64, kNcclSum, comm, s), "ncclAllReduce");
    }
    bool alltoallv_u64(const uint64_t* send, const size_t* scount, const size_t* sdispl, uint64_t* recv, const size_t* rcount,
                       const size_t* rdispl, hipStream_t s) override {
        ++n_alltoall;
        return ok(rccl().AllToAllv(send, scount, sdispl, recv, rcount, rdispl, kNcclUint64, comm, s), "ncclAllToAllv");
    }
    bool gatherv_bytes(const void* send, size_t n, void* recv, const size_t* count, const size_t* displ, int root, hipStream_t s) override {
        ++n_gather;
        if (!ok(rccl().GroupStart(), "ncclGroupStart")) return false;
        bool good = true;
        if (n) good = ok(rccl().Send(send, n, kNcclUint8, root, comm, s), "ncclSend");
        if (good && rank == root)
            for (int r = 0; r < world && good; ++r)
                if (count[r]) good = ok(rccl().Recv((char*)recv + displ[r], count[r], kNcclUint8, r, comm, s), "ncclRecv");
        const bool ended = ok(rccl().GroupEnd(), "ncclGroupEnd");
        return good && ended;
    }
};

// ---- ranks as threads of one process: collectives as device-to-device copies around a barrier ----
struct ThreadGroup {
    int world = 1;
    std::atomic<int> arrived{0};
    std::atomic<uint64_t> generation{0};
    std::vector<const void*> ptr;      // what every rank published for the collective in progress
    std::vector<const size_t*> cnt, dsp;
    std::vector<std::vector<uint64_t>> host;  // allreduce staging
    std::vector<uint64_t*> hptr;       // host all-reduce: every rank's words
    std::atomic<bool> failed{false};   // a collective of the run in progress went wrong on some rank
    std::atomic<bool> aborted{false};  // a rank left bdx_dist_run early: nobody may wait for it at a barrier
    explicit ThreadGroup(int w) : world(w), ptr(w), cnt(w), dsp(w), host(w), hptr(w) {}
    // false: the group was aborted (by a rank that gave up between two collectives) -- the caller fails its collective.
    // The ranks spin (a run's barriers are microseconds apart and a condition variable's wake-up cost 30-50 us each, twice per
    // collective: the larger part of round 5's 0.08-0.17 ms per all-reduce); a rank that has waited for a while yields its core.
    bool barrier() {
        if (aborted.load(std::memory_order_acquire)) return false;
        const uint64_t g = generation.load(std::memory_order_acquire);
        if (arrived.fetch_add(1, std::memory_order_acq_rel) + 1 == world) {
            arrived.store(0, std::memory_order_relaxed);
            generation.fetch_add(1, std::memory_order_release);
            return true;
        }
        for (uint32_t spin = 0;; ++spin) {
            if (generation.load(std::memory_order_acquire) != g) return true;
            if (aborted.load(std::memory_order_acquire)) return generation.load(std::memory_order_acquire) != g;
            if (spin < 20000u) __builtin_ia32_pause(); else std::this_thread::yield();
        }
    }
    void abort() { aborted.store(true, std::memory_order_release); }
    // every rank calls this at the start of a run, before its first collective: the flags of the previous run are history.
    // (Two barriers: nobody clears while somebody may still be reading, nobody proceeds before the flags are clear.)
    void begin_run(int rank) {
        if (aborted.load()) return;  // an aborted group stays aborted: its ranks are out of step for good
        barrier();
        if (rank == 0) failed.store(false);
        barrier();
    }
};

struct ThreadComm : Comm {
    std::shared_ptr<ThreadGroup> g;
    bool hip(hipError_t e, const char* what) {
        if (e == hipSuccess) return true;
        err = std::string(what) + ": " + hipGetErrorString(e);
        g->failed.store(true);
        return false;
    }
    bool gone() { err = "another rank left the run"; return false; }
    void begin_run() override { n_allreduce = n_alltoall = n_gather = 0; g->begin_run(rank); }
    void abort() override { g->abort(); }
    bool allreduce_host_u64(uint64_t* v, size_t n, bool* done) override {
        *done = true;
        ++n_allreduce;
        g->hptr[rank] = v;
        if (!g->barrier()) return gone();
        std::vector<uint64_t>& sum = g->host[rank];
        sum.assign(n, 0);
        for (int r = 0; r < world; ++r)
            for (size_t i = 0; i < n; ++i) sum[i] += g->hptr[r][i];
        if (!g->barrier()) return gone();  // (everybody has read everybody's words)
        memcpy(v, sum.data(), n * 8);
        return !g->failed;
    }
    bool allreduce_u64(uint64_t* dev, size_t n, hipStream_t s) override {
        ++n_allreduce;
        std::vector<uint64_t>& mine = g->host[rank];
        mine.resize(n);
        bool good = hip(hipMemcpyAsync(mine.data(), dev, n * 8, hipMemcpyDeviceToHost, s), "hipMemcpyAsync") && hip(hipStreamSynchronize(s), "sync");
        if (!g->barrier()) return gone();
        std::vector<uint64_t> sum(n, 0);
        for (int r = 0; r < world; ++r)
            for (size_t i = 0; i < n && i < g->host[r].size(); ++i) sum[i] += g->host[r][i];
        if (!g->barrier()) return gone();  // (everybody has read everybody's words)
        good = good && hip(hipMemcpyAsync(dev, sum.data(), n * 8, hipMemcpyHostToDevice, s), "hipMemcpyAsync") && hip(hipStreamSynchronize(s), "sync");
        return good && !g->failed;
    }
    bool alltoallv_u64(const uint64_t* send, const size_t* scount, const size_t* sdispl, uint64_t* recv, const size_t* rcount,
                       const size_t* rdispl, hipStream_t s) override {
        ++n_alltoall;
        bool good = hip(hipStreamSynchronize(s), "sync");  // the send buffer is complete
        g->ptr[rank] = send; g->cnt[rank] = scount; g->dsp[rank] = sdispl;
        if (!g->barrier()) return gone();
        for (int r = 0; r < world && good; ++r) {
            const size_t n = g->cnt[r][rank];
            if (n != rcount[r]) { err = "all-to-all counts disagree"; g->failed.store(true); good = false; break; }
            if (n) good = hip(hipMemcpyAsync(recv + rdispl[r], (const uint64_t*)g->ptr[r] + g->dsp[r][rank], n * 8, hipMemcpyDefault, s), "hipMemcpyAsync");
        }
        good = good && hip(hipStreamSynchronize(s), "sync");
        if (!g->barrier()) return gone();  // (the send buffers may be reused)
        return good && !g->failed;
    }
    bool gatherv_bytes(const void* send, size_t n, void* recv, const size_t* count, const size_t* displ, int root, hipStream_t s) override {
        ++n_gather;
        bool good = hip(hipStreamSynchronize(s), "sync");
        g->ptr[rank] = send;
        if (!g->barrier()) return gone();
        if (rank == root) {
            for (int r = 0; r < world && good; ++r)
                if (count[r]) good = hip(hipMemcpyAsync((char*)recv + displ[r], g->ptr[r], count[r], hipMemcpyDefault, s), "hipMemcpyAsync");
            good = good && hip(hipStreamSynchronize(s), "sync");
        }
        (void)n;
        if (!g->barrier()) return gone();
        return good && !g->failed;
    }
};

}  // namespace

struct bdx_dist {
    // Order of release: bdx_dist_destroy destroys the two contexts first (the streams everything here runs on are theirs: each is
    // synchronised as its context goes); the buffers and the event below go with the members, behind them and before `comm`'s turn.
    int device = 0, ntids = 0, nlibs = 0, nbams = 0, nkeys = 0, w0 = 0;
    bdx_opts opts{};
    std::vector<bdx_lib> libs;
    std::unique_ptr<Comm> comm;
    bdx_ctx* reads = nullptr;        // ALL chromosomes this rank owns, one after the other in ascending order: one launch sequence
    bdx_ctx* util = nullptr;         // rank 0: holds the result
    int last_tid = -1;               // bdx_dist_chromosome: the chromosomes must be fed in ascending order
    size_t sorted_n = 0;             // the reads whose reference-id column has been checked (check_order): this many ...
    const void* sorted_ptr = nullptr;  // ... at this address
    size_t n_at_last = 0;
    bool use_check = false;
    DevBuf b_words, b_tab, b_send, b_recv, b_pack, b_all, b_nsend, b_nrecv, b_ntab, b_nflag, b_foreign, b_rg_rec, b_rg_pk, b_x, b_merge, b_chk, b_bucket;
    PinBuf h_words;                  // staging of the all-reduces' words (pinned: the copies either side of a collective are asynchronous)
    PinBuf h_tab;                    // what the small kernels report: per-chromosome tables, counts, ready words
    Event ev_side;                   // the name census runs on the context's second stream, beside the joins
    uint32_t seq = 0;
    std::string err;
    uint64_t ctx_sent = 0, ctx_received = 0, gathered_bytes = 0;
    float ms_total = 0, ms_exchange = 0;
    bool ran = false;
    float phase_ms[kDistPhases] = {0};   // bdx_dist_get_phase_ms: where the last run's time went on this rank
    bool table_lent = false;         // (one rank) the result context holds this rank's pinned table buffers until the next run
    bool collect_support = false;    // bdx_dist_set_collect_support: the supporting reads of every SV (-g / -d) come with the result
};

namespace {

int dfail(bdx_dist* d, int code, const std::string& msg) {
    if (d) d->err = msg;
    return code;
}
#define DHIP(d, expr)                                                                                   \
    do {                                                                                                \
        hipError_t _e = (expr);                                                                         \
        if (_e != hipSuccess) return dfail(d, BDX_EHIP, std::string(#expr) + ": " + hipGetErrorString(_e)); \
    } while (0)
#define DCTX(d, c, expr)                                                                     \
    do {                                                                                     \
        const int _rc = (expr);                                                              \
        if (_rc != BDX_OK) return dfail(d, _rc, std::string(#expr) + ": " + (c)->err);       \
    } while (0)

// host vector -> device words -> all-reduce -> host vector
int allreduce_host(bdx_dist* d, std::vector<uint64_t>& v, hipStream_t s) {
    if (v.empty()) return BDX_OK;
    // (one rank: the sum is the vector itself -- no copies, no collective, and above all no wait for the stream: the device walk that is
    // enqueued when the host's share is agreed on keeps running beside the host's walk, as in bdx_run)
    if (d->comm->world == 1) return BDX_OK;
    {   // (ranks of one process: the words never leave the host)
        bool done = false;
        if (!d->comm->allreduce_host_u64(v.data(), v.size(), &done)) return dfail(d, BDX_EHIP, d->comm->err);
        if (done) return BDX_OK;
    }
    DHIP(d, d->b_words.ensure(v.size() * 8));
    DHIP(d, d->h_words.ensure(v.size() * 8));
    memcpy(d->h_words.p, v.data(), v.size() * 8);
    DHIP(d, hipMemcpyAsync(d->b_words.p, d->h_words.p, v.size() * 8, hipMemcpyHostToDevice, s));
    if (!d->comm->allreduce_u64(d->b_words.as<uint64_t>(), v.size(), s)) return dfail(d, BDX_EHIP, d->comm->err);
    DHIP(d, hipMemcpyAsync(d->h_words.p, d->b_words.p, v.size() * 8, hipMemcpyDeviceToHost, s));
    DHIP(d, hipStreamSynchronize(s));
    memcpy(v.data(), d->h_words.p, v.size() * 8);
    return BDX_OK;
}

int dist_create_common(bdx_dist** out, const bdx_opts* opts, const bdx_lib* libs, int nlibs, int nbams, int ntids, int w0, int device,
                       std::unique_ptr<Comm> comm) {
    if (!out || !opts || !libs || nlibs < 1 || nbams < 1 || ntids < 1) return BDX_EINVAL;
    if (comm->world >= kMaxRanks || ntids >= (1 << 24) - 1) return BDX_ELIMIT;   // (one table package per rank and one for rank 0's result context: k9_merge_tables)
    bdx_dist* d = new (std::nothrow) bdx_dist;
    if (!d) return BDX_ENOMEM;
    d->device = device; d->ntids = ntids; d->nlibs = nlibs; d->nbams = nbams; d->w0 = w0;
    d->opts = *opts;
    d->libs.assign(libs, libs + nlibs);
    d->nkeys = opts->cn_lib ? nlibs : nbams;
    d->comm = std::move(comm);
    int rc = bdx_create(&d->reads, opts, libs, nlibs, nbams, ntids, w0, device);
    if (rc == BDX_OK && d->comm->rank == 0) rc = bdx_create(&d->util, opts, libs, nlibs, nbams, ntids, w0, device);
    if (rc == BDX_OK && d->ev_side.create(hipEventDisableTiming) != hipSuccess) rc = BDX_EHIP;
    if (rc != BDX_OK) { bdx_dist_destroy(d); return rc; }
    d->reads->force_direct_join = true;
    *out = d;
    return BDX_OK;
}

inline size_t nkeys_words(int nkeys) { return (size_t)nkeys + 1; }

// pinned report area of a rank: ready words, then the tables the small kernels write
struct TabLayout {
    size_t flags = 0, tidtab = 0, first = 0, rtab = 0, cnts = 0, misc = 0, up_off = 0, up_tail = 0, up_misc = 0, up_cur = 0, up_stats = 0, up_counts = 0, words = 0;
    TabLayout(int ntids, int ncols, int nkeys, int ncnt, int world) {
        size_t o = 16;
        tidtab = o; o += (size_t)(ntids + 1) * (1 + ncols) + 2;
        first = o; o += (size_t)ntids * 4;
        rtab = o; o += (size_t)ntids + 3;
        cnts = o; o += (size_t)ntids + 2 * (size_t)world;   // (inter-chromosomal reads by mate chromosome | census records by owner)
        misc = o; o += 16;
        // staging of the small tables that go UP to the device: pinned, so that the copies are asynchronous and the vectors they were
        // built in need not outlive them (every table has its own place: nothing is overwritten within a run)
        up_off = o; o += (size_t)ntids * (1 + nkeys);
        up_tail = o; o += (size_t)ntids * 4;
        up_misc = o; o += (size_t)3 * ntids + 1;
        up_cur = o; o += (size_t)2 * world;
        up_stats = o; o += (size_t)2 + ncnt + 64;
        up_counts = o; o += sizeof(StageCounts) / 4;
        words = o;
    }
};

// the small device tables of a rank (b_tab): tid_off [ntids][1 + nkeys] | tid_tail [ntids][4] | roff [ntids] | owner [ntids] | tid_start [ntids + 1] |
// cnt [4 world] | n_total [8] | rbase u64 [ntids + 1] | inter-chromosomal reads by mate chromosome [ntids]
struct DevTabLayout {
    size_t off = 0, tail = 0, roff = 0, owner = 0, start = 0, cnt = 0, ntot = 0, rbase = 0, mt = 0, words = 0;
    DevTabLayout(int ntids, int nkeys, int world) {
        size_t o = 0;
        off = o; o += (size_t)ntids * (1 + nkeys);
        tail = o; o += (size_t)ntids * 4;
        roff = o; o += (size_t)ntids;
        owner = o; o += (size_t)ntids;
        start = o; o += (size_t)ntids + 1;
        cnt = o; o += 4 * (size_t)world;
        ntot = o; o += 8;
        rbase = (o + 1) / 2 * 2; o = rbase + 2 * ((size_t)ntids + 1);   // (64-bit words: on an even word)
        mt = o; o += (size_t)ntids;
        words = o;
    }
};

// spin on a pinned word a one-thread kernel sets behind the kernels whose results it announces
bool wait_word(volatile uint32_t* w, uint32_t value) {
    const auto t0 = std::chrono::steady_clock::now();
    for (uint32_t spin = 0;; ++spin) {
        if (*w == value) { std::atomic_thread_fence(std::memory_order_acquire); return true; }
        __builtin_ia32_pause();
        if ((spin & 1023u) == 1023u && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(500)) return false;
    }
}

}  // namespace

extern "C" {

int bdx_dist_unique_id(bdx_unique_id* out) {
    if (!out) return BDX_EINVAL;
    if (!rccl().load()) return BDX_EHIP;
    return rccl().GetUniqueId(out) == 0 ? BDX_OK : BDX_EHIP;
}

int bdx_dist_create(bdx_dist** out, const bdx_opts* opts, const bdx_lib* libs, int nlibs, int nbams, int ntids,
                    int max_read_window_size0, int device, int rank, int world, const bdx_unique_id* id) {
    if (!out || world < 1 || rank < 0 || rank >= world || !id) return BDX_EINVAL;
    if (!rccl().load()) return BDX_EHIP;
    if (hipSetDevice(device) != hipSuccess) return BDX_EHIP;
    std::unique_ptr<RcclComm> c(new RcclComm);
    c->rank = rank; c->world = world;
    if (const int nrc = rccl().CommInitRank(&c->comm, world, *id, rank)) {   // (no handle yet to keep the message in)
        fprintf(stderr, "[bdx] ncclCommInitRank(rank %d of %d, device %d) failed: %s (%d)\n", rank, world, device,
                rccl().GetErrorString ? rccl().GetErrorString(nrc) : "RCCL error", nrc);
        return BDX_EHIP;
    }
    return dist_create_common(out, opts, libs, nlibs, nbams, ntids, max_read_window_size0, device, std::move(c));
}

int bdx_dist_create_threads(bdx_dist** out, const bdx_opts* opts, const bdx_lib* libs, int nlibs, int nbams, int ntids,
                            int max_read_window_size0, const int* devices, int world) {
    if (!out || !devices || world < 1) return BDX_EINVAL;
    std::shared_ptr<ThreadGroup> g(new ThreadGroup(world));
    for (int r = 0; r < world; ++r) out[r] = nullptr;
    // every rank's context (device set-up, streams, pinned words) on its own thread: side by side on different devices
    std::vector<int> rcs(world, BDX_OK);
    std::vector<std::thread> th;
    for (int r = 0; r < world; ++r)
        th.emplace_back([&, r] {
            std::unique_ptr<ThreadComm> c(new ThreadComm);
            c->rank = r; c->world = world; c->g = g;
            rcs[r] = dist_create_common(&out[r], opts, libs, nlibs, nbams, ntids, max_read_window_size0, devices[r], std::move(c));
        });
    for (auto& t : th) t.join();
    for (int r = 0; r < world; ++r)
        if (rcs[r] != BDX_OK) {
            const int rc = rcs[r];
            for (int q = 0; q < world; ++q) { if (out[q]) bdx_dist_destroy(out[q]); out[q] = nullptr; }
            return rc;
        }
    return BDX_OK;
}

void bdx_dist_destroy(bdx_dist* d) {
    if (!d) return;
    (void)hipSetDevice(d->device);
    if (d->reads) bdx_destroy(d->reads);
    if (d->util) bdx_destroy(d->util);
    delete d;
}

const char* bdx_dist_last_error(const bdx_dist* d) { return d ? d->err.c_str() : ""; }
int bdx_dist_rank(const bdx_dist* d) { return d ? d->comm->rank : -1; }
int bdx_dist_world(const bdx_dist* d) { return d ? d->comm->world : 0; }

// One context per rank takes all of the rank's chromosomes; the handle is the same for every tid.  What the caller must keep to
// is the order: a rank's chromosomes ascending, each chromosome's records together (the position-sorted stream gives both).
bdx_ctx* bdx_dist_chromosome(bdx_dist* d, int tid) {
    if (!d || tid < 0 || tid >= d->ntids) return nullptr;
    bdx_ctx* c = d->reads;
    if (tid < d->last_tid && c->n != d->n_at_last) {
        d->err = "bdx_dist_chromosome: a rank's chromosomes are fed in ascending order";
        return nullptr;
    }
    if (tid != d->last_tid) { d->last_tid = tid; }
    d->n_at_last = c->n;
    return c;
}

int bdx_dist_reset_reads(bdx_dist* d) {
    if (!d) return BDX_EINVAL;
    const int rc = bdx_reset_reads(d->reads);
    if (rc != BDX_OK) return dfail(d, rc, d->reads->err);
    d->last_tid = -1;
    d->n_at_last = 0;
    d->ran = false;
    d->sorted_n = 0; d->sorted_ptr = nullptr;   // (the next set of reads may have this one's count and address: its order is checked again)
    return BDX_OK;
}

namespace {
// The chromosome table is found by binary searches in the reference-id column (k9_tid_table_kernel): that column must be ascending with
// every id inside the header's sequences -- a rank's chromosomes fed in order, each chromosome's records together.  bdx_dist_chromosome
// sees to the order of the CALLS; what the batches hold is checked here, once per set of reads.
int check_order(bdx_dist* d) {
    bdx_ctx* c = d->reads;
    if (!c->n || (d->sorted_n == c->n && d->sorted_ptr == (const void*)c->d.tid)) return BDX_OK;
    DHIP(d, d->b_chk.ensure(64));
    uint32_t* err = d->b_chk.as<uint32_t>();
    uint32_t bad = 0;
    DHIP(d, hipMemsetAsync(err, 0, 4, c->stream));
    if (c->copy_pending) { DHIP(d, hipStreamWaitEvent(c->stream, c->ev_copy, 0)); }
    launch_k9_check_sorted((const int32_t*)c->d.tid, c->n, d->ntids, err, c->stream);
    DHIP(d, hipMemcpyAsync(&bad, err, 4, hipMemcpyDeviceToHost, c->stream));
    DHIP(d, hipStreamSynchronize(c->stream));
    if (bad) return dfail(d, BDX_EINVAL, "the reads of a rank are not in ascending order of their reference ids (or an id lies outside the header's sequences)");
    d->sorted_n = c->n; d->sorted_ptr = (const void*)c->d.tid;
    return BDX_OK;
}
}  // namespace

int bdx_dist_prepare(bdx_dist* d) {
    if (!d) return BDX_EINVAL;
    bdx_ctx* c = d->reads;
    DHIP(d, hipSetDevice(d->device));
    if (bdx_warm_up(d->device) != BDX_OK) return dfail(d, BDX_EHIP, "bdx_warm_up");
    {
        const int orc = check_order(d);
        if (orc != BDX_OK) return orc;
    }
    // the later stages' buffers for the prior a first run goes by (bdx_reserve does the same for a single context), with K6's
    // per-region arrays sized for the genome's regions rather than this rank's
    {
        const int ncols = 2 + d->nkeys, ncnt = d->nlibs * kNumFlags + d->nlibs + d->nbams, world = d->comm->world;
        const TabLayout L(d->ntids, ncols, d->nkeys, ncnt, world);
        DHIP(d, d->h_tab.ensure(L.words * 4));
        const size_t v1_words = (size_t)d->ntids * (ncols + 7 + (size_t)world) + ncnt + d->nbams + 11 * (size_t)world + (size_t)world * world + 64;   // (the first all-reduce's vector, the largest)
        DHIP(d, d->h_words.ensure(v1_words * 8));
        DHIP(d, d->b_words.ensure(v1_words * 8));
        DHIP(d, d->b_tab.ensure(((size_t)d->ntids * (nkeys_words(d->nkeys) + 12) + 8 * (size_t)world + 64) * 4));
        if (c->n && c->n < ((size_t)1 << 32)) {   // pass 1's tables for the reads that are loaded (a store that grew while it was filled lost them)
            const int rc = pass1_prepare(c, (uint32_t)((c->n + kTile - 1) / kTile));
            if (rc != BDX_OK) return dfail(d, rc, c->err);
            c->k1_live = false;
        }
    }
    if (c->n >= (1u << 20) && !c->ran) {
        const uint64_t prior = (uint64_t)c->n / 32 + 4096;
        if (prior <= kMaxAnomalous) {
            StageDims dm = stage_dims(c, (uint32_t)prior);   // (what a run sets on the context at its start: pass1_and_counts, globalize_and_scatter)
            dm.k6_cap = (uint32_t)std::min<uint64_t>(prior, kMaxRegions);
            dm.table_in_hbm = dm.groups_in_hbm = d->comm->world > 1;
            const int rc = presize_stages_here(c, dm);
            if (rc != BDX_OK) return dfail(d, rc, c->err);
            const size_t nr = (size_t)prior;
            DHIP(d, d->b_rg_rec.ensure(nr * sizeof(RegionRec)));
            DHIP(d, d->b_rg_pk.ensure(nr * 2 * d->nkeys * 4));
            DHIP(d, d->b_x.ensure(nr + nr / 8 + 1024));   // (taint bytes: one per region / anomalous read of the upper bound)
            const size_t nn = (size_t)prior;
            DHIP(d, d->b_ntab.ensure((size_t)k7_names_slots(nn) * 16));
            DHIP(d, d->b_pack.ensure(nn * 40)); DHIP(d, d->b_all.ensure(nn * 40));
            DHIP(d, d->b_foreign.ensure(nn * 20 / 8 + 64));
            DHIP(d, d->b_send.ensure(nn * 20 + 4096)); DHIP(d, d->b_recv.ensure(nn * 20 + 4096));   // (a census record of 16 bytes per anomalous read; an eighth of them inter-chromosomal and travelling, 32 bytes each)
            if (d->comm->rank == 0) {   // the genome's region table in pinned memory (regions: about a tenth of the anomalous reads)
                const size_t nreg = (size_t)c->n / 256 + 4096;
                DHIP(d, c->sb.h_regs.ensure(nreg * sizeof(RegionRec)));
                DHIP(d, c->sb.h_pk.ensure(nreg * 2 * d->nkeys * 4));
            }
        }
    }
    return BDX_OK;
}

int bdx_dist_get_phase_ms(const bdx_dist* d, float* out, int n) {
    if (!d || !out) return BDX_EINVAL;
    for (int i = 0; i < n; ++i) out[i] = i < kDistPhases ? d->phase_ms[i] : 0.0f;
    return BDX_OK;
}

const char* bdx_dist_phase_name(int i) { return i >= 0 && i < kDistPhases ? kDistPhaseName[i] : ""; }

int bdx_dist_set_collect_support(bdx_dist* d, int on) {
    if (!d) return BDX_EINVAL;
    d->collect_support = on != 0;
    return BDX_OK;
}

bdx_ctx* bdx_dist_result(bdx_dist* d) { return d && d->ran && d->comm->rank == 0 ? d->util : nullptr; }

// a test / measurement switch (bdx_set_debug's names) for the contexts of this rank: its own and, on rank 0, the result context
int bdx_dist_set_debug(bdx_dist* d, const char* name, int value) {
    if (!d || !name) return BDX_EINVAL;
    int rc = d->reads ? bdx_set_debug(d->reads, name, value) : BDX_OK;
    if (rc == BDX_OK && d->util) rc = bdx_set_debug(d->util, name, value);
    return rc;
}

// bdx_set_mark_duplicates for this rank's reads: a chromosome lives whole on one rank, so every run of equal (tid, pos) does too
int bdx_dist_set_mark_duplicates(bdx_dist* d, int on) {
    if (!d || !d->reads) return BDX_EINVAL;
    const int rc = bdx_set_mark_duplicates(d->reads, on);
    return rc == BDX_OK ? rc : dfail(d, rc, d->reads->err);
}

// bdx_insert_size_histogram over this rank's own store; the caller sums the ranks (threads of one process: no collective)
int bdx_dist_insert_size_histogram(bdx_dist* d, uint64_t* hist, uint64_t* n_over) {
    if (!d || !d->reads) return BDX_EINVAL;
    const int rc = bdx_insert_size_histogram(d->reads, hist, n_over);
    return rc == BDX_OK ? rc : dfail(d, rc, d->reads->err);
}

// bdx_set_libs for this rank's reads, for the result context on rank 0 and for the rank's own copy
int bdx_dist_set_libs(bdx_dist* d, const bdx_lib* libs, int nlibs, int max_read_window_size0) {
    if (!d || !d->reads) return BDX_EINVAL;
    int rc = bdx_set_libs(d->reads, libs, nlibs, max_read_window_size0);
    if (rc != BDX_OK) return dfail(d, rc, d->reads->err);
    if (d->util) {
        rc = bdx_set_libs(d->util, libs, nlibs, max_read_window_size0);
        if (rc != BDX_OK) return dfail(d, rc, d->util->err);
    }
    d->libs.assign(libs, libs + nlibs);
    d->w0 = max_read_window_size0;
    d->ran = false;
    return BDX_OK;
}

int bdx_dist_get_duplicates(const bdx_dist* d, uint64_t* n_marked, uint64_t* n_groups) {
    if (!d || !d->reads) return BDX_EINVAL;
    if (!d->ran) return BDX_ESTATE;
    const bdx_ctx* c = d->reads;
    const bool have = c->mark_dup && c->dup_done;
    if (n_marked) *n_marked = have ? c->dup_marked : 0;
    if (n_groups) *n_groups = have ? c->dup_groups : 0;
    return BDX_OK;
}

int bdx_dist_get_exchange(const bdx_dist* d, uint64_t* ctx_records_sent, uint64_t* ctx_records_received, uint64_t* gathered_bytes,
                          float* ms_total, float* ms_exchange) {
    if (!d) return BDX_EINVAL;
    if (!d->ran) return BDX_ESTATE;
    if (ctx_records_sent) *ctx_records_sent = d->ctx_sent;
    if (ctx_records_received) *ctx_records_received = d->ctx_received;
    if (gathered_bytes) *gathered_bytes = d->gathered_bytes;
    if (ms_total) *ms_total = d->ms_total;
    if (ms_exchange) *ms_exchange = d->ms_exchange;
    return BDX_OK;
}

int bdx_dist_get_collectives(const bdx_dist* d, uint32_t out[3], const char** backend, int* rccl_version) {
    if (!d) return BDX_EINVAL;
    if (!d->ran) return BDX_ESTATE;
    if (out) { out[0] = d->comm->n_allreduce; out[1] = d->comm->n_alltoall; out[2] = d->comm->n_gather; }
    const bool is_rccl = dynamic_cast<const RcclComm*>(d->comm.get()) != nullptr;
    if (backend) *backend = is_rccl ? rccl().path.c_str() : "threads";
    if (rccl_version) *rccl_version = is_rccl ? rccl().version : 0;
    return BDX_OK;
}

int bdx_dist_owner(uint64_t name_key, int world) { return world > 0 ? (int)exchange_owner(name_key, (uint32_t)world) : -1; }

// longest-processing-time packing: chromosomes in descending weight, each onto the least loaded rank (ties: lower rank)
int bdx_dist_plan(const uint64_t* weight, int ntids, int world, int* rank_of_tid) {
    if (!weight || !rank_of_tid || ntids < 0 || world < 1) return BDX_EINVAL;
    std::vector<int> order(ntids);
    for (int i = 0; i < ntids; ++i) order[i] = i;
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return weight[a] > weight[b]; });
    std::vector<uint64_t> load(world, 0);
    for (int t : order) {
        int best = 0;
        for (int r = 1; r < world; ++r)
            if (load[r] < load[best]) best = r;
        rank_of_tid[t] = best;
        load[best] += weight[t];
    }
    return BDX_OK;
}

}  // extern "C"

namespace {

// A failure that only one rank sees (its own data, its own device) must not make that rank leave while the others enter
// the next collective: they would wait for it for ever.  Every stage between two collectives therefore runs as a local
// phase whose status travels with the next all-reduce (one word per rank behind the payload); all ranks look at the
// summed words and give up together.  What cannot be folded (a device allocation failing between the size exchange and
// the all-to-all, anything behind collective S) aborts the communicator of the thread backend, which wakes its waiters
// with an error: DistRun::others_wait and the one exit rule in bdx_dist_run.
struct RunStatus {
    int rc = BDX_OK;      // this rank's first failure
    std::string msg;
};

int agreed_failure(bdx_dist* d, const RunStatus& st, const uint64_t* words, int world) {
    int first = -1, code = BDX_OK;
    for (int q = 0; q < world; ++q)
        if (words[q]) { first = q; code = (int)words[q]; break; }
    if (first < 0) return BDX_OK;
    if (st.rc != BDX_OK) return dfail(d, st.rc, st.msg);
    return dfail(d, code, "rank " + std::to_string(first) + " failed (" + bdx_strerror(code) + "); all ranks stop");
}

// the result of a rank's context becomes the result context's: the pinned buffers the device assembled the table in change
// hands (no copy), the counters are taken over
void swap_table_buffers(bdx_ctx* U, bdx_ctx* C) {
    std::swap(U->sb.h_sv_out, C->sb.h_sv_out); std::swap(U->sb.h_lib_index, C->sb.h_lib_index); std::swap(U->sb.h_lib_pairs, C->sb.h_lib_pairs);
    std::swap(U->sb.h_cn_key, C->sb.h_cn_key); std::swap(U->sb.h_cn_value, C->sb.h_cn_value); std::swap(U->sb.h_ltail_dev, C->sb.h_ltail_dev);
}
void adopt_table(bdx_ctx* U, bdx_ctx* C) {
    swap_table_buffers(U, C);
    std::swap(U->walk, C->walk); std::swap(U->log_tail, C->log_tail);
    U->materialized = C->materialized; U->rows_packed = C->rows_packed;
    U->n_sv_total = C->n_sv_total; U->n_terms_total = C->n_terms_total; U->n_cn_total = C->n_cn_total; U->n_printed = C->n_printed;
    U->n_sv_host = C->n_sv_host; U->n_groups_total = C->n_groups_total;
    U->counts = C->counts;
    C->k6 = K6Arrays{};   // (its pointers into the swapped buffers are history)
}

// BDX_DIST_TRACE=1 (a measurement / debugging aid, like BDX_ALLOC_TRACE): waits for the stream at every step and names it on stderr
bool dist_tracing() {
    static const bool tracing = getenv("BDX_DIST_TRACE") != nullptr;
    return tracing;
}

// A ready word, else synchronise and look again, else the kernels that set it were never launched.  Two flavours: a word of this
// rank's report area (a one-thread kernel sets it), and a context's own ready word (await_ready; the context's error is the run's).
int await_word(bdx_dist* d, volatile uint32_t* w, uint32_t value, hipStream_t s, const char* what) {
    if (wait_word(w, value)) return BDX_OK;
    DHIP(d, hipStreamSynchronize(s));
    if (*w != value) return dfail(d, BDX_EINTERNAL, std::string(what) + " did not arrive: its kernels were not launched");
    return BDX_OK;
}
int await_flag(bdx_dist* d, bdx_ctx* c, ReadyWord w, hipEvent_t ev, const char* missing) {
    const int rc = await_ready(c, w, ev, missing);
    return rc == BDX_OK ? rc : dfail(d, rc, c->err);
}

// the first all-reduce's vector (collective A): one place that knows the order of its parts
struct StatWords {
    size_t tw = 0;   // per chromosome: anomalous reads, normal pairs, proper reads per key
    size_t cnt = 0, ref_len = 0, tot = 0, reads = 0, claim = 0, owner = 0, first = 0, mt = 0, cen = 0, flags = 0, words = 0;
    StatWords(int ntids, int ncols, int ncnt, int nbams, int world) : tw((size_t)ncols) {
        size_t o = 0;
        cnt = o; o += (size_t)ncnt;                  // pass 1's counters
        ref_len = o; o += (size_t)nbams;             // per-file reference lengths
        tot = o; o += (size_t)ntids * tw;            // per-chromosome totals
        reads = o; o += (size_t)ntids;               // reads of every chromosome
        claim = o; o += (size_t)ntids;               // ranks that hold reads of it (one at most)
        owner = o; o += (size_t)ntids;               // ... and which (rank + 1)
        first = o; o += (size_t)ntids * 3;           // every chromosome's first anomalous read
        mt = o; o += (size_t)world * ntids;          // [rank][mate chromosome]: inter-chromosomal reads
        cen = o; o += (size_t)world * world;         // [rank][owner]: census records
        flags = o; o += 5;                           // supporting reads wanted | name check on | name check off | clip words on | clip words off
        words = o;
    }
};

// ---- what the ranks agree on: one struct per collective, filled once by the code behind it and const to everything after ----

// after A: the genome's statistics, who owns which chromosome, what the one all-to-all will carry
struct Stats {
    uint64_t want_support = 0;            // (0, or the number of ranks)
    bool with_check = false;
    std::vector<int32_t> owner;           // [ntids], -1: nobody has reads of it
    std::vector<uint64_t> read_base;      // [ntids + 1] a chromosome's first read in the merged stream (position sorted: chromosomes ascending)
    std::vector<uint32_t> cnt_g;          // pass 1's counters, genome-wide
    uint32_t covered = 0;
    int32_t window = 0;
    size_t tw = 0;
    std::vector<uint64_t> base;           // [(ntids + 1) * tw] exclusive prefix of the chromosomes' totals in stream order
    uint64_t na_all = 0;
    int last_anom_tid = -1;
    std::vector<uint64_t> first_read;     // [ntids][3] every chromosome's first anomalous read with the genome's normal-pair count: {has one, read length, count}
    // per destination: inter-chromosomal join records (to the owner of the mate's later chromosome), census records (to the owner of the name key)
    std::vector<uint32_t> h_cnt, h_ncnt, r_cnt, r_ncnt;
    size_t nsend = 0, nrecv = 0, nnrecv = 0;
    uint64_t tot(int tid, int k) const { return base[(size_t)(tid + 1) * tw + k] - base[(size_t)tid * tw + k]; }
};

// after B: genome-wide region ids, flush windows per rank
struct Regions {
    std::vector<uint64_t> rbase;          // [ntids + 1] a chromosome's first region in the genome's numbering
    uint64_t NR = 0;
    int32_t lm = 0;                       // last_maxq of the genome's last region
    uint32_t nr_local = 0;                // this rank's regions
    std::vector<uint64_t> nr_of_rank;
    uint32_t period = 1, NW = 0, capG = 1;
    std::vector<uint32_t> nwin;           // flush windows whose last region (id (w + 1) period - 1) is rank q's: its read length is what every rank's walk uses at that flush
};

// the one all-to-all (X), in 64-bit words: what goes where, and where the three kinds of records of every source start
struct ExchangePlan {
    std::vector<size_t> scount, sdispl, rcount, rdispl;
    size_t swords = 0, rwords = 0;
    SegList seg_ctx{}, seg_cen{}, seg_win{};
    uint32_t nwin_recv = 0;
};

// A finished table in numbers: the ten words a rank reports in S (the tenth is spare), and what rank 0 counts for its own walk of the
// gathered groups.  put / get are the one place that knows the order on the wire.
struct TableCounts {
    uint64_t n_groups = 0;   // pair groups the device's walk leaves: a rank's go to rank 0, the result context's to its host
    uint64_t n_sv = 0, n_terms = 0, n_cn = 0, n_printed = 0, n_sv_host = 0, n_pairs = 0, n_groups_total = 0, n_old = 0;
    static constexpr size_t kWords = 10;
    static TableCounts of(const bdx_ctx* c) {
        TableCounts t;
        t.n_groups = c->counts.n_groups;
        t.n_sv = c->n_sv_total; t.n_terms = c->n_terms_total; t.n_cn = c->n_cn_total; t.n_printed = c->n_printed;
        t.n_sv_host = c->n_sv_host; t.n_pairs = c->counts.n_pairs; t.n_groups_total = c->n_groups_total; t.n_old = c->counts.n_old;
        return t;
    }
    void put(uint64_t* w) const {
        w[0] = n_groups; w[1] = n_sv; w[2] = n_terms; w[3] = n_cn; w[4] = n_printed; w[5] = n_sv_host; w[6] = n_pairs; w[7] = n_groups_total; w[8] = n_old;
    }
    static TableCounts get(const uint64_t* w) {
        TableCounts t;
        t.n_groups = w[0]; t.n_sv = w[1]; t.n_terms = w[2]; t.n_cn = w[3]; t.n_printed = w[4]; t.n_sv_host = w[5]; t.n_pairs = w[6]; t.n_groups_total = w[7]; t.n_old = w[8];
        return t;
    }
    // another table's rows join this one's (the pairs were counted where they were joined; the groups left over are each walk's own)
    void add_table(const TableCounts& o) {
        n_sv += o.n_sv; n_terms += o.n_terms; n_cn += o.n_cn; n_printed += o.n_printed; n_sv_host += o.n_sv_host;
        n_groups_total += o.n_groups_total; n_old += o.n_old;
    }
};

// after S: every rank's table in numbers, which route the run takes, and the ranks' region packages (either route gathers them)
struct Summary {
    std::vector<TableCounts> of_rank;
    bool replay = false;
    std::vector<size_t> gcount, gdispl;   // bytes: a rank's region records and their prefix samples, one after the other
    size_t region_bytes = 0;
};

// the one gather (G): every rank's package -- region records | pair groups | table -- in rank 0's gather buffer
struct Packages {
    std::vector<size_t> pcount, pdispl, grp_off;
    size_t pbytes = 0, ng_all = 0;
    TableDesc TD{};
    TableCounts sum;          // over the ranks' tables
    uint32_t max_sv = 0;
};

// One bdx_dist_run.  What is fixed for the run, this rank's own state between its phases, the status and the clock; what the ranks
// agree on travels between the phase functions as the structs above.
struct DistRun {
    using Clock = std::chrono::steady_clock;
    bdx_dist* const d;
    Comm& comm;
    bdx_ctx* const C;    // this rank's reads
    bdx_ctx* const U;    // rank 0: the result context
    const hipStream_t s;
    const int world, rank, nlibs, nbams, nkeys, ntids, ncnt, ncols, nkeys2;
    const bool solo;     // nothing travels: no census, no counts, no all-to-all, no gather
    const size_t rrec = sizeof(RegionRec), rpk;
    const TabLayout L;   // the report area (pinned) ...
    const DevTabLayout O;   // ... and the small device tables
    const StatWords W;
    uint32_t* H = nullptr;             // (also the staging places of L.up_*)
    volatile uint32_t* flags = nullptr;
    uint32_t* T = nullptr;
    const Clock::time_point t_begin;
    Clock::time_point t_x0, t_x1;      // bdx_dist_get_exchange's ms_exchange: from the plan of the all-to-all to the joins
    RunStatus st;
    // a failure of this rank now would leave the others waiting in a collective it does not enter (see the exit rule in bdx_dist_run)
    bool others_wait = false;
    // this rank's own, from phase to phase
    std::vector<uint32_t> tidtab;      // [t][0] first read, [t][1 + c] counters in front of it
    uint32_t na = 0;                   // this rank's anomalous reads
    std::vector<uint32_t> rtab;        // this rank's regions: first region of every chromosome, count, last_maxq
    uint8_t* taint = nullptr;          // [capG] bytes: this rank's regions that are an end of a group formed on another rank, or of one formed here with another rank's region
    RegionRec* regs = nullptr;         // rank 0: the genome's region table (pinned: the copy runs beside the result context's walk)
    uint32_t* pk = nullptr;
    bool regs_pending = false;

    DistRun(bdx_dist* d_, Clock::time_point t0)
        : d(d_), comm(*d_->comm), C(d_->reads), U(d_->util), s(d_->reads->stream), world(d_->comm->world), rank(d_->comm->rank), nlibs(d_->nlibs),
          nbams(d_->nbams), nkeys(d_->nkeys), ntids(d_->ntids), ncnt(d_->nlibs * kNumFlags + d_->nlibs + d_->nbams), ncols(2 + d_->nkeys), nkeys2(2 * d_->nkeys),
          solo(d_->comm->world == 1), rpk((size_t)nkeys2 * 4), L(ntids, ncols, nkeys, ncnt, world), O(ntids, nkeys, world), W(ntids, ncols, ncnt, nbams, world),
          t_begin(t0), tidtab((size_t)(ntids + 1) * (1 + ncols), 0), rtab((size_t)ntids + 3, 0) {}

    // ---- the phase clock: phase_ms[slot] of DistPhase.  A local phase and the collective behind it are timed by local() and collective() ----
    static Clock::time_point now() { return Clock::now(); }
    float& ms(DistPhase p) { return d->phase_ms[p]; }
    float since(Clock::time_point t) const { return ms_between(t, now()); }
    // a phase: local work between two collectives; its failure is recorded, not returned
    template <class Body>
    void local(DistPhase slot, Body&& body) {
        const auto tp = now();
        if (st.rc == BDX_OK) {
            d->err.clear();
            const int rc = body();
            if (rc != BDX_OK) { st.rc = rc; st.msg = d->err; }
        }
        ms(slot) += since(tp);
    }
    // a collective (its time includes waiting for the slowest rank).  One that fails on this rank may have left the others inside it
    template <class Call>
    int collective(DistPhase slot, Call&& call) {
        const auto tp = now();
        const int rc = call();
        ms(slot) += since(tp);
        if (rc != BDX_OK) others_wait = true;
        return rc;
    }
    // all-reduce of v with the ranks' status words appended; afterwards every rank knows whether anybody failed
    int exchange(DistPhase slot, std::vector<uint64_t>& v) {
        const size_t at = v.size();
        const int rc = collective(slot, [&]() -> int {
            v.resize(at + (size_t)world, 0);
            v[at + (size_t)rank] = (uint64_t)st.rc;
            return allreduce_host(d, v, s);
        });
        if (rc != BDX_OK) return rc;
        const int f = agreed_failure(d, st, &v[at], world);
        v.resize(at);
        return f;
    }
    int gather(const void* send, const std::vector<size_t>& count, const std::vector<size_t>& displ) {
        if (comm.gatherv_bytes(send, count[rank], d->b_all.p, count.data(), displ.data(), 0, s)) return BDX_OK;
        others_wait = true;
        return dfail(d, BDX_EHIP, comm.err);
    }
    void trace(const char* what) {
        if (!dist_tracing()) return;
        const hipError_t e = hipStreamSynchronize(s);
        fprintf(stderr, "[bdx dist %d/%d] %s: %s (%.3f ms)\n", rank, world, what, hipGetErrorString(e), since(t_begin));
    }
    int finished() {
        d->ran = true;
        d->ms_total = since(t_begin);
        return BDX_OK;
    }
    // (a negative -s: shifted region ids are the read-level walk's business; the pair model's device walk is not enqueued for them, as in bdx_run)
    bool ph_opt() const { return 0 > d->opts.min_len && 0.0f < (float)d->opts.seq_coverage_lim; }
    bool force_host() const { return (rank == 0 ? U->host_walk_only : false) || C->host_walk_only || d->opts.min_read_pair < 1 || ph_opt(); }
    uint32_t phantom(const Stats& A) const { return (A.na_all && ph_opt()) ? 1u : 0u; }

    int begin();
    int pass1_and_counts(std::vector<uint64_t>& v1);
    int agree_statistics(std::vector<uint64_t>& v1, Stats* A);
    int cut_regions(const Stats& A, std::vector<uint64_t>& v3);
    int agree_regions(const Stats& A, std::vector<uint64_t>& v3, Regions* B);
    int seed_result(const Stats& A, const Regions& B);
    void plan_exchange(const Stats& A, const Regions& B, ExchangePlan* X);
    int globalize_and_scatter(const Stats& A, const Regions& B, const ExchangePlan& X);
    int all_to_all(const Stats& A, const ExchangePlan& X);
    int join_walk_table(const Stats& A, const Regions& B, const ExchangePlan& X, TableCounts* mine, uint64_t* irregular);
    int agree_packages(const Stats& A, const Regions& B, const TableCounts& mine, uint64_t irregular, Summary* S);
    int place_regions(const Regions& B, const std::vector<size_t>& displ, bool with_pk);
    int wait_regions();
    bool pack_regions(const Regions& B, char* dst);
    int replay_route(const Stats& A, const Regions& B, const Summary& S);
    int adopt_own_table(const Regions& B);
    int plan_packages(const Summary& S, Packages* G);
    int pack_and_gather(const Regions& B, const Summary& S, const Packages& G);
    int result_as_k6_context(const Regions& B, uint32_t ng, const GroupRec* in_groups, const uint32_t* in_goff);
    int walk_gathered(const Stats& A, const Regions& B, const Summary& S, const Packages& G, TableCounts* walked, TablePackage* table);
    int merge_tables(const Regions& B, const Packages& G, const TableCounts& walked, const TablePackage& walked_table);
};

// the previous result is history; the report area and the small device tables
int DistRun::begin() {
    d->ran = false;
    d->ctx_sent = d->ctx_received = d->gathered_bytes = 0;
    if (d->table_lent && U) {   // (the previous result is history: its buffers go back to the context that fills them)
        swap_table_buffers(U, C);
        U->ran = false;
        d->table_lent = false;
    }
    if (U) { U->reg = nullptr; U->nreg = 0; U->rpk = nullptr; }
    ++d->seq;
    comm.begin_run();
    for (float& x : d->phase_ms) x = 0;
    DHIP(d, d->h_tab.ensure(L.words * 4));
    H = d->h_tab.as<uint32_t>();
    flags = (volatile uint32_t*)H;
    DHIP(d, d->b_tab.ensure(O.words * 4));
    T = d->b_tab.as<uint32_t>();
    if ((uint64_t)world * (uint64_t)ntids > (1u << 22)) return dfail(d, BDX_ELIMIT, "ranks x sequences beyond the first all-reduce's table (2^22 words)");   // (every rank alike)
    return BDX_OK;
}

// ---- A: pass 1 over all of this rank's chromosomes, where each chromosome starts and what the counters read there; the compaction
// (it needs nothing of the other ranks); what the compact records say before anything is known of the other ranks: every chromosome's
// first anomalous read, the inter-chromosomal reads by mate chromosome, the census records by owner.  ONE all-reduce carries all of it
// (round 5: three -- statistics, first reads + exchange counts, regions) ----
int DistRun::pass1_and_counts(std::vector<uint64_t>& v1) {
    C->table_in_hbm = world > 1;
    C->groups_in_hbm = world > 1;
    C->k6_cap = 0; C->k6_r_rec = nullptr; C->k6_r_pk = nullptr; C->k6_taint = nullptr;
    {   // (a set of reads bdx_dist_prepare has not seen: its order is checked before the chromosome table is searched in it)
        const int orc = check_order(d);
        if (orc != BDX_OK) return orc;
    }
    DCTX(d, C, do_pass1(C, {}));   // (its record is waited for together with the chromosome table)
    TidTableParams tp{};
    tp.tid = C->d.tid; tp.lib = C->d.lib; tp.cls = C->b_cls.as<uint8_t>(); tp.n = C->n; tp.ntiles = C->ntiles; tp.tstride = C->tstride;
    tp.ntids = ntids; tp.nkeys = nkeys; tp.nlibs = nlibs; tp.ncols = ncols; tp.libs = C->b_libs.as<DevLib>();
    tp.tile_tot = C->b_tile_tot.as<uint32_t>(); tp.tile_pre = C->b_tile_pre.as<uint32_t>(); tp.chunk_base = C->fp_deferred.chunk_base;
    tp.chunk_super = C->fp_deferred.chunk_super; tp.p1 = C->b_p1.as<Pass1>(); tp.out = H + L.tidtab;
    launch_k9_tid_table(tp, s);
    launch_k9_signal(H + 0, d->seq, s);
    DCTX(d, C, wait_pass1(C));
    if (const int rc = await_word(d, flags + 0, d->seq, s, "the chromosome table")) return rc;
    trace("chromosome table");
    memcpy(tidtab.data(), H + L.tidtab, tidtab.size() * 4);
    const uint32_t* terr = H + L.tidtab + tidtab.size();
    if (terr[0] || terr[1]) return dfail(d, BDX_EINVAL, "record with a reference id outside [0, ntids)");
    na = C->p1.n_anom;
    // the compaction, and what its records say
    {
        UploadList ul{};
        ul.fill(T + O.cnt, 0u, (size_t)world * 4 + 8);   // (the exchange's counters, the error words of the later kernels)
        ul.fill(T + O.mt, 0u, (size_t)ntids);
        launch_k9_upload(ul, s);
    }
    DCTX(d, C, do_compact(C));
    trace("compaction");
    memset(H + L.first, 0, (size_t)ntids * 16);
    if (na) {
        FirstCountsParams fc{};
        fc.cp = C->cp; fc.mtid_col = C->d.mtid; fc.n_ptr = &C->b_p1.as<Pass1>()->n_anom; fc.ntids = ntids; fc.world = (uint32_t)world;
        fc.first_tab = H + L.first; fc.cnt_mtid = T + O.mt; fc.cnt_owner = T + O.cnt + world;
        launch_k9_first_counts(fc, na, s);
        if (solo) {
            launch_k9_signal(H + 1, d->seq, s);
        } else {
            UploadList rl{};   // (device words -> the pinned report area, then the ready word: one launch each)
            rl.copy(H + L.cnts, T + O.mt, (size_t)ntids);
            rl.copy(H + L.cnts + ntids, T + O.cnt + world, (size_t)world);
            launch_k9_upload(rl, s);
            launch_k9_signal(H + 1, d->seq, s);
        }
        if (const int rc = await_word(d, flags + 1, d->seq, s, "the chromosomes' first reads")) return rc;
        trace("first reads and counts");
    } else {
        C->k4 = K4Arrays{};
    }
    for (int i = 0; i < ncnt; ++i) v1[W.cnt + i] = C->cnt_local[i];
    for (int b = 0; b < nbams; ++b) v1[W.ref_len + b] = C->p1.ref_len[b];
    for (int t = 0; t < ntids; ++t) {
        const uint32_t* a = &tidtab[(size_t)t * (1 + ncols)];
        const uint32_t* b = a + (1 + ncols);
        const uint64_t nreads = (uint64_t)b[0] - a[0];
        if (!nreads) continue;
        for (int c = 0; c < ncols; ++c) v1[W.tot + (size_t)t * W.tw + c] = (uint32_t)(b[1 + c] - a[1 + c]);
        v1[W.reads + t] = nreads;
        v1[W.claim + t] = 1;
        v1[W.owner + t] = (uint64_t)rank + 1;
        const uint32_t* f = H + L.first + (size_t)t * 4;
        if (na && f[0]) {   // {has one, its read length, normal pairs of THIS chromosome in front of it (the chromosomes before are added by everybody alike)}
            v1[W.first + (size_t)t * 3] = 1; v1[W.first + (size_t)t * 3 + 1] = f[1];
            v1[W.first + (size_t)t * 3 + 2] = (uint32_t)(f[2] - a[1 + kColNormal]);
        }
    }
    if (na && !solo) {
        for (int t = 0; t < ntids; ++t) v1[W.mt + (size_t)rank * ntids + t] = H[L.cnts + t];
        for (int q = 0; q < world; ++q) v1[W.cen + (size_t)rank * world + q] = H[L.cnts + ntids + q];
    }
    v1[W.flags] = d->collect_support ? 1 : 0;
    if (C->n) v1[W.flags + (C->use_check ? 1 : 2)] = 1;
    if (C->n) v1[W.flags + (C->use_clips ? 3 : 4)] = 1;
    return BDX_OK;
}

// collective A, and what every rank derives from the sums: owners, prefixes, the window, what the one all-to-all will carry, the
// limits that trip everywhere at once
int DistRun::agree_statistics(std::vector<uint64_t>& v1, Stats* out) {
    BDX_TRY(exchange(kPhAllreduceStatistics, v1));
    Stats& A = *out;
    A.want_support = v1[W.flags];
    if (A.want_support != 0 && A.want_support != (uint64_t)world) return dfail(d, BDX_EINVAL, "bdx_dist_set_collect_support is set on some ranks only");
    if (v1[W.flags + 1] && v1[W.flags + 2]) return dfail(d, BDX_EINVAL, "bdx_use_name_check is set on some ranks' contexts only");
    if (v1[W.flags + 3] && v1[W.flags + 4]) return dfail(d, BDX_EINVAL, "bdx_use_clips is set on some ranks' contexts only");
    A.with_check = v1[W.flags + 1] != 0;
    A.owner.assign(ntids, -1);
    for (int t = 0; t < ntids; ++t) {
        if (v1[W.claim + t] > 1) return dfail(d, BDX_EINVAL, "chromosome " + std::to_string(t) + " has reads on more than one rank");
        if (v1[W.claim + t]) A.owner[t] = (int32_t)v1[W.owner + t] - 1;
    }
    A.read_base.assign((size_t)ntids + 1, 0);
    for (int t = 0; t < ntids; ++t) A.read_base[(size_t)t + 1] = A.read_base[t] + v1[W.reads + (size_t)t];
    A.cnt_g.resize(ncnt);
    for (int i = 0; i < ncnt; ++i) A.cnt_g[i] = (uint32_t)v1[W.cnt + i];
    A.covered = 0;  // BamSummary.cpp:123-126: a uint32 maximum compared against each file's size_t sum
    for (int b = 0; b < nbams; ++b)
        if ((uint64_t)A.covered < v1[W.ref_len + b]) A.covered = (uint32_t)v1[W.ref_len + b];
    A.window = window_from(C, A.cnt_g.data(), A.covered);
    const size_t tw = A.tw = W.tw;
    A.base.assign((size_t)(ntids + 1) * tw, 0);
    for (int t = 0; t < ntids; ++t)
        for (size_t k = 0; k < tw; ++k) A.base[(size_t)(t + 1) * tw + k] = A.base[(size_t)t * tw + k] + v1[W.tot + (size_t)t * tw + k];
    A.na_all = A.base[(size_t)ntids * tw];
    // (the same sum on every rank: all of them return here, together)
    if (A.na_all > kMaxAnomalous) return dfail(d, BDX_ELIMIT, "more than 2^31 anomalous reads in one run");
    A.last_anom_tid = -1;
    for (int t = 0; t < ntids; ++t)
        if (A.tot(t, 0) > 0) A.last_anom_tid = t;
    A.first_read.assign((size_t)ntids * 3, 0);
    for (int t = 0; t < ntids; ++t)
        if (v1[W.first + (size_t)t * 3]) {
            A.first_read[(size_t)t * 3] = 1; A.first_read[(size_t)t * 3 + 1] = v1[W.first + (size_t)t * 3 + 1];
            A.first_read[(size_t)t * 3 + 2] = (uint32_t)(A.base[(size_t)t * tw + kColNormal] + v1[W.first + (size_t)t * 3 + 2]);
        }
    // what the one all-to-all will carry, per destination: inter-chromosomal join records (to the owner of the mate's later chromosome),
    // census records (to the owner of the name key), window read lengths (plan_exchange, once the regions are counted)
    A.h_cnt.assign(world, 0); A.h_ncnt.assign(world, 0); A.r_cnt.assign(world, 0); A.r_ncnt.assign(world, 0);
    if (!solo)
        for (int q = 0; q < world; ++q) {
            for (int t = 0; t < ntids; ++t) {
                if (A.owner[t] < 0) continue;
                if (A.owner[t] == q && q != rank) A.h_cnt[q] += (uint32_t)v1[W.mt + (size_t)rank * ntids + t];
                if (A.owner[t] == rank && q != rank) A.r_cnt[q] += (uint32_t)v1[W.mt + (size_t)q * ntids + t];
            }
            A.h_ncnt[q] = (uint32_t)v1[W.cen + (size_t)rank * world + q];
            A.r_ncnt[q] = (uint32_t)v1[W.cen + (size_t)q * world + rank];
        }
    for (int q = 0; q < world; ++q) { A.nsend += A.h_cnt[q]; A.nrecv += A.r_cnt[q]; A.nnrecv += A.r_ncnt[q]; }
    // (the same matrices on every rank: the limits trip everywhere at once)
    for (int r = 0; r < world && !solo; ++r) {
        uint64_t col = 0, ncol = 0;
        for (int q = 0; q < world; ++q) {
            ncol += v1[W.cen + (size_t)q * world + r];
            for (int t = 0; t < ntids; ++t)
                if (A.owner[t] == r && q != r) col += v1[W.mt + (size_t)q * ntids + t];
        }
        if (col > (1u << 28) || ncol > 0x7FFFFFFFull) return dfail(d, BDX_ELIMIT, "too many inter-chromosomal join records / names on one rank");
    }
    return BDX_OK;
}

// ---- B: the statistics every kernel from here on runs with; the compact records' counters start where the chromosomes in front
// (anybody's) left them; regions -- the first anomalous read of the next chromosome that has one closes a chromosome's last candidate.
// The second all-reduce: every chromosome's region count ----
int DistRun::cut_regions(const Stats& A, std::vector<uint64_t>& v3) {
    const size_t tw = A.tw;
    DCTX(d, C, set_pass1(C, A.cnt_g.data(), A.covered, A.window, false));
    {
        uint32_t* st_up = H + L.up_stats;
        st_up[0] = A.covered; st_up[1] = (uint32_t)A.window;
        memcpy(st_up + 2, A.cnt_g.data(), (size_t)ncnt * 4);
        memcpy(st_up + 2 + ncnt, C->key_density.data(), C->key_density.size() * 4);
        // (window and covered length -- Pass1's first words --, flag histogram, densities; with anomalous reads the chromosomes' offsets, owners
        // and closing reads: ONE launch that reads them from the pinned report area)
        UploadList ul{};
        ul.copy(C->b_p1.p, st_up, 2);
        ul.copy(C->b_cnt.p, st_up + 2, (size_t)ncnt);
        ul.copy(C->b_kdens.p, st_up + 2 + ncnt, C->key_density.size());
        if (na) {
            uint32_t* up = H + L.up_off;
            for (int t = 0; t < ntids; ++t) {
                const uint32_t* a = &tidtab[(size_t)t * (1 + ncols)];
                for (int k = 0; k < 1 + nkeys; ++k) up[(size_t)t * (1 + nkeys) + k] = (uint32_t)A.base[(size_t)t * tw + 1 + k] - a[1 + 1 + k];
            }
            ul.copy(T + O.off, up, (size_t)ntids * (1 + nkeys));
            uint32_t* um = H + L.up_misc;   // owner [ntids] | first read of every chromosome in this context [ntids + 1]   (roff follows later)
            for (int t = 0; t < ntids; ++t) { um[t] = (uint32_t)A.owner[t]; um[(size_t)ntids + t] = tidtab[(size_t)t * (1 + ncols)]; }
            um[(size_t)2 * ntids] = tidtab[(size_t)ntids * (1 + ncols)];
            ul.copy(T + O.owner, um, (size_t)2 * ntids + 1);
            uint32_t* tails = H + L.up_tail;
            int nx = -1;
            for (int t = ntids - 1; t >= 0; --t) {
                uint32_t* q = &tails[(size_t)t * 4];
                q[0] = nx >= 0 ? 1u : 0u;
                q[1] = nx >= 0 ? (uint32_t)A.first_read[(size_t)nx * 3 + 1] : 0u;
                q[2] = nx >= 0 ? (uint32_t)A.first_read[(size_t)nx * 3 + 2] : (uint32_t)A.base[(size_t)ntids * tw + 1];
                q[3] = 0;
                if (A.first_read[(size_t)t * 3]) nx = t;
            }
            ul.copy(T + O.tail, tails, (size_t)ntids * 4);
        }
        launch_k9_upload(ul, s);
    }
    if (!na) return BDX_OK;
    launch_k9_rebase(C->cp, &C->b_p1.as<Pass1>()->n_anom, na, nkeys, T + O.off, nullptr, s);
    DCTX(d, C, do_cut(C, T + O.tail, RegionDst::Hbm));
    trace("region cut");
    launch_k9_tid_regions(C->sb.b_r_rec.as<RegionRec>(), C->b_counts.as<StageCounts>(), ntids, H + L.rtab, s);
    launch_k9_signal(H + 2, d->seq, s);
    if (const int rc = await_word(d, flags + 2, d->seq, s, "the chromosomes' region counts")) return rc;
    memcpy(rtab.data(), H + L.rtab, rtab.size() * 4);
    for (int t = 0; t < ntids; ++t) v3[t] = rtab[t + 1] - rtab[t];
    if (A.last_anom_tid >= 0 && A.owner[A.last_anom_tid] == rank) v3[ntids] = rtab[ntids + 2];
    return BDX_OK;
}

// collective B, and what follows from it: genome-wide region ids, flush windows per rank
int DistRun::agree_regions(const Stats& A, std::vector<uint64_t>& v3, Regions* out) {
    BDX_TRY(exchange(kPhAllreduceRegions, v3));
    Regions& B = *out;
    B.rbase.assign(ntids + 1, 0);
    for (int t = 0; t < ntids; ++t) B.rbase[t + 1] = B.rbase[t] + v3[t];
    B.NR = B.rbase[ntids];
    if (B.NR > kMaxRegions) return dfail(d, BDX_ELIMIT, "too many regions for the packed group key");  // (all ranks alike)
    B.lm = (int32_t)(uint32_t)v3[ntids];
    B.nr_local = rtab[ntids + 1];
    B.nr_of_rank.assign(world, 0);
    for (int t = 0; t < ntids; ++t)
        if (A.owner[t] >= 0) B.nr_of_rank[A.owner[t]] += v3[t];
    B.period = (uint32_t)std::max(1, d->opts.buffer_size + 1);
    B.NW = (uint32_t)(B.NR / B.period);
    B.capG = (uint32_t)std::max<uint64_t>(std::max<uint64_t>(C->na_alloc, B.NR), 1);
    B.nwin.assign(world, 0);
    const uint64_t wend = (uint64_t)B.NW * B.period;
    for (int t = 0; t < ntids; ++t)
        if (A.owner[t] >= 0 && B.rbase[t + 1] > B.rbase[t]) B.nwin[A.owner[t]] += (uint32_t)(std::min<uint64_t>(B.rbase[t + 1], wend) / B.period - std::min<uint64_t>(B.rbase[t], wend) / B.period);
    return BDX_OK;
}

// the result context takes the run's statistics; with no region anywhere the run is over: an empty table
int DistRun::seed_result(const Stats& A, const Regions& B) {
    if (rank == 0) {
        DCTX(d, U, set_pass1(U, A.cnt_g.data(), A.covered, A.window, false));
        U->n = 0;
        U->p1 = Pass1{};
        U->p1.n_anom = (uint32_t)A.na_all; U->p1.covered_ref_len = A.covered; U->p1.window = A.window;
        U->replayed = false;
        U->sup_off.clear(); U->sup_idx.clear(); U->sup_flag.clear();
        U->collect_support = false;
        if (!U->walk_scratch) U->walk_scratch.reset(walk_scratch_new());
    }
    if (!B.NR && rank == 0) {
        U->regions.clear(); U->r_pk.clear(); U->reg = nullptr; U->nreg = 0; U->rpk = nullptr;
        U->walk.clear(); U->log_tail.clear();
        U->n_sv_total = U->n_terms_total = U->n_cn_total = U->n_printed = U->n_sv_host = U->n_groups_total = 0;
        memset(&U->counts, 0, sizeof(U->counts));
        U->materialized = true; U->ran = true;
        if (A.want_support) { U->collect_support = true; U->sup_off.assign(1, 0); }   // (no SV, no supporting read: an empty list, not a missing one)
    }
    return BDX_OK;
}

// ---- C: genome-wide region ids; ONE all-to-all carries, per destination, the inter-chromosomal join records (32 bytes), the census
// records (16) and the read lengths of the flush windows this rank closes (8) -- round 5: two all-to-alls and, for the windows and the
// taint bytes, an all-reduce of device words.  No host round trip from here to the rank's finished table ----
constexpr size_t kxw = sizeof(ExchangeEntry) / 8;
void DistRun::plan_exchange(const Stats& A, const Regions& B, ExchangePlan* out) {
    ExchangePlan& X = *out;
    X.scount.assign(world, 0); X.sdispl.assign(world, 0); X.rcount.assign(world, 0); X.rdispl.assign(world, 0);
    for (int q = 0; q < world; ++q) {
        const size_t sw = (size_t)A.h_cnt[q] * kxw + (size_t)A.h_ncnt[q] * 2 + (q != rank ? B.nwin[rank] : 0);
        const size_t rw = (size_t)A.r_cnt[q] * kxw + (size_t)A.r_ncnt[q] * 2 + (q != rank ? B.nwin[q] : 0);
        X.scount[q] = sw; X.sdispl[q] = X.swords; X.swords += round_up(sw, 4);   // (blocks start on 32-byte boundaries: a join record is stored as one)
        X.rcount[q] = rw; X.rdispl[q] = X.rwords; X.rwords += round_up(rw, 4);
    }
    uint32_t a = 0, b = 0, c = 0;
    X.seg_ctx.n = X.seg_cen.n = X.seg_win.n = world;
    for (int q = 0; q < world; ++q) {
        X.seg_ctx.off[q] = X.rdispl[q]; X.seg_ctx.start[q] = a; a += A.r_cnt[q];
        X.seg_cen.off[q] = X.rdispl[q] + (size_t)A.r_cnt[q] * kxw; X.seg_cen.start[q] = b; b += A.r_ncnt[q];
        X.seg_win.off[q] = X.rdispl[q] + (size_t)A.r_cnt[q] * kxw + (size_t)A.r_ncnt[q] * 2; X.seg_win.start[q] = c; c += q != rank ? B.nwin[q] : 0;
    }
    X.seg_ctx.start[world] = a; X.seg_cen.start[world] = b; X.seg_win.start[world] = c;
    X.nwin_recv = X.seg_win.start[world];
}

// local: the regions get their genome-wide ids, the windows this rank closes and its travelling join / census records go into the send buffer
int DistRun::globalize_and_scatter(const Stats& A, const Regions& B, const ExchangePlan& X) {
    const uint64_t NR = B.NR;
    DHIP(d, d->b_send.ensure(std::max<size_t>(X.swords, 4) * 8));
    DHIP(d, d->b_recv.ensure(std::max<size_t>(X.rwords, 4) * 8));
    DHIP(d, d->b_rg_rec.ensure((size_t)NR * sizeof(RegionRec)));
    DHIP(d, d->b_rg_pk.ensure(std::max<size_t>((size_t)NR * nkeys2 * 4, 16)));
    DHIP(d, size_out_deg(C->sb, B.capG));
    DHIP(d, d->b_x.ensure((size_t)B.capG + 64));
    taint = d->b_x.as<uint8_t>();
    DHIP(d, hipMemsetAsync(d->b_rg_rec.p, 0, (size_t)NR * sizeof(RegionRec), s));
    DHIP(d, hipMemsetAsync(taint, 0, (size_t)B.capG, s));
    {   // (the chromosomes' region offsets and the exchange's cursors: one launch, as above)
        UploadList ul{};
        uint32_t* ur = H + L.up_misc + (size_t)2 * ntids + 1;
        for (int t = 0; t < ntids; ++t) ur[t] = (uint32_t)B.rbase[t] - rtab[t];
        ul.copy(T + O.roff, ur, (size_t)ntids);
        if (na && !solo) {   // where a destination's join records / census records start in the ONE send buffer, in records of their own size
            uint32_t* cur = H + L.up_cur;
            for (int q = 0; q < world; ++q) {
                cur[q] = (uint32_t)(X.sdispl[q] / kxw);
                cur[(size_t)world + q] = (uint32_t)((X.sdispl[q] + (size_t)A.h_cnt[q] * kxw) / 2);
            }
            ul.copy(T + O.cnt + 2 * (size_t)world, cur, (size_t)world * 2);
        }
        launch_k9_upload(ul, s);
    }
    GlobalizeParams gp{};
    gp.tid = C->cp.tid; gp.region_of = C->k3.region_of; gp.n_ptr = &C->b_p1.as<Pass1>()->n_anom;
    gp.r_rec = C->sb.b_r_rec.as<RegionRec>(); gp.r_pk = C->sb.b_r_pk.as<uint32_t>(); gp.nr_local = B.nr_local; gp.roff = T + O.roff;
    gp.rg_rec = d->b_rg_rec.as<RegionRec>(); gp.rg_pk = d->b_rg_pk.as<uint32_t>(); gp.nkeys2 = nkeys2;
    gp.scratch = C->sb.b_out_deg.as<uint32_t>(); gp.cap = B.capG; gp.counts = C->b_counts.as<StageCounts>(); gp.nr_global = (uint32_t)NR; gp.last_maxq = B.lm;
    launch_k9_globalize(gp, na, s);
    trace("globalize");
    C->k6_cap = (uint32_t)NR; C->k6_r_rec = d->b_rg_rec.as<RegionRec>(); C->k6_r_pk = d->b_rg_pk.as<uint32_t>();
    C->k6_taint = solo ? nullptr : taint;
    if (solo && rank == 0) {   // one rank: the genome's table is this rank's -- to pinned memory beside the joins, for the host's share of the walk and the result
        if (C->sb.h_regs.ensure((size_t)NR * sizeof(RegionRec)) != hipSuccess || C->sb.h_pk.ensure(std::max<size_t>((size_t)NR * nkeys2 * 4, 16)) != hipSuccess)
            return dfail(d, BDX_ENOMEM, "region table");
        regs = C->sb.h_regs.as<RegionRec>();
        pk = C->sb.h_pk.as<uint32_t>();
        DHIP(d, hipEventRecord(C->ev_copy, s));
        DHIP(d, hipStreamWaitEvent(C->copy_stream, C->ev_copy, 0));
        static_assert(sizeof(RegionRec) % 4 == 0, "copied by words");
        UploadList ul{};   // (a kernel, not copy commands: the first device-to-host copy command of a process sets up a copy-engine queue, round 5)
        ul.copy(regs, d->b_rg_rec.p, (size_t)NR * sizeof(RegionRec) / 4);
        if (nkeys2) ul.copy(pk, d->b_rg_pk.p, (size_t)NR * nkeys2);
        launch_k9_upload(ul, C->copy_stream);
    }
    if (!solo) {
        if (B.nwin[rank]) {
            WindowDst wd{};
            wd.world = world;
            for (int q = 0; q < world; ++q)
                wd.dst[q] = q == rank ? nullptr : d->b_send.as<unsigned long long>() + X.sdispl[q] + (size_t)A.h_cnt[q] * kxw + (size_t)A.h_ncnt[q] * 2;
            launch_k9_window_pack(d->b_rg_rec.as<RegionRec>(), (uint32_t)NR, B.period, wd, B.nwin[rank], T + O.ntot + 3, s);
        }
        if (na) {
            ExchangeSrc xs{};
            xs.key = C->cp.key; xs.check = C->cp.check; xs.meta = C->cp.meta; xs.tid = C->cp.tid; xs.idx = C->cp.idx; xs.mtid_col = C->d.mtid;
            xs.region_of = C->k3.region_of; xs.n_ptr = &C->b_p1.as<Pass1>()->n_anom; xs.owner_of_tid = (const int32_t*)(T + O.owner);
            xs.ntids = ntids; xs.me = rank; xs.world = (uint32_t)world; xs.taint = taint;
            launch_k7_scatter(xs, na, T + O.cnt + 2 * (size_t)world, d->b_send.as<ExchangeEntry>(), d->b_send.as<unsigned long long>(), s);
        }
    }
    trace("scatter");
    return BDX_OK;
}

// collective X
int DistRun::all_to_all(const Stats& A, const ExchangePlan& X) {
    const int rc = collective(kPhAlltoall, [&]() -> int {
        if (!solo && !comm.alltoallv_u64(d->b_send.as<uint64_t>(), X.scount.data(), X.sdispl.data(), d->b_recv.as<uint64_t>(), X.rcount.data(), X.rdispl.data(), s))
            return dfail(d, BDX_EHIP, comm.err);
        return BDX_OK;
    });
    if (rc == BDX_OK) { d->ctx_sent = A.nsend; d->ctx_received = A.nrecv; }
    return rc;
}

// ---- D: the joins (own reads + foreign entries), the name census beside them, the pair groups per region, the components, the device's
// walk of the ones that lie inside this rank, the rank's table -- enqueued in one go: nothing of it waits for the host or for another rank.
// A component that spans ranks is known as such WITHOUT an exchange: a region that sent a join record away is an end of a group another
// rank forms (k7_scatter marks it), a region joined with a foreign entry by a gate-passing group is one too (k6_pairs marks it) -- its
// groups go to rank 0 (round 5 all-reduced the marks).  The third all-reduce: what every rank will send to rank 0, and whether a name misbehaved ----
int DistRun::join_walk_table(const Stats& A, const Regions& B, const ExchangePlan& X, TableCounts* mine, uint64_t* irregular) {
    const uint64_t NR = B.NR;
    const unsigned long long* R = d->b_recv.as<unsigned long long>();
    if (X.nwin_recv) launch_k9_window_unpack(d->b_rg_rec.as<RegionRec>(), (uint32_t)NR, B.period, R, X.seg_win, X.nwin_recv, T + O.ntot + 4, s);
    if (A.nnrecv) {   // the census of the names this rank owns: on the second stream, beside the joins (its verdict is read below)
        const uint32_t slots = k7_names_slots(A.nnrecv);
        DHIP(d, d->b_ntab.ensure((size_t)slots * 16));
        DHIP(d, d->b_nflag.ensure(16));
        DHIP(d, hipEventRecord(d->ev_side, s));
        DHIP(d, hipStreamWaitEvent(C->copy_stream, d->ev_side, 0));
        launch_k7_names_clear(d->b_ntab.as<unsigned long long>(), slots, d->b_nflag.as<uint32_t>(), C->copy_stream);
        launch_k7_names_census_seg(R, X.seg_cen, (uint32_t)A.nnrecv, d->b_ntab.as<unsigned long long>(), slots, d->b_nflag.as<uint32_t>(), C->copy_stream);
    }
    if (na) {
        if ((uint64_t)C->na_alloc + A.nrecv > (1u << 28)) return dfail(d, BDX_ELIMIT, "too many join entries on one rank");
        const uint32_t nf = (uint32_t)A.nrecv;
        DHIP(d, d->b_foreign.ensure(std::max<size_t>(nf, 1) * 20 + 64));
        uint64_t* fkey = d->b_foreign.as<uint64_t>();
        uint64_t* fcheck = fkey + std::max<size_t>(nf, 1);
        int32_t* fregion = (int32_t*)(fcheck + std::max<size_t>(nf, 1));
        launch_k7_unpack_seg(R, X.seg_ctx, nf, fkey, A.with_check ? fcheck : nullptr, fregion, &C->b_p1.as<Pass1>()->n_anom, T + O.ntot, s);
        Entries en{};
        en.key = C->cp.key; en.check = C->cp.check; en.region = C->k3.region_of; en.meta = C->cp.meta; en.isize = C->cp.isize;
        en.n_local = &C->b_p1.as<Pass1>()->n_anom; en.fkey = fkey; en.fcheck = fcheck; en.fregion = fregion; en.want_pair_lo = 1;
        DCTX(d, C, do_join_local(C, C->na_alloc + nf, en, T + O.ntot));
    }
    trace("join");
    t_x1 = now();
    DCTX(d, C, k6_prepare(C, force_host(), 0));
    k6_pairs(C);
    DCTX(d, C, k6_then_walk(C, launch_k6_components));   // (components and, right behind them, the device's walk)
    trace("components and walk");
    if (solo && rank == 0) {   // one rank: its host walks what the device walk leaves, as in bdx_run -- on the table that went to pinned memory beside the joins
        DHIP(d, hipStreamSynchronize(C->copy_stream));
        decode_regions(C, regs, pk, (uint32_t)NR, 0, true);
    }
    if (const int rc = await_flag(d, C, kGroupsReady, C->ev_groups, "the pair groups did not arrive: their kernels were not launched")) return rc;
    C->counts = *C->h_counts.as<StageCounts>();
    if (C->counts.irregular) *irregular = 1;   // a read name seen more than twice: the run is replayed read by read on rank 0 (replay_route)
    if (C->counts.overflow) return dfail(d, BDX_EINTERNAL, "group list overflow");
    if (A.nnrecv) {
        uint32_t flag = 0;
        DHIP(d, hipMemcpyAsync(&flag, d->b_nflag.p, 4, hipMemcpyDeviceToHost, C->copy_stream));
        DHIP(d, hipStreamSynchronize(C->copy_stream));
        if (flag) *irregular = 1;
    }
    if (X.nwin_recv) {
        uint32_t werr = 0;
        DHIP(d, hipMemcpy(&werr, T + O.ntot + 4, 4, hipMemcpyDeviceToHost));
        if (werr) return dfail(d, BDX_EINTERNAL, "window read lengths of the exchange do not fit the region table");
    }
    // (the read-level walk on rank 0 serves supporting reads and a negative -s whatever the names look like)
    if (*irregular || A.want_support != 0 || phantom(A) != 0) return BDX_OK;   // (the table of this model is not wanted)
    C->walk.clear();
    if (solo && rank == 0) {
        decode_groups(C, C->sb.h_groups.as<GroupRec>(), C->counts.n_groups, 0);
        C->last_big_groups = (int64_t)C->counts.n_groups + C->counts.n_groups_big;
        const auto tw0 = now();
        DCTX(d, C, host_walk(C, B.lm, A.na_all != 0));
        ms(kPhHostWalk) = since(tw0);
    }
    C->counts.last_maxq = B.lm;
    DCTX(d, C, do_k6_table(C));
    DCTX(d, C, finish_table(C));
    trace("table");
    *mine = TableCounts::of(C);   // (several ranks: n_groups are the groups of the components that go to rank 0)
    return BDX_OK;
}

// collective S: every rank's table in numbers, and which route the run takes
int DistRun::agree_packages(const Stats& A, const Regions& B, const TableCounts& mine, uint64_t irregular, Summary* out) {
    std::vector<uint64_t> v5((size_t)world * TableCounts::kWords + 1, 0);
    if (st.rc == BDX_OK) mine.put(&v5[(size_t)rank * TableCounts::kWords]);
    v5[(size_t)world * TableCounts::kWords] = irregular;
    BDX_TRY(exchange(kPhAllreducePackages, v5));
    Summary& S = *out;
    for (int q = 0; q < world; ++q) S.of_rank.push_back(TableCounts::get(&v5[(size_t)q * TableCounts::kWords]));
    // some rank met a read name more than twice -- or the caller wants the reads behind every SV, which only the read-level walk knows
    // ... or -s is negative: the very first anomalous read of the genome then registers a read-less region 0 (BreakDancer.cpp:216-231,
    // 244-252; bdx_run's `ph`), every real region's id shifts by one and with it the flush cadence -- the read-level walk knows how
    // (ReadWalkInput::phantom), the pair model's kernels do not
    S.replay = v5[(size_t)world * TableCounts::kWords] != 0 || A.want_support != 0 || phantom(A) != 0;
    // the genome's region table on rank 0: the ranks' dense tables placed by genome-wide id (several ranks: from a gather's packages)
    S.gcount.resize(world); S.gdispl.resize(world);
    for (int q = 0; q < world; ++q) { S.gcount[q] = round_up((size_t)B.nr_of_rank[q] * (rrec + rpk), 8); S.gdispl[q] = S.region_bytes; S.region_bytes += S.gcount[q]; }
    return BDX_OK;
}

// rank 0, several ranks: the packages' region records (in the gather buffer at displ[q]) -> the result context's table in HBM and, on the side stream, in pinned memory
int DistRun::place_regions(const Regions& B, const std::vector<size_t>& displ, bool with_pk) {
    const uint64_t NR = B.NR;
    GatherDesc D{};
    D.world = world;
    uint32_t max_nr = 0;
    for (int q = 0; q < world; ++q) {
        const size_t nr = (size_t)B.nr_of_rank[q];
        D.p[q] = GatherPackage{displ[q], displ[q] + nr * rrec, 0, (uint32_t)nr, 0};
        max_nr = std::max(max_nr, (uint32_t)nr);
    }
    if (C->sb.h_regs.ensure((size_t)NR * rrec) != hipSuccess || C->sb.h_pk.ensure(std::max<size_t>((size_t)NR * rpk, 16)) != hipSuccess) return dfail(d, BDX_ENOMEM, "region table");
    regs = C->sb.h_regs.as<RegionRec>();
    pk = C->sb.h_pk.as<uint32_t>();
    if (U->sb.b_r_rec.ensure((size_t)NR * rrec) != hipSuccess || U->sb.b_r_pk.ensure(std::max<size_t>((size_t)NR * rpk, 16)) != hipSuccess) return dfail(d, BDX_ENOMEM, "region table");
    DHIP(d, hipMemcpyAsync(T + O.rbase, B.rbase.data(), ((size_t)ntids + 1) * 8, hipMemcpyHostToDevice, s));
    launch_k8_place_regions((const char*)d->b_all.p, D, max_nr, (const uint64_t*)(T + O.rbase), ntids, nkeys2, U->sb.b_r_rec.as<RegionRec>(), U->sb.b_r_pk.as<uint32_t>(),
                            T + O.ntot + 1, s);
    DHIP(d, hipEventRecord(C->ev_copy, s));
    DHIP(d, hipStreamWaitEvent(C->copy_stream, C->ev_copy, 0));
    UploadList ul{};
    ul.copy(regs, U->sb.b_r_rec.p, (size_t)NR * rrec / 4);
    if (nkeys2 && with_pk) ul.copy(pk, U->sb.b_r_pk.p, (size_t)NR * rpk / 4);   // (without: the rows the host's walk touches follow, launch_k9_pk_rows)
    launch_k9_upload(ul, C->copy_stream);
    regs_pending = true;
    return BDX_OK;
}
int DistRun::wait_regions() {
    if (regs_pending) {
        DHIP(d, hipStreamSynchronize(C->copy_stream));
        regs_pending = false;
        uint32_t perr = 0;
        DHIP(d, hipMemcpy(&perr, T + O.ntot + 1, 4, hipMemcpyDeviceToHost));
        if (perr) return dfail(d, BDX_EINTERNAL, "region table of the gather does not add up");
    }
    return BDX_OK;
}
// this rank's region records and their prefix samples, one after the other, at dst (device memory)
bool DistRun::pack_regions(const Regions& B, char* dst) {
    if (!B.nr_local) return true;
    return hipMemcpyAsync(dst, C->sb.b_r_rec.p, (size_t)B.nr_local * rrec, hipMemcpyDeviceToDevice, s) == hipSuccess &&
           hipMemcpyAsync(dst + (size_t)B.nr_local * rrec, C->sb.b_r_pk.p, (size_t)B.nr_local * rpk, hipMemcpyDeviceToDevice, s) == hipSuccess;
}

// ---- a read name seen more than twice (clashing names across merged files): the pair model does not hold, and the reference's
// behaviour (ReadRegionData.cpp:108-113,152-175, SvBuilder.cpp:101-118) depends on the order of ALL sightings.  Every rank sends
// its region records and the compact records of its chromosomes (name key, genome-wide region id, meta, |isize|, tid, second name
// hash, index in the chromosome's stream: 40 bytes per anomalous read) to rank 0, which replays the run read by read (H2,
// bdx_walk_reads.cpp) on the gathered region table.  The same route serves bdx_dist_set_collect_support: the supporting reads of an
// SV (-g / -d dumps, BreakDancer.cpp:514-534) are known to the read-level walk only ----
int DistRun::replay_route(const Stats& A, const Regions& B, const Summary& S) {
    const auto t_r0 = now();
    const uint64_t NR = B.NR, na_all = A.na_all;
    const uint32_t ph = phantom(A);
    constexpr size_t kw = 5;
    DHIP(d, hipStreamSynchronize(s));   // (K6's kernels were enqueued on the pair model: let them finish, their results are dropped)
    if (!solo) {
        if (d->b_pack.ensure(std::max<size_t>(S.gcount[rank], 8)) != hipSuccess) return dfail(d, BDX_ENOMEM, "region package");
        if (!pack_regions(B, (char*)d->b_pack.p)) return dfail(d, BDX_EHIP, "region package");
        if (rank == 0 && d->b_all.ensure(std::max<size_t>(S.region_bytes, 8)) != hipSuccess) return dfail(d, BDX_ENOMEM, "gather buffer");
        if (const int rc = gather(d->b_pack.p, S.gcount, S.gdispl)) return rc;
        d->gathered_bytes += S.region_bytes;
        if (rank == 0) {
            if (const int rc = place_regions(B, S.gdispl, true)) return rc;
            if (const int rc = wait_regions()) return rc;   // (the packages sit in b_all, which the records' gather takes next)
        }
    }
    std::vector<size_t> rp_count(world), rp_displ(world);
    size_t rp_bytes = 0;
    std::vector<uint64_t> na_of_rank(world, 0);
    for (int t = 0; t < ntids; ++t)
        if (A.owner[t] >= 0) na_of_rank[A.owner[t]] += A.tot(t, 0);
    for (int q = 0; q < world; ++q) { rp_count[q] = (size_t)na_of_rank[q] * kw * 8; rp_displ[q] = rp_bytes; rp_bytes += rp_count[q]; }
    if (d->b_pack.ensure(std::max<size_t>(rp_count[rank], 8)) != hipSuccess) return dfail(d, BDX_ENOMEM, "record package");
    if (na) launch_k9_pack_replay(C->cp, C->k3.region_of, &C->b_p1.as<Pass1>()->n_anom, na, T + O.start, d->b_pack.as<unsigned long long>(), s);
    if (rank == 0 && d->b_all.ensure(std::max<size_t>(rp_bytes, 8)) != hipSuccess) return dfail(d, BDX_ENOMEM, "gather buffer");
    if (const int rc = gather(d->b_pack.p, rp_count, rp_displ)) return rc;
    others_wait = false;   // (the route's last collective: from here a rank answers to itself alone)
    DHIP(d, hipStreamSynchronize(s));
    d->gathered_bytes += rp_bytes;
    if (rank == 0) {
        const size_t tw = A.tw;
        std::vector<uint64_t> rp_host(rp_bytes / 8);
        if (rp_bytes) DHIP(d, hipMemcpy(rp_host.data(), d->b_all.p, rp_bytes, hipMemcpyDeviceToHost));
        // the records of all chromosomes in stream order: chromosomes ascending, each rank's package holds its own in order
        if (rp_host.size() != (size_t)na_all * kw) return dfail(d, BDX_EINTERNAL, "compact records of the gather do not add up");
        std::vector<uint64_t> key(na_all), chk(A.with_check ? na_all : 0);
        std::vector<int32_t> reg(na_all), isz(na_all);
        std::vector<uint32_t> meta(na_all);
        std::vector<uint64_t> sidx(A.want_support ? na_all : 0);   // index in the merged stream
        std::vector<uint64_t> at(ntids);
        for (int t = 0; t < ntids; ++t) at[t] = A.base[(size_t)t * tw];
        for (size_t i = 0; i < (size_t)na_all; ++i) {
            const uint64_t w0 = rp_host[i * kw], w1 = rp_host[i * kw + 1], w2 = rp_host[i * kw + 2];
            const uint32_t t = (uint32_t)(w2 >> 32);
            if (t >= (uint32_t)ntids || at[t] >= A.base[(size_t)(t + 1) * tw]) return dfail(d, BDX_EINTERNAL, "compact records of the gather do not add up");
            const size_t o = (size_t)at[t]++;
            key[o] = w0; reg[o] = (int32_t)(uint32_t)w1; meta[o] = (uint32_t)(w1 >> 32); isz[o] = (int32_t)(uint32_t)w2;
            if (ph && reg[o] >= 0) reg[o] += (int32_t)ph;   // (the read-less region 0 in front: replay_reads does the same)
            if (A.with_check) chk[o] = rp_host[i * kw + 3];
            if (A.want_support) sidx[o] = A.read_base[t] + rp_host[i * kw + 4];
        }
        if (solo && !regs) {   // (one rank: its table went to pinned memory beside the walk)
            if (C->sb.h_regs.ensure((size_t)NR * rrec) != hipSuccess || C->sb.h_pk.ensure(std::max<size_t>((size_t)NR * rpk, 16)) != hipSuccess) return dfail(d, BDX_ENOMEM, "region table");
            regs = C->sb.h_regs.as<RegionRec>(); pk = C->sb.h_pk.as<uint32_t>();
            DHIP(d, hipMemcpy(regs, d->b_rg_rec.p, (size_t)NR * rrec, hipMemcpyDeviceToHost));
            if (nkeys2) DHIP(d, hipMemcpy(pk, d->b_rg_pk.p, (size_t)NR * rpk, hipMemcpyDeviceToHost));
        }
        // (a region's first read: its index in its rank's list -> in the genome-wide one)
        {
            std::vector<uint64_t> seen(world, 0), adj(ntids, 0);
            for (int t = 0; t < ntids; ++t)
                if (A.owner[t] >= 0) { adj[t] = A.base[(size_t)t * tw] - seen[A.owner[t]]; seen[A.owner[t]] += A.tot(t, 0); }
            decode_regions(U, regs, pk, (uint32_t)NR, ph, false);
            for (size_t r = ph; r < NR + ph; ++r) U->regions[r].first += (uint32_t)adj[U->regions[r].tid];
        }
        memset(&U->counts, 0, sizeof(U->counts));
        U->counts.n_regions = (uint32_t)NR;
        U->counts.last_maxq = B.lm;
        if (A.with_check) unify_names(key.data(), chk.data(), (size_t)na_all);
        std::vector<uint32_t> sup;
        U->collect_support = A.want_support != 0;
        DCTX(d, U, replay_arrays(U, (uint32_t)na_all, key.data(), reg.data(), meta.data(), isz.data(), ph, A.want_support ? &sup : nullptr));
        if (A.want_support) {   // compact indices -> indices in the merged stream, and the reads' flags
            U->sup_idx.resize(sup.size());
            U->sup_flag.resize(sup.size());
            for (size_t i = 0; i < sup.size(); ++i) { U->sup_idx[i] = sidx[sup[i]]; U->sup_flag[i] = (uint8_t)meta_flag(meta[sup[i]]); }
        }
        U->p1.n_anom = (uint32_t)na_all;
    }
    ms(kPhReplayRoute) = since(t_r0);
    return finished();
}

// the one-rank result: the rank's table is the genome's
int DistRun::adopt_own_table(const Regions& B) {
    adopt_table(U, C);
    d->table_lent = true;
    U->reg = C->reg; U->nreg = C->nreg; U->rpk = C->rpk;   // (the genome's region table stays in this rank's pinned buffers until the next run)
    C->reg = nullptr; C->nreg = 0; C->rpk = nullptr;
    U->counts.n_regions = (uint32_t)B.NR;
    U->ran = true;
    ms(kPhMerge) = 0;
    return finished();
}

// ---- E: ONE gather takes every rank's package to rank 0: its region records, the pair groups of the components it could not walk
// alone, its finished table (rows sorted by order key) -- round 5: three gathers with two all-reduces of sizes between them.  Rank 0 then
// walks the gathered groups in its result context (K6 once more: the groups bucketed by later region stand where a rank's K6 has its
// reads, components of up to 64 regions on the device, the rest by the host -- round 5's host walked all of them, BreakDancer.cpp:266-346
// being one global walk) and merges the ranks' tables and that one by order key into the result context's pinned buffers ----
// The layout of the packages, from S's sums: the same on every rank, and so are the limits.
int DistRun::plan_packages(const Summary& S, Packages* out) {
    Packages& G = *out;
    G.TD.world = world;
    G.pcount.resize(world); G.pdispl.resize(world); G.grp_off.resize(world);
    for (int q = 0; q < world; ++q) {
        const TableCounts& c = S.of_rank[q];
        const size_t ng = (size_t)c.n_groups, nsv = (size_t)c.n_sv, nt = (size_t)c.n_terms, nc = (size_t)c.n_cn;
        size_t o = G.pbytes + S.gcount[q];          // (the package starts with the rank's region records: gdispl[q] is NOT their place here, pdispl[q] is)
        G.grp_off[q] = o; o += ng * sizeof(GroupRec);
        TablePackage& P = G.TD.p[q];
        P.n_sv = (uint32_t)nsv; P.n_terms = (uint32_t)nt; P.n_cn = (uint32_t)nc;
        P.rows_off = o; o += round_up(nsv * sizeof(SvOut), 8);
        P.keys_off = o; o += nsv * 8;
        P.lib_index_off = o; o += round_up(nt * 4, 8);
        P.lib_pairs_off = o; o += round_up(nt * 4, 8);
        P.ltail_off = o; o += nt * 8;
        P.cn_key_off = o; o += round_up(nc * 4, 8);
        P.cn_value_off = o; o += round_up(nc * 4, 8);
        G.pdispl[q] = G.pbytes; G.pcount[q] = o - G.pbytes; G.pbytes = o;
        G.ng_all += ng;
        G.sum.add_table(c); G.sum.n_pairs += c.n_pairs;
        G.max_sv = std::max(G.max_sv, (uint32_t)nsv);
    }
    if (dist_tracing() && rank == 0) fprintf(stderr, "[bdx dist] pair groups gathered on rank 0: %zu\n", G.ng_all);
    if (G.ng_all > kMaxAnomalous / 4) return dfail(d, BDX_ELIMIT, "too many pair groups of components that span ranks");   // (the same sums on every rank)
    if (G.max_sv >= (1u << 26) || G.sum.n_sv > 0xFFFFFFF0ull) return dfail(d, BDX_ELIMIT, "too many SV candidates for the merge");
    return BDX_OK;
}

// local: this rank's package; collective G
int DistRun::pack_and_gather(const Regions& B, const Summary& S, const Packages& G) {
    const TablePackage& P = G.TD.p[rank];
    if (d->b_pack.ensure(std::max<size_t>(G.pcount[rank], 8)) != hipSuccess) return dfail(d, BDX_ENOMEM, "package for rank 0");
    char* pp = (char*)d->b_pack.p - G.pdispl[rank];
    bool good = pack_regions(B, (char*)d->b_pack.p);
    auto put = [&](size_t off, const void* src, size_t bytes) { if (bytes && good) good = hipMemcpyAsync(pp + off, src, bytes, hipMemcpyDeviceToDevice, s) == hipSuccess; };
    put(G.grp_off[rank], C->k4.g_rec, (size_t)S.of_rank[rank].n_groups * sizeof(GroupRec));
    put(P.rows_off, C->sb.b_sv_out.p, (size_t)P.n_sv * sizeof(SvOut)); put(P.keys_off, C->sb.b_sv_key.p, (size_t)P.n_sv * 8);
    put(P.lib_index_off, C->sb.b_lib_index_out.p, (size_t)P.n_terms * 4); put(P.lib_pairs_off, C->sb.b_lib_pairs_out.p, (size_t)P.n_terms * 4);
    put(P.ltail_off, C->sb.b_ltail_out.p, (size_t)P.n_terms * 8);
    put(P.cn_key_off, C->sb.b_cn_key_out.p, (size_t)P.n_cn * 4); put(P.cn_value_off, C->sb.b_cn_value_out.p, (size_t)P.n_cn * 4);
    if (!good) return dfail(d, BDX_EHIP, "package for rank 0");
    trace("package");
    if (rank == 0 && d->b_all.ensure(std::max<size_t>(G.pbytes, 8)) != hipSuccess) return dfail(d, BDX_ENOMEM, "gather buffer");
    if (const int rc = collective(kPhGather, [&] { return gather(d->b_pack.p, G.pcount, G.pdispl); })) return rc;
    d->gathered_bytes += G.pbytes;
    trace("gathered");
    return BDX_OK;
}

// The result context as a K6 context: the genome's statistics and region table, no reads.  The gathered groups stand where a rank's K6
// has its reads -- bucketed by later region for the device's walk (in_groups, in_goff), or none of them for the host's.
// (K6 sizes its lists for a context's anomalous reads -- candidates and list entries <= reads / 2, each consuming a read pair; here
// a candidate consumes at least one pair GROUP and a list entry is a part of one: twice the groups stands for the reads)
int DistRun::result_as_k6_context(const Regions& B, uint32_t ng, const GroupRec* in_groups, const uint32_t* in_goff) {
    const uint32_t nr = (uint32_t)B.NR;
    const uint32_t capU = 2 * std::max(nr, ng) + 2;
    hipStream_t su = U->stream;
    DHIP(d, U->b_counts.ensure(sizeof(StageCounts))); DHIP(d, U->h_counts.ensure(sizeof(StageCounts)));
    DHIP(d, U->b_cnt.ensure((size_t)ncnt * 4)); DHIP(d, U->b_p1.ensure(sizeof(Pass1))); DHIP(d, U->b_kdens.ensure(64 * 4));
    DHIP(d, U->h_flags.ensure(64)); DHIP(d, U->sb.h_groups.ensure(((size_t)ng + 1) * sizeof(GroupRec)));
    if (in_groups) DHIP(d, size_out_deg(U->sb, capU));
    {
        StageCounts sc{};
        sc.n_regions = nr; sc.last_maxq = B.lm;
        memcpy(H + L.up_counts, &sc, sizeof(sc));
        const uint32_t* st_up = H + L.up_stats;   // (covered, window | flag histogram | densities: as this rank's own context got them)
        UploadList ul{};
        ul.copy(U->b_counts.p, H + L.up_counts, sizeof(StageCounts) / 4);
        ul.copy(U->b_p1.p, st_up, 2);
        ul.copy(U->b_cnt.p, st_up + 2, (size_t)ncnt);
        ul.copy(U->b_kdens.p, st_up + 2 + ncnt, U->key_density.size());
        launch_k9_upload(ul, su);
    }
    if (in_groups) launch_k6_scratch_init(U->sb.b_out_deg.as<uint32_t>(), capU, su);
    ++U->seq;
    U->na_alloc = 0; U->k6_cap = capU;
    U->k6_r_rec = U->sb.b_r_rec.as<RegionRec>(); U->k6_r_pk = U->sb.b_r_pk.as<uint32_t>(); U->k6_taint = nullptr;
    U->k6_in_groups = in_groups; U->k6_in_goff = in_goff;
    U->cp = Compact{}; U->k3 = K3Arrays{}; U->k4 = K4Arrays{};
    U->k4.g_rec = U->sb.h_groups.as<GroupRec>(); U->k4.g_cap = ng + 1;
    U->table_in_hbm = true; U->groups_in_hbm = false;
    memset(&U->counts, 0, sizeof(U->counts));
    return BDX_OK;
}

// rank 0: the gathered groups are walked in the result context, on its host or on its device; its table joins the ranks' in the merge
int DistRun::walk_gathered(const Stats& A, const Regions& B, const Summary& S, const Packages& G, TableCounts* walked, TablePackage* table) {
    const auto tw0 = now();
    const uint32_t ng = (uint32_t)G.ng_all, nr = (uint32_t)B.NR;
    const int32_t lm = B.lm;
    hipStream_t su = U->stream;
    // FEW gathered groups (a real genome's inter-chromosomal clusters: dozens of components) are walked by rank 0's HOST: K6 once more on
    // the device is twenty launches -- 0.3 ms of rank 0's time alone for 52 components -- where the host walks them in microseconds.  MANY
    // (thousands of translocations) stay on the device: round 5's host took 1.1-1.3 ms for 13 k groups.  Test switch "gather_walk" on the
    // result context: 1 always the device, 2 always the host.
    const bool host_gather = U->dbg_gather_walk == 2 || (U->dbg_gather_walk == 0 && G.ng_all <= kGatherHostMax);
    uint32_t* bucket_err = nullptr;   // (device walk: the bucket kernel's verdict)
    if (host_gather) {
        // the gathered groups: out of every rank's package into pinned memory, behind the gather
        DHIP(d, U->sb.h_groups.ensure(((size_t)ng + 1) * sizeof(GroupRec)));
        {
            GroupRec* hg = U->sb.h_groups.as<GroupRec>();
            size_t at = 0;
            for (int q = 0; q < world; ++q) {
                const size_t nq = (size_t)S.of_rank[q].n_groups;
                if (nq) DHIP(d, hipMemcpyAsync(hg + at, (const char*)d->b_all.p + G.grp_off[q], nq * sizeof(GroupRec), hipMemcpyDeviceToHost, s));
                at += nq;
            }
        }
        DHIP(d, hipEventRecord(d->ev_side, s));   // (the gather, the region table placed behind it, the groups' copies)
        DHIP(d, hipStreamWaitEvent(su, d->ev_side, 0));
        if (const int rc = result_as_k6_context(B, ng, nullptr, nullptr)) return rc;
        DCTX(d, U, k6_prepare(U, false, 0));   // (K6's arrays, no launch: the table stage below finds no candidate of the device's; NOT force_host -- that zeroes
                                          // the host candidates' order keys, which the merge of the ranks' tables goes by)
        DHIP(d, hipMemsetAsync(U->k6.own_nsv, 0, (size_t)U->k6_cap * 3 * 4, su));   // own_nsv | own_nacc | own_ncn: no vertex has candidates of its own
        DHIP(d, hipStreamSynchronize(s));   // (the groups are in pinned memory)
        U->counts.n_regions = nr; U->counts.n_groups = ng; U->counts.last_maxq = lm;
    } else {
        // buckets: cnt | goff | cur ([nr + 1] each) | scan workspace | n | err, then the groups in bucket order
        const size_t w_scan = 2 * ((size_t)scan_grid(nr + 1) + 2), o_goff = (size_t)nr + 1, o_cur = 2 * o_goff, o_ws = 3 * o_goff, o_n = o_ws + w_scan, o_err = o_n + 1,
                     o_grp = (o_err + 1 + 3) / 4 * 4;
        DHIP(d, d->b_bucket.ensure(o_grp * 4 + (size_t)ng * sizeof(GroupRec)));
        uint32_t* BK = d->b_bucket.as<uint32_t>();
        GroupRec* sorted = (GroupRec*)(BK + o_grp);
        SegList seg_grp{};
        seg_grp.n = world;
        {
            uint32_t a = 0;
            for (int q = 0; q < world; ++q) { seg_grp.off[q] = G.grp_off[q] / 8; seg_grp.start[q] = a; a += (uint32_t)S.of_rank[q].n_groups; }
            seg_grp.start[world] = a;
        }
        DHIP(d, hipEventRecord(d->ev_side, s));   // (the gather, and the region table placed behind it)
        DHIP(d, hipStreamWaitEvent(su, d->ev_side, 0));
        launch_k9_bucket_groups((const unsigned long long*)d->b_all.p, seg_grp, ng, nr, BK, BK + o_goff, BK + o_cur, sorted, BK + o_ws, BK + o_n, BK + o_err, su);
        bucket_err = BK + o_err;
        if (const int rc = result_as_k6_context(B, ng, sorted, BK + o_goff)) return rc;
        if (U->big_walk_mode < 0) U->last_big_groups = 1 << 20;   // (components of 5..64 regions on the device as well: what is left is the host's, sequentially)
        // (components that span ranks are mostly a translocation's two regions and their neighbours: three rounds of label propagation settle
        // them -- the eight of a context that walks large components are seven launches on rank 0's own part of the run; what has not
        // converged fails the closure check and is the host's)
        DCTX(d, U, k6_prepare(U, force_host(), kK6LabelRoundsGather));
        DCTX(d, U, k6_then_walk(U, launch_k6_groups));
        if (const int rc = await_flag(d, U, kGroupsReady, nullptr, "the pair groups of the gathered components did not arrive: their kernels were not launched")) return rc;
        U->counts = *U->h_counts.as<StageCounts>();
        if (U->counts.overflow) return dfail(d, BDX_EINTERNAL, "group list overflow (gathered components)");
    }
    decode_groups(U, U->sb.h_groups.as<GroupRec>(), U->counts.n_groups, 0);
    U->last_big_groups = (int64_t)U->counts.n_groups + U->counts.n_groups_big;
    if (U->counts.n_groups) {   // (the host's share of this walk reads the table in pinned memory: its copy ran beside the device's walk)
        // ... and the proper-read samples of the regions its groups name: those rows only
        // (on the stream of the table's copy, behind it: the result context's own stream is still walking)
        launch_k9_pk_rows(U->sb.h_groups.as<GroupRec>(), U->counts.n_groups, U->sb.b_r_pk.as<uint32_t>(), pk, (uint32_t)nkeys2, nr, C->copy_stream);
        regs_pending = true;
        if (const int rc = wait_regions()) return rc;
    }
    decode_regions(U, regs, pk, nr, 0, true);
    const auto tw1 = now();
    DCTX(d, U, host_walk(U, lm, A.na_all != 0));
    ms(kPhHostWalk) = since(tw1);
    U->counts.last_maxq = lm;
    DCTX(d, U, do_k6_table(U));
    DCTX(d, U, finish_table(U));
    if (bucket_err) {   // (the bucket kernel's verdict, read once the table is there: a wait for it in front of the host's share of the walk kept the host from
        // enqueueing the table stage while the device walked -- 40 us of rank 0's time alone; a group outside the table is skipped by the kernels)
        uint32_t berr = 0;
        DHIP(d, hipMemcpyAsync(&berr, bucket_err, 4, hipMemcpyDeviceToHost, U->stream));
        DHIP(d, hipStreamSynchronize(U->stream));
        if (berr) return dfail(d, BDX_EINTERNAL, "a gathered pair group names a region outside the genome's table");
    }
    *walked = TableCounts::of(U);   // (n_groups: what the host's walk took -- components the device walk leaves out)
    ms(kPhDeviceWalkGathered) = since(tw0) - ms(kPhHostWalk);
    TablePackage& P = *table;   // the table of the gathered components, where the result context's K6 left it (byte offsets relative to the gather buffer)
    P.n_sv = (uint32_t)walked->n_sv; P.n_terms = (uint32_t)walked->n_terms; P.n_cn = (uint32_t)walked->n_cn;
    auto off = [&](const DevBuf& b) { return (uint64_t)((uintptr_t)b.p - (uintptr_t)d->b_all.p); };
    P.rows_off = off(U->sb.b_sv_out); P.keys_off = off(U->sb.b_sv_key); P.lib_index_off = off(U->sb.b_lib_index_out); P.lib_pairs_off = off(U->sb.b_lib_pairs_out);
    P.ltail_off = off(U->sb.b_ltail_out); P.cn_key_off = off(U->sb.b_cn_key_out); P.cn_value_off = off(U->sb.b_cn_value_out);
    DHIP(d, hipEventRecord(d->ev_side, U->stream));   // (its table kernel: finish_table has seen its ready word, this orders the streams)
    DHIP(d, hipStreamWaitEvent(s, d->ev_side, 0));
    return BDX_OK;
}

// rank 0: the ranks' tables and the one of the gathered components, merged by order key into the result context's pinned buffers
int DistRun::merge_tables(const Regions& B, const Packages& G, const TableCounts& walked, const TablePackage& walked_table) {
    TableDesc TD = G.TD;
    TableCounts all = G.sum;
    uint32_t max_sv = G.max_sv;
    if (G.ng_all) {   // (one more package: the table of the gathered components)
        TD.p[world] = walked_table;
        TD.world = world + 1;
        all.add_table(walked);
        max_sv = std::max(max_sv, (uint32_t)walked.n_sv);
        if (max_sv >= (1u << 26) || all.n_sv > 0xFFFFFFF0ull) return dfail(d, BDX_ELIMIT, "too many SV candidates for the merge");
    }
    const uint32_t n_total = (uint32_t)all.n_sv;
    const uint64_t n_terms_all = all.n_terms, n_cn_all = all.n_cn;
    DHIP(d, U->sb.h_sv_out.ensure(std::max<size_t>(n_total, 1) * sizeof(SvOut)));
    DHIP(d, U->sb.h_lib_index.ensure(std::max<size_t>(n_terms_all, 1) * 4)); DHIP(d, U->sb.h_lib_pairs.ensure(std::max<size_t>(n_terms_all, 1) * 4));
    DHIP(d, U->sb.h_ltail_dev.ensure(std::max<size_t>(n_terms_all, 1) * 8));
    DHIP(d, U->sb.h_cn_key.ensure(std::max<size_t>(n_cn_all, 1) * 4 + 16)); DHIP(d, U->sb.h_cn_value.ensure(std::max<size_t>(n_cn_all, 1) * 4 + 16));
    if (n_total) {
        const size_t ws_words = ((size_t)scan_grid(n_total) + 4) * 4;
        DHIP(d, d->b_merge.ensure((size_t)n_total * 12 + ws_words * 4 + sizeof(TableDesc) + 128));
        uint2* begins = d->b_merge.as<uint2>();
        uint32_t* src = (uint32_t*)(begins + n_total);
        uint32_t* ws = (uint32_t*)(((uintptr_t)(src + n_total) + 15) & ~(uintptr_t)15);
        TableDesc* d_td = (TableDesc*)(((uintptr_t)(ws + ws_words) + 15) & ~(uintptr_t)15);
        DHIP(d, hipMemcpyAsync(d_td, &TD, sizeof(TableDesc), hipMemcpyHostToDevice, s));
        DHIP(d, hipMemcpyAsync(T + O.ntot + 2, &n_total, 4, hipMemcpyHostToDevice, s));
        MergeOut mo{U->sb.h_sv_out.as<SvOut>(), U->sb.h_lib_index.as<int32_t>(), U->sb.h_lib_pairs.as<int32_t>(), d->opts.fisher ? U->sb.h_ltail_dev.as<double>() : nullptr,
                    U->sb.h_cn_key.as<int32_t>(), U->sb.h_cn_value.as<float>()};
        if (dist_tracing()) {   // are the ranks' tables sorted by key, and are the keys distinct?
            DHIP(d, hipStreamSynchronize(s));
            for (int q = 0; q < TD.world; ++q) {
                std::vector<unsigned long long> kk(TD.p[q].n_sv);
                if (!kk.empty()) DHIP(d, hipMemcpy(kk.data(), (const char*)d->b_all.p + TD.p[q].keys_off, kk.size() * 8, hipMemcpyDeviceToHost));
                size_t bad = 0;
                for (size_t i = 1; i < kk.size(); ++i) bad += kk[i] < kk[i - 1];
                fprintf(stderr, "[bdx dist] table of rank %d: %zu rows, %zu out of key order; first keys", q, kk.size(), bad);
                for (size_t i = 0; i < kk.size() && i < 6; ++i) fprintf(stderr, " (T %llu own %llu start %llu)", kk[i] >> kKeyShiftT, (kk[i] >> kKeyShiftOwn) & 1, (kk[i] >> kKeyShiftStart) & kKeyStartMask);
                fprintf(stderr, "\n");
            }
        }
        DHIP(d, hipMemsetAsync(src, 0xFF, (size_t)n_total * 4, s));
        launch_k9_merge_tables((const char*)d->b_all.p, d_td, TD.world, n_total, max_sv, src, begins, ws, T + O.ntot + 2, mo, s);
    }
    DHIP(d, hipStreamSynchronize(s));
    DHIP(d, hipGetLastError());
    trace("merge");
    U->walk.clear(); U->log_tail.clear();
    U->n_sv_total = n_total; U->n_terms_total = (uint32_t)n_terms_all; U->n_cn_total = (uint32_t)n_cn_all; U->n_printed = (uint32_t)all.n_printed;
    U->n_sv_host = (uint32_t)all.n_sv_host; U->n_groups_total = (uint32_t)all.n_groups_total;
    memset(&U->counts, 0, sizeof(U->counts));
    U->counts.n_regions = (uint32_t)B.NR; U->counts.last_maxq = B.lm; U->counts.n_pairs = (uint32_t)all.n_pairs; U->counts.n_old = (uint32_t)all.n_old;
    U->counts.n_sv_dev = n_total - U->n_sv_host; U->counts.n_groups = (uint32_t)walked.n_groups;   // (what the host's walk took: components the device walk leaves out)
    U->materialized = false; U->rows_packed = true;   // (k9_merge_tables writes SvWire rows, like a single context's table kernel)
    {   // the genome's region table: in rank 0's pinned buffers until the next run
        if (const int rc = wait_regions()) return rc;
        decode_regions(U, regs, pk, (uint32_t)B.NR, 0, true);
        C->reg = nullptr; C->nreg = 0; C->rpk = nullptr;
    }
    if (d->opts.fisher) {  // Fisher's combination (BreakDancer.cpp:71-81) uses the host's exp / log
        materialize(U);
        finish_scores(U->opts, U->log_tail.data(), U->walk.svs.data(), U->walk.svs.size(), &U->n_printed);
    }
    U->ran = true;
    return BDX_OK;
}

}  // namespace

// The protocol of the header comment, phase by phase: local work whose failure travels with the next all-reduce, then the collective.
extern "C" int bdx_dist_run(bdx_dist* d) {
    if (!d) return BDX_EINVAL;
    const auto t_begin = std::chrono::steady_clock::now();
    DHIP(d, hipSetDevice(d->device));
    if (d->reads->sizing.load(std::memory_order_acquire)) return dfail(d, BDX_ESTATE, "the buffers of the later stages are being sized on another thread (bdx_bamdec_finish has not returned)");
    DistRun R(d, t_begin);
    auto protocol = [&]() -> int {
        int rc = R.begin();
        if (rc != BDX_OK) return rc;
        std::vector<uint64_t> v1(R.W.words, 0), v3((size_t)R.ntids + 1, 0);
        Stats A; Regions B; ExchangePlan X; Summary S; Packages G;
        R.local(kPhPass1, [&] { return R.pass1_and_counts(v1); });
        if ((rc = R.agree_statistics(v1, &A)) != BDX_OK) return rc;                  // A
        R.local(kPhRegionCut, [&] { return R.cut_regions(A, v3); });
        if ((rc = R.agree_regions(A, v3, &B)) != BDX_OK) return rc;                  // B
        if ((rc = R.seed_result(A, B)) != BDX_OK) return rc;
        if (!B.NR) return R.finished();   // no region anywhere: an empty table
        R.t_x0 = DistRun::now();
        R.plan_exchange(A, B, &X);
        R.local(kPhGlobalizePack, [&] { return R.globalize_and_scatter(A, B, X); });
        if (R.st.rc != BDX_OK) {   // (a rank that cannot take part in the all-to-all: the others would wait for it -- the communicator is given up)
            R.others_wait = true;
            return dfail(d, R.st.rc, R.st.msg);
        }
        if ((rc = R.all_to_all(A, X)) != BDX_OK) return rc;                          // X
        TableCounts mine, walked;
        TablePackage walked_table{};
        uint64_t irregular = 0;
        R.t_x1 = DistRun::now();
        R.local(kPhJoinsWalkTable, [&] { return R.join_walk_table(A, B, X, &mine, &irregular); });
        d->ms_exchange = ms_between(R.t_x0, R.t_x1);
        if ((rc = R.agree_packages(A, B, mine, irregular, &S)) != BDX_OK) return rc;  // S
        // ---- nothing can be folded into an all-reduce any more: until this rank's last collective is behind it, its failure leaves the others waiting ----
        R.others_wait = true;
        if (!R.solo && (uint64_t)B.nr_local != B.nr_of_rank[R.rank]) return dfail(d, BDX_EINTERNAL, "region counts of the chromosomes do not add up");
        if (S.replay) return R.replay_route(A, B, S);
        if (R.solo) return R.adopt_own_table(B);
        const auto t_m0 = DistRun::now();
        R.others_wait = false;   // (limits computed from S's sums: every rank returns alike)
        if ((rc = R.plan_packages(S, &G)) != BDX_OK) return rc;
        R.others_wait = true;
        if ((rc = R.pack_and_gather(B, S, G)) != BDX_OK) return rc;                  // G
        R.others_wait = false;   // ---- rank 0 alone from here ----
        if (R.rank == 0) {
            // (the packages start with the region records: their own displacements place them)
            if ((rc = R.place_regions(B, G.pdispl, false)) != BDX_OK) return rc;
            if (G.ng_all && (rc = R.walk_gathered(A, B, S, G, &walked, &walked_table)) != BDX_OK) return rc;
            if ((rc = R.merge_tables(B, G, walked, walked_table)) != BDX_OK) return rc;
        }
        R.ms(kPhMerge) = R.rank != 0 ? R.since(t_m0) : std::max(0.0f, R.since(t_m0) - R.ms(kPhHostWalk) - R.ms(kPhDeviceWalkGathered) - R.ms(kPhGather));
        return R.finished();
    };
    const int rc = protocol();
    // The ONE exit rule for what cannot be folded: a failure that every rank computes alike, or that rank 0 meets alone behind the last
    // collective, is returned; any other would leave the other ranks waiting for this one -- the communicator is given up, which wakes them.
    if (rc != BDX_OK && R.others_wait && R.world > 1) d->comm->abort();
    return rc;
}
