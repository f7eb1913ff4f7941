// Test-only harness (tests/test_gpu_regions.py) around the two launchers between K2 and the walk, linked with their translation units
// unchanged: launch_k3 (csrc/k3_regions.hip: head scan, accept scan, region table, k3_region_of_kernel) and launch_k4_join_only
// (csrc/k4_join.hip: the direct join with its fused region-of and its forward of the region table, the bucketed join).  Built into
// tests/prims/libbdx_stages.so; nothing of it is part of libbdx.so.  Every entry point takes host pointers, does its own copies, waits
// for the stream and returns HIP's error code.  A handle keeps one buffer set from call to call, as a context does; every output starts
// a call as 0xA5 bytes, with a guard of 0xA5 bytes behind every array.  The launchers' preconditions are kept here: c_maxq zero on
// entry, the look-back words zero at allocation and sized 5 x scan_grid(cap, 1), a stamp that is not 0 and has not been used, counts
// that fit their arrays, indices that stay inside their tables.  A call that breaks one gets hipErrorInvalidValue and is never launched
// (a look-back launch with a stale stamp would spin).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <new>
#include <unordered_set>
#include <vector>

#include "bdx_k3.h"
#include "bdx_scan.h"

using namespace bdx;

namespace {

#define CK(x) do { const hipError_t e_ = (x); if (e_ != hipSuccess) return (int)e_; } while (0)

constexpr unsigned char kFill = 0xA5;
constexpr size_t kGuard = 256;                      // bytes of 0xA5 behind every array
constexpr uint32_t kLbMaxN = (1u << 20) + 1;        // no look-back grid beyond 4,097 workgroups from a test
constexpr uint32_t kMaxSlots = 1u << 20;            // the direct table of a test
constexpr int kMaxKeys = 8;
constexpr uint32_t kRecWords = sizeof(RegionRec) / 4;

// an array in HBM or in pinned host memory and the guard behind it
struct Buf {
    void* p = nullptr;
    size_t bytes = 0;
    bool pinned = false;
    ~Buf() { if (p) (void)(pinned ? hipHostFree(p) : hipFree(p)); }
    hipError_t alloc(size_t b, bool pin = false) {
        bytes = b; pinned = pin;
        const hipError_t e = pin ? hipHostMalloc(&p, b + kGuard, hipHostMallocDefault) : hipMalloc(&p, b + kGuard);
        return e != hipSuccess ? e : set(kFill, b + kGuard);
    }
    hipError_t set(int v, size_t b) {
        if (pinned) { memset(p, v, b); return hipSuccess; }
        return hipMemset(p, v, b);
    }
    hipError_t fill() { return set(kFill, bytes + kGuard); }
    hipError_t zero() { return set(0, bytes); }
    hipError_t put(const void* src, size_t b) {
        if (!b) return hipSuccess;
        if (pinned) { memcpy(p, src, b); return hipSuccess; }
        return hipMemcpy(p, src, b, hipMemcpyHostToDevice);
    }
    hipError_t get(void* dst, size_t b) const {
        if (!b) return hipSuccess;
        if (pinned) { memcpy(dst, p, b); return hipSuccess; }
        return hipMemcpy(dst, p, b, hipMemcpyDeviceToHost);
    }
    hipError_t guard(uint32_t* bad) const {
        unsigned char g[kGuard];
        if (pinned) memcpy(g, (const char*)p + bytes, kGuard);
        else if (const hipError_t e = hipMemcpy(g, (const char*)p + bytes, kGuard, hipMemcpyDeviceToHost)) return e;
        for (unsigned char b : g)
            if (b != kFill) *bad = 1;
        return hipSuccess;
    }
    template <class T> T* as() const { return (T*)p; }
};

bool pow2(uint32_t v) { return v && !(v & (v - 1)); }

struct CutHandle {
    uint32_t cap = 0, ntids = 0;
    int nkeys = 0;
    Buf tid, pos, meta, nn, pk, p1, tail;                                                      // inputs
    Buf cand, pre_q, pre_rev, pre_nonctx, c_first, c_maxq, c_rid, region_of, r_rec_dev, r_pk_dev, out_deg, counts, lb;
    Buf r_rec, r_pk, counts_host;                                                              // pinned
    std::unordered_set<uint32_t> used;                                                         // the stamps the look-back words have seen
    Buf* all[23] = {&tid, &pos, &meta, &nn, &pk, &p1, &tail, &cand, &pre_q, &pre_rev, &pre_nonctx, &c_first, &c_maxq, &c_rid, &region_of,
                    &r_rec_dev, &r_pk_dev, &out_deg, &counts, &lb, &r_rec, &r_pk, &counts_host};
};

struct JoinHandle {
    uint32_t cap = 0, fcap = 0, slots = 0, rcap = 0, ccap = 0;
    Buf key, check, region, cand, c_rid, fkey, fcheck, fregion, nwords, counts;                // inputs
    Buf partner, pair_lo, region_out, scratch, t_key, t_idx, bcnt, boff, bcur, e_key, e_idx;
    Buf r_rec_dev, r_pk_dev;
    Buf r_rec_host, r_pk_host;                                                                 // pinned
    Buf* all[25] = {&key, &check, &region, &cand, &c_rid, &fkey, &fcheck, &fregion, &nwords, &counts, &partner, &pair_lo, &region_out, &scratch,
                    &t_key, &t_idx, &bcnt, &boff, &bcur, &e_key, &e_idx, &r_rec_dev, &r_pk_dev, &r_rec_host, &r_pk_host};
};

}  // namespace

extern "C" {

// out: [4] kScanBlock, kJoinLdsSlots, kMaxBuckets, words of a region record: what tests/region_cases.py's models are built on
void stages_constants(uint32_t* out) {
    const uint32_t v[4] = {(uint32_t)kScanBlock, (uint32_t)kJoinLdsSlots, (uint32_t)kMaxBuckets, kRecWords};
    memcpy(out, v, sizeof(v));
}

// a buffer set for up to cap anomalous reads, nkeys counter keys and (ntids > 0) a tid_tail table of ntids chromosomes
int stages_cut_open(uint32_t cap, int nkeys, uint32_t ntids, void** out) {
    if (!cap || cap > kLbMaxN || nkeys < 1 || nkeys > kMaxKeys || ntids > 4096) return (int)hipErrorInvalidValue;
    CutHandle* h = new (std::nothrow) CutHandle;
    if (!h) return (int)hipErrorOutOfMemory;
    h->cap = cap; h->nkeys = nkeys; h->ntids = ntids;
    const size_t c4 = (size_t)cap * 4;
    hipError_t e = hipSuccess;
    auto A = [&](Buf& b, size_t bytes, bool pin = false) { if (e == hipSuccess) e = b.alloc(bytes, pin); };
    A(h->tid, c4); A(h->pos, c4); A(h->meta, c4); A(h->nn, c4); A(h->pk, c4 * nkeys); A(h->p1, sizeof(Pass1)); A(h->tail, (size_t)(ntids ? ntids : 1) * 16);
    A(h->cand, c4); A(h->pre_q, c4); A(h->pre_rev, c4); A(h->pre_nonctx, c4); A(h->c_first, c4); A(h->c_maxq, c4); A(h->c_rid, c4); A(h->region_of, c4);
    A(h->r_rec_dev, (size_t)cap * sizeof(RegionRec)); A(h->r_pk_dev, c4 * 2 * nkeys); A(h->out_deg, c4 * 6); A(h->counts, sizeof(StageCounts));
    A(h->lb, (size_t)5 * scan_grid(cap, 1) * 8);
    A(h->r_rec, (size_t)cap * sizeof(RegionRec), true); A(h->r_pk, c4 * 2 * nkeys, true); A(h->counts_host, sizeof(StageCounts), true);
    if (e == hipSuccess) e = h->lb.zero();   // once
    if (e != hipSuccess) { delete h; return (int)e; }
    *out = h;
    return 0;
}
void stages_cut_close(void* handle) { delete (CutHandle*)handle; }

// tid, pos, meta, nn: [n_anom]; pk: [nkeys][n_anom]; tid_tail: [ntids][4] or null.  n_anom is the device-side count, n_anom_host what the launches
// are sized with (>= n_anom, as an enqueue-ahead guess is).  Outputs, as the launches left them: cand, c_first, c_maxq, c_rid, region_of: [cap];
// scratch: [6][cap]; rec_host, rec_dev: [cap][9]; pk_host, pk_dev: [cap][2 * nkeys]; out_counts: [8] the device's n_cand, n_regions, last_maxq
// (0 before the launch), the host mirror's (0xA5A5A5A5 before it), 1 where a guard byte changed, 0
int stages_cut_run(void* handle, const int32_t* tid, const int32_t* pos, const uint32_t* meta, const uint32_t* nn, const uint32_t* pk, int32_t window,
                   uint32_t n_anom, uint32_t n_normal, uint32_t n_anom_host, int min_len, int seq_coverage_lim, const uint32_t* tid_tail,
                   int host_copy_later, int region_of_launch, uint32_t stamp, int32_t* cand, uint32_t* c_first, int32_t* c_maxq, int32_t* c_rid,
                   int32_t* region_of, uint32_t* scratch, uint32_t* rec_host, uint32_t* pk_host, uint32_t* rec_dev, uint32_t* pk_dev, uint32_t* out_counts) {
    CutHandle* h = (CutHandle*)handle;
    if (!h || n_anom > n_anom_host || n_anom_host > h->cap) return (int)hipErrorInvalidValue;
    if (tid_tail) {
        if (!h->ntids) return (int)hipErrorInvalidValue;
        for (uint32_t j = 0; j < n_anom; ++j)
            if (tid[j] < 0 || (uint32_t)tid[j] >= h->ntids) return (int)hipErrorInvalidValue;
    }
    if (stamp == 0 || stamp > 0x3FFFFFFFu || !h->used.insert(stamp).second) return (int)hipErrorInvalidValue;
    const size_t cap = h->cap, c4 = cap * 4, n4 = (size_t)n_anom * 4;
    for (Buf* b : h->all)
        if (b != &h->lb) CK(b->fill());
    CK(h->c_maxq.zero());
    CK(h->tid.put(tid, n4)); CK(h->pos.put(pos, n4)); CK(h->meta.put(meta, n4)); CK(h->nn.put(nn, n4));
    for (int k = 0; k < h->nkeys; ++k)
        if (n4) CK(hipMemcpy(h->pk.as<uint32_t>() + (size_t)k * cap, pk + (size_t)k * n_anom, n4, hipMemcpyHostToDevice));
    if (tid_tail) CK(h->tail.put(tid_tail, (size_t)h->ntids * 16));
    {
        std::vector<unsigned char> raw(sizeof(Pass1), kFill);
        Pass1* p = (Pass1*)raw.data();
        p->window = window; p->n_anom = n_anom; p->n_normal = n_normal;
        CK(h->p1.put(p, sizeof(Pass1)));
    }
    CK(h->counts.zero());
    K3Arrays a;
    memset(&a, 0, sizeof(a));
    a.cap = h->cap;
    a.cand = h->cand.as<int32_t>(); a.pre_q = h->pre_q.as<uint32_t>(); a.pre_rev = h->pre_rev.as<uint32_t>(); a.pre_nonctx = h->pre_nonctx.as<uint32_t>();
    a.c_first = h->c_first.as<uint32_t>(); a.c_maxq = h->c_maxq.as<int32_t>(); a.c_rid = h->c_rid.as<int32_t>(); a.region_of = h->region_of.as<int32_t>();
    a.r_rec = h->r_rec.as<RegionRec>(); a.r_pk = h->r_pk.as<uint32_t>(); a.r_rec_dev = h->r_rec_dev.as<RegionRec>(); a.r_pk_dev = h->r_pk_dev.as<uint32_t>();
    a.host_copy_later = host_copy_later ? 1 : 0;
    a.out_deg = h->out_deg.as<uint32_t>();
    a.lb_state = h->lb.as<unsigned long long>(); a.lb_stamp = stamp;
    a.counts = h->counts.as<StageCounts>(); a.counts_host = h->counts_host.as<StageCounts>();
    Compact cp;
    memset(&cp, 0, sizeof(cp));
    cp.tid = h->tid.as<int32_t>(); cp.pos = h->pos.as<int32_t>(); cp.meta = h->meta.as<uint32_t>(); cp.nn = h->nn.as<uint32_t>(); cp.pk = h->pk.as<uint32_t>();
    cp.cap = h->cap;
    launch_k3(a, cp, h->p1.as<Pass1>(), n_anom_host, min_len, seq_coverage_lim, h->nkeys, tid_tail ? h->tail.as<uint32_t>() : nullptr, region_of_launch != 0, nullptr);
    CK(hipGetLastError());
    CK(hipStreamSynchronize(nullptr));
    CK(h->cand.get(cand, c4)); CK(h->c_first.get(c_first, c4)); CK(h->c_maxq.get(c_maxq, c4)); CK(h->c_rid.get(c_rid, c4)); CK(h->region_of.get(region_of, c4));
    CK(h->out_deg.get(scratch, c4 * 6));
    CK(h->r_rec.get(rec_host, cap * sizeof(RegionRec))); CK(h->r_rec_dev.get(rec_dev, cap * sizeof(RegionRec)));
    CK(h->r_pk.get(pk_host, c4 * 2 * h->nkeys)); CK(h->r_pk_dev.get(pk_dev, c4 * 2 * h->nkeys));
    StageCounts sc, sh;
    CK(h->counts.get(&sc, sizeof(sc))); CK(h->counts_host.get(&sh, sizeof(sh)));
    out_counts[0] = sc.n_cand; out_counts[1] = sc.n_regions; out_counts[2] = (uint32_t)sc.last_maxq;
    out_counts[3] = sh.n_cand; out_counts[4] = sh.n_regions; out_counts[5] = (uint32_t)sh.last_maxq;
    out_counts[6] = 0; out_counts[7] = 0;
    for (Buf* b : h->all) CK(b->guard(&out_counts[6]));
    return 0;
}

// a buffer set for up to cap own entries, fcap foreign ones, ccap candidates and a region table of rcap regions to forward.  slots > 0: the direct join's
// table of that many words (a power of two); slots == 0: the bucketed join's arrays, bcnt zero here and never again
int stages_join_open(uint32_t cap, uint32_t fcap, uint32_t ccap, uint32_t slots, uint32_t rcap, void** out) {
    if (!cap || cap > kLbMaxN || fcap > kLbMaxN || ccap > kLbMaxN || rcap > kLbMaxN || (slots && (!pow2(slots) || slots < 2 || slots > kMaxSlots)))
        return (int)hipErrorInvalidValue;
    if (!slots && (fcap || rcap)) return (int)hipErrorInvalidValue;   // foreign entries and the forward are the direct kernel's
    JoinHandle* h = new (std::nothrow) JoinHandle;
    if (!h) return (int)hipErrorOutOfMemory;
    h->cap = cap; h->fcap = fcap; h->ccap = ccap; h->slots = slots; h->rcap = rcap;
    const size_t c4 = (size_t)cap * 4, f4 = (size_t)(fcap ? fcap : 1) * 4, r = rcap ? rcap : 1;
    hipError_t e = hipSuccess;
    auto A = [&](Buf& b, size_t bytes, bool pin = false) { if (e == hipSuccess) e = b.alloc(bytes, pin); };
    A(h->key, c4 * 2); A(h->check, c4 * 2); A(h->region, c4); A(h->cand, c4); A(h->c_rid, (size_t)(ccap ? ccap : 1) * 4);
    A(h->fkey, f4 * 2); A(h->fcheck, f4 * 2); A(h->fregion, f4); A(h->nwords, 8); A(h->counts, sizeof(StageCounts));
    A(h->partner, c4); A(h->pair_lo, c4); A(h->region_out, c4); A(h->scratch, c4 * 6);
    A(h->t_key, slots ? (size_t)slots * 8 : c4 * 4); A(h->t_idx, slots ? 16 : c4 * 2);
    A(h->bcnt, (size_t)kMaxBuckets * 4); A(h->boff, (size_t)(kMaxBuckets + 1) * 4); A(h->bcur, (size_t)kMaxBuckets * 4);
    A(h->e_key, c4 * 2); A(h->e_idx, c4);
    A(h->r_rec_dev, r * sizeof(RegionRec)); A(h->r_pk_dev, r * 4 * 2 * kMaxKeys);
    A(h->r_rec_host, r * sizeof(RegionRec), true); A(h->r_pk_host, r * 4 * 2 * kMaxKeys, true);
    if (e == hipSuccess) e = h->bcnt.zero();   // once
    if (e != hipSuccess) { delete h; return (int)e; }
    *out = h;
    return 0;
}
void stages_join_close(void* handle) { delete (JoinHandle*)handle; }

// key: [n_own]; check: [n_own] or null; the regions either as region: [n_own] or as cand: [n_own] + c_rid: [n_cand] (the fused region-of: direct only, with
// region_out and, with_scratch, the K6 scratch).  foreign != 0: fkey, fcheck (with check), fregion: [n_foreign] behind the own entries, n_local on the device.
// n_host >= n_own + n_foreign sizes the launches.  forward != 0: rec: [n_regions][9] and pk: [n_regions][nkeys2] go to the device, the join forwards them.
// nbuckets / log2b: the bucketed join's (slots == 0 handles).  Outputs: partner, pair_lo, region_out: [cap]; scratch: [6][cap]; fwd_rec: [rcap][9]; fwd_pk:
// [rcap * 16] (rows of nkeys2 words); boff: [nbuckets + 1]; out_counts: [8] irregular, n_entries (0xA5A5A5A5 before the launches), 1 where a guard byte changed, buckets of
// bcnt that are not zero after the run, 0 ...
int stages_join_run(void* handle, const uint64_t* key, const uint64_t* check, const int32_t* region, const int32_t* cand, const int32_t* c_rid, uint32_t n_cand,
                    uint32_t n_own, int foreign, const uint64_t* fkey, const uint64_t* fcheck, const int32_t* fregion, uint32_t n_foreign, uint32_t n_host,
                    int want_pair_lo, int with_scratch, int forward, const uint32_t* rec, const uint32_t* pk, uint32_t n_regions, int nkeys2, uint32_t nbuckets,
                    uint32_t log2b, int32_t* partner, int32_t* pair_lo, int32_t* region_out, uint32_t* scratch, uint32_t* fwd_rec, uint32_t* fwd_pk, uint32_t* boff,
                    uint32_t* out_counts) {
    JoinHandle* h = (JoinHandle*)handle;
    if (!h || !key) return (int)hipErrorInvalidValue;
    const bool direct = h->slots != 0, fused = cand != nullptr;
    const uint64_t n_total = (uint64_t)n_own + (foreign ? n_foreign : 0);
    if (n_own > h->cap || n_total > n_host || n_host > (uint64_t)h->cap + h->fcap) return (int)hipErrorInvalidValue;
    if (fused ? (!c_rid || region || n_cand > h->ccap) : !region) return (int)hipErrorInvalidValue;
    if (foreign && (!fkey || !fregion || (check && !fcheck) || n_foreign > h->fcap)) return (int)hipErrorInvalidValue;
    if (forward && (!rec || !pk || n_regions > h->rcap || nkeys2 < 2 || nkeys2 > 2 * kMaxKeys)) return (int)hipErrorInvalidValue;
    if (direct) {
        if (n_total * 2 > h->slots) return (int)hipErrorInvalidValue;   // the table at most half full
        if (fused)
            for (uint32_t j = 0; j < n_own; ++j)
                if (cand[j] < 0 || (uint32_t)cand[j] >= n_cand) return (int)hipErrorInvalidValue;
    } else {
        if (fused || foreign || forward || with_scratch || !pow2(nbuckets) || nbuckets > (uint32_t)kMaxBuckets || (1u << log2b) != nbuckets) return (int)hipErrorInvalidValue;
    }
    for (Buf* b : h->all)
        if (b != &h->bcnt) CK(b->fill());
    const size_t o4 = (size_t)n_own * 4, f4 = (size_t)n_foreign * 4, c4 = (size_t)h->cap * 4;
    CK(h->key.put(key, o4 * 2));
    if (check) CK(h->check.put(check, o4 * 2));
    if (region) CK(h->region.put(region, o4));
    if (fused) { CK(h->cand.put(cand, o4)); CK(h->c_rid.put(c_rid, (size_t)n_cand * 4)); }
    if (foreign) {
        CK(h->fkey.put(fkey, f4 * 2)); CK(h->fregion.put(fregion, f4));
        if (check) CK(h->fcheck.put(fcheck, f4 * 2));
    }
    const uint32_t nw[2] = {(uint32_t)n_total, n_own};
    CK(h->nwords.put(nw, 8));
    StageCounts sc;
    memset(&sc, 0, sizeof(sc));
    sc.n_regions = forward ? n_regions : 0u; sc.n_entries = 0xA5A5A5A5u;
    CK(h->counts.put(&sc, sizeof(sc)));
    if (forward) { CK(h->r_rec_dev.put(rec, (size_t)n_regions * sizeof(RegionRec))); CK(h->r_pk_dev.put(pk, (size_t)n_regions * nkeys2 * 4)); }
    K4Arrays k4;
    memset(&k4, 0, sizeof(k4));
    k4.partner = h->partner.as<int32_t>();
    k4.t_key = h->t_key.as<uint64_t>(); k4.t_idx = h->t_idx.as<int32_t>();
    const bool with_lo = direct && (fused || want_pair_lo);
    if (direct) {   // the table all ones, partner and pair_lo at -1
        CK(hipMemset(h->t_key.p, 0xFF, (size_t)h->slots * 8));
        if (o4) CK(hipMemset(h->partner.p, 0xFF, o4));
        if (with_lo) {
            if (o4) CK(hipMemset(h->pair_lo.p, 0xFF, o4));
            k4.pair_lo = h->pair_lo.as<int32_t>();
        }
        k4.direct = 1; k4.t_mask = h->slots - 1;
    } else {
        k4.nbuckets = nbuckets; k4.log2b = log2b;
        k4.bcnt = h->bcnt.as<uint32_t>(); k4.boff = h->boff.as<uint32_t>(); k4.bcur = h->bcur.as<uint32_t>();
        k4.e_key = h->e_key.as<uint64_t>(); k4.e_idx = h->e_idx.as<uint32_t>();
    }
    Entries en;
    memset(&en, 0, sizeof(en));
    en.key = h->key.as<uint64_t>(); en.check = check ? h->check.as<uint64_t>() : nullptr;
    en.region = region ? h->region.as<int32_t>() : nullptr;
    if (fused) {
        en.cand = h->cand.as<int32_t>(); en.c_rid = h->c_rid.as<int32_t>(); en.region_out = h->region_out.as<int32_t>();
        if (with_scratch) { en.k6_scratch = h->scratch.as<uint32_t>(); en.scratch_cap = h->cap; }
    }
    if (forward) {
        en.r_rec_dev = h->r_rec_dev.as<RegionRec>(); en.r_pk_dev = h->r_pk_dev.as<uint32_t>();
        en.r_rec_host = h->r_rec_host.as<RegionRec>(); en.r_pk_host = h->r_pk_host.as<uint32_t>();
        en.nkeys2 = nkeys2;
    }
    en.counts = h->counts.as<StageCounts>();
    if (foreign) {
        en.n_local = h->nwords.as<uint32_t>() + 1;
        en.fkey = h->fkey.as<uint64_t>(); en.fcheck = check ? h->fcheck.as<uint64_t>() : nullptr; en.fregion = h->fregion.as<int32_t>();
    }
    en.want_pair_lo = want_pair_lo;
    launch_k4_join_only(k4, en, h->nwords.as<uint32_t>(), n_host, h->counts.as<StageCounts>(), nullptr);
    CK(hipGetLastError());
    CK(hipStreamSynchronize(nullptr));
    CK(h->partner.get(partner, c4)); CK(h->pair_lo.get(pair_lo, c4)); CK(h->region_out.get(region_out, c4)); CK(h->scratch.get(scratch, c4 * 6));
    if (h->rcap) { CK(h->r_rec_host.get(fwd_rec, h->r_rec_host.bytes)); CK(h->r_pk_host.get(fwd_pk, h->r_pk_host.bytes)); }
    if (!direct) CK(h->boff.get(boff, (size_t)(nbuckets + 1) * 4));
    CK(h->counts.get(&sc, sizeof(sc)));
    memset(out_counts, 0, 8 * 4);
    out_counts[0] = sc.irregular; out_counts[1] = sc.n_entries;
    for (Buf* b : h->all) CK(b->guard(&out_counts[2]));
    if (!direct) {
        std::vector<uint32_t> bc(kMaxBuckets);
        CK(h->bcnt.get(bc.data(), bc.size() * 4));
        for (uint32_t v : bc)
            if (v) ++out_counts[3];
    }
    return 0;
}

}  // extern "C"
