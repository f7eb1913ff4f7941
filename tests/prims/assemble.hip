// Test-only harness (tests/test_gpu_assemble.py) around K6's launchers between the mate join and the final table, linked with their
// translation units unchanged: launch_k6_scratch_init, launch_k6_groups, launch_k6_walk and launch_k6_table (csrc/k6_assemble.hip) and the
// host's share of the walk, greedy_walk (csrc/bdx_walk.cpp).  Built into tests/prims/libbdx_assemble.so; nothing of it is part of
// libbdx.so.  Every entry point takes host pointers (one record of them, AsmIO), does its own copies, waits for the stream and returns HIP's
// error code.  A handle keeps one buffer set from call to call, uncleared, as a context does; every output starts a call as 0xA5 bytes, with
// a guard of 0xA5 bytes behind every array.  The launchers' preconditions are kept here: the six scratch arrays as launch_k6_scratch_init
// leaves them, the counters K6 bumps zero, the look-back words zero once and a stamp that is neither 0 nor used, capacities that fit,
// region ids below cap, first + n inside the read arrays, at most 255 libraries, consistent in_goff sums.  A call that breaks one gets
// hipErrorInvalidValue and is never launched.
//   assemble_groups   scratch init + launch_k6_groups (stage 1; with mirror_in_walk the walk's launch follows -- its first wave mirrors the counters -- and the walk's preconditions hold)
//   assemble_walk     ... + launch_k6_walk (stage 2)
//   assemble_chain    ... + the host's share through greedy_walk on the returned g_rec, decoded as decode_groups does and staged as
//                     stage_host_svs does (host_order_key, csrc/bdx_k3.h) + launch_k6_table (stage 3)
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <new>
#include <unordered_set>
#include <vector>

#include "bdx_k3.h"
#include "bdx_scan.h"
#include "bdx_walk.h"

using namespace bdx;

namespace {

#define CK(x) do { const hipError_t e_ = (x); if (e_ != hipSuccess) return (int)e_; } while (0)

constexpr unsigned char kFill = 0xA5;
constexpr size_t kGuard = 256;              // bytes of 0xA5 behind every array
constexpr uint32_t kMaxCap = 4094;          // sv_cap <= 2,048: no rank-sort launch, as in a context of that size (k6_layout)
constexpr int kMaxKeys = 32, kMaxLibs = 255;

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
        if (!b || !src) return hipSuccess;
        if (b > bytes) return hipErrorInvalidValue;
        if (pinned) { memcpy(p, src, b); return hipSuccess; }
        return hipMemcpy(p, src, b, hipMemcpyHostToDevice);
    }
    hipError_t get(void* dst, size_t b) const {
        if (!b || !dst) return hipSuccess;
        if (b > bytes) return hipErrorInvalidValue;
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

struct Handle {
    uint32_t cap = 0, g_alloc = 0, nt_alloc = 0;
    int nkeys = 0, nlibs = 0;
    K6Caps k{};
    // inputs
    Buf rec, pk, region_of, partner, pair_lo, meta, isize, in_groups, in_goff, taint, hist, kdens, lib_mean, p1, counts;
    // K6's own
    Buf parts, rs, scratch, members, member_ids, own_nsv, own_nacc, own_ncn, own_first, slot_next, owners, owners_big, emit_part;
    Buf sv_stage, lib_stage, cn_stage, sv_src, sv_begin, old_key, old_slot, hs_key_dev, ins_T, ins_src, ins_pre_l, ins_pre_c, lb;
    // pinned
    Buf g_rec, counts_host, counts_host2, sv_out, lib_index, lib_pairs, cn_key, cn_value, printed;
    Buf hs_rec, hs_key, hs_cnt, hs_lambda, hs_lib_index, hs_lib_pairs, hs_cn_key, hs_cn_value;
    std::unordered_set<uint32_t> used;   // the stamps the look-back words have seen
    WalkScratch* ws = nullptr;
    std::vector<Buf*> all;
    ~Handle() { if (ws) walk_scratch_free(ws); }
};

}  // namespace

extern "C" {

// What a call takes and returns.  Inputs -- rec: [n_regions][9]; pk: [n_regions][2 * nkeys]; per-read arrays: [n_reads] (pair_lo may be null), or
// in_groups: [n_agg][4] (key lo, key hi, pairs, sum) with in_goff: [n_regions + 1] and taint: [cap] bytes or null; hist: [nlibs][11]; key_density:
// [nkeys]; lib_mean: [nlibs].  Outputs, each as the launches left it (null: not wanted) -- rs: [cap][20]; parts: [cap][4]; scratch: [6][cap];
// members: [cap][4][28]; member_ids: [cap][64]; owners, owners_big, own_*, slot_next: [cap]; g_rec: [g_alloc][4]; counts_dev / counts_host /
// counts2: the three counter records; taint_out: [cap]; sv_stage: [cap][24]; lib_stage: [cap][lib_stride][4]; cn_stage: [cap][nkeys][2];
// old_key: [p2]; old_slot: [p2]; sv_out: [sv_cap][24] (wire_rows: the same bytes hold [sv_cap][12]); lib_index, lib_pairs: [term_cap]; cn_key,
// cn_value: [cn_cap]; info: [8] 1 where a guard byte changed, the host walk's candidates, printed candidates, the host walk's groups, 0 ...
struct AsmIO {
    uint32_t n_regions, n_host, n_reads, n_agg, g_cap, stamp, covered_ref_len;
    int32_t last_maxq, nlibs, nkeys, min_read_pair, chr_restricted, period, force_host, big_walk, asm_plain, ins_plain, propagation_rounds,
        mirror_in_walk, stage, wire_rows, score_threshold;
    const uint32_t *rec, *pk;
    const int32_t *region_of, *partner, *pair_lo;
    const uint32_t* meta;
    const int32_t* isize;
    const uint32_t *in_groups, *in_goff;
    const uint8_t* taint;
    const uint32_t* hist;
    const float *key_density, *lib_mean;
    uint32_t *rs, *parts, *scratch, *members, *member_ids, *owners, *owners_big, *g_rec, *counts_dev, *counts_host, *counts2;
    uint8_t* taint_out;
    uint32_t *sv_stage, *lib_stage, *cn_stage, *own_nsv, *own_nacc, *own_ncn, *own_first, *slot_next;
    uint64_t* old_key;
    uint32_t* old_slot;
    uint32_t *sv_out, *lib_index, *lib_pairs, *cn_key, *cn_value, *info;
};

// out: [16] what tests/assemble_cases.py's models are built on
void assemble_constants(uint32_t* out) {
    const uint32_t v[16] = {(uint32_t)kK6MaxMembers, (uint32_t)kK6MaxIn, (uint32_t)kK6BigMembers, (uint32_t)kK6LibStride, (uint32_t)kKeyShiftT, (uint32_t)kKeyShiftOwn,
                            (uint32_t)kKeyShiftStart, kKeySeqMask, (uint32_t)(sizeof(RegSum) / 4), (uint32_t)(sizeof(SvOut) / 4), (uint32_t)kWireWords,
                            (uint32_t)kMemberWords, (uint32_t)(sizeof(StageCounts) / 4), (uint32_t)kNumFlags, (uint32_t)(sizeof(RegionRec) / 4), kMaxCap};
    memcpy(out, v, sizeof(v));
}

// out: [6] sv_cap, term_cap, cn_cap, lib_stride, p2, g_alloc of a handle
void assemble_caps(void* handle, uint32_t* out) {
    const Handle* h = (const Handle*)handle;
    const uint32_t v[6] = {h->k.sv, h->k.term, h->k.cn, h->k.lib_stride, (uint32_t)h->k.p2, h->g_alloc};
    memcpy(out, v, sizeof(v));
}

// a buffer set for up to cap reads (and regions, and aggregates), nkeys counter keys and nlibs libraries
int assemble_open(uint32_t cap, int nkeys, int nlibs, void** out) {
    if (!cap || cap > kMaxCap || nkeys < 1 || nkeys > kMaxKeys || nlibs < 1 || nlibs > kMaxLibs) return (int)hipErrorInvalidValue;
    Handle* h = new (std::nothrow) Handle;
    if (!h) return (int)hipErrorOutOfMemory;
    h->cap = cap; h->nkeys = nkeys; h->nlibs = nlibs;
    h->k = k6_caps_of(cap, nkeys, nlibs);
    h->g_alloc = 2 * cap + 64;           // every read a part of its own, and room to see what an overflow leaves alone
    h->nt_alloc = cap + 16;              // a term consumes a pair
    h->ws = walk_scratch_new();
    const size_t c4 = (size_t)cap * 4, sv = h->k.sv;
    hipError_t e = hipSuccess;
    auto A = [&](Buf& b, size_t bytes, bool pin = false) { if (e == hipSuccess) e = b.alloc(bytes, pin); h->all.push_back(&b); };
    A(h->rec, (size_t)cap * sizeof(RegionRec)); A(h->pk, c4 * 2 * nkeys); A(h->region_of, c4); A(h->partner, c4); A(h->pair_lo, c4); A(h->meta, c4); A(h->isize, c4);
    A(h->in_groups, (size_t)cap * sizeof(GroupRec)); A(h->in_goff, c4 + 4); A(h->taint, cap); A(h->hist, (size_t)nlibs * kNumFlags * 4); A(h->kdens, (size_t)nkeys * 4);
    A(h->lib_mean, (size_t)nlibs * 4); A(h->p1, sizeof(Pass1)); A(h->counts, sizeof(StageCounts));
    A(h->parts, (size_t)cap * sizeof(PartRec)); A(h->rs, (size_t)cap * sizeof(RegSum)); A(h->scratch, c4 * 6); A(h->members, (size_t)cap * kK6MaxMembers * sizeof(MemberInfo));
    A(h->member_ids, c4 * kK6BigMembers); A(h->own_nsv, c4); A(h->own_nacc, c4); A(h->own_ncn, c4); A(h->own_first, c4); A(h->slot_next, c4); A(h->owners, c4);
    A(h->owners_big, c4); A(h->emit_part, 64 * 4 * 4);
    A(h->sv_stage, (size_t)cap * sizeof(SvOut)); A(h->lib_stage, (size_t)cap * h->k.lib_stride * sizeof(LibStage)); A(h->cn_stage, (size_t)cap * nkeys * sizeof(CnStage));
    A(h->sv_src, sv * 4); A(h->sv_begin, sv * 8); A(h->old_key, h->k.p2 * 8); A(h->old_slot, h->k.p2 * 4); A(h->hs_key_dev, sv * 8);
    A(h->ins_T, (sv + 1) * 4); A(h->ins_src, (sv + 1) * 4); A(h->ins_pre_l, (sv + 1) * 4); A(h->ins_pre_c, (sv + 1) * 4);
    A(h->lb, (size_t)4 * (scan_grid(cap, 1) + 1) * 8);
    A(h->g_rec, (size_t)h->g_alloc * sizeof(GroupRec), true); A(h->counts_host, sizeof(StageCounts), true); A(h->counts_host2, sizeof(StageCounts), true);
    A(h->sv_out, sv * sizeof(SvOut), true); A(h->lib_index, (size_t)h->k.term * 4, true); A(h->lib_pairs, (size_t)h->k.term * 4, true);
    A(h->cn_key, (size_t)h->k.cn * 4, true); A(h->cn_value, (size_t)h->k.cn * 4, true); A(h->printed, 1024 * 4, true);
    A(h->hs_rec, sv * sizeof(SvOut), true); A(h->hs_key, sv * 8, true); A(h->hs_cnt, sv * 4, true); A(h->hs_lambda, (size_t)h->nt_alloc * 8, true);
    A(h->hs_lib_index, (size_t)h->nt_alloc * 4, true); A(h->hs_lib_pairs, (size_t)h->nt_alloc * 4, true);
    A(h->hs_cn_key, (size_t)h->k.cn * 4, true); A(h->hs_cn_value, (size_t)h->k.cn * 4, true);
    if (e == hipSuccess) e = h->lb.zero();   // once
    if (e != hipSuccess) { delete h; return (int)e; }
    *out = h;
    return 0;
}
void assemble_close(void* handle) { delete (Handle*)handle; }

}  // extern "C"

namespace {

// the launchers' preconditions on what a call hands in
bool admits(const Handle* h, const AsmIO& io) {
    const uint32_t cap = h->cap, NR = io.n_regions;
    if (io.stage < 1 || io.stage > 3) return false;
    if (NR > io.n_host || io.n_host > cap || io.n_reads > cap || io.n_agg > cap || io.g_cap > h->g_alloc) return false;
    if (io.nlibs < 1 || io.nlibs > h->nlibs || io.nkeys < 1 || io.nkeys > h->nkeys || io.period < 1 || io.propagation_rounds < 1 || io.propagation_rounds > 64) return false;
    if (io.stamp == 0 || io.stamp > 0x3FFFFFFFu || h->used.count(io.stamp)) return false;
    if (io.mirror_in_walk && io.force_host) return false;       // (no walk launch would mirror the counters: k6_prepare never asks for it)
    if (!io.rec || !io.pk || !io.hist || !io.key_density || !io.lib_mean || !io.covered_ref_len) return false;
    const RegionRec* R = (const RegionRec*)io.rec;
    const bool agg = io.in_groups != nullptr;
    const bool walks = io.stage >= 2 || io.mirror_in_walk;   // (whatever launches the walk: it looks every library up)
    if (agg) {
        if (!io.in_goff || io.in_goff[0] != 0 || io.in_goff[NR] != io.n_agg) return false;
        for (uint32_t r = 0; r < NR; ++r) {
            if (io.in_goff[r + 1] < io.in_goff[r]) return false;
            for (uint32_t i = io.in_goff[r]; i < io.in_goff[r + 1]; ++i) {
                const GroupRec* g = (const GroupRec*)io.in_groups + i;
                const uint32_t lo = (uint32_t)(g->key >> 38), hi = (uint32_t)((g->key >> 12) & ((1u << 26) - 1)), lib = (uint32_t)((g->key >> 4) & 255);
                if (hi != r || lo > r || lo >= cap || !g->pairs) return false;
                if (walks && lib >= (uint32_t)io.nlibs) return false;
            }
        }
    } else {
        if (io.taint) return false;
        if (io.n_reads && (!io.region_of || !io.partner || !io.meta || !io.isize)) return false;
        for (uint32_t r = 0; r < NR; ++r) {
            if ((uint64_t)R[r].first + R[r].n > io.n_reads) return false;
            for (uint32_t j = R[r].first; j < R[r].first + R[r].n; ++j) {   // a pair is keyed by the region of its second-observed mate: the other region is no later one
                const int32_t p = io.partner[j];
                const int32_t plo = io.pair_lo ? io.pair_lo[j] : ((p >= 0 && (uint32_t)p < j) ? io.region_of[p] : -1);
                if (plo > (int32_t)r) return false;
            }
        }
        for (uint32_t j = 0; j < io.n_reads; ++j) {
            if (io.partner[j] < -2 || io.partner[j] >= (int32_t)io.n_reads) return false;
            if (io.region_of[j] < -1 || io.region_of[j] >= (int32_t)cap) return false;
            if (io.pair_lo && (io.pair_lo[j] < -1 || io.pair_lo[j] >= (int32_t)cap)) return false;
            if (walks && ((io.meta[j] >> 8) & 255u) >= (uint32_t)io.nlibs) return false;
            if ((io.meta[j] & 15u) >= (uint32_t)kNumFlags || io.isize[j] < 0) return false;
        }
    }
    return true;
}

int run(Handle* h, AsmIO& io) {
    if (!h || !admits(h, io)) return (int)hipErrorInvalidValue;
    h->used.insert(io.stamp);
    const uint32_t cap = h->cap, NR = io.n_regions;
    const size_t c4 = (size_t)cap * 4;
    const bool agg = io.in_groups != nullptr;
    for (Buf* b : h->all)
        if (b != &h->lb) CK(b->fill());
    CK(h->rec.put(io.rec, (size_t)NR * sizeof(RegionRec))); CK(h->pk.put(io.pk, (size_t)NR * 2 * io.nkeys * 4));
    if (agg) {
        CK(h->in_groups.put(io.in_groups, (size_t)io.n_agg * sizeof(GroupRec))); CK(h->in_goff.put(io.in_goff, (size_t)(NR + 1) * 4));
        if (io.taint) CK(h->taint.put(io.taint, cap));
    } else {
        const size_t n4 = (size_t)io.n_reads * 4;
        CK(h->region_of.put(io.region_of, n4)); CK(h->partner.put(io.partner, n4)); CK(h->meta.put(io.meta, n4)); CK(h->isize.put(io.isize, n4));
        if (io.pair_lo) CK(h->pair_lo.put(io.pair_lo, n4));
    }
    CK(h->hist.put(io.hist, (size_t)io.nlibs * kNumFlags * 4)); CK(h->kdens.put(io.key_density, (size_t)io.nkeys * 4)); CK(h->lib_mean.put(io.lib_mean, (size_t)io.nlibs * 4));
    {
        std::vector<unsigned char> raw(sizeof(Pass1), kFill);
        ((Pass1*)raw.data())->covered_ref_len = io.covered_ref_len;
        CK(h->p1.put(raw.data(), sizeof(Pass1)));
    }
    StageCounts sc;
    memset(&sc, 0, sizeof(sc));       // the counters K6 bumps: zero
    sc.n_regions = NR; sc.last_maxq = io.last_maxq;
    CK(h->counts.put(&sc, sizeof(sc)));
    CK(h->counts_host2.zero());       // (k6_prepare: the placement writes `overflow` only where it is set)
    launch_k6_scratch_init(h->scratch.as<uint32_t>(), cap, nullptr);
    CK(hipGetLastError());

    K6Arrays a;
    memset(&a, 0, sizeof(a));
    a.cap = cap;
    a.r_rec = h->rec.as<RegionRec>(); a.r_pk = h->pk.as<uint32_t>();
    if (agg) {
        a.in_groups = h->in_groups.as<GroupRec>(); a.in_goff = h->in_goff.as<uint32_t>(); a.first_of = a.in_goff;
        a.taint = io.taint ? h->taint.as<uint8_t>() : nullptr;
    } else {
        a.region_of = h->region_of.as<int32_t>(); a.partner = h->partner.as<int32_t>(); a.pair_lo = io.pair_lo ? h->pair_lo.as<int32_t>() : nullptr;
        a.meta = h->meta.as<uint32_t>(); a.isize = h->isize.as<int32_t>();
    }
    a.parts = h->parts.as<PartRec>(); a.rs = h->rs.as<RegSum>();
    a.out_deg = h->scratch.as<uint32_t>(); a.label = a.out_deg + cap; a.bad_v = a.out_deg + 2 * (size_t)cap; a.bad = a.out_deg + 3 * (size_t)cap;
    a.mcount = a.out_deg + 4 * (size_t)cap; a.pcount = a.out_deg + 5 * (size_t)cap;
    a.members = h->members.as<MemberInfo>();
    a.own_nsv = h->own_nsv.as<uint32_t>(); a.own_nacc = h->own_nacc.as<uint32_t>(); a.own_ncn = h->own_ncn.as<uint32_t>(); a.own_first = h->own_first.as<uint32_t>();
    a.slot_next = h->slot_next.as<uint32_t>(); a.owners = h->owners.as<uint32_t>(); a.owners_big = h->owners_big.as<uint32_t>(); a.emit_part = h->emit_part.as<uint32_t>();
    a.big_walk = io.big_walk ? 1 : 0;
    a.member_ids = a.big_walk ? h->member_ids.as<uint32_t>() : nullptr;
    a.sv_stage = h->sv_stage.as<SvOut>(); a.lib_stage = h->lib_stage.as<LibStage>(); a.cn_stage = h->cn_stage.as<CnStage>();
    const K6Caps k = k6_caps_of(cap, io.nkeys, io.nlibs);
    a.sv_cap = k.sv; a.term_cap = k.term; a.cn_cap = k.cn; a.lib_stride = k.lib_stride;
    a.sv_src = h->sv_src.as<uint32_t>(); a.sv_begin = h->sv_begin.as<uint2>();
    a.old_key = h->old_key.as<uint64_t>(); a.old_slot = h->old_slot.as<uint32_t>(); a.hs_key_dev = h->hs_key_dev.as<uint64_t>();
    a.ins_T = h->ins_T.as<uint32_t>(); a.ins_src = h->ins_src.as<uint32_t>(); a.ins_pre_l = h->ins_pre_l.as<uint32_t>(); a.ins_pre_c = h->ins_pre_c.as<uint32_t>();
    a.sv_out = h->sv_out.as<SvOut>(); a.lib_index = h->lib_index.as<int32_t>(); a.lib_pairs = h->lib_pairs.as<int32_t>();
    a.cn_key = h->cn_key.as<int32_t>(); a.cn_value = h->cn_value.as<float>();
    a.g_rec = h->g_rec.as<GroupRec>(); a.g_cap = io.g_cap;
    a.lb_state = h->lb.as<unsigned long long>(); a.lb_stamp = io.stamp;
    a.counts = h->counts.as<StageCounts>(); a.counts_host = h->counts_host.as<StageCounts>(); a.counts_host2 = h->counts_host2.as<StageCounts>();
    a.hist = h->hist.as<uint32_t>(); a.key_density = h->kdens.as<float>(); a.lib_mean = h->lib_mean.as<float>(); a.p1 = h->p1.as<Pass1>();
    a.nlibs = io.nlibs; a.nkeys = io.nkeys; a.min_read_pair = io.min_read_pair; a.chr_restricted = io.chr_restricted ? 1 : 0; a.period = io.period;
    a.force_host = io.force_host ? 1 : 0; a.mirror_in_walk = io.mirror_in_walk ? 1 : 0;
    a.asm_plain = io.asm_plain; a.ins_plain = io.ins_plain; a.propagation_rounds = io.propagation_rounds;

    launch_k6_groups(a, io.n_host, nullptr);
    if (io.stage >= 2 || io.mirror_in_walk) launch_k6_walk(a, io.n_host, nullptr);
    CK(hipGetLastError());
    CK(hipStreamSynchronize(nullptr));

    uint32_t n_host_svs = 0, n_printed = 0, n_walk_groups = 0;
    if (io.stage == 3) {
        const StageCounts ch = *h->counts_host.as<StageCounts>();
        WalkResult H;
        std::vector<GroupPart> parts;
        if (io.n_host && !ch.overflow && ch.n_groups <= io.g_cap) {
            const GroupRec* gr = h->g_rec.as<GroupRec>();
            parts.resize(ch.n_groups);
            for (uint32_t i = 0; i < ch.n_groups; ++i) {   // (decode_groups)
                const uint64_t key = gr[i].key;
                parts[i] = GroupPart{(uint32_t)(key >> 38), (uint32_t)((key >> 12) & ((1u << 26) - 1)), (uint8_t)(key & 15), (uint8_t)((key >> 4) & 255), gr[i].pairs,
                                     gr[i].sum_isize};
                if (parts[i].lo >= NR || parts[i].hi >= NR || parts[i].lib >= io.nlibs) return (int)hipErrorInvalidValue;   // (the walk would index past its tables)
            }
            std::vector<bdx_lib> libs((size_t)io.nlibs);
            for (int l = 0; l < io.nlibs; ++l) { memset(&libs[l], 0, sizeof(bdx_lib)); libs[l].mean_insertsize = io.lib_mean[l]; }
            WalkInput wi{};
            memset(&wi.opts, 0, sizeof(wi.opts));   // (the walk reads -r, -b, and whether -o was given)
            wi.opts.min_read_pair = io.min_read_pair; wi.opts.chr_restricted = io.chr_restricted ? 1 : 0; wi.opts.buffer_size = io.period - 1;
            wi.opts.score_threshold = io.score_threshold;
            wi.libs = libs.data(); wi.nlibs = io.nlibs; wi.nbams = 1; wi.nkeys = io.nkeys;
            wi.hist = io.hist; wi.covered_ref_len = io.covered_ref_len; wi.key_density = io.key_density;
            wi.regions = (const HostRegion*)io.rec; wi.nregions = NR; wi.r_pk = io.pk; wi.parts = &parts; wi.last_maxq = io.last_maxq;
            wi.any_anomalous = true;
            if (!parts.empty()) greedy_walk(wi, h->ws, H);
        }
        const uint32_t nh = (uint32_t)H.svs.size(), nt = (uint32_t)H.terms.size(), nc = (uint32_t)H.cn_key.size();
        if (nh > a.sv_cap || nt > h->nt_alloc || nc > a.cn_cap) return (int)hipErrorInvalidValue;
        a.nh = nh;
        if (nh) {   // (stage_host_svs)
            memcpy(h->hs_rec.p, H.svs.data(), (size_t)nh * sizeof(HostSv));
            uint64_t* hkey = h->hs_key.as<uint64_t>();
            uint32_t* hcnt = h->hs_cnt.as<uint32_t>();
            for (uint32_t j = 0; j < nh; ++j) {
                hkey[j] = a.force_host ? 0 : host_order_key(H.sv_key[j], (uint64_t)io.period);
                hcnt[j] = (uint32_t)H.svs[j].sv.lib_count | ((uint32_t)H.svs[j].sv.cn_count << 16);
            }
            for (uint32_t i = 0; i < nt; ++i) {
                h->hs_lambda.as<double>()[i] = H.terms[i].lambda; h->hs_lib_index.as<int32_t>()[i] = H.lib_index[i]; h->hs_lib_pairs.as<int32_t>()[i] = H.lib_pairs[i];
            }
            for (uint32_t i = 0; i < nc; ++i) { h->hs_cn_key.as<int32_t>()[i] = H.cn_key[i]; h->hs_cn_value.as<float>()[i] = H.cn_value[i]; }
            a.hs_rec = h->hs_rec.as<SvOut>(); a.hs_key = hkey; a.hs_cnt = hcnt;
            a.hs_lambda = h->hs_lambda.as<double>(); a.hs_lib_index = h->hs_lib_index.as<int32_t>(); a.hs_lib_pairs = h->hs_lib_pairs.as<int32_t>();
            a.hs_cn_key = h->hs_cn_key.as<int32_t>(); a.hs_cn_value = h->hs_cn_value.as<float>();
        }
        n_host_svs = nh; n_walk_groups = H.n_groups;
        a.fin_regions = (ch.n_regions && ch.n_regions <= cap) ? ch.n_regions : cap;
        a.printed_host = h->printed.as<uint32_t>();
        a.wire_rows = io.wire_rows ? 1 : 0;
        if (k6_score_grid(a) > 1024) return (int)hipErrorInvalidValue;
        launch_k6_table(a, io.n_host, log(10.0), io.score_threshold, 1, nullptr);
        CK(hipGetLastError());
        CK(hipStreamSynchronize(nullptr));
        if (io.n_host)
            for (uint32_t i = 0; i < k6_score_grid(a); ++i) n_printed += a.printed_host[i];
    }

    CK(h->rs.get(io.rs, (size_t)cap * sizeof(RegSum))); CK(h->parts.get(io.parts, (size_t)cap * sizeof(PartRec))); CK(h->scratch.get(io.scratch, c4 * 6));
    CK(h->members.get(io.members, (size_t)cap * kK6MaxMembers * sizeof(MemberInfo))); CK(h->member_ids.get(io.member_ids, c4 * kK6BigMembers));
    CK(h->owners.get(io.owners, c4)); CK(h->owners_big.get(io.owners_big, c4)); CK(h->g_rec.get(io.g_rec, (size_t)h->g_alloc * sizeof(GroupRec)));
    CK(h->counts.get(io.counts_dev, sizeof(StageCounts))); CK(h->counts_host.get(io.counts_host, sizeof(StageCounts))); CK(h->counts_host2.get(io.counts2, sizeof(StageCounts)));
    CK(h->taint.get(io.taint_out, cap));
    CK(h->sv_stage.get(io.sv_stage, (size_t)cap * sizeof(SvOut))); CK(h->lib_stage.get(io.lib_stage, (size_t)cap * a.lib_stride * sizeof(LibStage)));
    CK(h->cn_stage.get(io.cn_stage, (size_t)cap * io.nkeys * sizeof(CnStage)));
    CK(h->own_nsv.get(io.own_nsv, c4)); CK(h->own_nacc.get(io.own_nacc, c4)); CK(h->own_ncn.get(io.own_ncn, c4)); CK(h->own_first.get(io.own_first, c4));
    CK(h->slot_next.get(io.slot_next, c4)); CK(h->old_key.get(io.old_key, k.p2 * 8)); CK(h->old_slot.get(io.old_slot, k.p2 * 4));
    CK(h->sv_out.get(io.sv_out, (size_t)a.sv_cap * sizeof(SvOut))); CK(h->lib_index.get(io.lib_index, (size_t)a.term_cap * 4)); CK(h->lib_pairs.get(io.lib_pairs, (size_t)a.term_cap * 4));
    CK(h->cn_key.get(io.cn_key, (size_t)a.cn_cap * 4)); CK(h->cn_value.get(io.cn_value, (size_t)a.cn_cap * 4));
    if (io.info) {
        memset(io.info, 0, 8 * 4);
        io.info[1] = n_host_svs; io.info[2] = n_printed; io.info[3] = n_walk_groups;
        for (Buf* b : h->all) CK(b->guard(&io.info[0]));
    }
    return 0;
}

}  // namespace

extern "C" {

int assemble_groups(void* handle, AsmIO* io) { io->stage = 1; return run((Handle*)handle, *io); }
int assemble_walk(void* handle, AsmIO* io) { io->stage = 2; return run((Handle*)handle, *io); }
int assemble_chain(void* handle, AsmIO* io) { io->stage = 3; return run((Handle*)handle, *io); }

}  // extern "C"
