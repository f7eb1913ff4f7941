// Test-only harness (tests/test_gpu_compact.py) around the links between K1 and K3, linked with their translation units unchanged:
// launch_k2 (csrc/k2_compact.hip: k2_compact_kernel, k2_compact_side_kernel) and launch_finalize (csrc/k1_classify.hip: finalize_kernel,
// finalize2_kernel; finalize2_body also as K2's extra workgroup), and launch_k1 -> launch_finalize -> launch_k2 in a row on a store.
// Built into tests/prims/libbdx_compact.so; nothing of it is part of libbdx.so.  Every entry point takes host pointers (in one
// argument block per call), does its own copies, waits for the stream and returns HIP's error code.  A handle keeps one buffer set
// from call to call, as a context does; every output starts a call as 0xA5 bytes, with a guard of 0xA5 bytes behind every array, and
// the stash slots K1 would not have written are 0xA5 too (the caller hands the whole table).  The launchers' preconditions are kept
// here -- row lengths, zero padding of the totals, 0xFF monoid records of absent files, chunk counts, key and library limits, stash
// records that agree with the totals and point inside the store, segment tables that are sorted and cover the store -- and a call that
// breaks one gets hipErrorInvalidValue and is never launched.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <new>
#include <vector>

#include "bdx_dev.h"

using namespace bdx;

namespace {

#define CK(x) do { const hipError_t e_ = (x); if (e_ != hipSuccess) return (int)e_; } while (0)
#define REQUIRE(x) do { if (!(x)) return (int)hipErrorInvalidValue; } while (0)

constexpr unsigned char kFill = 0xA5;
constexpr size_t kGuard = 256;       // bytes of 0xA5 behind every array
constexpr uint32_t kSegGap = 64;     // entries of 0xA5 between two pinned segments: a read looked up in the wrong segment finds another read's entry or these
constexpr int kMaxSeg = 32;
constexpr int kMaxKeysAll = 60, kMaxLibs = 255, kMaxBams = 256;

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
    hipError_t put(const void* src, size_t b, size_t at = 0) {
        if (!b) return hipSuccess;
        if (at + b > bytes) return hipErrorInvalidValue;
        if (pinned) { memcpy((char*)p + at, src, b); return hipSuccess; }
        return hipMemcpy((char*)p + at, src, b, hipMemcpyHostToDevice);
    }
    hipError_t get(void* dst, size_t b) const {
        if (!b || !dst) return hipSuccess;
        if (b > bytes) return hipErrorInvalidValue;
        if (pinned) { memcpy(dst, p, b); return hipSuccess; }
        return hipMemcpy(dst, p, b, hipMemcpyDeviceToHost);
    }
    hipError_t guard(uint32_t* bad) const {
        if (!p) return hipSuccess;
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
    uint64_t ncap = 0;                         // reads
    uint32_t tcap = 0, tstride_cap = 0;        // tiles, row length of the per-tile tables
    uint32_t cap = 0, fill_cap = 0;            // compact records, words of a fill target
    int nkeys_cap = 0, nbams_cap = 0;
    bool with_seg = false, with_k1 = false;
    // the store
    Buf tid, pos, isize, flag, qlen, lib, key, check, mtid, mpos, mapq, bam;
    Buf seg_key, seg_qlen, seg_check, seg_tab;                             // pinned entries, the device's segment table
    // pass 1
    Buf libs, cls, tile_tot, tile_pre, tile_mono, chunk_tot, chunk_base, stash, blk_cnt, fold, cnt, p1, kdens;
    Buf cnt_host, p1_host, flag_host, count_host;                          // pinned
    // K2's output
    Buf c_tid, c_pos, c_isize, c_meta, c_key, c_check, c_idx, c_nn, c_pk, fills[4];
    std::vector<Buf*> all() {
        return {&tid, &pos, &isize, &flag, &qlen, &lib, &key, &check, &mtid, &mpos, &mapq, &bam, &seg_key, &seg_qlen, &seg_check, &seg_tab,
                &libs, &cls, &tile_tot, &tile_pre, &tile_mono, &chunk_tot, &chunk_base, &stash, &blk_cnt, &fold, &cnt, &p1, &kdens,
                &cnt_host, &p1_host, &flag_host, &count_host, &c_tid, &c_pos, &c_isize, &c_meta, &c_key, &c_check, &c_idx, &c_nn, &c_pk,
                &fills[0], &fills[1], &fills[2], &fills[3]};
    }
    std::vector<Buf*> outputs() {
        return {&c_tid, &c_pos, &c_isize, &c_meta, &c_key, &c_check, &c_idx, &c_nn, &c_pk, &fills[0], &fills[1], &fills[2], &fills[3],
                &cnt, &p1, &kdens, &cnt_host, &p1_host, &flag_host, &count_host};
    }
};

uint32_t row16(uint32_t tiles) { return (std::max<uint32_t>(tiles, 16) + 15) / 16 * 16; }

}  // namespace

extern "C" {

// The argument blocks.  Every pointer is a host pointer; an output pointer that is null is not copied back.
struct CompactFin {   // the finalisation: all of it for compact_finalize, the second level's part for compact_k2 with side = 1
    const uint32_t* tile_tot;    // [ncols][tstride]
    const void* tile_mono;       // MonoRec [nbams][tstride]
    const uint32_t* blk_cnt;     // [kCntCopies][ncnt]
    const int32_t* lib_key;      // [nlibs]
    const void* fold_in;         // MonoRec [nbams][nfold]: compact_k2 with side = 1 (the first level's result)
    uint32_t* o_tile_pre;        // [ncols][tstride]
    uint32_t* o_chunk_tot;       // [ncols][kMaxChunks]
    uint32_t* o_chunk_base;      // [ncols][kMaxChunks]
    void* o_fold;                // MonoRec [nbams][nfold]
    uint32_t* o_cnt;             // [ncnt]
    uint32_t* o_cnt_host;        // [ncnt]
    uint32_t* o_p1;              // [sizeof(Pass1) / 4]
    uint32_t* o_p1_host;         // likewise
    float* o_density;            // [64]
    uint32_t* o_flag;            // [16] the pinned flag word and the 15 behind it
    uint64_t* o_count_host;      // [kMaxChunks]
    uint32_t* o_status;          // [4] 1 where a guard byte changed, 0 ...
    uint32_t ntiles, tstride, nfold, chunk_super, nchunk, na_cap, stamp;
    int32_t nlibs, nbams, nkeys, w0, cn_lib, second_level;
};

struct CompactK2 {
    const int32_t *tid, *pos, *isize;
    const uint16_t *flag, *qlen;
    const uint8_t *lib, *cls;
    const uint64_t *key, *check;           // check null: the stream has no second name hash
    const uint32_t *tile_tot, *tile_pre, *chunk_tot, *chunk_base;   // [ncols][tstride] twice, [ncols][kMaxChunks] twice (chunk_base: side = 0 only)
    const uint32_t* stash;                 // [ntiles][kStashCap][8] or null
    const int32_t* lib_key;                // [nlibs]
    const uint64_t* seg_begin;             // [nseg + 1] or null
    int32_t *o_tid, *o_pos, *o_isize;      // [cap of the handle] each
    uint32_t* o_meta;
    uint64_t *o_key, *o_check;
    uint32_t *o_idx, *o_nn, *o_pk;         // o_pk: [nkeys cap * cap of the handle], rows of `cap` words from its start
    uint32_t* o_fill[4];                   // [fill cap of the handle] each
    uint32_t* o_status;                    // [4] 1 where a guard byte changed, 0 ...
    uint64_t n;
    uint32_t ntiles, tstride, cap, chunk_super;
    uint32_t fill_words[4], fill_value[4];
    int32_t nkeys, nlibs, nseg, side;
};

struct CompactChain {   // what launch_k1 needs beside CompactK2's store, and what pass 1 leaves
    const int32_t *mtid, *mpos;
    const uint8_t *mapq, *bam;
    const float *upper, *lower;            // [nlibs]
    const int32_t* min_mapq;               // [nlibs]
    uint8_t* o_cls;                        // [n]
    uint32_t* o_tile_tot;                  // [ncols][tstride]
    uint32_t* o_stash;                     // [ntiles][kStashCap][8]
    uint32_t *o_tile_pre, *o_chunk_tot, *o_chunk_base;
    uint32_t* o_dims;                      // [4] ntiles, tstride, chunk_super, nchunk as the harness sized them
    int32_t nbams, max_sd, opt_t, opt_l, use_stash, w0;
};

// out: [9] what tests/compact_cases.py's models are built on
void compact_constants(uint32_t* out) {
    const uint32_t v[9] = {(uint32_t)kTile, (uint32_t)kK2TilesPerWave, (uint32_t)kStashCap, (uint32_t)kStashKeys, (uint32_t)kMaxChunks, (uint32_t)kCntCopies,
                           (uint32_t)sizeof(StashRec), (uint32_t)sizeof(Pass1), (uint32_t)sizeof(MonoRec)};
    memcpy(out, v, sizeof(v));
}

// a buffer set for up to n_cap reads, cap compact records, fill targets of fill_cap words, nkeys_cap counter keys and nbams_cap source
// files; tiles_cap > 0: per-tile tables for that many tiles (a finalisation without a store).  with_seg: pinned copies of the name keys, read lengths and check words for up to kMaxSeg segments; with_k1: K1's other columns
int compact_open(uint64_t n_cap, uint32_t tiles_cap, uint32_t cap, uint32_t fill_cap, int nkeys_cap, int nbams_cap, int with_seg, int with_k1, void** out) {
    REQUIRE(n_cap <= (1ull << 26) && tiles_cap <= (1u << 21) && cap <= (1u << 22) && fill_cap <= (1u << 22) && nkeys_cap >= 1 && nkeys_cap <= kMaxKeysAll && nbams_cap >= 1 && nbams_cap <= kMaxBams);
    Handle* h = new (std::nothrow) Handle;
    if (!h) return (int)hipErrorOutOfMemory;
    h->ncap = n_cap; h->cap = cap; h->fill_cap = fill_cap; h->nkeys_cap = nkeys_cap; h->nbams_cap = nbams_cap;
    h->with_seg = with_seg != 0; h->with_k1 = with_k1 != 0;
    h->tcap = (uint32_t)((n_cap + kTile - 1) / kTile);
    h->tstride_cap = row16(std::max(h->tcap, tiles_cap));
    const size_t n = std::max<uint64_t>(n_cap, 16), c = std::max<uint32_t>(cap, 1), ts = h->tstride_cap, ncols = 2 + nkeys_cap;
    hipError_t e = hipSuccess;
    auto A = [&](Buf& b, size_t bytes, bool pin = false) { if (e == hipSuccess) e = b.alloc(bytes, pin); };
    A(h->tid, n * 4); A(h->pos, n * 4); A(h->isize, n * 4); A(h->flag, n * 2); A(h->qlen, n * 2); A(h->lib, n); A(h->key, n * 8); A(h->check, n * 8);
    if (with_k1) { A(h->mtid, n * 4); A(h->mpos, n * 4); A(h->mapq, n); A(h->bam, n); }
    if (with_seg) {
        const size_t m = n + (size_t)kMaxSeg * kSegGap;
        A(h->seg_key, m * 8, true); A(h->seg_qlen, m * 2, true); A(h->seg_check, m * 8, true); A(h->seg_tab, (size_t)(4 * kMaxSeg + 1) * 8);
    }
    A(h->libs, (size_t)kMaxLibs * sizeof(DevLib)); A(h->cls, n); A(h->tile_tot, ncols * ts * 4); A(h->tile_pre, ncols * ts * 4);
    A(h->tile_mono, (size_t)nbams_cap * ts * sizeof(MonoRec)); A(h->chunk_tot, ncols * kMaxChunks * 4); A(h->chunk_base, ncols * kMaxChunks * 4);
    A(h->stash, std::max<size_t>((size_t)h->tcap * kStashCap * sizeof(StashRec), 64));
    A(h->blk_cnt, (size_t)kCntCopies * (kMaxLibs * 12 + kMaxBams) * 4); A(h->fold, (size_t)nbams_cap * 64 * sizeof(MonoRec));
    A(h->cnt, (size_t)(kMaxLibs * 12 + kMaxBams) * 4); A(h->p1, sizeof(Pass1)); A(h->kdens, 64 * 4);
    A(h->cnt_host, (size_t)(kMaxLibs * 12 + kMaxBams) * 4, true); A(h->p1_host, sizeof(Pass1), true); A(h->flag_host, 64, true); A(h->count_host, (size_t)kMaxChunks * 8, true);
    A(h->c_tid, c * 4); A(h->c_pos, c * 4); A(h->c_isize, c * 4); A(h->c_meta, c * 4); A(h->c_key, c * 8); A(h->c_check, c * 8); A(h->c_idx, c * 4); A(h->c_nn, c * 4);
    A(h->c_pk, c * 4 * nkeys_cap);
    for (Buf& f : h->fills) A(f, (size_t)std::max<uint32_t>(fill_cap, 4) * 4);
    if (e != hipSuccess) { delete h; return (int)e; }
    *out = h;
    return 0;
}
void compact_close(void* handle) { delete (Handle*)handle; }

}  // extern "C"

namespace {

int put_libs(Handle* h, int nlibs, int nkeys, int nbams, int cn_lib, const int32_t* lib_key, const float* upper, const float* lower, const int32_t* min_mapq) {
    REQUIRE(nlibs >= 1 && nlibs <= kMaxLibs && lib_key);
    std::vector<DevLib> v(nlibs);
    for (int i = 0; i < nlibs; ++i) {
        REQUIRE(lib_key[i] >= 0 && lib_key[i] < nkeys && (cn_lib || nbams < 0 || lib_key[i] < nbams));   // (bam_cnt[key] without -a)
        v[i].upper = upper ? upper[i] : 0.f; v[i].lower = lower ? lower[i] : 0.f; v[i].min_mapq = min_mapq ? min_mapq[i] : 0; v[i].key = lib_key[i];
    }
    CK(h->libs.fill());
    CK(h->libs.put(v.data(), (size_t)nlibs * sizeof(DevLib)));
    return 0;
}

// the finalisation's arguments over the handle's buffers; what both kernels write starts as 0xA5
int make_fin(Handle* h, const CompactFin& f, bool first_level, FinalizeParams* out) {
    REQUIRE(f.nlibs >= 1 && f.nlibs <= kMaxLibs && f.nbams >= 1 && f.nbams <= h->nbams_cap && f.nkeys >= 1 && f.nkeys <= h->nkeys_cap);
    REQUIRE(f.tstride % 16 == 0 && f.tstride >= 16 && f.tstride >= f.ntiles && f.tstride <= h->tstride_cap);
    REQUIRE(f.nfold >= 1 && f.nfold <= 64 && f.nchunk >= 1 && f.nchunk <= (uint32_t)kMaxChunks && f.chunk_super >= 1 && f.chunk_super < (1u << 20));
    const uint32_t nsuper = (f.ntiles + kK2TilesPerWave - 1) / kK2TilesPerWave;
    REQUIRE((uint64_t)f.nchunk * f.chunk_super >= nsuper);
    if (first_level) REQUIRE(f.chunk_super % 4096 == 0);   // (a chunk is a whole number of the scan's rounds)
    const int ncols = 2 + f.nkeys, ncnt = f.nlibs * kNumFlags + f.nlibs + f.nbams;
    REQUIRE(f.blk_cnt && f.lib_key);
    if (int rc = put_libs(h, f.nlibs, f.nkeys, f.nbams, f.cn_lib, f.lib_key, nullptr, nullptr, nullptr)) return rc;
    CK(h->blk_cnt.fill());
    CK(h->blk_cnt.put(f.blk_cnt, (size_t)kCntCopies * ncnt * 4));
    FinalizeParams fp;
    memset(&fp, 0, sizeof(fp));
    fp.ntiles = f.ntiles; fp.tstride = f.tstride; fp.nblk = 0; fp.nfold = f.nfold; fp.fold_part = h->fold.as<MonoRec>();
    fp.nlibs = f.nlibs; fp.nbams = f.nbams; fp.nkeys = f.nkeys; fp.ncols = ncols; fp.ncnt = ncnt; fp.w0 = f.w0;
    fp.tile_tot = h->tile_tot.as<uint32_t>(); fp.tile_pre = h->tile_pre.as<uint32_t>();
    fp.chunk_tot = h->chunk_tot.as<uint32_t>(); fp.chunk_base = h->chunk_base.as<uint32_t>();
    fp.chunk_super = f.chunk_super; fp.nchunk = f.nchunk;
    fp.tile_mono = h->tile_mono.as<MonoRec>(); fp.blk_cnt = h->blk_cnt.as<uint32_t>(); fp.cnt = h->cnt.as<uint32_t>(); fp.p1 = h->p1.as<Pass1>();
    fp.cnt_host = h->cnt_host.as<uint32_t>(); fp.p1_host = h->p1_host.as<Pass1>();
    fp.libs = h->libs.as<DevLib>(); fp.cn_lib = f.cn_lib; fp.key_density = h->kdens.as<float>();
    fp.flag_host = h->flag_host.as<uint32_t>(); fp.flag_value = f.stamp;
    fp.count_host = h->count_host.as<uint64_t>(); fp.count_stamp = f.stamp;
    fp.na_cap = f.na_cap;
    *out = fp;
    return 0;
}

int get_fin(Handle* h, const CompactFin& f) {
    const size_t ncols = 2 + f.nkeys, ncnt = (size_t)f.nlibs * kNumFlags + f.nlibs + f.nbams;
    CK(h->tile_pre.get(f.o_tile_pre, ncols * f.tstride * 4)); CK(h->chunk_tot.get(f.o_chunk_tot, ncols * kMaxChunks * 4));
    CK(h->chunk_base.get(f.o_chunk_base, ncols * kMaxChunks * 4)); CK(h->fold.get(f.o_fold, (size_t)f.nbams * f.nfold * sizeof(MonoRec)));
    CK(h->cnt.get(f.o_cnt, ncnt * 4)); CK(h->cnt_host.get(f.o_cnt_host, ncnt * 4)); CK(h->p1.get(f.o_p1, sizeof(Pass1))); CK(h->p1_host.get(f.o_p1_host, sizeof(Pass1)));
    CK(h->kdens.get(f.o_density, 64 * 4)); CK(h->flag_host.get(f.o_flag, 64)); CK(h->count_host.get(f.o_count_host, (size_t)kMaxChunks * 8));
    return 0;
}

int check_guards(Handle* h, uint32_t* status) {
    if (!status) return 0;
    memset(status, 0, 16);
    for (Buf* b : h->all()) CK(b->guard(&status[0]));
    return 0;
}

// tile_tot [ncols][tstride] from the host: zero behind ntiles
int put_tile_tot(Handle* h, const uint32_t* tt, int ncols, uint32_t ntiles, uint32_t tstride) {
    REQUIRE(tt);
    for (int c = 0; c < ncols; ++c)
        for (uint32_t t = ntiles; t < tstride; ++t) REQUIRE(tt[(size_t)c * tstride + t] == 0);
    CK(h->tile_tot.fill());
    CK(h->tile_tot.put(tt, (size_t)ncols * tstride * 4));
    return 0;
}

int fill_outputs(Handle* h) {
    for (Buf* b : h->outputs()) CK(b->fill());
    return 0;
}

// K2's arguments over the handle's buffers, the store and the tables copied in
int make_k2(Handle* h, const CompactK2& k, bool tables_from_host, K2Params* out) {
    REQUIRE(k.n >= 1 && k.n <= h->ncap && k.ntiles == (uint32_t)((k.n + kTile - 1) / kTile));
    REQUIRE(k.tstride % 16 == 0 && k.tstride >= 16 && k.tstride >= k.ntiles && k.tstride <= h->tstride_cap);
    REQUIRE(k.nkeys >= 1 && k.nkeys <= h->nkeys_cap && k.nlibs >= 1 && k.nlibs <= kMaxLibs && k.cap <= h->cap);
    REQUIRE(k.tid && k.pos && k.isize && k.flag && k.qlen && k.lib && k.key);
    REQUIRE(k.nseg >= 0 && k.nseg <= kMaxSeg && (!k.nseg || (h->with_seg && k.seg_begin)));
    for (int f = 0; f < 4; ++f) REQUIRE(k.fill_words[f] <= h->fill_cap);   // (allocation bases: 16-byte aligned)
    const size_t n = k.n;
    CK(h->tid.put(k.tid, n * 4)); CK(h->pos.put(k.pos, n * 4)); CK(h->isize.put(k.isize, n * 4)); CK(h->flag.put(k.flag, n * 2)); CK(h->lib.put(k.lib, n));
    K2Params p;
    memset(&p, 0, sizeof(p));
    if (k.nseg) {   // name keys, lengths and check words only in pinned memory; the device columns keep their 0xA5
        for (int s = 0; s < k.nseg; ++s) REQUIRE(k.seg_begin[s] < k.seg_begin[s + 1]);
        REQUIRE(k.seg_begin[0] == 0 && k.seg_begin[k.nseg] == n);
        CK(h->key.fill()); CK(h->qlen.fill()); CK(h->check.fill());
        CK(h->seg_key.fill()); CK(h->seg_qlen.fill()); CK(h->seg_check.fill());
        std::vector<uint64_t> tab(4 * k.nseg + 1);
        for (int s = 0; s < k.nseg; ++s) {
            const size_t b = k.seg_begin[s], m = k.seg_begin[s + 1] - b, at = b + (size_t)s * kSegGap;
            CK(h->seg_key.put(k.key + b, m * 8, at * 8)); CK(h->seg_qlen.put(k.qlen + b, m * 2, at * 2));
            if (k.check) CK(h->seg_check.put(k.check + b, m * 8, at * 8));
            tab[s] = b;
            tab[k.nseg + 1 + s] = (uint64_t)(uintptr_t)(h->seg_key.as<uint64_t>() + (size_t)s * kSegGap);       // biased by -seg_begin[s]
            tab[2 * k.nseg + 1 + s] = (uint64_t)(uintptr_t)(h->seg_qlen.as<uint16_t>() + (size_t)s * kSegGap);
            tab[3 * k.nseg + 1 + s] = (uint64_t)(uintptr_t)(h->seg_check.as<uint64_t>() + (size_t)s * kSegGap);
        }
        tab[k.nseg] = n;
        CK(h->seg_tab.fill());
        CK(h->seg_tab.put(tab.data(), tab.size() * 8));
        p.nseg = k.nseg;
        p.seg_begin = h->seg_tab.as<uint64_t>();
        p.seg_ptr = (const uint64_t* const*)(h->seg_tab.as<uint64_t>() + k.nseg + 1);
        p.seg_qlen = (const uint16_t* const*)(h->seg_tab.as<uint64_t>() + 2 * k.nseg + 1);
        p.seg_check = (const uint64_t* const*)(h->seg_tab.as<uint64_t>() + 3 * k.nseg + 1);
    } else {
        CK(h->key.put(k.key, n * 8)); CK(h->qlen.put(k.qlen, n * 2));
        if (k.check) CK(h->check.put(k.check, n * 8)); else CK(h->check.fill());
    }
    const int ncols = 2 + k.nkeys;
    if (tables_from_host) {
        REQUIRE(k.cls && k.tile_tot && k.tile_pre && k.chunk_tot && (k.side || k.chunk_base) && k.lib_key);
        REQUIRE(k.chunk_super >= 1 && ((uint64_t)(k.ntiles + kK2TilesPerWave - 1) / kK2TilesPerWave + k.chunk_super - 1) / k.chunk_super <= (uint64_t)kMaxChunks);
        REQUIRE(!k.stash || k.nkeys <= kStashKeys);
        if (int rc = put_libs(h, k.nlibs, k.nkeys, -1, 1, k.lib_key, nullptr, nullptr, nullptr)) return rc;
        if (int rc = put_tile_tot(h, k.tile_tot, ncols, k.ntiles, k.tstride)) return rc;
        CK(h->cls.fill()); CK(h->cls.put(k.cls, n));
        CK(h->tile_pre.fill()); CK(h->tile_pre.put(k.tile_pre, (size_t)ncols * k.tstride * 4));
        CK(h->chunk_tot.fill()); CK(h->chunk_tot.put(k.chunk_tot, (size_t)ncols * kMaxChunks * 4));
        CK(h->chunk_base.fill());
        if (!k.side) CK(h->chunk_base.put(k.chunk_base, (size_t)ncols * kMaxChunks * 4));
        if (k.stash) {   // the slots K2 reads are K1's records or its mark, every other slot is untouched, and a record's read is in its tile and in the store
            const uint32_t(*st)[kStashCap][8] = (const uint32_t(*)[kStashCap][8])k.stash;
            for (uint32_t t = 0; t < k.ntiles; ++t) {
                const uint32_t a = std::min<uint32_t>(k.tile_tot[(size_t)kColAnom * k.tstride + t], kStashCap);
                for (uint32_t s = 0; s < (uint32_t)kStashCap; ++s) {
                    const uint32_t* r = st[t][s];
                    if (s >= a) { for (int w = 0; w < 8; ++w) REQUIRE(r[w] == 0xA5A5A5A5u); continue; }
                    if (r[4] == 0xFFFFFFFFu) continue;
                    REQUIRE(r[6] == 0 && r[7] == 0 && (uint64_t)t * kTile + (r[4] & 255u) < n && ((r[4] >> 20) & 63u) < (uint32_t)k.nkeys);
                }
            }
            CK(h->stash.put(k.stash, (size_t)k.ntiles * kStashCap * sizeof(StashRec)));
        }
    }
    p.r.tid = h->tid.as<int32_t>(); p.r.pos = h->pos.as<int32_t>(); p.r.isize = h->isize.as<int32_t>(); p.r.flag = h->flag.as<uint16_t>();
    p.r.qlen = h->qlen.as<uint16_t>(); p.r.lib = h->lib.as<uint8_t>(); p.r.key = h->key.as<uint64_t>(); p.r.check = h->check.as<uint64_t>();
    p.r.mtid = h->mtid.as<int32_t>(); p.r.mpos = h->mpos.as<int32_t>(); p.r.mapq = h->mapq.as<uint8_t>(); p.r.bam = h->bam.as<uint8_t>();
    p.n = n; p.ntiles = k.ntiles; p.tstride = k.tstride; p.nkeys = k.nkeys; p.nlibs = k.nlibs; p.libs = h->libs.as<DevLib>();
    p.cls = h->cls.as<uint8_t>(); p.tile_pre = h->tile_pre.as<uint32_t>(); p.chunk_tot = h->chunk_tot.as<uint32_t>(); p.chunk_base = h->chunk_base.as<uint32_t>();
    p.chunk_super = k.chunk_super; p.tile_tot = h->tile_tot.as<uint32_t>(); p.stash = k.stash ? h->stash.as<StashRec>() : nullptr;
    p.c.tid = h->c_tid.as<int32_t>(); p.c.pos = h->c_pos.as<int32_t>(); p.c.isize = h->c_isize.as<int32_t>(); p.c.meta = h->c_meta.as<uint32_t>();
    p.c.key = h->c_key.as<uint64_t>(); p.c.check = k.check ? h->c_check.as<uint64_t>() : nullptr; p.c.idx = h->c_idx.as<uint32_t>(); p.c.nn = h->c_nn.as<uint32_t>();
    p.c.pk = h->c_pk.as<uint32_t>(); p.c.cap = k.cap;
    for (int f = 0; f < 4; ++f) { p.fill_ptr[f] = h->fills[f].as<uint32_t>(); p.fill_words[f] = k.fill_words[f]; p.fill_value[f] = k.fill_value[f]; }
    *out = p;
    return 0;
}

int get_k2(Handle* h, const CompactK2& k) {
    const size_t c = std::max<uint32_t>(h->cap, 1);
    CK(h->c_tid.get(k.o_tid, c * 4)); CK(h->c_pos.get(k.o_pos, c * 4)); CK(h->c_isize.get(k.o_isize, c * 4)); CK(h->c_meta.get(k.o_meta, c * 4));
    CK(h->c_key.get(k.o_key, c * 8)); CK(h->c_check.get(k.o_check, c * 8)); CK(h->c_idx.get(k.o_idx, c * 4)); CK(h->c_nn.get(k.o_nn, c * 4));
    CK(h->c_pk.get(k.o_pk, c * 4 * h->nkeys_cap));
    for (int f = 0; f < 4; ++f) CK(h->fills[f].get(k.o_fill[f], (size_t)std::max<uint32_t>(h->fill_cap, 4) * 4));
    return 0;
}

}  // namespace

extern "C" {

// launch_finalize(fp, stream, second_level) on the tables handed in
int compact_finalize(void* handle, const CompactFin* f) {
    Handle* h = (Handle*)handle;
    REQUIRE(h && f && f->tile_tot && f->tile_mono);
    FinalizeParams fp;
    if (int rc = make_fin(h, *f, true, &fp)) return rc;
    const int ncols = 2 + f->nkeys;
    if (int rc = put_tile_tot(h, f->tile_tot, ncols, f->ntiles, f->tstride)) return rc;
    {   // a record of an absent file is 0xFF throughout, as pass 1 starts the table
        const MonoRec* m = (const MonoRec*)f->tile_mono;
        static const unsigned char ff[sizeof(MonoRec)] = {0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF};
        for (size_t i = 0; i < (size_t)f->nbams * f->tstride; ++i)
            if (m[i].ft == -1 || i % f->tstride >= f->ntiles) REQUIRE(!memcmp(&m[i], ff, sizeof(MonoRec)));
        CK(h->tile_mono.fill());
        CK(h->tile_mono.put(f->tile_mono, (size_t)f->nbams * f->tstride * sizeof(MonoRec)));
    }
    CK(h->tile_pre.fill()); CK(h->chunk_tot.fill()); CK(h->chunk_base.fill()); CK(h->fold.fill());
    if (int rc = fill_outputs(h)) return rc;
    launch_finalize(fp, nullptr, f->second_level != 0);
    CK(hipGetLastError());
    CK(hipStreamSynchronize(nullptr));
    if (int rc = get_fin(h, *f)) return rc;
    return check_guards(h, f->o_status);
}

// launch_k2 on the inputs handed in: side = 0 k2_compact_kernel, side = 1 k2_compact_side_kernel with the second level of fin beside it
int compact_k2(void* handle, const CompactK2* k, const CompactFin* fin) {
    Handle* h = (Handle*)handle;
    REQUIRE(h && k && (!k->side || fin));
    K2Params p;
    if (int rc = make_k2(h, *k, true, &p)) return rc;
    FinalizeParams fp;
    if (k->side) {
        REQUIRE(fin->nkeys == k->nkeys && fin->nlibs == k->nlibs && fin->ntiles == k->ntiles && fin->tstride == k->tstride && fin->chunk_super == k->chunk_super && fin->fold_in);
        if (int rc = make_fin(h, *fin, false, &fp)) return rc;   // (the libraries again: with the second level's limits on their keys)
        CK(h->fold.fill());
        CK(h->fold.put(fin->fold_in, (size_t)fin->nbams * fin->nfold * sizeof(MonoRec)));
    }
    if (int rc = fill_outputs(h)) return rc;
    launch_k2(p, k2_lds_bytes(k->nkeys), nullptr, k->side ? &fp : nullptr);
    CK(hipGetLastError());
    CK(hipStreamSynchronize(nullptr));
    if (int rc = get_k2(h, *k)) return rc;
    if (k->side)
        if (int rc = get_fin(h, *fin)) return rc;
    return check_guards(h, k->o_status);
}

// launch_k1 -> launch_finalize -> launch_k2 on a store, the tables sized as bdx_api.hip sizes them
int compact_chain(void* handle, const CompactK2* k, const CompactChain* c, const CompactFin* fin) {
    Handle* h = (Handle*)handle;
    REQUIRE(h && k && c && fin && h->with_k1 && !k->nseg && !k->side);
    REQUIRE(c->mtid && c->mpos && c->mapq && c->bam && c->upper && c->lower && c->min_mapq && k->lib_key);
    REQUIRE(c->nbams >= 1 && c->nbams <= h->nbams_cap && k->n >= 1 && k->n <= h->ncap);
    REQUIRE(!c->use_stash || k->nkeys <= kStashKeys);
    CompactK2 kk = *k;
    kk.ntiles = (uint32_t)((k->n + kTile - 1) / kTile);
    kk.tstride = row16(kk.ntiles);
    const uint32_t nsuper = (kk.ntiles + kK2TilesPerWave - 1) / kK2TilesPerWave, round = 4096, rounds = std::max<uint32_t>(1, (nsuper + round - 1) / round);
    kk.chunk_super = round * ((rounds + kMaxChunks - 1) / kMaxChunks);
    uint32_t dummy_stash = 0;
    kk.stash = c->use_stash ? &dummy_stash : nullptr;   // (only whether there is one)
    K2Params p;
    if (int rc = make_k2(h, kk, false, &p)) return rc;
    const size_t n = k->n;
    const int ncols = 2 + k->nkeys, ncnt = k->nlibs * kNumFlags + k->nlibs + c->nbams;
    CK(h->mtid.put(c->mtid, n * 4)); CK(h->mpos.put(c->mpos, n * 4)); CK(h->mapq.put(c->mapq, n)); CK(h->bam.put(c->bam, n));
    CompactFin f = *fin;
    f.ntiles = kk.ntiles; f.tstride = kk.tstride; f.chunk_super = kk.chunk_super; f.nchunk = std::max<uint32_t>(1, (nsuper + kk.chunk_super - 1) / kk.chunk_super);
    f.nfold = std::max<uint32_t>(1, std::min<uint32_t>(64, (kk.ntiles + 1023) / 1024));
    f.nlibs = k->nlibs; f.nkeys = k->nkeys; f.nbams = c->nbams; f.w0 = c->w0; f.lib_key = k->lib_key; f.second_level = 1;
    std::vector<uint32_t> zeros((size_t)kCntCopies * ncnt, 0u);
    f.blk_cnt = zeros.data();
    FinalizeParams fp;
    if (int rc = make_fin(h, f, true, &fp)) return rc;
    if (int rc = put_libs(h, k->nlibs, k->nkeys, f.cn_lib ? -1 : c->nbams, f.cn_lib, k->lib_key, c->upper, c->lower, c->min_mapq)) return rc;
    // as pass1_prepare leaves them: totals and counters zero, the monoid table 0xFF; what K1 does not write stays 0xA5
    CK(h->cls.fill()); CK(h->stash.fill()); CK(h->tile_pre.fill()); CK(h->chunk_tot.fill()); CK(h->chunk_base.fill()); CK(h->fold.fill());
    CK(h->tile_tot.fill()); CK(h->tile_tot.set(0, (size_t)ncols * kk.tstride * 4));
    CK(h->tile_mono.fill()); CK(h->tile_mono.set(0xFF, (size_t)c->nbams * kk.tstride * sizeof(MonoRec)));
    if (int rc = fill_outputs(h)) return rc;
    K1Params k1;
    memset(&k1, 0, sizeof(k1));
    k1.r = p.r; k1.n = n; k1.ntiles = kk.ntiles; k1.tstride = kk.tstride; k1.tile0 = 0;
    k1.nlibs = k->nlibs; k1.nbams = c->nbams; k1.nkeys = k->nkeys; k1.max_sd = c->max_sd; k1.opt_t = c->opt_t; k1.opt_l = c->opt_l;
    k1.libs = h->libs.as<DevLib>(); k1.cls = h->cls.as<uint8_t>(); k1.tile_tot = h->tile_tot.as<uint32_t>(); k1.tile_mono = h->tile_mono.as<MonoRec>();
    k1.blk_cnt = h->blk_cnt.as<uint32_t>(); k1.stash = c->use_stash ? h->stash.as<StashRec>() : nullptr;
    const int grid1 = (int)std::min<uint32_t>((kk.ntiles + kWaves - 1) / kWaves, 8192u);
    launch_k1(k1, grid1, k1_lds_bytes(k->nlibs, c->nbams, k->nkeys), nullptr);
    launch_finalize(fp, nullptr, true);
    launch_k2(p, k2_lds_bytes(k->nkeys), nullptr, nullptr);
    CK(hipGetLastError());
    CK(hipStreamSynchronize(nullptr));
    if (int rc = get_k2(h, kk)) return rc;
    if (int rc = get_fin(h, f)) return rc;
    CK(h->cls.get(c->o_cls, n)); CK(h->tile_tot.get(c->o_tile_tot, (size_t)ncols * kk.tstride * 4));
    CK(h->stash.get(c->o_stash, (size_t)kk.ntiles * kStashCap * sizeof(StashRec)));
    CK(h->tile_pre.get(c->o_tile_pre, (size_t)ncols * kk.tstride * 4)); CK(h->chunk_tot.get(c->o_chunk_tot, (size_t)ncols * kMaxChunks * 4));
    CK(h->chunk_base.get(c->o_chunk_base, (size_t)ncols * kMaxChunks * 4));
    if (c->o_dims) { c->o_dims[0] = kk.ntiles; c->o_dims[1] = kk.tstride; c->o_dims[2] = kk.chunk_super; c->o_dims[3] = f.nchunk; }
    return check_guards(h, k->o_status);
}

}  // extern "C"
