// What the kernels that answer queries over the resident store (K8, KS, KI: kq_queries.hip) are made of besides their own test per record:
// the walk over a window of the (tid, pos)-sorted store, the per-wave counters per key, and the rule that says which records count for an
// SV site.  The walk and the counters are pinned on their own, against numpy, by tests/test_gpu_prims.py (harness: tests/prims/prims.hip).
#pragma once
#include "../../include/bdx.h"
#include "bdx_wave_search.h"

namespace bdx {

// ---- the window walk ------------------------------------------------------------------------------------------------------------
// One wavefront visits the records of chromosome t with pos in [wlo, whi]: their first is found by the 64-ary ballot search, then the
// lanes stride the store 64 records at a time and body(i, s, in) is called once per lane per step -- i the lane's record index, s its
// pos (0 where i >= n), in whether the record lies inside the window.  The contract:
//   * all 64 lanes call it, and the body is called on all 64 lanes of every step, those with in == false too (the bodies hold ballots);
//   * the records seen with in == true are exactly [L, R), each once: L = wave_lower_bound(t, wlo), R the first index >= L with
//     tid != t, pos > whi or == n (sorted: the first record behind the window ends it);
//   * the lanes of a step hold consecutive records from lane 0 on, and the first step starts at L;
//   * the walk returns after the first step with a lane outside: (R - L) / 64 + 1 steps -- a window whose records fill whole steps gets
//     one more, all of it outside and possibly all of it behind n; n == 0 is legal: one step with nothing inside;
//   * nothing is loaded at an index >= n.
template <class Body>
__device__ __forceinline__ void wave_window_walk(const int32_t* __restrict__ tid, const int32_t* __restrict__ pos, uint64_t n, int32_t t, int64_t wlo,
                                                 int64_t whi, Body&& body) {
    const int lane = lane_id();
    for (uint64_t base = wave_lower_bound(tid, pos, n, t, wlo);; base += 64) {
        const uint64_t i = base + (uint64_t)lane;
        bool in = i < n;
        int64_t s = 0;
        if (in) {
            s = pos[i];
            in = tid[i] == t && s <= whi;
        }
        const uint64_t m_in = ballot64(in);
        body(i, s, in);
        if (m_in != ~0ull) break;
    }
}

// ---- the index walk (KR: kr_depth.hip) ----------------------------------------------------------------------------------------------
// One wavefront visits the records [L, R) of the store, the range given by index: the lanes stride it 64 records at a time and
// body(i, in) is called once per lane per step -- i the lane's record index, in whether i < R.  The contract:
//   * all 64 lanes call it, and the body is called on all 64 lanes of every step, those with in == false too (the bodies hold ballots);
//   * the indices seen with in == true are exactly [L, R), each once, consecutive from lane 0 on, the first step starting at L;
//   * (R - L + 63) / 64 steps: none when L >= R;
//   * the walk itself loads nothing: what the body loads at an index with in == true lies below R.
template <class Body>
__device__ __forceinline__ void wave_index_walk(uint64_t L, uint64_t R, Body&& body) {
    const int lane = lane_id();
    for (uint64_t base = L; base < R; base += 64) {
        const uint64_t i = base + (uint64_t)lane;
        body(i, i < R);
    }
}

// ---- per-wave counters per key (K8, KS, KR) -------------------------------------------------------------------------------------------
// One key: a ballot + popcount per step into a register.  Several (at most 255): the wave's row of [waves][nkeys] words of dynamic LDS
// and one LDS atomic per hit.  open() and close() hold a workgroup barrier each when nkeys > 1, so every wave of the block calls both,
// the waves without a query too (`live` false); add() is called on all 64 lanes (it holds the ballot).
struct WaveKeyCounts {
    uint32_t* row;
    int nkeys;
    uint32_t single;

    __device__ __forceinline__ void open(uint32_t* lds, int nk) {
        nkeys = nk;
        single = 0;
        row = lds + wave_id() * nk;
        if (nk > 1) {
            for (int k = lane_id(); k < nk; k += 64) row[k] = 0;
            __syncthreads();
        }
    }
    // key: the store's library or source-file column, read only for a hit with nkeys > 1
    __device__ __forceinline__ void add(bool hit, const uint8_t* __restrict__ key, uint64_t i) {
        if (nkeys > 1) {
            if (hit) {
                const uint32_t k = key[i];
                atomicAdd(&row[k < (uint32_t)nkeys ? k : 0u], 1u);   // (an index out of range counts as 0, like everywhere in the store)
            }
        } else {
            single += (uint32_t)popc64(ballot64(hit));
        }
    }
    // counts: [queries][nkeys]; row q is written by the wave of a live query alone
    __device__ __forceinline__ void close(bool live, uint32_t* __restrict__ counts, uint32_t q) {
        if (nkeys > 1) {
            __syncthreads();
            if (live)
                for (int k = lane_id(); k < nkeys; k += 64) counts[(uint64_t)q * nkeys + k] = row[k];
        } else if (live && lane_id() == 0) {
            counts[q] = single;
        }
    }
};

// ---- the site rule (KS, KI; in words: include/bdx.h, bdx_count_site_pairs) ----------------------------------------------------------
// A record is near P on T when its tid == T and |pos + 1 - P| <= window; its mate when mtid == T and |mpos + 1 - P| <= window.
__device__ __forceinline__ bool site_near(int32_t t, int64_t s, int32_t T, int64_t P, int64_t w) {
    const int64_t d = s + 1 - P;
    return t == T && d <= w && -d <= w;
}

enum SiteRoute : int { kSiteNone = 0, kSiteForward = 1, kSiteReverse = 2 };
struct SiteMatch {
    SiteRoute route;   // forward: near pos1 with the mate near pos2 (a record that matches both ways is forward); reverse: the other way only
    int64_t ms;        // of a record that counts: its mpos ...
    uint32_t fl;       // ... and its SAM flag
};

// A site and its read-start windows [p1 - 1 - win, p1 - 1 + win] and [p2 - 1 - win, p2 - 1 + win] on t1 / t2.  A lower mate near pos2
// whose mate is near pos1 exists only when the two overlap (same chromosome, pos2 - pos1 <= 2 window): then [wlo, whi] is their union and
// both routes are tested; otherwise it is window 1 alone, forward only.  All arithmetic on positions is 64-bit: window may be 2^30 and
// positions 2^31 - 1.
struct SiteRule {
    int32_t t1, t2;
    int64_t p1, p2, win;
    uint32_t mask;
    bool overlap;
    int64_t wlo, whi;

    __device__ __forceinline__ SiteRule(const KsSite& st, int32_t window)
        : t1(st.tid1), t2(st.tid2), p1(st.pos1), p2(st.pos2), win(window), mask(st.flag_mask) {
        overlap = t1 == t2 && p2 - p1 <= 2 * win;
        wlo = p1 - 1 - win;
        whi = (overlap ? p2 : p1) - 1 + win;
    }

    // Record i of the walk over (t1, [wlo, whi]), s its pos: it counts when K1 let it pass and its ReadFlag is in the mask (the class byte
    // alone says so; the mate columns and the SAM flag are loaded for such records only), it is its pair's lower mate ((tid, pos) <
    // (mtid, mpos), or equal and first in pair: each pair once) and one of the routes holds.
    __device__ __forceinline__ SiteMatch match(const StoreView& v, uint64_t i, int64_t s) const {
        SiteMatch m{kSiteNone, 0, 0};
        const uint32_t c = v.cls[i];
        if ((c & BDX_CLS_PASS) && ((mask >> BDX_CLS_FLAG(c)) & 1u)) {
            const int32_t mt = v.mtid[i];
            m.ms = v.mpos[i];
            m.fl = v.flag[i];
            // (the record's tid is t1 here)
            const bool lower = t1 < mt || (t1 == mt && (s < m.ms || (s == m.ms && (m.fl & 0x40))));
            const bool fwd = site_near(t1, s, t1, p1, win) && site_near(mt, m.ms, t2, p2, win);
            const bool rev = overlap && site_near(t1, s, t2, p2, win) && site_near(mt, m.ms, t1, p1, win);
            if (lower && (fwd || rev)) m.route = fwd ? kSiteForward : kSiteReverse;
        }
        return m;
    }
};

}  // namespace bdx
