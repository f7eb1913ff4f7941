"""Cases, CPU reference and route model of tests/test_gpu_insert.py, which holds K6's order-key insertion merge (csrc/bdx_insert.h:
k6_ranksort_kernel, k6_insert_kernel) to them through tests/prims/prims.hip.  Nothing here needs a GPU: tests/test_insert_cases.py
checks the reference against a naive placement, the model against the routes the cases are there for, and the cases against slips
of the two index computations no library restates.

Order key (csrc/bdx_k3.h): T << 35 | own << 34 | start << 8 | sequence number.  The device's list (any order, keys that differ) and the host's
(ascending, runs of equal keys) never share a (T, own, start).  The reference is a plain stable merge: numpy's stable argsort over
the host's keys followed by the device's sorted ones; the running totals are numpy's cumulative sums in uint32."""
import numpy as np

# ---- the header's constants (tests/test_gpu_insert.py pins them to prims_insert_constants) ------------------------------------

INS_THREADS = 1024       # kInsThreads
INS_LDS = 2048           # kInsLds
INS_BUCKET_MAX = 8192    # kInsBucketMax
INS_CNT_LDS = 10240      # kInsCntLds
INS_BUCKETS = 2048       # kInsBuckets
INS_BUCKET_DEPTH = 128   # kInsBucketDepth
RANK_SORT_MAX = 1 << 17  # kK6RankSortMax
RANK_SLICES = 16         # kK6RankSlices
RANK_GRID = 256          # kRankGrid
RANK_TILE = 2048         # kRankTile
SCAN_BLOCK = 256         # kScanBlock
CONSTANTS = [INS_THREADS, INS_LDS, INS_BUCKET_MAX, INS_CNT_LDS, INS_BUCKETS, INS_BUCKET_DEPTH, RANK_SORT_MAX, RANK_SLICES, RANK_GRID, RANK_TILE, SCAN_BLOCK]
INS_SUB = 64             # kInsSub
FILL = 0xA5A5A5A5
HOST_BIT = 0x80000000
SHIFT_T, SHIFT_OWN, SHIFT_START = 35, 34, 8     # kKeyShiftT, kKeyShiftOwn, kKeyShiftStart
SEQ_MASK = 255                                # kKeySeqMask
START_MASK = 0x3FFFFFF

ROUTES = ("rank", "bucket", "lds_bitonic", "hbm_bitonic", "ranksort")


def make_key(T, own, start, seq):
    return (np.asarray(T, np.uint64) << np.uint64(SHIFT_T)) | (np.asarray(own, np.uint64) << np.uint64(SHIFT_OWN)) | (np.asarray(start, np.uint64) << np.uint64(SHIFT_START)) | np.asarray(seq, np.uint64)


# ---- the route model ----------------------------------------------------------------------------------------------------------

def bucket_model(keys, n_regions, period, clamp=True):
    """ins_bucket_of over an array of keys, with ins_bucket_span's span of the run"""
    period = max(int(period), 1)
    span = (n_regions // period + 2) * INS_SUB + 1
    k = np.asarray(keys, np.uint64)
    T = (k >> np.uint64(SHIFT_T)).astype(np.int64)
    own = ((k >> np.uint64(SHIFT_OWN)) & np.uint64(1)).astype(np.int64)
    start = ((k >> np.uint64(SHIFT_START)) & np.uint64(START_MASK)).astype(np.int64)
    W = T // period
    r = T - W * period
    half = INS_SUB // 2
    second = half + ((start + period - T) * half) // period
    if clamp:
        second = np.minimum(INS_SUB - 1, second)     # == half + min(half - 1, ...)
    first = (start * half) // np.maximum(T, 1)
    sub = np.where(start >= T, INS_SUB - 1, np.where(start + period >= T, second, first))
    sub = np.where((r == 0) & (own == 0), sub, INS_SUB)
    return np.minimum(INS_BUCKETS - 1, ((W * INS_SUB + sub) * INS_BUCKETS) // span).astype(np.uint32)


def rank_layout(nd):
    nchunk = (nd + SCAN_BLOCK - 1) // SCAN_BLOCK
    nslice = min(RANK_SLICES, max(1, RANK_GRID // nchunk))
    return nchunk, nslice, (nd + nslice - 1) // nslice


def pow2_at_least(n):
    m = 1
    while m < n:
        m <<= 1
    return m


def route_model(nd, nh, sv_cap, with_rank, ins_plain, deepest_bucket, depth_slip=False):
    """which way a launch goes: 'overflow', 'empty' or one of ROUTES.  deepest_bucket: entries of the device's fullest bucket"""
    n = nd + nh
    if n > sv_cap:
        return "overflow"
    if n == 0:
        return "empty"
    if nd <= INS_THREADS:
        return "rank"
    if nd <= INS_BUCKET_MAX and ins_plain != 1:
        crowded = ins_plain == 2 or (deepest_bucket - 1 > INS_BUCKET_DEPTH if depth_slip else deepest_bucket - 1 >= INS_BUCKET_DEPTH)
        if not crowded:
            return "bucket"
    if with_rank and nd > INS_LDS and nd <= RANK_SORT_MAX and (nd > INS_BUCKET_MAX or ins_plain == 1):
        return "ranksort"
    return "lds_bitonic" if pow2_at_least(nd) <= INS_LDS else "hbm_bitonic"


def host_keys_in_lds(nh):
    return nh <= INS_LDS


def totals_in_lds(nd, nh):
    return nd + nh <= INS_CNT_LDS


# ---- key generators -----------------------------------------------------------------------------------------------------------

def host_keys(rng, nh, n_regions, period, mode="any"):
    """as bdx_api.hip writes them: any T, the own bit either way, sequence number 0, ascending, with runs of equal keys"""
    if nh == 0:
        return np.zeros(0, np.uint64)
    if mode == "zeros":
        return np.zeros(nh, np.uint64)
    nu = max(1, (nh * 3) // 4)
    T = rng.integers(0, max(1, n_regions), nu)
    if mode == "windows":            # thresholds of whole windows, not their own candidates: the bucket function's sub-slots apply to them
        T = (T // period) * period
        own = np.zeros(nu, np.int64)
    else:
        own = rng.integers(0, 2, nu)
    start = np.minimum(np.where(own == 1, T, rng.integers(0, 1 << 40, nu) % np.maximum(T + 50, 1)), START_MASK)
    k = make_key(T, own, start, 0)
    k = np.concatenate([k, rng.choice(k, nh - nu)])
    k.sort()
    return k


def device_pool(rng, want, n_regions, period, far=0.25, ge=0.0, w_lo=1, w_hi=None):
    """keys as the walks write them: T = W * period, own bit 0, sequence number <= SEQ_MASK; the start vertex in the window before T, far
    before it (translocations), or -- ge -- at or behind it.  More than `want` distinct keys in random order"""
    period = max(period, 1)
    w_max = n_regions // period if w_hi is None else w_hi
    m = want + want // 2 + 256
    if w_max < w_lo:                 # period larger than n_regions: window 0 alone, T = 0
        W = np.zeros(m, np.int64)
    else:
        W = rng.integers(w_lo, w_max + 1, m)
    T = W * period
    u = rng.random(m)
    local = np.maximum(T - 1 - rng.integers(0, period, m), 0)
    farv = (rng.integers(0, 1 << 40, m) % np.maximum(T - period, 1))
    gev = np.minimum(T + rng.integers(0, 1000, m), START_MASK)
    start = np.where(u < ge, gev, np.where(u < ge + far, farv, local))
    start = np.where(T == 0, gev, start)
    k = np.unique(make_key(T, 0, start, rng.integers(0, SEQ_MASK + 1, m)))
    rng.shuffle(k)
    return k


def without_hosts(pool, hk):
    """the keys of pool whose (T, own, start) no key of the host's list has"""
    if len(hk) == 0:
        return pool
    return pool[~np.isin(pool >> np.uint64(SHIFT_START), hk >> np.uint64(SHIFT_START))]


def thin(pool, n_regions, period, most=64, keep_out=()):
    """at most `most` keys of any bucket, none of the buckets keep_out"""
    b = bucket_model(pool, n_regions, period)
    order = np.argsort(b, kind="stable")
    bs = b[order]
    first = np.searchsorted(bs, bs, "left")
    ok = (np.arange(len(bs)) - first) < most
    for x in keep_out:
        ok &= bs != x
    out = pool[np.sort(order[ok])]
    return out


def window_pool(W, period, starts=None, nseq=128):
    """every key of window W's threshold with a start vertex of the window before (or the given ones) and the sequence numbers 0 .. nseq - 1"""
    T = W * period
    s = np.arange(max(T - period, 0), max(T, 1)) if starts is None else np.asarray(starts)
    s, q = np.meshgrid(s, np.arange(nseq), indexing="ij")
    return make_key(T, 0, s.ravel(), q.ravel())


# ---- cases --------------------------------------------------------------------------------------------------------------------

SV_BIG = (1 << 17) + 1 + 700          # the handle most cases share: every nd of the list with 700 host entries
BIG = (SV_BIG, 1)
NORANK = (2048, 0)                    # rank_part null as the product has it: sv_cap <= 2,048
TIGHT = (3000, 1)
REGIONS, PERIOD = 300_000, 101        # 2,972 windows: 1.45 to a bucket

ND_BOUNDARIES = [0, 1, 63, 64, 65, 1023, 1024, 1025, 2047, 2048, 2049, 4096, 4097, 8191, 8192, 8193, 10240, 10241, 32768, 32769, 65536, 65537,
                 1 << 17, (1 << 17) + 1]
NH_BOUNDARIES = [1023, 1024, 1025, 2047, 2048, 2049]


def case(name, nd, nh, handle=BIG, ins_plain=0, gen="default", counts="rand", n_regions=REGIONS, period=PERIOD, crowded=False, expect=None, **args):
    sv_cap, with_rank = handle
    if expect is None:
        expect = route_model(nd, nh, sv_cap, with_rank, ins_plain, INS_BUCKET_DEPTH + 1 if crowded else 1)
    return dict(name=name, nd=nd, nh=nh, handle=handle, ins_plain=ins_plain, gen=gen, counts=counts, n_regions=n_regions, period=period, expect=expect,
                crowded=crowded, args=args)


def _cases():
    out = []
    for nd in ND_BOUNDARIES:
        for nh in (0, 1, 700):
            out.append(case("nd-%d-nh-%d" % (nd, nh), nd, nh))
    for plain in (1, 2):
        for nd in (1025, 2048, 2049, 4096, 4097, 8192):
            out.append(case("plain%d-nd-%d" % (plain, nd), nd, 700, ins_plain=plain))
    for nd, nh in ((2048, 2049), (2048, 9000), (4096, 2049), (4096, 8000)):      # the sorts beside host keys in HBM and totals scanned in place
        out.append(case("plain2-nd-%d-nh-%d" % (nd, nh), nd, nh, ins_plain=2))
    for nd, nh in ((1025, 700), (2048, 0)):
        out.append(case("norank-plain1-nd-%d" % nd, nd, nh, handle=NORANK, ins_plain=1))
    for nd in (1000, 5000, 9000):
        for nh in NH_BOUNDARIES:
            out.append(case("nh-%d-nd-%d" % (nh, nd), nd, nh))
    for nd, nh in ((8192, 2048), (8192, 2049), (1024, 9216), (1024, 9217), (0, 10240), (0, 10241), (10240, 0), (10241, 0), (5000, 6264), (1024, 10240)):
        out.append(case("n-%d+%d" % (nd, nh), nd, nh))          # (the last two: n = 11,264, eleven whole rounds of the in-place scan)
    # bucket depth: the deep bucket first, in the middle, last; host keys inside it
    for where, W in (("first", 0), ("middle", 1500), ("last", REGIONS // PERIOD)):
        out.append(case("depth-128-%s" % where, 2048, 300, gen="deep", W=W, depth=INS_BUCKET_DEPTH))
        out.append(case("depth-129-%s-lds" % where, 2048, 300, gen="deep", W=W, depth=INS_BUCKET_DEPTH + 1, crowded=True))
        out.append(case("depth-129-%s-hbm" % where, 4000, 300, gen="deep", W=W, depth=INS_BUCKET_DEPTH + 1, crowded=True))
    # the same bucket filled with sequence numbers 128 ... 255 alone (the key's eighth bit): rank counting, the buckets, the LDS sort
    out.append(case("depth-128-high-seq-rank", 1000, 300, gen="deep", W=1500, depth=INS_BUCKET_DEPTH, seqs=SEQ_MASK + 1))
    out.append(case("depth-128-high-seq", 2048, 300, gen="deep", W=1500, depth=INS_BUCKET_DEPTH, seqs=SEQ_MASK + 1))
    out.append(case("depth-129-high-seq-lds", 2048, 300, gen="deep", W=1500, depth=INS_BUCKET_DEPTH + 1, crowded=True, seqs=SEQ_MASK + 1))
    # interleaving
    for nd in (900, 3000, 9000):
        out.append(case("device-below-host-%d" % nd, nd, 900, gen="split", device_first=True))
        out.append(case("host-below-device-%d" % nd, nd, 900, gen="split", device_first=False))
        out.append(case("alternating-%d" % nd, nd, nd, gen="alternating"))
        out.append(case("equal-host-runs-%d" % nd, nd, 600, gen="runs"))
    out.append(case("force-host-zeros", 0, 1500, gen="default", host_mode="zeros"))
    out.append(case("host-window-thresholds", 5000, 2000, host_mode="windows"))
    # periods and windows
    for nd in (700, 4000, 9000):
        out.append(case("period-1-%d" % nd, nd, 500, n_regions=5000, period=1, far=0.6))
        out.append(case("few-windows-%d" % nd, nd, 500, n_regions=1000, period=101, far=0.1))     # span = 705 < kInsBuckets
        out.append(case("most-regions-%d" % nd, nd, 500, n_regions=(1 << 26) - 2, period=101))
        out.append(case("starts-behind-T-%d" % nd, nd, 500, far=0.3, ge=0.3))
    out.append(case("period-above-regions-100", 100, 300, n_regions=50, period=101))
    out.append(case("period-above-regions-1500", 1500, 300, n_regions=50, period=101, crowded=True))   # T = 0 throughout: one bucket
    out.append(case("threshold-0", 3000, 300, gen="default", w_lo=0, w_hi=40, ge=0.1, n_regions=5000))
    # counts
    for name, nd, nh, kw in (("rank", 700, 700, {}), ("bucket", 5000, 1500, {}), ("lds", 2048, 700, dict(ins_plain=2)), ("hbm", 4096, 700, dict(ins_plain=2)),
                             ("ranksort", 9000, 700, {}), ("bitonic", 2048, 0, dict(handle=NORANK, ins_plain=1)), ("in-place", 9000, 2100, {})):
        for counts in ("zero", "max"):
            out.append(case("counts-%s-%s" % (counts, name), nd, nh, counts=counts, **kw))
    # capacity
    out.append(case("full-%d" % TIGHT[0], 2300, 700, handle=TIGHT))
    out.append(case("full-host-only", 0, 3000, handle=TIGHT))
    out.append(case("one-too-many", 2048, 953, handle=TIGHT))
    out.append(case("one-too-many-host", 1, 3000, handle=TIGHT))
    out.append(case("nothing", 0, 0, handle=TIGHT))
    return out


CASES = _cases()
BY_NAME = {c["name"]: c for c in CASES}
assert len(BY_NAME) == len(CASES)
# one handle, in this order: nothing of a call may show in the next
SEQUENCE = [case("seq-0", 1 << 17, 700), case("seq-1", 2049, 700, ins_plain=1), case("seq-2", 1025, 700), case("seq-3", 3, 2)]

FAMILY_OF = {"rank": "rank", "bucket": "bucket", "lds_bitonic": "bitonic", "hbm_bitonic": "bitonic", "ranksort": "ranksort", "overflow": "capacity", "empty": "capacity"}


def family(c):
    """the test a case runs in: its route, the crowded bucket cases and the capacity edges on their own"""
    if c["handle"] == TIGHT:
        return "capacity"
    if c["gen"] == "deep" or c["ins_plain"] == 2 or c["crowded"]:
        return "crowded" if c["expect"] != "bucket" else "bucket"
    return FAMILY_OF[c["expect"]]


FAMILIES = ("rank", "bucket", "crowded", "ranksort", "bitonic", "capacity")


def _seed(name):
    return [ord(ch) for ch in name]


_STAGE = {}


def stage_counts(sv_cap, counts):
    """[2 * sv_cap][2]: lib_count 0 ... 255 and cn_count 0 ... 60 of every staging record (all 0, all 65,535); one array per handle size, shared and read-only"""
    if (sv_cap, counts) not in _STAGE:
        rng = np.random.default_rng([sv_cap, 17])
        cnt = np.stack([rng.integers(0, 256, 2 * sv_cap), rng.integers(0, 61, 2 * sv_cap)], axis=1).astype(np.uint32)
        if counts != "rand":
            cnt[:] = 0 if counts == "zero" else 65535
        cnt.setflags(write=False)
        _STAGE[sv_cap, counts] = cnt
    return _STAGE[sv_cap, counts]


def build(c):
    """the arrays of a case: old_key, old_slot [nd], cnt_by_slot [2 * sv_cap][2], hs_key, hs_cnt [nh]"""
    rng = np.random.default_rng(_seed(c["name"]))
    nd, nh, R, P, a = c["nd"], c["nh"], c["n_regions"], c["period"], c["args"]
    sv_cap = c["handle"][0]
    gen = c["gen"]
    pool_kw = {k: a[k] for k in ("far", "ge", "w_lo", "w_hi") if k in a}
    if gen == "default":
        hk = host_keys(rng, nh, R, P, a.get("host_mode", "any"))
        dk = without_hosts(device_pool(rng, nd, R, P, **pool_kw), hk)
        if c["expect"] == "bucket":
            dk = thin(dk, R, P)
    elif gen == "deep":
        # `depth` entries in the bucket of window W's last sub-slots (T = 0: of its only one), host keys of the same threshold among them, and a
        # list around them that leaves this bucket alone and is thin elsewhere
        W, depth = a["W"], a["depth"]
        seqs = a.get("seqs", 128)
        wp = window_pool(W, P, None if W else np.arange(0, 400), nseq=seqs)
        if seqs > 128:
            wp = wp[(wp & np.uint64(SEQ_MASK)) >= np.uint64(128)]
        b = bucket_model(wp, R, P)
        target = int(b.max())
        inside = wp[b == target]
        starts = (inside >> np.uint64(SHIFT_START)) & np.uint64(START_MASK)
        odd = np.unique(starts[starts % np.uint64(2) == 1])
        hin = make_key(W * P, 0, odd[:40], 0)                      # host thresholds of the same window at the start vertices in between
        hk = np.concatenate([host_keys(rng, nh - 2 * len(hin), R, P), hin, hin])
        hk.sort()
        even = without_hosts(inside[starts % np.uint64(2) == 0], hk)
        rng.shuffle(even)
        deep = even[:depth]
        assert len(deep) == depth
        rest = thin(without_hosts(device_pool(rng, nd, R, P), hk), R, P, keep_out=(target,))
        dk = np.concatenate([deep, rest[:nd - depth]])
        rng.shuffle(dk)
    elif gen == "split":
        mid = (R // P) // 2
        lo, hi = dict(w_lo=1, w_hi=mid - 1), dict(w_lo=mid + 1, w_hi=R // P)
        dk = device_pool(rng, nd, R, P, **(lo if a["device_first"] else hi))
        hp = device_pool(rng, nh, R, P, **(hi if a["device_first"] else lo))[:nh] & ~np.uint64(SEQ_MASK)
        extra = make_key((hp >> np.uint64(SHIFT_T)) + np.uint64(3), 1, hp >> np.uint64(SHIFT_T), 0)[: nh // 3]   # thresholds inside a window, own bit set
        hk = np.concatenate([hp[: nh - len(extra)], extra])
        hk.sort()
        dk = without_hosts(dk, hk)
        if c["expect"] == "bucket":
            dk = thin(dk, R, P)
    elif gen == "alternating":
        p = device_pool(rng, 2 * (nd + nh), R, P)
        _, idx = np.unique(p >> np.uint64(SHIFT_START), return_index=True)     # one key per (T, start), ascending
        p = p[idx]
        if c["expect"] == "bucket":
            p = np.sort(thin(p, R, P, most=100))
        p = p[: nd + nh]
        dk, hk = p[0::2].copy(), (p[1::2] & ~np.uint64(SEQ_MASK))
        rng.shuffle(dk)
    elif gen == "runs":
        # runs of one host key, device keys of the same threshold at the start vertices on both sides of it
        W = rng.choice(np.arange(2, R // P), nh // 3, replace=False)
        T = W * P
        hk = np.repeat(make_key(T, 0, T - 50, 0), 3)
        hk.sort()
        side = np.concatenate([make_key(T, 0, T - 51, rng.integers(0, 128, len(T))), make_key(T, 0, T - 49, rng.integers(0, 128, len(T)))])
        rest = thin(without_hosts(device_pool(rng, nd, R, P), hk), R, P, most=60)
        dk = np.concatenate([side, rest[~np.isin(rest, side)][: nd - len(side)]])
        rng.shuffle(dk)
    else:
        raise ValueError(gen)
    dk, hk = dk[:nd], hk[:nh]
    assert len(dk) == nd and len(hk) == nh, (c["name"], len(dk), len(hk))
    stage_n = 2 * sv_cap
    slots = (rng.permutation(stage_n - 2)[:nd] + 1).astype(np.uint32)
    if nd > 2:
        slots[0], slots[1] = stage_n - 1, 0          # the first and the last staging record
    cnt = stage_counts(sv_cap, c["counts"])
    hcnt = (rng.integers(0, 256, nh) | (rng.integers(0, 61, nh) << 16)).astype(np.uint32)
    if c["counts"] == "zero":
        hcnt[:] = 0
    elif c["counts"] == "max":
        hcnt[:] = 0xFFFFFFFF
    return dict(old_key=np.ascontiguousarray(dk, np.uint64), old_slot=np.ascontiguousarray(slots), cnt_by_slot=np.ascontiguousarray(cnt),
                hs_key=np.ascontiguousarray(hk, np.uint64), hs_cnt=np.ascontiguousarray(hcnt))


def deepest_bucket(c, d):
    if c["nd"] == 0:
        return 0
    return int(np.bincount(bucket_model(d["old_key"], c["n_regions"], c["period"]), minlength=INS_BUCKETS).max())


def route_of(c, d, depth_slip=False):
    return route_model(c["nd"], c["nh"], c["handle"][0], c["handle"][1], c["ins_plain"], deepest_bucket(c, d), depth_slip)


# ---- the reference ------------------------------------------------------------------------------------------------------------

def _packed(d, slots):
    return d["cnt_by_slot"][slots, 0] | (d["cnt_by_slot"][slots, 1] << np.uint32(16))


def finish(c, T, src, cnt):
    """the four arrays as a launch leaves them, [sv_cap + 1] each, from the merged list's T, source and packed counts; n_ins, overflow"""
    sv1 = c["handle"][0] + 1
    n = len(T)
    out = [np.full(sv1, FILL, np.uint32) for _ in range(4)]
    out[0][:n], out[1][:n] = T, src
    for k, field in ((2, cnt & np.uint32(0xFFFF)), (3, cnt >> np.uint32(16))):
        out[k][1:n + 1] = np.cumsum(field, dtype=np.uint32)
        out[k][0] = 0
    return out, n, 0


def reference(c, d):
    """a plain stable merge of the host's list with the device's sorted one -> (ins_T, ins_src, ins_pre_l, ins_pre_c), n_ins, overflow"""
    nd, nh = c["nd"], c["nh"]
    if nd + nh > c["handle"][0]:
        out = [np.full(c["handle"][0] + 1, FILL, np.uint32) for _ in range(4)]
        out[2][0] = out[3][0] = 0
        return out, 0, 1
    order = np.argsort(d["old_key"], kind="stable")
    keys = np.concatenate([d["hs_key"], d["old_key"][order]])
    src = np.concatenate([np.arange(nh, dtype=np.uint32) | np.uint32(HOST_BIT), d["old_slot"][order]])
    cnt = np.concatenate([d["hs_cnt"], _packed(d, d["old_slot"][order])])
    m = np.argsort(keys, kind="stable")
    return finish(c, (keys[m] >> np.uint64(SHIFT_T)).astype(np.uint32), src[m], cnt[m])


def naive_reference(c, d):
    """every entry placed by counting, O(n^2): the entries with a smaller key, and of the host's equal keys the earlier ones"""
    nd, nh = c["nd"], c["nh"]
    keys = np.concatenate([d["hs_key"], d["old_key"]])
    idx = np.arange(nd + nh)
    less = keys[None, :] < keys[:, None]
    tie = (keys[None, :] == keys[:, None]) & (idx[None, :] < idx[:, None])
    pos = (less | tie).sum(axis=1)
    src = np.concatenate([np.arange(nh, dtype=np.uint32) | np.uint32(HOST_BIT), d["old_slot"]])
    cnt = np.concatenate([d["hs_cnt"], _packed(d, d["old_slot"])])
    T, s, k = np.zeros(nd + nh, np.uint32), np.zeros(nd + nh, np.uint32), np.zeros(nd + nh, np.uint32)
    T[pos], s[pos], k[pos] = (keys >> np.uint64(SHIFT_T)).astype(np.uint32), src, cnt
    return finish(c, T, s, k)


# ---- a model of the two index computations no library restates, with its slips -------------------------------------------------

SLIPS = ("slice_end", "hc0", "small_by_nd", "depth_gt")


def model(c, d, slip=None):
    """the bucket placement (histogram, running sums, every entry counted against its own bucket) and the rank sort (rank_layout's chunks,
    slices and tiles over an old_key with stale keys behind nd) as the kernels index them; the other routes sort with numpy.
    -> (arrays, n_ins, overflow), route"""
    nd, nh = c["nd"], c["nh"]
    route = route_of(c, d, depth_slip=slip == "depth_gt")
    if route in ("overflow", "empty"):
        return reference(c, d), route
    n = nd + nh
    dk, hk = d["old_key"], d["hs_key"]
    T, src, cnt = np.full(n, FILL, np.uint32), np.full(n, FILL, np.uint32), np.zeros(n, np.uint32)
    dcnt = _packed(d, d["old_slot"])
    if route == "bucket":
        bk = bucket_model(dk, c["n_regions"], c["period"])
        hist = np.bincount(bk, minlength=INS_BUCKETS)
        first = np.concatenate([[0], np.cumsum(hist)])             # s_hist after the running sums, s_hist[kInsBuckets] = nd
        order = np.argsort(bk, kind="stable")                      # s_ord: bucket by bucket, arrival order inside
        s_ord = dk[order]

        def below(x, b):
            return first[b] + int((s_ord[first[b]:first[b + 1]] < x).sum())
        dpos = np.array([below(dk[i], bk[i]) for i in range(nd)], np.int64) + np.searchsorted(hk, dk, "left")
        hb = bucket_model(hk, c["n_regions"], c["period"])
        hpos = np.arange(nh) + np.array([below(hk[j], hb[j]) for j in range(nh)], np.int64)
        hc = d["hs_cnt"].copy()
        if slip == "hc0" and nh <= INS_LDS:
            hc[INS_THREADS:] = d["hs_cnt"][: max(nh - INS_THREADS, 0)]      # hc[0] of the thread: the entry 1,024 before
    else:
        if route == "ranksort":
            nchunk, nslice, per = rank_layout(nd)
            stale = np.concatenate([dk, np.zeros(pow2_at_least(max(c["handle"][0], 1)) - nd, np.uint64)])   # an earlier call's small keys behind nd
            rank = np.zeros(nd, np.int64)
            for sl in range(nslice):
                k0 = min(nd, sl * per)
                k1 = k0 + per if slip == "slice_end" else min(nd, k0 + per)
                for t0 in range(k0, k1, RANK_TILE):
                    tile = np.sort(stale[t0:t0 + min(RANK_TILE, k1 - t0)])
                    rank += np.searchsorted(tile, dk, "left")
            sorted_key = np.zeros(nd, np.uint64)
            sorted_at = np.zeros(nd, np.int64)
            ok = rank < nd
            sorted_key[rank[ok]] = dk[ok]
            sorted_at[rank[ok]] = np.flatnonzero(ok)
        else:
            sorted_at = np.argsort(dk, kind="stable")
            sorted_key = dk[sorted_at]
        dpos_sorted = np.arange(nd) + np.searchsorted(hk, sorted_key, "left")
        dpos = np.zeros(nd, np.int64)
        dpos[sorted_at] = dpos_sorted
        hpos = np.arange(nh) + np.searchsorted(sorted_key, hk, "left")
        hc = d["hs_cnt"]
    ok = dpos < n
    T[dpos[ok]], src[dpos[ok]], cnt[dpos[ok]] = (dk[ok] >> np.uint64(SHIFT_T)).astype(np.uint32), d["old_slot"][ok], dcnt[ok]
    T[hpos], src[hpos], cnt[hpos] = (hk >> np.uint64(SHIFT_T)).astype(np.uint32), np.arange(nh, dtype=np.uint32) | np.uint32(HOST_BIT), hc
    out, n_ins, ovf = finish(c, T, src, cnt)
    small = (nd if slip == "small_by_nd" else n) <= INS_CNT_LDS
    if small and n > INS_CNT_LDS:      # counts written past s_cnt are lost, and ten entries a thread end at 10,240
        kept = cnt.copy()
        kept[INS_CNT_LDS:] = 0
        out, n_ins, ovf = finish(c, T, src, kept)
        out[2][INS_CNT_LDS:n], out[3][INS_CNT_LDS:n] = FILL, FILL
    return (out, n_ins, ovf), route
