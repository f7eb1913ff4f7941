"""Cases, plain references and route models of tests/test_gpu_compact.py, which holds K2 (csrc/k2_compact.hip: k2_compact_kernel,
k2_compact_side_kernel) and the pass-1 finalisation (csrc/k1_classify.hip: finalize_kernel; csrc/bdx_finalize.h: finalize2_body) to plain
references on their own.  Nothing here needs a GPU: tests/test_compact_cases.py checks the references against all-pairs statements, the
models against the references, the cases against the routes they are there for, and the cases' strength against a list of slips.

A K2 CASE is a store (random columns, every value distinct per read, so that a gather from the wrong index shows), class bytes written
directly (flag | 0x10 pass | 0x20 proper | 0x40 normal-left, only in combinations K1 writes: free control of every tile's counts), the
libraries' counter keys and the call's capacity, fills and segments.  k2_reference() is one pass over the reads in stream order with three
running counts.  k1_model() is what K1 and the finalisation leave K2 (tile totals, ready-made records, marks, chunk-local prefixes and the
chunks' totals); k2_model() is K2's own way through those tables (record route, column route in slice rounds), on which the routes a
case takes are read off and the slips of the kernel's own logic are applied.

A FINALISATION CASE is a table of tile totals, a table of monoid records and 64 copies of the counters; fin_reference() restates both
kernels: running sums in uint32 per column that restart per chunk, a sequential mono_combine in Python ints wrapped to 64 bits, W and
the densities in float32 (IEEE division, round to nearest: what __fdiv_rn is), the counters as a sum over the copies."""
import functools

import numpy as np

# ---- the kernels' constants (tests/test_gpu_compact.py asserts them against the harness) ------------------------------------------------
TILE = 256            # kTile
SUB = 4               # kK2TilesPerWave
TILE2 = TILE * SUB    # reads per super tile = per wave of K2
PER_LANE = 16
STASH_CAP = 16        # kStashCap
STASH_KEYS = 2        # kStashKeys
MAX_CHUNKS = 64       # kMaxChunks
CNT_COPIES = 64       # kCntCopies
SLICE = 256           # kSlice
STASH_WORDS = 8       # sizeof(StashRec) / 4
P1_BYTES = 2304       # sizeof(Pass1)
P1_WORDS = P1_BYTES // 4
P1_REF_WORD = 64      # offsetof(Pass1, ref_len) / 4
MONO_BYTES = 24       # sizeof(MonoRec)
NUM_FLAGS = 11
F_LARGE, F_SMALL = 2, 3
NORMAL_FR, NORMAL_RF = 6, 7
ROUND = 4096          # super tiles a workgroup of finalize_kernel scans per round: a chunk is a whole number of them
K2_GRID_CAP = 8192
SEG_GAP = 64          # the harness's gap between two pinned segments
FILL = 0xA5A5A5A5
FILL64 = 0xA5A5A5A5A5A5A5A5
M32 = 0xFFFFFFFF
COL_ANOM, COL_NORMAL, COL_KEY0 = 0, 1, 2

MONO = np.dtype([("ft", "<i4"), ("fp", "<i4"), ("lt", "<i4"), ("lp", "<i4"), ("sum", "<i8")])
assert MONO.itemsize == MONO_BYTES

# the buffer set the small cases share (tests/test_gpu_compact.py opens it once)
H = dict(n_cap=64 * 3 * TILE2 + TILE2, cap=8192, fill_cap=2048, nkeys_cap=60, nbams_cap=4)

ANOM_FLAGS = (1, 2, 3, 4, 8)              # what an anomalous read's nibble can be: FF (RR is folded into it), LARGE, SMALL, RF, CTX


def row16(tiles):
    return (max(tiles, 16) + 15) // 16 * 16


# ---- K2: stores and class bytes -----------------------------------------------------------------------------------------------------------

def columns(n, seed, nlibs=1, lib_mode="random", lib_high=False):
    """random columns, distinct per read; isize of both signs (never INT_MIN), qlen up to 65,535, SAM flag 0x10 both ways"""
    rng = np.random.default_rng([seed, n])
    perm = rng.permutation(n).astype(np.int64)
    d = dict(tid=(perm * 7 + 11).astype(np.int32), pos=(rng.permutation(n).astype(np.int64) * 5 + 1000003).astype(np.int32))
    mag = rng.permutation(n).astype(np.int64) + 1
    mag[: min(n, 2)] = (1 << 31) - 1 - np.arange(min(n, 2))
    d["isize"] = (mag * rng.choice([-1, 1], n)).astype(np.int32)
    d["flag"] = rng.integers(0, 1 << 16, n).astype(np.uint16)
    q = rng.integers(0, 1 << 16, n)
    q[rng.integers(0, n)] = 65535
    d["qlen"] = q.astype(np.uint16)
    d["key"] = (rng.permutation(n).astype(np.uint64) * np.uint64(0x9E3779B97F4A7C15)) ^ np.uint64(0x1234567)
    d["check"] = (rng.permutation(n).astype(np.uint64) * np.uint64(0xC2B2AE3D27D4EB4F)) ^ np.uint64(0x7654321)
    top = 256 if lib_high or nlibs == 1 else nlibs     # (with one library the column is not read: any byte)
    if lib_mode == "tile":       # one library per tile: K1 leaves ready-made records
        lib = np.repeat(rng.integers(0, top, (n + TILE - 1) // TILE), TILE)[:n]
    else:
        lib = rng.integers(0, top, n)
    d["lib"] = lib.astype(np.uint8)
    return d


def class_bytes(n, anom, seed, p_pass=0.7, p_left=0.4, p_proper=0.5):
    """class bytes with the reads `anom` (indices) anomalous and no others"""
    rng = np.random.default_rng([seed, n, 77])
    passing = rng.random(n) < p_pass
    cls = rng.integers(0, 11, n).astype(np.uint8)                                 # not passing: the bare flag, any of the eleven
    normal = np.where(rng.random(n) < 0.5, NORMAL_FR, NORMAL_RF).astype(np.uint8)
    left = rng.random(n) < p_left
    cls[passing] = normal[passing] | 0x10 | np.where(left[passing], 0x40, 0).astype(np.uint8)
    a = np.asarray(anom, np.int64)
    cls[a] = np.asarray(ANOM_FLAGS, np.uint8)[rng.integers(0, len(ANOM_FLAGS), len(a))] | 0x10
    ok = (cls & 0x10) != 0
    cls[ok & (rng.random(n) < p_proper)] |= 0x20
    return cls


def spread(counts, seed, n=None, pins=()):
    """indices of counts[t] anomalous reads in tile t, at random offsets; pins: indices that must be among them"""
    rng = np.random.default_rng([seed, len(counts), 5])
    out = []
    for t, k in enumerate(counts):
        lo, hi = t * TILE, (t + 1) * TILE if n is None else min((t + 1) * TILE, n)
        forced = [p for p in pins if lo <= p < hi]
        rest = np.setdiff1d(np.arange(lo, hi), forced)
        out += forced + rng.choice(rest, k - len(forced), replace=False).tolist()
    return np.sort(np.asarray(out, np.int64))


def k2_case(name, n, anom, seed=1, nkeys=1, nlibs=1, lib_key=(0,), lib_mode="random", lib_high=False, cap=None, chunk_super=1 << 14, pre_off=None,
            chunk_off=None, check=True, seg=None, fills=((0, 0), (0, 0), (0, 0), (0, 0)), cls=None, cls_kw=None, edit=None):
    d = columns(n, seed, nlibs, lib_mode, lib_high)
    c = dict(d, name=name, n=n, nkeys=nkeys, nlibs=nlibs, lib_key=np.asarray(lib_key, np.int32), chunk_super=chunk_super, seg=seg, fills=fills,
             has_check=check, ntiles=(n + TILE - 1) // TILE)
    c["cls"] = class_bytes(n, anom, seed, **(cls_kw or {})) if cls is None else cls
    if edit:
        edit(c)
    c["tstride"] = row16(c["ntiles"])
    c["nsuper"] = (c["ntiles"] + SUB - 1) // SUB
    ncols = 2 + nkeys
    c["pre_off"] = np.zeros(ncols, np.uint32) if pre_off is None else np.asarray(pre_off, np.uint32)
    c["chunk_off"] = np.zeros(ncols, np.uint32) if chunk_off is None else np.asarray(chunk_off, np.uint32)
    c["count"] = int(masks(c)["anom"].sum())
    c["cap"] = c["count"] if cap is None else cap
    assert len(c["lib_key"]) == nlibs and c["cap"] <= H["cap"] or name == "strided"
    for k, v in c.items():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


# ---- K2: the reference ----------------------------------------------------------------------------------------------------------------------

def masks(c, slip=None):
    cls = c["cls"]
    f = cls & 15
    passing = (cls & 0x10) != 0 if slip != "pass_ignored" else np.ones(len(cls), bool)
    normal = (f == NORMAL_FR) | ((f == NORMAL_RF) if slip != "normal_rf_anomalous" else False)
    lib = c["lib"].astype(np.int64) if c["nlibs"] > 1 else np.zeros(c["n"], np.int64)
    if slip == "lib_not_clamped":
        lib = c["lib"].astype(np.int64) % max(c["nlibs"], 1) if c["nlibs"] > 1 else lib
    else:
        lib = np.where(lib < c["nlibs"], lib, 0)
    return dict(anom=passing & ~normal, nleft=passing & ((cls & 0x40) != 0), proper=passing & ((cls & 0x20) != 0), lib=lib, key=c["lib_key"][lib].astype(np.int64),
                flag=f)


def blank_out(c):
    """the Compact arrays of the handle before a launch (hcap: a case that needs a larger handle than the shared one)"""
    hc = c.get("hcap", H["cap"])
    return dict(tid=np.full(hc, FILL, np.uint32).view(np.int32), pos=np.full(hc, FILL, np.uint32).view(np.int32), isize=np.full(hc, FILL, np.uint32).view(np.int32),
                meta=np.full(hc, FILL, np.uint32), key=np.full(hc, FILL64, np.uint64), check=np.full(hc, FILL64, np.uint64), idx=np.full(hc, FILL, np.uint32),
                nn=np.full(hc, FILL, np.uint32), pk=np.full(hc * H["nkeys_cap"], FILL, np.uint32))


OUT_FIELDS = ("tid", "pos", "isize", "meta", "key", "check", "idx", "nn", "pk")


def base_of_read(c):
    """what the hand-made prefixes add in front of every read's counts, per column: [ncols][n] (uint32, wrapping)"""
    chunk = (np.arange(c["n"]) // TILE2) // c["chunk_super"]
    return (c["pre_off"][:, None] + np.where(chunk[None, :] >= 1, c["chunk_off"][:, None], np.uint32(0))).astype(np.uint32)


def k2_reference(c, slip=None):
    """one pass over the reads in stream order: running counts of normal-left reads (exclusive), of proper reads per key (inclusive) and of
    the anomalous rank; one record per passing read whose flag is not NORMAL_FR / NORMAL_RF while rank < cap.  (The running counts are
    cumulative sums: the loop, vectorised -- k2_loop() is the loop itself.)"""
    m = masks(c, slip)
    n, cap, nkeys = c["n"], c["cap"], c["nkeys"]
    base = base_of_read(c)
    u32 = lambda a: (a.astype(np.int64) & M32).astype(np.uint32)
    nn = np.cumsum(m["nleft"]) - (0 if slip == "nn_inclusive" else m["nleft"])
    rank = u32(np.cumsum(m["anom"]) - m["anom"] + base[COL_ANOM])
    nn = u32(nn + base[COL_NORMAL])
    sel = np.flatnonzero(m["anom"] & ((rank <= cap) if slip == "cap_le" else (rank < cap)))
    j = rank[sel].astype(np.int64)
    o = blank_out(c)
    keep = j < len(o["tid"])        # (only the cap_le slip can step past the handle's arrays)
    sel, j = sel[keep], j[keep]
    o["tid"][j] = c["tid"][sel]
    o["pos"][j] = c["pos"][sel]
    isz = c["isize"][sel].astype(np.int64)
    o["isize"][j] = (isz if slip == "isize_no_abs" else np.abs(isz)).astype(np.int32)
    rev = (c["flag"][sel].astype(np.uint32) >> (5 if slip == "rev_from_0x20" else 4)) & 1
    o["meta"][j] = m["flag"][sel].astype(np.uint32) | (rev << 4) | (m["lib"][sel].astype(np.uint32) << 8) | (c["qlen"][sel].astype(np.uint32) << 16)
    o["key"][j] = c["key"][sel]
    if c["has_check"]:
        o["check"][j] = c["check"][sel]
    o["idx"][j] = sel.astype(np.uint32)
    o["nn"][j] = nn[sel]
    stride = c["count"] if slip == "pk_stride_by_count" else cap
    for k in range(nkeys):
        mk = m["proper"] & (m["key"] == k)
        pk = u32(np.cumsum(mk) - (mk if slip == "pk_exclusive" else 0) + base[COL_KEY0 + k])
        at = k * stride + j
        ok = at < len(o["pk"])
        o["pk"][at[ok]] = pk[sel][ok]
    return o


def k2_loop(c):
    """the same, one read at a time"""
    m = masks(c)
    base = base_of_read(c).astype(np.int64)
    o = blank_out(c)
    nn, rank, pk = 0, 0, [0] * c["nkeys"]
    for i in range(c["n"]):
        if m["proper"][i]:
            pk[int(m["key"][i])] += 1
        if m["anom"][i]:
            j = (rank + int(base[COL_ANOM][i])) & M32
            if j < c["cap"]:
                o["tid"][j], o["pos"][j], o["isize"][j] = c["tid"][i], c["pos"][i], abs(int(c["isize"][i]))
                o["meta"][j] = int(m["flag"][i]) | (((int(c["flag"][i]) >> 4) & 1) << 4) | (int(m["lib"][i]) << 8) | (int(c["qlen"][i]) << 16)
                o["key"][j] = c["key"][i]
                if c["has_check"]:
                    o["check"][j] = c["check"][i]
                o["idx"][j] = i
                o["nn"][j] = (nn + int(base[COL_NORMAL][i])) & M32
                for k in range(c["nkeys"]):
                    o["pk"][k * c["cap"] + j] = (pk[k] + int(base[COL_KEY0 + k][i])) & M32
            rank += 1
        if m["nleft"][i]:
            nn += 1
    return o


def k2_all_pairs(c):
    """the O(n^2) statement: every count as a sum of a mask over all earlier reads"""
    m = masks(c)
    base = base_of_read(c).astype(np.int64)
    i = np.arange(c["n"])
    earlier = i[None, :] < i[:, None]            # [read, other]
    upto = i[None, :] <= i[:, None]
    o = blank_out(c)
    for r in np.flatnonzero(m["anom"]):
        j = (int((earlier[r] & m["anom"]).sum()) + int(base[COL_ANOM][r])) & M32
        if j >= c["cap"]:
            continue
        o["idx"][j] = r
        o["nn"][j] = (int((earlier[r] & m["nleft"]).sum()) + int(base[COL_NORMAL][r])) & M32
        for k in range(c["nkeys"]):
            o["pk"][k * c["cap"] + j] = (int((upto[r] & m["proper"] & (m["key"] == k)).sum()) + int(base[COL_KEY0 + k][r])) & M32
    return o


def differs(a, b, fields=OUT_FIELDS):
    for f in fields:
        if not np.array_equal(np.asarray(a[f]).view(np.uint8), np.asarray(b[f]).view(np.uint8)):
            return f
    return None


# ---- what K1 and the finalisation leave K2 ----------------------------------------------------------------------------------------------------

def k1_model(c):
    """tile_tot [ncols][tstride]; stash [ntiles][kStashCap][8] (0xA5 where K1 writes nothing) and which tiles are marked; tile_pre
    [ncols][tstride] (chunk-local exclusive prefixes at the super tiles, plus the case's hand-made offsets), chunk_tot and chunk_base
    [ncols][kMaxChunks]"""
    m = masks(c)
    n, nt, ts, nkeys = c["n"], c["ntiles"], c["tstride"], c["nkeys"]
    ncols = 2 + nkeys
    pad = nt * TILE - n
    per_tile = lambda b: np.concatenate([b, np.zeros(pad, bool)]).reshape(nt, TILE).sum(axis=1)
    tt = np.zeros((ncols, ts), np.uint32)
    tt[COL_ANOM, :nt] = per_tile(m["anom"])
    tt[COL_NORMAL, :nt] = per_tile(m["nleft"])
    for k in range(nkeys):
        tt[COL_KEY0 + k, :nt] = per_tile(m["proper"] & (m["key"] == k))
    # ready-made records: a full tile whose reads -- all of them, passing or not -- count for one key; else the slots K2 would read are marked
    keyp = np.concatenate([m["key"], np.full(pad, -1)]).reshape(nt, TILE)
    one_key = (keyp == keyp[:, :1]).all(axis=1)
    stash = np.full((nt, STASH_CAP, STASH_WORDS), FILL, np.uint32)
    marked = np.zeros(nt, bool)
    for t in np.flatnonzero(tt[COL_ANOM, :nt]):
        lo = t * TILE
        hi = min(lo + TILE, n)
        a = np.flatnonzero(m["anom"][lo:hi])[:STASH_CAP]
        if not one_key[t]:
            marked[t] = True
            stash[t, :len(a), 4] = M32
            continue
        i = lo + a
        rn = np.cumsum(m["nleft"][lo:hi])[a] - m["nleft"][lo:hi][a]
        rk = np.cumsum(m["proper"][lo:hi])[a]
        stash[t, :len(a), 0] = c["tid"][i].view(np.uint32)
        stash[t, :len(a), 1] = c["pos"][i].view(np.uint32)
        stash[t, :len(a), 2] = np.abs(c["isize"][i].astype(np.int64)).astype(np.uint32)
        stash[t, :len(a), 3] = m["flag"][i].astype(np.uint32) | (((c["flag"][i].astype(np.uint32) >> 4) & 1) << 4) | (m["lib"][i].astype(np.uint32) << 8)
        stash[t, :len(a), 4] = a.astype(np.uint32) | (rn.astype(np.uint32) << 8) | (np.uint32(keyp[t, 0]) << 20)
        stash[t, :len(a), 5] = rk.astype(np.uint32)
        stash[t, :len(a), 6:] = 0
    pre, ctot, cbase = scan_tables(tt, nt, ts, c["chunk_super"])
    pre = (pre + c["pre_off"][:, None]).astype(np.uint32)
    ctot[:, 0] += c["chunk_off"]
    cbase[:, 1:] += c["chunk_off"][:, None]
    return dict(tile_tot=tt, stash=stash, marked=marked, tile_pre=pre, chunk_tot=ctot, chunk_base=cbase)


def scan_tables(tt, ntiles, tstride, chunk_super):
    """chunk-local exclusive prefixes of the super tiles' totals, the chunks' totals, the totals of the chunks before each (all 64 words)"""
    ncols = tt.shape[0]
    nsuper = (ntiles + SUB - 1) // SUB
    st = tt[:, : tstride // SUB * SUB].reshape(ncols, -1, SUB).sum(axis=2, dtype=np.uint32)[:, :nsuper] if nsuper else np.zeros((ncols, 0), np.uint32)
    pre = np.zeros((ncols, tstride), np.uint32)
    ctot = np.zeros((ncols, MAX_CHUNKS), np.uint32)
    cs = chunk_super
    for g in range((nsuper + cs - 1) // cs):
        seg = st[:, g * cs:(g + 1) * cs]
        inc = np.cumsum(seg, axis=1, dtype=np.uint32)
        pre[:, g * cs:g * cs + seg.shape[1]] = inc - seg
        ctot[:, g] = inc[:, -1]
    inc = np.cumsum(ctot, axis=1, dtype=np.uint32)
    return pre, ctot, (inc - ctot).astype(np.uint32)


def seg_layout(c):
    """the harness's pinned copies: segment s lies SEG_GAP * s entries behind its place, 0xA5 between"""
    nseg = len(c["seg"]) - 1
    m = c["n"] + nseg * SEG_GAP
    key, qlen, check = np.full(m, FILL64, np.uint64), np.full(m, 0xA5A5, np.uint16), np.full(m, FILL64, np.uint64)
    for s in range(nseg):
        b, e = c["seg"][s], c["seg"][s + 1]
        key[b + s * SEG_GAP:e + s * SEG_GAP] = c["key"][b:e]
        qlen[b + s * SEG_GAP:e + s * SEG_GAP] = c["qlen"][b:e]
        check[b + s * SEG_GAP:e + s * SEG_GAP] = c["check"][b:e]
    return key, qlen, check


# ---- K2's own way through the tables ------------------------------------------------------------------------------------------------------------

def k2_model(c, stash=True, side=0, slip=None, routes=None, tables=None):
    """what k2_body writes, super tile by super tile, from the tables of k1_model(): the record route (every tile of the super tile within
    kStashCap and none marked), else the column route in rounds of kSlice.  routes: a dict that collects what the case reaches."""
    t = tables or k1_model(c)
    m = masks(c)
    n, nt, nkeys, cap = c["n"], c["ntiles"], c["nkeys"], c["cap"]
    use_stash = stash and nkeys <= STASH_KEYS
    R = routes if routes is not None else {}
    for k in ("route", "tq", "rec_key", "rounds", "chunk", "last_key", "seg_edge", "template"):
        R.setdefault(k, set())
    R["template"].add("bases" if side == 0 else "sums")
    o = blank_out(c)
    tt, pre, ctot, cbase = t["tile_tot"], t["tile_pre"], t["chunk_tot"], t["chunk_base"]
    if c["seg"] is not None:
        skey, sqlen, scheck = seg_layout(c)
        seg = np.asarray(c["seg"], np.int64)

    def name_of(i):
        if c["seg"] is None:
            return c["key"][i], int(c["qlen"][i]), c["check"][i]
        s = int(np.searchsorted(seg[:-1], i, "left" if slip == "segment_lt" else "right")) - 1
        s = max(s, 0)
        if i == seg[s]:
            R["seg_edge"].add("first")
        if i == seg[s + 1] - 1:
            R["seg_edge"].add("last")
        at = i + s * SEG_GAP
        return skey[at], int(sqlen[at]), scheck[at]

    def put(j, i, tid, pos, isz, meta_lo, nn, pks):
        key, qlen, chk = name_of(i)
        o["tid"][j], o["pos"][j], o["isize"][j] = tid, pos, isz
        o["meta"][j] = (meta_lo | (qlen << 16)) & M32
        o["key"][j] = key
        if c["has_check"]:
            o["check"][j] = chk
        o["idx"][j] = i
        o["nn"][j] = nn & M32
        for k, v in pks:
            o["pk"][k * cap + j] = v & M32

    for t2 in range(c["nsuper"]):
        chunk = (t2 * SUB if slip == "chunk_super_on_tiles" else t2) // c["chunk_super"]
        chunk = min(chunk, MAX_CHUNKS - 1)

        def prefix(col):
            if side == 0:
                return (int(pre[col, t2]) + int(cbase[col, chunk])) & M32
            return (int(pre[col, t2]) + int(ctot[col, :chunk + (1 if slip == "chunk_sum_inclusive" else 0)].sum(dtype=np.uint32))) & M32

        tiles = [t2 * SUB + q for q in range(SUB)]
        a = [int(tt[COL_ANOM, x]) if x < nt else 0 for x in tiles]
        A = sum(a)
        lo = t2 * TILE2
        hi = min(lo + TILE2, n)
        if use_stash:
            if A == 0:
                continue
            if max(a) <= STASH_CAP:
                seen = [x for q, x in enumerate(tiles) if a[q] and t["marked"][x]]
                if slip == "mark_first_tile_only":
                    seen = [x for x in seen if x == tiles[0]]
                if not seen:
                    R["route"].add("records")
                    R["chunk"].add(chunk)
                    bases = [prefix(COL_NORMAL), prefix(COL_ANOM), prefix(COL_KEY0), prefix(COL_KEY0 + 1) if nkeys > 1 else 0]
                    for q in range(A):
                        tq = (q >= a[0]) + (q >= a[0] + a[1]) + (q >= a[0] + a[1] + a[2])
                        R["tq"].add(tq)
                        before = sum(a[:tq])
                        if slip == "before_off_by_a_tile":
                            before = sum(a[:max(tq - 1, 0)]) if tq else 0
                        e = [int(tt[col, tiles[0]:tiles[0] + tq].sum()) for col in (1, 2, 3) if col < 2 + nkeys] + [0, 0]
                        if slip == "e_wrong_column":
                            e = [e[1], e[0]] + e[2:]
                        tile = tiles[tq]
                        r = t["stash"][tile, min(q - before, STASH_CAP - 1)]
                        if int(r[4]) == M32:      # (only a slipped model gets here)
                            r = np.zeros(STASH_WORDS, np.uint32)
                        j = (bases[1] + q) & M32
                        if j >= cap:
                            continue
                        i = tile * TILE + (int(r[4]) & 255)
                        k0 = (int(r[4]) >> 20) & 63
                        if slip == "tile_key_ignored":
                            k0 = 0
                        R["rec_key"].add(k0)
                        pks = [(0, bases[2] + e[1] + (int(r[5]) if k0 == 0 else 0))]
                        if nkeys > 1:
                            pks.append((1, bases[3] + e[2] + (int(r[5]) if k0 == 1 else 0)))
                        put(j, min(i, n - 1), np.int32(r[0].view(np.int32)), np.int32(r[1].view(np.int32)), np.int32(r[2].view(np.int32)), int(r[3]),
                            bases[0] + e[0] + ((int(r[4]) >> 8) & 511), pks)
                    continue
                R["route"].add("marked")
        an = np.flatnonzero(m["anom"][lo:hi])
        if len(an) == 0:
            continue
        R["route"].add("columns")
        R["chunk"].add(chunk)
        R["rounds"].add((len(an) + SLICE - 1) // SLICE)
        R["last_key"].add((nkeys - 1) % 2 if nkeys > 2 else None)
        pre_norm, rank0 = prefix(COL_NORMAL), prefix(COL_ANOM)
        nl_before = np.cumsum(m["nleft"][lo:hi]) - m["nleft"][lo:hi]
        if slip == "nn_inclusive":      # the scan over the lanes taken inclusive: every read gets its own lane's count on top
            per_lane = np.add.reduceat(m["nleft"][lo:hi].astype(np.int64), np.arange(0, hi - lo, PER_LANE))
            nl_before = nl_before + np.repeat(per_lane, PER_LANE)[:hi - lo]
        pk_upto = [np.cumsum(m["proper"][lo:hi] & (m["key"][lo:hi] == k)) for k in range(nkeys)]
        kb = [prefix(COL_KEY0 + k) for k in range(nkeys)]
        for local, off in enumerate(an):
            j = (rank0 + local) & M32
            if j >= cap:
                continue
            i = lo + int(off)
            pks = [(k, kb[k] + int(pk_upto[k][off])) for k in range(nkeys)]
            if slip == "slice_at_255" and local % SLICE == SLICE - 1:      # the slot behind a slice of 255: nobody gathers it, only its pk rows
                for k, v in pks:
                    o["pk"][k * cap + j] = v & M32
                continue
            meta_lo = int(c["cls"][i] & 15) | (((int(c["flag"][i]) >> 4) & 1) << 4) | (int(m["lib"][i]) << 8)
            put(j, i, c["tid"][i], c["pos"][i], abs(int(c["isize"][i])), meta_lo, pre_norm + int(nl_before[off]), pks)
    return o


def fill_model(c, slip=None):
    out = []
    for words, value in c["fills"]:
        f = np.full(max(H["fill_cap"], 4), FILL, np.uint32)
        f[: (words // 4 * 4) if slip == "fill_tail_dropped" else words] = value
        out.append(f)
    return out


def k2_grid(c):
    return min((c["nsuper"] + 3) // 4, K2_GRID_CAP)


# ---- K2: the cases --------------------------------------------------------------------------------------------------------------------------------

def _random_anom(n, seed, p):
    rng = np.random.default_rng([seed, n, 3])
    a = np.flatnonzero(rng.random(n) < p)
    return a if len(a) else np.asarray([n - 1])


def _all_left_tile(tile, count, anom_last=False):
    """edit: `count` reads of the tile normal-left and proper from its start, none elsewhere in it; anom_last: the tile's last read anomalous"""
    def edit(c):
        cls = c["cls"].copy()
        lo = tile * TILE
        cls[lo:lo + TILE] = 0
        cls[lo:lo + count] = NORMAL_FR | 0x10 | 0x20 | 0x40
        if anom_last:
            cls[lo + TILE - 1] = 8 | 0x10 | 0x20
        c["cls"] = cls
    return edit


def _mixed_tiles(tiles, nlibs):
    """edit: the given tiles hold reads of every library in turn (K1 marks them when the libraries' keys differ)"""
    def edit(c):
        lib = c["lib"].copy()
        for t in tiles:
            lo, hi = t * TILE, min((t + 1) * TILE, c["n"])
            lib[lo:hi] = np.arange(hi - lo) % nlibs
        c["lib"] = lib
    return edit


@functools.lru_cache(maxsize=1)
def k2_cases():
    C = []
    add = lambda *a, **k: C.append(k2_case(*a, **k))
    for n in (1, 15, 16, 17, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097, 5 * TILE + 3):
        add("n_%d_sparse" % n, n, _random_anom(n, 1, 0.02), seed=n)
        add("n_%d_dense" % n, n, _random_anom(n, 2, 0.4), seed=n + 1)
    add("no_anomalous_read", 3 * TILE2 + 5, [], seed=3, fills=((5, 7), (4, 9), (3, 11), (1, 13)))
    add("empty_super_tile_between", 3 * TILE2, spread((3, 0, 0, 1, 0, 0, 0, 0, 0, 2, 17, 0), 4), seed=4)
    for counts in ((0, 0, 0, 1), (1, 0, 0, 0), (16, 16, 16, 16), (16, 16, 16, 17), (17, 0, 0, 0), (0, 0, 0, 256), (64, 64, 64, 64), (64, 64, 64, 65),
                   (128, 128, 128, 128), (128, 128, 128, 129), (256, 256, 256, 256), (3, 1, 0, 2, 16, 0, 16, 1, 0, 0, 0, 0, 5, 5, 5)):
        add("counts_" + "_".join(map(str, counts)), len(counts) * TILE, spread(counts, 5), seed=5 + sum(counts))
    add("lane_0_and_lane_63", 2 * TILE2, spread((1, 0, 0, 1, 40, 0, 0, 40), 6, pins=(0, TILE2 - 1, TILE2, 2 * TILE2 - 1)), seed=6)
    # marks: two libraries with a key each; tiles of one library leave records, tiles of both are marked
    two = dict(nkeys=2, nlibs=2, lib_key=(0, 1), lib_mode="tile")
    add("two_keys_records", 4 * TILE2, spread((3, 2, 1, 4, 16, 0, 16, 16, 0, 0, 1, 0, 5, 5, 5, 5), 7), seed=7, **two)
    add("one_marked_among_four", 2 * TILE2, spread((3, 2, 1, 4, 2, 2, 2, 2), 8), seed=8, edit=_mixed_tiles((2,), 2), **two)
    add("marked_tile_not_the_first", TILE2, spread((3, 2, 1, 4), 8), seed=18, edit=_mixed_tiles((3,), 2), **two)
    add("all_four_marked", TILE2, spread((3, 2, 1, 4), 9), seed=9, edit=_mixed_tiles((0, 1, 2, 3), 2), **two)
    add("marked_and_beyond_the_stash", TILE2, spread((3, 20, 1, 4), 10), seed=10, edit=_mixed_tiles((0,), 2), **two)
    add("marked_ragged_end", TILE2 + 100, spread((3, 2, 1, 4, 5), 11, n=TILE2 + 100), seed=11, **two)
    add("many_libraries_one_key", 2 * TILE2, spread((3, 2, 1, 4, 9, 9, 9, 30), 12), seed=12, nkeys=1, nlibs=9, lib_key=(0,) * 9)
    add("libraries_many_to_one", 2 * TILE2, spread((3, 2, 1, 4, 9, 9, 9, 30), 13), seed=13, nkeys=2, nlibs=5, lib_key=(0, 1, 1, 0, 1))
    add("library_bytes_out_of_range", 2 * TILE2, spread((3, 2, 1, 4, 9, 9, 9, 30), 14), seed=14, nkeys=2, nlibs=3, lib_key=(1, 0, 1), lib_high=True)
    add("library_bytes_out_of_range_per_tile", 2 * TILE2, spread((3, 2, 1, 4, 9, 9, 9, 3), 15), seed=15, nkeys=2, nlibs=3, lib_key=(1, 0, 1), lib_high=True, lib_mode="tile")
    for nkeys in (3, 4, 5, 60):
        add("keys_%d" % nkeys, 2 * TILE2 + 77, spread((3, 2, 1, 4, 9, 40, 9, 3, 7), 16, n=2 * TILE2 + 77), seed=16 + nkeys, nkeys=nkeys, nlibs=nkeys + 3,
            lib_key=tuple((5 * i + 1) % nkeys for i in range(nkeys + 3)), cls_kw=dict(p_pass=0.9, p_proper=0.8))
    # a tile's normal-left and proper counts at 0, 1, 255, 256; the 9-bit field of `where` at 255
    add("tile_counts_0_1_255_256", 2 * TILE2, spread((2, 2, 2, 2, 2, 2, 2, 2), 20), seed=20,
        edit=lambda c: [_all_left_tile(1, 256)(c), _all_left_tile(2, 1)(c), _all_left_tile(3, 255, True)(c), _all_left_tile(5, 0)(c), _all_left_tile(6, 255, True)(c)])
    add("tile_counts_two_keys", 2 * TILE2, spread((2, 2, 2, 2, 2, 2, 2, 2), 21), seed=21,
        edit=lambda c: [_all_left_tile(1, 256)(c), _all_left_tile(2, 1)(c), _all_left_tile(3, 255, True)(c), _all_left_tile(6, 255, True)(c)], **two)
    big = 0x100000000
    add("prefixes_wrap", 3 * TILE2, spread((3, 2, 1, 4, 9, 40, 9, 3, 0, 0, 7, 1), 22), seed=22, chunk_super=2, pre_off=(big - 4, big - 100, big - 300, big - 2),
        chunk_off=(0, big - 77, big - 1, big - 5), **two)
    add("prefixes_wrap_columns_only", 3 * TILE2, spread((30, 2, 1, 4, 9, 40, 9, 3, 0, 0, 70, 1), 23), seed=23, chunk_super=1, pre_off=(big - 20, big - 1, big - 3, big - 2, big - 1),
        chunk_off=(0, big - 7, big - 1, big - 5, 6), nkeys=3, nlibs=3, lib_key=(0, 1, 2))
    for cs in (1, 2, 3):      # chunks 0, 1, 62 and 63 on a few thousand reads
        ns = 64 * cs
        counts = [0] * (ns * SUB)
        for s in (0, 1, cs, 2 * cs - 1, 62 * cs, 63 * cs - 1, 63 * cs, ns - 1):
            counts[s * SUB:(s + 1) * SUB] = [(3, 0, 2, 1), (20, 1, 0, 0)][s % 2]
        for s in range(2, ns, 5):
            counts[s * SUB + s % SUB] += 1
        add("chunk_super_%d" % cs, ns * TILE2, spread(counts, 24 + cs), seed=24 + cs, chunk_super=cs, **two)
    add("chunk_super_3_five_keys", 192 * TILE2 - 300, _random_anom(192 * TILE2 - 300, 28, 0.01), seed=28, chunk_super=3, nkeys=5, nlibs=5, lib_key=(0, 1, 2, 3, 4))
    add("one_chunk", 8 * TILE2, _random_anom(8 * TILE2, 29, 0.01), seed=29, chunk_super=1 << 19)
    dense = spread((100, 100, 100, 100, 50, 50, 50, 50), 30)
    for cap, tag in ((600, "count"), (599, "count_minus_1"), (1, "1"), (607, "count_plus_7"), (300, "inside_a_slice_round"), (0, "0")):
        add("cap_" + tag, 2 * TILE2, dense, seed=30, cap=cap, **two)
    add("cap_records", 2 * TILE2, spread((3, 2, 1, 4, 2, 2, 2, 2), 31), seed=31, cap=9, **two)
    add("check_null", 2 * TILE2, spread((3, 2, 1, 4, 20, 2, 2, 2), 32), seed=32, check=False, **two)
    n = 3 * TILE2 + 40
    sa = spread((3, 2, 1, 4, 20, 2, 2, 2, 1, 1, 1, 1, 5), 33, n=n, pins=(0, TILE - 1, TILE, TILE2 + 7, TILE2 + 8, n - 2, n - 1, 2 * TILE2, 2 * TILE2 - 1))
    add("seg_1", n, sa, seed=33, seg=(0, n), **two)
    add("seg_2_tile_edge", n, sa, seed=33, seg=(0, TILE, n), **two)
    add("seg_3_inside_a_lane", n, sa, seed=33, seg=(0, TILE2 + 8, n - 1, n), **two)
    add("seg_17", n, sa, seed=33, seg=tuple([0] + [TILE2 + 8 + 140 * i for i in range(14)] + [n - 2, n - 1, n]), **two)
    add("seg_3_check_null", n, sa, seed=33, seg=(0, 2 * TILE2, n - 1, n), check=False, **two)
    add("fills_0_1_3_4", 300, _random_anom(300, 34, 0.05), seed=34, fills=((0, 1), (1, 2), (3, 3), (4, 0xFFFFFFFF)))
    add("fills_5_1027_2047_1026", 300, _random_anom(300, 35, 0.05), seed=35, fills=((5, 0), (1027, 0xFFFFFFFF), (2047, 0x01020304), (1026, 9)))
    add("fills_two_workgroups", 5 * TILE2, _random_anom(5 * TILE2, 36, 0.05), seed=36, fills=((2047, 5), (1027, 6), (7, 7), (2048, 8)))
    return tuple(C)


def k2_case_named(name):
    return next(c for c in k2_cases() if c["name"] == name)


SHRINKING = ("n_4097_dense", "n_1025_sparse", "n_257_dense", "n_17_sparse")

STRIDED_SUPER = K2_GRID_CAP * 4 + 5      # launch_k2's grid cap: every wave takes two super tiles, some a third
STRIDED_N = STRIDED_SUPER * TILE2


def strided_case():
    """33.6 M reads in 9 chunks of 4,096 super tiles: dense zero columns, a few hundred anomalous reads in the first, the 32,768th, the
    32,769th and the last super tile (not cached: 600 MB)"""
    n = STRIDED_N
    rng = np.random.default_rng(99)
    at = []
    for s, k in ((0, 40), (K2_GRID_CAP * 4 - 1, 150), (K2_GRID_CAP * 4, 30), (STRIDED_SUPER - 1, 90)):
        at.append(s * TILE2 + np.sort(rng.choice(TILE2, k, replace=False)))
    at = np.concatenate(at)
    d = dict(tid=np.zeros(n, np.int32), pos=np.zeros(n, np.int32), isize=np.zeros(n, np.int32), flag=np.zeros(n, np.uint16), qlen=np.zeros(n, np.uint16),
             lib=np.zeros(n, np.uint8), key=np.zeros(n, np.uint64), check=np.zeros(n, np.uint64))
    small = columns(len(at), 98)
    for k in ("tid", "pos", "isize", "flag", "qlen", "key", "check"):
        d[k][at] = small[k]
    cls = np.zeros(n, np.uint8)
    cls[::3] = NORMAL_FR | 0x10 | 0x20 | 0x40
    cls[1::3] = NORMAL_RF | 0x10 | 0x20
    cls[at] = 8 | 0x10
    c = dict(d, name="strided", n=n, nkeys=1, nlibs=1, lib_key=np.zeros(1, np.int32), chunk_super=ROUND, seg=None, fills=((0, 0),) * 4, has_check=True,
             ntiles=n // TILE, cls=cls, tstride=row16(n // TILE), nsuper=STRIDED_SUPER, pre_off=np.zeros(3, np.uint32), chunk_off=np.zeros(3, np.uint32),
             count=len(at), cap=len(at))
    return c


K2_REFERENCE_SLIPS = ("pk_exclusive", "normal_rf_anomalous", "pass_ignored", "isize_no_abs", "rev_from_0x20", "lib_not_clamped", "cap_le",
                      "pk_stride_by_count")
K2_MODEL_SLIPS = ("nn_inclusive", "tile_key_ignored", "e_wrong_column", "before_off_by_a_tile", "mark_first_tile_only", "slice_at_255", "chunk_sum_inclusive",
                  "chunk_super_on_tiles", "segment_lt")
FILL_SLIPS = ("fill_tail_dropped",)
# What no input can show: nn taken inclusive of the read itself (k2_reference's "nn_inclusive").  K1 sets 0x40 only on a normal read, so an
# anomalous read never counts for nn; the slip that can show is the lane's scan taken inclusive (k2_model's "nn_inclusive": the counts of
# the lane's own 16 reads added in front of them).
INVISIBLE_SLIPS = ("nn_inclusive",)


# ---- the finalisation -----------------------------------------------------------------------------------------------------------------------------------

def wrap64(v):
    v &= (1 << 64) - 1
    return v - (1 << 64) if v >> 63 else v


def mono_combine(a, b, slip=None):
    """(ft, fp, lt, lp, sum) tuples of Python ints; ft == -1: absent"""
    if slip == "fold_wrong_order":
        a, b = b, a
    if a[0] == -1:
        return b
    if b[0] == -1:
        return a
    return (a[0], a[1], b[2], b[3], wrap64(a[4] + b[4] + ((b[1] - a[3]) if a[2] == b[0] else 0)))


ABSENT = (-1, 0, 0, 0, 0)


def fin_case(name, ntiles, nkeys=1, nlibs=1, nbams=1, seed=1, chunk_super=ROUND, nchunk=None, nfold=1, w0=1000, cn_lib=0, na_cap=0, stamp=7, tot_max=257,
             lib_key=None, absent=(), mono="random", cnt=None, edit=None):
    rng = np.random.default_rng([seed, ntiles, nkeys])
    ncols, ts = 2 + nkeys, row16(ntiles)
    nsuper = (ntiles + SUB - 1) // SUB
    tt = np.zeros((ncols, ts), np.uint32)
    tt[:, :ntiles] = rng.integers(0, tot_max, (ncols, ntiles), dtype=np.uint64).astype(np.uint32)
    tm = np.zeros((nbams, ts), MONO)
    tm.view(np.uint8)[:] = 0xFF
    if ntiles:
        present = rng.random((nbams, ntiles)) < 0.8
        for b, lo, hi in absent:
            present[b, lo:hi] = False
        # tiles of a chromosome in a row, positions rising; a.lt == b.ft mostly, and not where the chromosome changes
        tid = np.cumsum(rng.random(ntiles) < 0.05).astype(np.int32)
        first = np.sort(rng.integers(0, 1 << 20, ntiles)).astype(np.int32)
        for b in range(nbams):
            r = tm[b, :ntiles]
            p = present[b]
            if mono == "wide":      # sums that need 64 bits: every step spans nearly the whole positive range
                fp = np.where(np.arange(ntiles) % 2 == 0, -(1 << 31) + 5, (1 << 31) - 7).astype(np.int64)
                lp = -fp - 1
                tid_b = np.zeros(ntiles, np.int32)
            else:
                fp, lp, tid_b = first.astype(np.int64) + b, first.astype(np.int64) + b + rng.integers(0, 5000, ntiles), tid
            r["ft"][p], r["fp"][p], r["lp"][p] = tid_b[p], fp[p], lp[p]
            cross = p & (rng.random(ntiles) < 0.03)      # a tile that a chromosome boundary runs through
            r["lt"][p] = tid_b[p] + cross[p]
            r["sum"][p] = (lp - fp)[p] * np.where(cross[p], 0, 1)
    ncnt = nlibs * NUM_FLAGS + nlibs + nbams
    blk = rng.integers(0, 1000, (CNT_COPIES, ncnt), dtype=np.uint64).astype(np.uint32)
    blk[rng.random((CNT_COPIES, ncnt)) < 0.5] = 0
    if cnt:
        for i, v in cnt.items():      # counter i in all: v
            blk[:, i] = 0
            blk[:, i] = np.asarray([v // CNT_COPIES + (1 if q < v % CNT_COPIES else 0) for q in range(CNT_COPIES)], np.uint32)
    if lib_key is None:
        lib_key = [i % (nkeys if cn_lib else min(nkeys, nbams)) for i in range(nlibs)]
    c = dict(name=name, ntiles=ntiles, tstride=ts, nsuper=nsuper, nkeys=nkeys, nlibs=nlibs, nbams=nbams, ncols=ncols, ncnt=ncnt, chunk_super=chunk_super,
             nchunk=max(1, (nsuper + chunk_super - 1) // chunk_super) if nchunk is None else nchunk, nfold=nfold, w0=w0, cn_lib=cn_lib, na_cap=na_cap, stamp=stamp,
             tile_tot=tt, tile_mono=tm, blk_cnt=blk, lib_key=np.asarray(lib_key, np.int32))
    if edit:
        edit(c)
    return c


def fin_reference(c, slip=None, second_level=True):
    """everything finalize_kernel and finalize2_body write, 0xA5 where they write nothing.  Where a fold comes out absent (ft == -1) only ft
    is stated: the kernel leaves the record's other fields as they fall."""
    nt, ts, ncols, cs, nchunk, nfold = c["ntiles"], c["tstride"], c["ncols"], c["chunk_super"], c["nchunk"], c["nfold"]
    tt = c["tile_tot"]
    pre = np.full((ncols, ts), FILL, np.uint32)
    ctot = np.full((ncols, MAX_CHUNKS), FILL, np.uint32)
    count_host = np.full(MAX_CHUNKS, FILL64, np.uint64)
    st = tt.reshape(ncols, ts // SUB, SUB).sum(axis=2, dtype=np.uint32)      # totals per super tile: the row is zero behind ntiles
    for g in range(nchunk):
        tile_lo, tile_hi = g * cs * SUB, min(nt, (g + 1) * cs * SUB)
        row_hi = min(ts, (g + 1) * cs * SUB)
        ctot[:, g] = 0
        if tile_lo < tile_hi:
            rounds = (tile_hi - tile_lo + ROUND * SUB - 1) // (ROUND * SUB)
            s_lo, s_hi = tile_lo // SUB, min(row_hi, tile_lo + rounds * ROUND * SUB) // SUB      # (the entries behind the last tile get the running total)
            seg = st[:, s_lo:s_hi]
            inc = np.cumsum(seg, axis=1, dtype=np.uint32)
            pre[:, s_lo:s_hi] = inc - seg
            ctot[:, g] = inc[:, -1]
        count_host[g] = (c["stamp"] << 32) | int(ctot[COL_ANOM, g])
    fold = np.zeros((c["nbams"], nfold), MONO)
    chunk = (nt + nfold - 1) // nfold
    for b in range(c["nbams"]):
        rows = c["tile_mono"][b, :nt].tolist()      # (tuples of Python ints)
        for fb in range(nfold):
            acc = ABSENT
            for r in rows[min(fb * chunk, nt):min(fb * chunk + chunk, nt)]:
                if r[0] != -1:
                    acc = mono_combine(acc, r, slip)
            fold[b, fb] = acc
    o = dict(tile_pre=pre, chunk_tot=ctot, count_host=count_host, fold=fold)
    if second_level:
        o.update(fin2_reference(c, ctot, fold, slip))
    else:
        o.update(fin2_blank(c))
    return o


def fin2_blank(c):
    return dict(chunk_base=np.full((c["ncols"], MAX_CHUNKS), FILL, np.uint32), cnt=np.full(c["ncnt"], FILL, np.uint32), cnt_host=np.full(c["ncnt"], FILL, np.uint32),
                p1=np.full(P1_WORDS, FILL, np.uint32), p1_host=np.full(P1_WORDS, FILL, np.uint32), density=np.full(64, FILL, np.uint32).view(np.float32),
                flag=np.full(16, FILL, np.uint32))


def fin2_reference(c, ctot, fold, slip=None):
    ncols, nchunk, nlibs, nbams, nkeys = c["ncols"], c["nchunk"], c["nlibs"], c["nbams"], c["nkeys"]
    o = fin2_blank(c)
    cnt = c["blk_cnt"].sum(axis=0, dtype=np.uint32)
    o["cnt"][:] = cnt
    o["cnt_host"][:] = cnt
    v = np.where(np.arange(MAX_CHUNKS)[None, :] < nchunk, ctot, 0).astype(np.uint32)
    inc = np.cumsum(v, axis=1, dtype=np.uint32)
    o["chunk_base"][:] = inc - v
    col = inc[:, -1]
    ref = []
    for b in range(nbams):
        acc = ABSENT
        for fb in range(c["nfold"]):
            r = fold[b, fb]
            if r["ft"] != -1:
                acc = mono_combine(acc, (int(r["ft"]), int(r["fp"]), int(r["lt"]), int(r["lp"]), int(r["sum"])), slip)
        ref.append(0 if acc[0] == -1 else acc[4] & ((1 << 64) - 1))
    covered = 0
    for r in ref:      # size_t against uint32, as the reference's comparison
        if covered < r:
            covered = r & M32
    W = c["w0"]
    for i in range(nlibs):
        nd = (int(cnt[i * NUM_FLAGS + F_LARGE]) + int(cnt[i * NUM_FLAGS + F_SMALL])) & M32
        nd -= (nd >> 31) << 32      # (int)
        if nd > 0:
            q = (np.float64(covered) / np.float64(nd)) if slip == "w_double_division" else (np.float32(covered) / np.float32(nd))
            tmp = int(q)
        else:
            tmp = 50
        W = min(W, tmp)
    dens = o["density"]
    dens[:nkeys] = np.float32(0.000001)
    lib_cnt, bam_cnt = cnt[nlibs * NUM_FLAGS:nlibs * NUM_FLAGS + nlibs], cnt[nlibs * NUM_FLAGS + nlibs:]
    with np.errstate(divide="ignore", invalid="ignore"):
        for i in range(nlibs):
            key = int(c["lib_key"][i])
            d = np.float32(0.000001)
            if c["cn_lib"]:
                if lib_cnt[i] != 0:
                    d = np.float32(lib_cnt[i]) / np.float32(covered)
            else:
                d = np.float32(bam_cnt[key]) / np.float32(covered)
            dens[key] = d
    n_anom = int(col[COL_ANOM])
    p1 = o["p1"]
    p1[0], p1[1] = covered, W & M32
    p1[2:2 + ncols] = col
    for b, r in enumerate(ref):
        p1[P1_REF_WORD + 2 * b], p1[P1_REF_WORD + 2 * b + 1] = r & M32, r >> 32
    h = o["p1_host"]
    h[:P1_REF_WORD + 2 * nbams] = p1[:P1_REF_WORD + 2 * nbams]
    h[2 + ncols:P1_REF_WORD] = 0
    if c["na_cap"] and n_anom > c["na_cap"]:
        p1[2] = 0      # the device's copy only
    o["flag"][0] = c["stamp"]
    o["covered"], o["W"], o["n_anom"] = covered, W, n_anom
    return o


FIN_FIELDS = ("tile_pre", "chunk_tot", "count_host", "chunk_base", "cnt", "cnt_host", "p1", "p1_host", "density", "flag")


def fin_differs(a, b):
    for f in FIN_FIELDS:
        if not np.array_equal(np.asarray(a[f]).view(np.uint8), np.asarray(b[f]).view(np.uint8)):
            return f
    fa, fb = a["fold"], b["fold"]
    if not np.array_equal(fa["ft"], fb["ft"]):
        return "fold.ft"
    here = fa["ft"] != -1
    if not np.array_equal(fa[here], fb[here]):
        return "fold"
    return None


def _set_cnt(lib, large, small, lib_cnt=None, nlibs=1):
    d = {lib * NUM_FLAGS + F_LARGE: large, lib * NUM_FLAGS + F_SMALL: small}
    if lib_cnt is not None:
        d[nlibs * NUM_FLAGS + lib] = lib_cnt
    return d


@functools.lru_cache(maxsize=1)
def fin_cases():
    C = []
    add = lambda *a, **k: C.append(fin_case(*a, **k))
    for nt in (0, 1, 3, 4, 5, 16380, 16383, 16384, 16385):      # (4,095, 4,096, 4,096 and 4,097 super tiles)
        add("ntiles_%d" % nt, nt, seed=nt + 1, nbams=2, nfold=2 if nt > 1 else 1, nkeys=2, nlibs=2)
    add("ntiles_65537", 65537, seed=40, nfold=64, nbams=2, nkeys=2, nlibs=2, lib_key=(0, 1), absent=((1, 0, 1), (0, 65536, 65537), (1, 1025 * 3, 1025 * 4)))
    add("chunks_64", 64 * 16384, seed=41, nfold=64, tot_max=1 << 12)
    add("chunks_64_one_tile_less", 64 * 16384 - 1, seed=42, nfold=64, tot_max=1 << 12)
    add("chunks_64_mostly_empty", 16385, seed=43, nchunk=64, nfold=2)
    add("chunks_of_two_rounds", 3 * 16384 + 9, seed=44, chunk_super=2 * ROUND, nfold=64)
    add("columns_4_wrap", 4099, seed=45, nkeys=2, tot_max=1 << 32, nfold=2, nlibs=2)
    add("columns_62", 4099, seed=46, nkeys=60, nlibs=60, nbams=1, cn_lib=1, nfold=64, tot_max=1 << 31)
    add("nfold_64_per_1", 64, seed=47, nfold=64, nbams=3, absent=((2, 0, 64), (1, 0, 1), (1, 63, 64)))
    add("nfold_1_per_2", 1025, seed=48, nfold=1, nbams=3, absent=((1, 0, 1025),))
    add("nfold_2_per_2", 2050, seed=49, nfold=2, nbams=2, absent=((1, 0, 1025),))
    add("sums_of_64_bits", 3000, seed=50, nfold=3, nbams=2, mono="wide")
    add("libraries_4", 100, seed=51, nlibs=4, nbams=2, nkeys=2, nfold=1)
    add("libraries_255", 100, seed=52, nlibs=255, nbams=4, nkeys=4, nfold=1)
    add("libraries_255_by_library", 100, seed=53, nlibs=255, nbams=4, nkeys=60, cn_lib=1, nfold=1)
    add("w_no_deletion_reads_large_w0", 100, seed=54, w0=1000, cnt=_set_cnt(0, 0, 0))
    add("w_no_deletion_reads_small_w0", 100, seed=54, w0=7, cnt=_set_cnt(0, 0, 0))
    # quotients that float32 rounds across an integer: covered is set by one tile's record (see _covered)
    for k, (cov, nd) in enumerate(((16777217, 1), (2147483520, 3), (4294967040, 65535), (100000007, 9), (33554431, 3), (3000000001, 30001))):
        add("w_quotient_%d" % k, 8, seed=60 + k, w0=1 << 30, cnt=_set_cnt(0, nd - nd // 2, nd // 2), edit=_covered(cov))
    add("density_by_library", 100, seed=70, nlibs=4, nbams=2, nkeys=4, cn_lib=1, cnt=_set_cnt(2, 5, 5, lib_cnt=0, nlibs=4))
    add("covered_0", 100, seed=71, nlibs=2, nbams=2, nkeys=2, absent=((0, 0, 100), (1, 0, 100)),
        edit=lambda c: c["blk_cnt"].__setitem__((slice(None), slice(2 * NUM_FLAGS + 2, None)), np.uint32(3)))
    for d in (-1, 0, 1):
        add("na_cap_count%+d" % d, 100, seed=72, edit=lambda c, d=d: c.update(na_cap=int(c["tile_tot"][COL_ANOM].sum()) + d))
    return tuple(C)


def _covered(cov):
    """edit: one source file whose reference length comes out as cov (two tiles of one chromosome)"""
    def edit(c):
        tm = c["tile_mono"]
        tm.view(np.uint8)[:] = 0xFF
        lo = -(1 << 31)
        tm[0, 0] = (0, lo, 0, lo + 5, 5)
        tm[0, 3] = (0, lo + 5 + 1000, 0, lo + cov, cov - 1005)
    return edit


def fin_case_named(name):
    return next(c for c in fin_cases() if c["name"] == name)


FIN_SLIPS = ("fold_wrong_order", "w_double_division")
