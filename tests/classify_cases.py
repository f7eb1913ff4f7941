"""Truth table, layouts, plain restatement and dispatch model of tests/test_gpu_classify.py, which holds K1's three tile bodies
(csrc/k1_classify.hip: classify_uniform_tile, classify_mixed_tile, the general body around classify_read) to the oracle.  Nothing here
needs a GPU: tests/test_classify_cases.py checks the restatement against the oracle, the layouts against the tiles they are there for,
and the table against slips of the classifier.

A ROW of the table is (SAM flag, mpos - pos, mtid, isize, mapq).  A row INSTANCE is a row with a library; it becomes two records 20 bp
apart (store() says which records share a read name).  A LAYOUT deals row instances to libraries and files so that its tiles go to one of K1's bodies; an ORDER
arranges them: "table" (flags outermost: passing rows cluster, tiles with none and with far more than kStashCap anomalous reads),
"spread" (eight passable rows in every tile of 128: never more than kStashCap anomalous reads) and "perm" (a seeded permutation)."""
import functools

import numpy as np

# ---- the kernel's constants -----------------------------------------------------------------------------------------------------
TILE = 256          # kTile: one wave64, lane l owns the reads [4l, 4l + 4)
ROWS_PER_TILE = TILE // 2
STASH_CAP = 16      # kStashCap
STASH_KEYS = 2      # kStashKeys: more counter keys and K1 leaves no ready-made records at all
MIXED_LIBS = 8      # kMixedLibs
UNIFORM, MIXED, GENERAL = 0, 1, 2
BODIES = ("uniform", "mixed", "general")

NA, ARP_FF, ARP_LARGE, ARP_SMALL, ARP_RF, ARP_RR, NORMAL_FR, NORMAL_RF, ARP_CTX, MATE_UNMAPPED, UNMAPPED = range(11)
CLS_PASS, CLS_PROPER, CLS_NORMAL_LEFT = 0x10, 0x20, 0x40

# ---- libraries: (name, lower, upper, mapqual or None).  Every side has an integer-valued and a fractional cutoff, and the same row
# changes class from library to library; libD's upper cutoff is 2^24, where int -> float32 first rounds --------------------------------
LIB_A = ("libA", 310.00, 490.50, None)
LIB_B = ("libB", 200.25, 350.00, 10)
LIB_C = ("libC", 100.00, 491.00, None)
LIB_D = ("libD", 99.50, 16777216.00, None)
LIBS4 = (LIB_A, LIB_B, LIB_C, LIB_D)
# (five more for the layouts at and beyond kMixedLibs: cutoffs and qualities of the table's own values)
LIBS9 = LIBS4 + (("libE", 350.00, 490.00, None), ("libF", 101.00, 200.00, 10), ("libG", 200.25, 16777216.00, None),
                 ("libH", 490.50, 491.00, 10), ("libI", 0.00, 100.00, None))
DEFAULT_MIN_MAPQ = 35
MAX_SD_DEFAULT = 1000000000
SMALL_MAX_SD = 491          # a -m that is a table value (492 is one too)
SMALL_MIN_MAPQ = 10         # a -q that is a table value

FLAG_BITS = (0x1, 0x2, 0x4, 0x8, 0x10, 0x20, 0x400)   # the bits the classifier reads
GEOMETRY = [(d, other) for d in (-200, 0, 200) for other in (0, 1)]   # (mpos - pos, mate on another chromosome)
ISIZE_ABS = sorted({309, 310, 311, 490, 491, 200, 201, 349, 350, 351, 99, 100, 101, 492,                 # c - 1, c, c + 1 / floor, ceiling
                    (1 << 24) - 1, 1 << 24, (1 << 24) + 1, (1 << 24) + 2,                                 # int -> float32 at libD's upper cutoff
                    MAX_SD_DEFAULT, MAX_SD_DEFAULT + 1, (1 << 31) - 1})                                   # (INT_MIN is left out: abs has no value there)
MAPQS = [DEFAULT_MIN_MAPQ - 1, DEFAULT_MIN_MAPQ, DEFAULT_MIN_MAPQ + 1, 9, 10, 11, 0, 255]
MID_ISIZE, MID_MAPQ = 400, 60
EXTRA_BITS = (0x100, 0x200, 0x800, 0xB00)   # secondary, QC fail, supplementary: no classifier reads them


def _table():
    v = [(s * a, MID_MAPQ) for a in ISIZE_ABS for s in (1, -1)] + [(MID_ISIZE, q) for q in MAPQS]
    rows = []
    # (the eight flag words that let a read pass come first, the one that is anomalous whatever else holds last of them: their rows fill
    # whole tiles, so that in table order every passing row lies in a tile with far more than kStashCap anomalous reads)
    passable = [m for m in range(128) if (m & 0b1001101) == 1]
    for m in passable[1:] + passable[:1] + [m for m in range(128) if m not in passable]:
        f = sum(b for k, b in enumerate(FLAG_BITS) if (m >> k) & 1) | (0x40 if m % 2 == 0 else 0x80)
        for d, other in GEOMETRY:
            for isz, q in v:
                rows.append((f, d, other, isz, q, -1))
    base_of = {}
    for i, r in enumerate(rows):
        base_of.setdefault(r[:5], i)
    for x in EXTRA_BITS:      # 4 x 32 rows that must come out as their base rows do
        for m in range(128):
            f = sum(b for k, b in enumerate(FLAG_BITS) if (m >> k) & 1) | (0x40 if m % 2 == 0 else 0x80)
            if (f & 0x40D) != 0x1:
                continue
            for d, other in ((200, 0), (0, 1), (-200, 0), (0, 0)):
                rows.append((f | x, d, other, MID_ISIZE, 255, base_of[(f, d, other, MID_ISIZE, 255)]))
    t = np.array(rows, dtype=np.int64)
    t.setflags(write=False)
    return t


TABLE = _table()                     # columns: flag, mpos - pos, mtid, isize, mapq, base row (-1: none)
T = len(TABLE)
PASSABLE = np.flatnonzero((TABLE[:, 0] & 0x40D) == 0x1)      # rows whose flag word lets a read pass at all
NOT_PASSABLE = np.flatnonzero((TABLE[:, 0] & 0x40D) != 0x1)
assert T % ROWS_PER_TILE == 0 and len(PASSABLE) % 8 == 0

OPTION_SETS = [dict(), dict(illumina_long_insert=1), dict(transchr_rearrange=1), dict(max_sd=SMALL_MAX_SD), dict(min_map_qual=SMALL_MIN_MAPQ),
               dict(cn_lib=1, print_af=1)]

# ---- layouts --------------------------------------------------------------------------------------------------------------------
# libs: the configuration; files: the file of each library; deal: how a row instance gets its library -- "row": dealt round the rows
# (every tile holds all of them), "tile": one library per tile, "bodies": tile k is uniform, mixed (libA / libB) or general in turn

LAYOUTS = {
    "one-library": dict(libs=(LIB_A,), files=(0,), deal="row", copies=2),
    "uniform": dict(libs=LIBS4, files=(0, 0, 0, 0), deal="tile", copies=8),
    "mixed": dict(libs=LIBS4, files=(0, 0, 0, 0), deal="row", copies=8),
    "mixed-two-keys": dict(libs=(LIB_A, LIB_B), files=(0, 0), deal="row", copies=4),      # -a: two counter keys, the slots K2 would read marked
    "eight-libraries": dict(libs=LIBS9[:8], files=(0,) * 8, deal="row", copies=2),
    "nine-libraries": dict(libs=LIBS9, files=(0,) * 9, deal="row", copies=2),
    "two-files": dict(libs=LIBS4, files=(0, 0, 1, 1), deal="row", copies=8),
    "three-bodies": dict(libs=LIBS4, files=(0, 0, 1, 1), deal="bodies", copies=2),
    "tail-1": dict(libs=LIBS4, files=(0, 0, 0, 0), deal="row", copies=2, tail=1),
    "tail-129": dict(libs=LIBS4, files=(0, 0, 0, 0), deal="row", copies=2, tail=129),
    "tail-255": dict(libs=LIBS4, files=(0, 0, 0, 0), deal="row", copies=2, tail=255),
}
ORDERS = ("table", "spread", "perm")


def orders_of(layout, opts=None):
    """the orders a layout is run in under an option set: a ragged end behind the spread order adds nothing, and under -t the spread
    order's lone pairs of inter-chromosomal reads make regions and no SV row"""
    if layout.startswith("tail") or (opts or {}).get("transchr_rearrange"):
        return ("table", "perm")
    return ORDERS


BODY_OF = {"one-library": UNIFORM, "uniform": UNIFORM, "mixed": MIXED, "mixed-two-keys": MIXED, "eight-libraries": MIXED,
           "nine-libraries": GENERAL, "two-files": GENERAL}   # the body of every full tile of the layout


def config_text(spec):
    out = ""
    for (name, lower, upper, mq), f in zip(spec["libs"], spec["files"]):
        out += "readgroup:rg%s\tplatform:illumina\tmap:file%d.bam\treadlen:100.00\tlib:%s\tnum:10001\tlower:%.2f\tupper:%.2f\tmean:400.00\tstd:30.00" % (
            name, f, name, lower, upper)
        out += ("\tmapqual:%d\n" % mq) if mq is not None else "\n"
    return out


def lib_params(spec, opts=None):
    """[(lower, upper, mapping-quality cutoff resolved against -q)] as float32 / int"""
    q = (opts or {}).get("min_map_qual", DEFAULT_MIN_MAPQ)
    return [(np.float32(lo), np.float32(up), q if mq is None else mq) for _, lo, up, mq in spec["libs"]]


def _libs_of(spec, pos, dealt):
    """library of the row instance at row position pos: dealt is what "row" dealing gives it"""
    nl = len(spec["libs"])
    tile = pos // ROWS_PER_TILE
    if spec["deal"] == "row":
        return dealt % nl
    if spec["deal"] == "tile":
        return tile % nl
    kind = tile % 3
    return np.where(kind == 0, (tile // 3) % nl, np.where(kind == 1, dealt % 2, dealt % nl))


def _sequence(spec, order, seed):
    """row and library of every row instance, in store order"""
    nl = len(spec["libs"])
    rng = np.random.default_rng([seed, len(spec["libs"]), spec["copies"]])
    if order == "spread":
        # every tile of 128 row instances: eight passable ones at lanes that move from tile to tile, the rest from the others in turn
        copies = min(nl, 4)
        P, N = rng.permutation(PASSABLE), rng.permutation(NOT_PASSABLE)
        ntile = copies * len(P) // 8
        k = np.arange(ntile)[:, None]
        u = np.arange(8)[None, :]
        at = (k * ROWS_PER_TILE + 16 * u + (k + 3 * u) % 16).ravel()
        rows = np.empty(ntile * ROWS_PER_TILE, np.int64)
        dealt = np.empty_like(rows)
        plain = np.zeros(len(rows), bool)
        plain[at] = True
        m = np.arange(len(at))
        rows[at] = P[m % len(P)]
        rest = np.arange(len(rows) - len(at))
        rows[~plain] = N[rest % len(N)]
        if spec["deal"] == "tile":      # a tile's library goes round with the copy, so that every row meets every library
            first = 8 * k.ravel()
            libs = np.repeat(((first % len(P)) // 8 + first // len(P)) % nl, ROWS_PER_TILE)
        else:
            dealt[at] = m % len(P) + m // len(P)
            dealt[~plain] = rest
            libs = _libs_of(spec, np.arange(len(rows)), dealt)
    else:
        rows, dealt = [], []
        for c in range(spec["copies"]):
            j = np.arange(T)
            if c % 2:     # the other slot pair and the other half of the wave: row q of a tile goes to ((q + 64) % 128) ^ 1
                q = j % ROWS_PER_TILE
                at = (j - q) + (((q + ROWS_PER_TILE // 2) % ROWS_PER_TILE) ^ 1)
                inv = np.empty(T, np.int64)
                inv[at] = j
                j = inv
            rows.append(j)
            dealt.append(j + c // 2)
        rows, dealt = np.concatenate(rows), np.concatenate(dealt)
        if order == "perm":
            p = rng.permutation(len(rows))
            rows, dealt = rows[p], dealt[p]
        if spec["deal"] == "tile":     # (table order: tile b of a copy holds the rows [128 b, 128 b + 128) in either arrangement)
            pos = np.arange(len(rows))
            libs = ((pos // ROWS_PER_TILE) % (T // ROWS_PER_TILE) + (pos // T) // 2) % nl if order == "table" else (pos // ROWS_PER_TILE) % nl
        else:
            libs = _libs_of(spec, np.arange(len(rows)), dealt)
    return rows, np.asarray(libs, np.int64)


@functools.lru_cache(maxsize=4)
def store(layout, order, seed=7):
    """the position-sorted store of a layout in the batch layout of include/bdx.h, with `row` (index into TABLE) beside it; read-only"""
    spec = LAYOUTS[layout]
    rows, libs = _sequence(spec, order, seed)
    rec_row, rec_lib = np.repeat(rows, 2), np.repeat(libs, 2)
    tail = spec.get("tail", 0)
    if tail:     # a whole number of tiles and `tail` more records: passable rows, so that the ragged lanes have something to say
        extra = PASSABLE[(np.arange(tail) * 37) % len(PASSABLE)]
        rec_row = np.concatenate([rec_row, extra])
        rec_lib = np.concatenate([rec_lib, np.arange(tail) % len(spec["libs"])])
    n = len(rec_row)
    assert (n - tail) % TILE == 0
    # Read names: the passable row instances are paired in store order, and the first records of a pair's two instances share one name,
    # their second records another.  Where the two lie further apart than the window -- the spread order throughout, the permuted one
    # mostly -- the pair links two regions, and the SV row between them has copy numbers: the only place where the proper-read counts of
    # the ready-made records show.  Every other instance has one name for its two records (they never pass).
    ninst = len(rows)
    can = np.isin(rows, PASSABLE)
    name = np.repeat(np.arange(ninst, dtype=np.int64), 2)
    pair = (np.cumsum(can) - 1) // 2
    e = np.tile(np.arange(2, dtype=np.int64), ninst)
    name = np.where(np.repeat(can, 2), ninst + 2 * np.repeat(pair, 2) + e, name)
    name = np.concatenate([name, 3 * ninst + np.arange(tail, dtype=np.int64)])
    t = TABLE[rec_row]
    pos = 1000 + 20 * np.arange(n, dtype=np.int64)
    d = dict(tid=np.zeros(n, np.int32), pos=pos.astype(np.int32), mtid=t[:, 2].astype(np.int32), mpos=(pos + t[:, 1]).astype(np.int32),
             isize=t[:, 3].astype(np.int32), flag=t[:, 0].astype(np.uint16), qlen=np.full(n, 100, np.int32), bdqual=t[:, 4].astype(np.uint8),
             lib=rec_lib.astype(np.int32), bam=np.asarray(spec["files"], np.uint8)[rec_lib],
             name_id=(name + 1).astype(np.uint64), row=rec_row)
    for a in d.values():
        a.setflags(write=False)
    return d


def nbams(spec):
    return max(spec["files"]) + 1


# ---- K1's dispatch, read off the kernel -----------------------------------------------------------------------------------------

def tile_body(d, nlibs, nbams):
    """the body every tile of the store goes to.  Uniform: the tile is full and every library and file byte equals lane 0's; mixed:
    otherwise, at most kMixedLibs libraries, full, one file; general: everything else.  (With one library / one file the column is not
    read and every index counts as 0; the bytes are compared as they are stored, out of range included.)"""
    n = len(d["tid"])
    ntile = (n + TILE - 1) // TILE
    lib = np.zeros(ntile * TILE, np.int64)
    bam = np.zeros(ntile * TILE, np.int64)
    if nlibs > 1:
        lib[:n] = np.asarray(d["lib"]).astype(np.int64) & 0xFF
    if nbams > 1:
        bam[:n] = np.asarray(d["bam"]).astype(np.int64) & 0xFF
    lib, bam = lib.reshape(ntile, TILE), bam.reshape(ntile, TILE)
    full = (np.arange(ntile) + 1) * TILE <= n
    one_lib = (lib == lib[:, :1]).all(axis=1)
    one_file = (bam == bam[:, :1]).all(axis=1)
    return np.where(full & one_lib & one_file, UNIFORM, np.where(full & one_file & (nlibs <= MIXED_LIBS), MIXED, GENERAL))


# ---- the plain restatement --------------------------------------------------------------------------------------------------------

SLIPS = {   # name -> the option set under which the slip must show
    "lower_le": {}, "upper_ge": {}, "pos_le_mpos": {}, "unmapped_order": {}, "pass_without_0x8": {}, "mapq_ge": {},
    "max_sd_lt": dict(max_sd=SMALL_MAX_SD), "max_sd_on_ctx": dict(max_sd=SMALL_MAX_SD), "rr_fold_when_not_passing": {},
    "proper_without_0x400": {}, "compare_as_double": {}, "compare_as_int": {},
    "no_remap_2": dict(illumina_long_insert=1), "no_remap_3": dict(illumina_long_insert=1),
    "hist_before_remap": dict(illumina_long_insert=1), "t_drops_ctx": dict(transchr_rearrange=1),
}
LAYOUT_SLIPS = ("mapq_of_slot_0", "lib_of_slot_0")
# What no input can show: the first -l line (NORMAL_RF above the upper cutoff -> ARP_RF) reads a class that only the second line makes,
# from reads below the upper cutoff; the classifier itself never says NORMAL_RF.  The line is dead in the reference, the oracle and K1 alike.
INVISIBLE_SLIPS = {"no_remap_1": dict(illumina_long_insert=1)}


def lay_out_slip(d, slip):
    """the store as a body would see it that takes slot 0's byte of the packed word for all four slots of a lane"""
    out = dict(d)
    i = np.arange(len(d["tid"]))
    first = i - i % 4
    key = {"mapq_of_slot_0": "bdqual", "lib_of_slot_0": "lib"}[slip]
    out[key] = np.asarray(d[key])[first]
    return out


def restate(d, libs, opts=None, nbams=1, slip=None):
    """io/IlluminaPEReadClassifier.cpp:13-101, the pass-1 body of io/BamSummary.cpp:68-114 and the filter chain, -l remaps and RR -> FF
    fold of BreakDancer.cpp:155-207 as array arithmetic.  libs: [(lower, upper, resolved mapping-quality cutoff)]; an index out of
    range counts as 0.  -> cls (flag | pass << 4 | proper << 5 | normal-and-leftmost << 6), lib_read_count, bam_read_count, flag_hist
    as the oracle returns them, and raw (the classifier's flag before any filter)"""
    opts = opts or {}
    opt_t, opt_l = bool(opts.get("transchr_rearrange")), bool(opts.get("illumina_long_insert"))
    max_sd = opts.get("max_sd", MAX_SD_DEFAULT)
    nl = len(libs)
    # (narrow types where they hold the value: the full-size tests restate 116 M records)
    sam = np.asarray(d["flag"]).astype(np.int32)
    tid, mtid, pos, mpos = (np.asarray(d[k]) for k in ("tid", "mtid", "pos", "mpos"))
    mapq = np.asarray(d["mapq"] if "mapq" in d else d["bdqual"]).astype(np.int32)
    ai = np.abs(np.asarray(d["isize"]).astype(np.int64))
    lib = np.asarray(d["lib"]).astype(np.int32) if nl > 1 else np.zeros(len(sam), np.int32)
    lib[lib >= nl] = 0
    bam = np.asarray(d["bam"]).astype(np.int32) if nbams > 1 and "bam" in d else np.zeros(len(sam), np.int32)
    bam[bam >= nbams] = 0
    lo = np.array([l[0] for l in libs], np.float32)[lib]
    up = np.array([l[1] for l in libs], np.float32)[lib]
    minq = np.array([l[2] for l in libs], np.int32)[lib]
    fi = ai.astype(np.float32)                      # the reference compares the int against the float cutoffs
    if slip == "compare_as_double":
        fi, lo, up = ai.astype(np.float64), lo.astype(np.float64), up.astype(np.float64)
    elif slip == "compare_as_int":
        lo, up = np.floor(lo.astype(np.float64)), np.floor(up.astype(np.float64))
        fi = ai.astype(np.float64)
    small = fi <= lo if slip == "lower_le" else fi < lo
    large = fi >= up if slip == "upper_ge" else fi > up
    left = pos <= mpos if slip == "pos_le_mpos" else pos < mpos
    rev, mrev = (sam & 0x10) != 0, (sam & 0x20) != 0
    ctx = tid != mtid
    f = np.full(len(sam), NORMAL_FR, np.uint8)
    f[small] = ARP_SMALL
    f[large] = ARP_LARGE
    f[left == rev] = ARP_RF
    f[(rev == mrev) & rev] = ARP_RR
    f[(rev == mrev) & ~rev] = ARP_FF
    f[ctx] = ARP_CTX
    if slip == "unmapped_order":
        f[(sam & 0x4) != 0] = UNMAPPED
        f[(sam & 0x8) != 0] = MATE_UNMAPPED
    else:
        f[(sam & 0x8) != 0] = MATE_UNMAPPED
        f[(sam & 0x4) != 0] = UNMAPPED
    f[((sam & 0x400) != 0) | ((sam & 0x1) == 0)] = NA
    mq_ok = mapq >= minq if slip == "mapq_ge" else mapq > minq
    unm = (sam & (0x4 if slip == "pass_without_0x8" else 0xC)) != 0
    drop_t = (ctx if slip == "t_drops_ctx" else ~ctx) if opt_t else np.zeros(len(sam), bool)
    near = ai < max_sd if slip == "max_sd_lt" else ai <= max_sd
    sd_ok = near if slip == "max_sd_on_ctx" else ((f == ARP_CTX) | near)
    h_ok = mq_ok & (f != NA) & ~unm & ~drop_t
    ok = h_ok & sd_ok
    proper = (sam & (0xF if slip == "proper_without_0x400" else 0x40F)) == 0x3
    # pass 1 (BamSummary.cpp:93-112)
    lib_cnt = np.bincount(lib[mq_ok & proper], minlength=nl).astype(np.uint32)
    bam_cnt = np.bincount(bam[mq_ok & proper], minlength=nbams).astype(np.uint32)
    f1 = f.copy()
    if opt_l:     # BreakDancer.cpp:182-192, one line after the other
        if slip != "no_remap_1":
            f1[(fi > up) & (f1 == NORMAL_RF)] = ARP_RF
        if slip != "no_remap_2":
            f1[(fi < up) & (f1 == ARP_RF)] = NORMAL_RF
        if slip != "no_remap_3":
            f1[(fi < lo) & (f1 == NORMAL_RF)] = ARP_SMALL
    fh = f if slip == "hist_before_remap" else f1
    counted = h_ok & (fh != NORMAL_FR) & (fh != NORMAL_RF)
    hist = np.bincount(lib[counted] * 11 + fh[counted].astype(np.int32), minlength=nl * 11).reshape(nl, 11).astype(np.uint32)
    # pass 2 (BreakDancer.cpp:159-206)
    g = np.where(ok, f1, f)
    g[(g == ARP_RR) & (ok | (slip == "rr_fold_when_not_passing"))] = ARP_FF      # RR clusters with FF (:196-197)
    normal = ok & ((g == NORMAL_FR) | (g == NORMAL_RF))
    cls = g | (ok.astype(np.uint8) << 4) | ((ok & proper).astype(np.uint8) << 5) | ((normal & (pos < mpos)).astype(np.uint8) << 6)
    return dict(cls=cls, lib_read_count=lib_cnt, bam_read_count=bam_cnt, flag_hist=hist, raw=f)


def class_bytes(d, libs, opts=None):
    return restate(d, libs, opts)["cls"]


def numpy_class_bytes(d, upper, lower, min_mapq, opt_t=False, max_sd=MAX_SD_DEFAULT):
    """(flag | pass << 4 | proper << 5) per record, the oracle's class byte, from per-library cutoff lists"""
    libs = [(np.float32(lo), np.float32(up), int(q)) for lo, up, q in zip(lower, upper, min_mapq)]
    return class_bytes(d, libs, dict(transchr_rearrange=int(opt_t), max_sd=max_sd)) & 0x3F


def normal_left_bit(cls, d):
    """bit 6 as include/bdx.h states it, from the oracle's own byte: pass & class in {NORMAL_FR, NORMAL_RF} & pos < mpos"""
    c = np.asarray(cls).astype(np.int64)
    return ((c & CLS_PASS) != 0) & (((c & 15) == NORMAL_FR) | ((c & 15) == NORMAL_RF)) & (np.asarray(d["pos"]) < np.asarray(d["mpos"]))


# ---- the oracle over a layout -----------------------------------------------------------------------------------------------------

def oracle_run(layout, order, opts, d=None):
    """one OracleRun over the store of a layout (or over d, a store of that layout's configuration)"""
    from helpers import OracleRun, make_opts
    spec = LAYOUTS[layout]
    d = store(layout, order) if d is None else d
    run = OracleRun(config_text(spec), make_opts(**opts))
    assert run.lib_names == [l[0] for l in spec["libs"]] and run.nbams == nbams(spec)
    run.set_targets(["c1", "c2"])
    run.targets = ["c1", "c2"]
    for b in range(run.nbams):
        m = np.asarray(d["bam"]) == b
        run.set_stream(b, {k: np.asarray(d[k])[m] for k in ("tid", "pos", "mtid", "mpos", "isize", "flag", "qlen", "bdqual", "lib", "name_id")})
    return run.run()
