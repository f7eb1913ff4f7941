"""K2 (launch_k2: k2_compact_kernel, k2_compact_side_kernel with finalize2_body as its extra workgroup) and the pass-1 finalisation
(launch_finalize: finalize_kernel, finalize2_kernel) on their own, through tests/prims/compact.hip, against the references of
tests/compact_cases.py (held to all-pairs statements, route models and slips by tests/test_compact_cases.py).  Every comparison is exact,
word for word; what a launch must not touch has to come back as the 0xA5 bytes it started as, and the guards behind every array intact.
K1's model is held to K1 itself through launch_k1 -> launch_finalize -> launch_k2 on the layouts of tests/classify_cases.py, so that K2
is not tested against an idea of its input.

The harness keeps the launchers' preconditions and refuses a call that would break one; no launch here is meant to fault.  What no
result shows: the fields behind ft of a fold that comes out absent (finalize_kernel leaves them as they fall; only ft is compared).

The whole file takes 4.3 s on the MI355X; the strided case (33.6 M reads to the device, the only place beside the full-size tests where
launch_k2's grid stride runs) 1.2 s of them."""
import ctypes
import os
import subprocess
import time

import numpy as np
import pytest

import classify_cases as kc
import compact_cases as cc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TARGET = "tests/prims/libbdx_compact.so"
HIP_INVALID_VALUE = 1

vp, u32, i32, u64 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int32, ctypes.c_uint64


class Fin(ctypes.Structure):
    _fields_ = [(k, vp) for k in ("tile_tot", "tile_mono", "blk_cnt", "lib_key", "fold_in", "o_tile_pre", "o_chunk_tot", "o_chunk_base", "o_fold", "o_cnt",
                                  "o_cnt_host", "o_p1", "o_p1_host", "o_density", "o_flag", "o_count_host", "o_status")] + \
               [(k, u32) for k in ("ntiles", "tstride", "nfold", "chunk_super", "nchunk", "na_cap", "stamp")] + \
               [(k, i32) for k in ("nlibs", "nbams", "nkeys", "w0", "cn_lib", "second_level")]


class K2(ctypes.Structure):
    _fields_ = [(k, vp) for k in ("tid", "pos", "isize", "flag", "qlen", "lib", "cls", "key", "check", "tile_tot", "tile_pre", "chunk_tot", "chunk_base", "stash",
                                  "lib_key", "seg_begin", "o_tid", "o_pos", "o_isize", "o_meta", "o_key", "o_check", "o_idx", "o_nn", "o_pk")] + \
               [("o_fill", vp * 4), ("o_status", vp), ("n", u64)] + [(k, u32) for k in ("ntiles", "tstride", "cap", "chunk_super")] + \
               [("fill_words", u32 * 4), ("fill_value", u32 * 4)] + [(k, i32) for k in ("nkeys", "nlibs", "nseg", "side")]


class Chain(ctypes.Structure):
    _fields_ = [(k, vp) for k in ("mtid", "mpos", "mapq", "bam", "upper", "lower", "min_mapq", "o_cls", "o_tile_tot", "o_stash", "o_tile_pre", "o_chunk_tot",
                                  "o_chunk_base", "o_dims")] + [(k, i32) for k in ("nbams", "max_sd", "opt_t", "opt_l", "use_stash", "w0")]


def ptr(a):
    return a.ctypes.data_as(vp)


@pytest.fixture(scope="module")
def lib():
    path = os.path.join(ROOT, TARGET)
    if not os.path.exists(path):
        env = dict(os.environ)
        env.setdefault("HIPCC", "/opt/rocm/bin/hipcc")
        subprocess.check_call(["make", "-C", ROOT, TARGET], env=env)
    so = ctypes.CDLL(path)
    so.compact_constants.argtypes = [np.ctypeslib.ndpointer(np.uint32, flags="C_CONTIGUOUS")]
    so.compact_constants.restype = None
    so.compact_open.argtypes = [u64, u32, u32, u32, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.POINTER(vp)]
    so.compact_close.argtypes = [vp]
    so.compact_close.restype = None
    so.compact_finalize.argtypes = [vp, ctypes.POINTER(Fin)]
    so.compact_k2.argtypes = [vp, ctypes.POINTER(K2), ctypes.POINTER(Fin)]
    so.compact_chain.argtypes = [vp, ctypes.POINTER(K2), ctypes.POINTER(Chain), ctypes.POINTER(Fin)]
    k = np.zeros(9, np.uint32)
    so.compact_constants(k)
    assert k.tolist() == [cc.TILE, cc.SUB, cc.STASH_CAP, cc.STASH_KEYS, cc.MAX_CHUNKS, cc.CNT_COPIES, cc.STASH_WORDS * 4, cc.P1_BYTES, cc.MONO_BYTES]
    return so


class Handle:
    def __init__(self, so, n_cap=cc.H["n_cap"], nbams_cap=cc.H["nbams_cap"], with_seg=1, with_k1=1, tiles_cap=0, cap=cc.H["cap"]):
        self.so, self.h = so, vp()
        assert so.compact_open(n_cap, tiles_cap, cap, cc.H["fill_cap"], cc.H["nkeys_cap"], nbams_cap, with_seg, with_k1, ctypes.byref(self.h)) == 0

    def close(self):
        self.so.compact_close(self.h)


@pytest.fixture(scope="module")
def handle(lib):
    h = Handle(lib)
    yield h
    h.close()


def fin_block(c, keep, fold_in=None, second_level=1):
    """the argument block of a finalisation case and the arrays it returns into"""
    ncols, ts = c["ncols"], c["tstride"]
    o = dict(tile_pre=np.zeros((ncols, ts), np.uint32), chunk_tot=np.zeros((ncols, cc.MAX_CHUNKS), np.uint32), chunk_base=np.zeros((ncols, cc.MAX_CHUNKS), np.uint32),
             fold=np.zeros((c["nbams"], c["nfold"]), cc.MONO), cnt=np.zeros(c["ncnt"], np.uint32), cnt_host=np.zeros(c["ncnt"], np.uint32),
             p1=np.zeros(cc.P1_WORDS, np.uint32), p1_host=np.zeros(cc.P1_WORDS, np.uint32), density=np.zeros(64, np.float32), flag=np.zeros(16, np.uint32),
             count_host=np.zeros(cc.MAX_CHUNKS, np.uint64), status=np.ones(4, np.uint32))
    f = Fin()
    ins = dict(tile_tot=np.ascontiguousarray(c["tile_tot"]), tile_mono=np.ascontiguousarray(c["tile_mono"]),
               blk_cnt=np.ascontiguousarray(c["blk_cnt"]), lib_key=np.ascontiguousarray(c["lib_key"], np.int32))
    if fold_in is not None:
        ins["fold_in"] = np.ascontiguousarray(fold_in)
    for k, a in ins.items():
        setattr(f, k, ptr(a))
    for k, a in o.items():
        setattr(f, "o_" + k, ptr(a))
    for k in ("ntiles", "tstride", "nfold", "chunk_super", "nchunk", "na_cap", "stamp", "nlibs", "nbams", "nkeys", "w0", "cn_lib"):
        setattr(f, k, int(c[k]))
    f.second_level = second_level
    keep += [ins, o]
    return f, o


def k2_block(c, tables, keep, stash=True, side=0):
    hc, nk = c.get("hcap", cc.H["cap"]), cc.H["nkeys_cap"]
    o = dict(tid=np.zeros(hc, np.int32), pos=np.zeros(hc, np.int32), isize=np.zeros(hc, np.int32), meta=np.zeros(hc, np.uint32), key=np.zeros(hc, np.uint64),
             check=np.zeros(hc, np.uint64), idx=np.zeros(hc, np.uint32), nn=np.zeros(hc, np.uint32), pk=np.zeros(hc * nk, np.uint32), status=np.ones(4, np.uint32))
    fills = [np.zeros(max(cc.H["fill_cap"], 4), np.uint32) for _ in range(4)]
    k = K2()
    ins = {f: np.ascontiguousarray(c[f]) for f in ("tid", "pos", "isize", "flag", "qlen", "lib", "key", "lib_key")}
    if c["has_check"]:
        ins["check"] = np.ascontiguousarray(c["check"])
    if tables is not None:
        ins["cls"] = np.ascontiguousarray(c["cls"])
        for f in ("tile_tot", "tile_pre", "chunk_tot") + (() if side else ("chunk_base",)):
            ins[f] = np.ascontiguousarray(tables[f])
        if stash and c["nkeys"] <= cc.STASH_KEYS:
            ins["stash"] = np.ascontiguousarray(tables["stash"])
    if c["seg"] is not None:
        ins["seg_begin"] = np.asarray(c["seg"], np.uint64)
        k.nseg = len(c["seg"]) - 1
    for f, a in ins.items():
        setattr(k, f, ptr(a))
    for f, a in o.items():
        setattr(k, "o_" + f, ptr(a))
    for q in range(4):
        k.o_fill[q] = fills[q].ctypes.data
        k.fill_words[q], k.fill_value[q] = c["fills"][q]
    k.n, k.ntiles, k.tstride, k.cap, k.chunk_super = c["n"], c["ntiles"], c["tstride"], c["cap"], c["chunk_super"]
    k.nkeys, k.nlibs, k.side = c["nkeys"], c["nlibs"], side
    o["fills"] = fills
    keep += [ins, o]
    return k, o


def side_fin(c, tables, keep):
    """a well-formed second level beside K2: one source file folded from two partial records, counters in 64 copies"""
    f = dict(name=c["name"], ntiles=c["ntiles"], tstride=c["tstride"], nsuper=c["nsuper"], nkeys=c["nkeys"], nlibs=c["nlibs"], nbams=1, ncols=2 + c["nkeys"],
             ncnt=c["nlibs"] * 12 + 1, chunk_super=c["chunk_super"], nchunk=max(1, (c["nsuper"] + c["chunk_super"] - 1) // c["chunk_super"]), nfold=2, w0=300, cn_lib=1,
             na_cap=0, stamp=11, tile_tot=tables["tile_tot"], tile_mono=np.zeros((1, c["tstride"]), cc.MONO), lib_key=c["lib_key"])
    rng = np.random.default_rng(c["n"])
    f["blk_cnt"] = rng.integers(0, 50, (cc.CNT_COPIES, f["ncnt"])).astype(np.uint32)
    fold = np.zeros((1, 2), cc.MONO)
    fold[0, 0] = (3, 100, 3, 5000, 4900)
    fold[0, 1] = (3, 6000, 4, 10, 77)
    blk, o = fin_block(f, keep, fold_in=fold)
    return f, fold, blk, o


def assert_same(got, want, fields, what):
    for f in fields:
        a, b = np.asarray(got[f]).view(np.uint8).ravel(), np.asarray(want[f]).view(np.uint8).ravel()
        if not np.array_equal(a, b):
            at = int(np.flatnonzero(a != b)[0])
            raise AssertionError("%s: %s differs from byte %d on (%d bytes differ)" % (what, f, at, int((a != b).sum())))


def run_k2(so, handle, c, tables, stash, side):
    keep = []
    k, o = k2_block(c, tables, keep, stash, side)
    if side:
        f, fold, fb, fo = side_fin(c, tables, keep)
        rc = so.compact_k2(handle.h, ctypes.byref(k), ctypes.byref(fb))
    else:
        rc = so.compact_k2(handle.h, ctypes.byref(k), None)
    assert rc == 0, (c["name"], rc)
    assert o["status"].tolist() == [0, 0, 0, 0]
    if side:      # the second level beside it: chunk_base, counters, the record and its mirror, the flag word
        want = cc.fin2_reference(f, tables["chunk_tot"], fold)
        assert_same(fo, want, ("chunk_base", "cnt", "cnt_host", "p1", "p1_host", "density", "flag"), c["name"] + " (second level)")
    return o


K2_NAMES = [c["name"] for c in cc.k2_cases()]


@pytest.mark.parametrize("name", K2_NAMES)
def test_k2_is_the_reference(lib, handle, name):
    """with the ready-made records and without, as k2_compact_kernel and as k2_compact_side_kernel: four times the same words"""
    c = cc.k2_case_named(name)
    want = cc.k2_reference(c)
    tables = cc.k1_model(c)
    fills = cc.fill_model(c)
    for stash in (True, False):
        for side in (0, 1):
            o = run_k2(lib, handle, c, tables, stash, side)
            assert_same(o, want, cc.OUT_FIELDS, "%s stash=%d side=%d" % (name, stash, side))
            for q in range(4):
                np.testing.assert_array_equal(o["fills"][q], fills[q], err_msg="%s fill %d" % (name, q))


def test_k2_four_calls_of_shrinking_size_on_one_handle(lib, handle):
    for name in cc.SHRINKING:
        c = cc.k2_case_named(name)
        o = run_k2(lib, handle, c, cc.k1_model(c), True, 0)
        assert_same(o, cc.k2_reference(c), cc.OUT_FIELDS, name)


def test_k2_strided_grid(lib):
    """launch_k2's grid cap: 8192 * 4 + 5 super tiles, 9 chunks of 4,096, through compact_finalize and then compact_k2 as either kernel (the
    one slow case: 33.6 M reads go to the device twice; 1.2 s on the MI355X, 1.0 s of it the reference on the host)"""
    t0 = time.time()
    c = cc.strided_case()
    want = cc.k2_reference(c)
    tables = cc.k1_model(c)
    t1 = time.time()
    h = Handle(lib, n_cap=c["n"], nbams_cap=1, with_seg=0, with_k1=0)
    try:
        keep = []
        mono = np.zeros((1, c["tstride"]), cc.MONO)
        mono.view(np.uint8)[:] = 0xFF
        f = dict(ntiles=c["ntiles"], tstride=c["tstride"], nkeys=1, nlibs=1, nbams=1, ncols=3, ncnt=13, chunk_super=cc.ROUND, nchunk=9, nfold=64, w0=100, cn_lib=0, na_cap=0,
                 stamp=5, tile_tot=tables["tile_tot"], tile_mono=mono, lib_key=c["lib_key"], blk_cnt=np.zeros((cc.CNT_COPIES, 13), np.uint32))
        fb, fo = fin_block(f, keep)
        assert lib.compact_finalize(h.h, ctypes.byref(fb)) == 0
        nsuper = c["nsuper"]
        np.testing.assert_array_equal(fo["tile_pre"][:, :nsuper], tables["tile_pre"][:, :nsuper])
        np.testing.assert_array_equal(fo["chunk_tot"][:, :9], tables["chunk_tot"][:, :9])
        np.testing.assert_array_equal(fo["chunk_base"], tables["chunk_base"])
        t2 = time.time()
        scanned = dict(tables, tile_pre=fo["tile_pre"], chunk_tot=fo["chunk_tot"], chunk_base=fo["chunk_base"])      # what the finalisation left, 0xA5 included
        for side in (0, 1):
            assert_same(run_k2(lib, h, c, scanned, True, side), want, cc.OUT_FIELDS, "strided side=%d" % side)
        print("strided case: reference %.1f s, finalisation %.1f s, two K2 calls %.1f s" % (t1 - t0, t2 - t1, time.time() - t2))
    finally:
        h.close()


# ---- the finalisation -----------------------------------------------------------------------------------------------------------------------------

FIN_NAMES = [c["name"] for c in cc.fin_cases()]


@pytest.fixture(scope="module")
def fin_handle(lib):
    h = Handle(lib, n_cap=16385 * cc.TILE, nbams_cap=4, with_seg=0, with_k1=0, tiles_cap=64 * 16384)
    yield h
    h.close()


@pytest.mark.parametrize("name", FIN_NAMES)
def test_the_finalisation_is_the_reference(lib, fin_handle, name):
    c = cc.fin_case_named(name)
    keep = []
    fb, o = fin_block(c, keep)
    assert lib.compact_finalize(fin_handle.h, ctypes.byref(fb)) == 0
    assert o["status"].tolist() == [0, 0, 0, 0]
    assert cc.fin_differs(o, cc.fin_reference(c)) is None


@pytest.mark.parametrize("name", ["ntiles_5", "ntiles_16385", "libraries_255", "na_cap_count-1", "chunks_64_mostly_empty"])
def test_the_second_level_beside_k2_is_the_second_level_alone(lib, fin_handle, name):
    """second_level = false leaves what only finalize2_body writes untouched; K2's extra workgroup then writes, word for word, what the two-launch route does"""
    c = cc.fin_case_named(name)
    keep = []
    fb, two = fin_block(c, keep)
    assert lib.compact_finalize(fin_handle.h, ctypes.byref(fb)) == 0
    fb, first = fin_block(c, keep, second_level=0)
    assert lib.compact_finalize(fin_handle.h, ctypes.byref(fb)) == 0
    assert cc.fin_differs(first, cc.fin_reference(c, second_level=False)) is None
    # a store of the case's size without a passing read: K2 writes nothing, its extra workgroup everything the second launch did
    n = c["ntiles"] * cc.TILE
    z = dict(name=name, n=n, ntiles=c["ntiles"], tstride=c["tstride"], nsuper=c["nsuper"], nkeys=c["nkeys"], nlibs=c["nlibs"], lib_key=c["lib_key"], chunk_super=c["chunk_super"],
             seg=None, fills=((0, 0),) * 4, has_check=True, cap=0, cls=np.zeros(n, np.uint8), tid=np.zeros(n, np.int32), pos=np.zeros(n, np.int32),
             isize=np.zeros(n, np.int32), flag=np.zeros(n, np.uint16), qlen=np.zeros(n, np.uint16), lib=np.zeros(n, np.uint8), key=np.zeros(n, np.uint64),
             check=np.zeros(n, np.uint64))
    k, o = k2_block(z, dict(tile_tot=c["tile_tot"], tile_pre=first["tile_pre"], chunk_tot=first["chunk_tot"]), keep, False, 1)
    fb, side = fin_block(c, keep, fold_in=first["fold"])
    assert lib.compact_k2(fin_handle.h, ctypes.byref(k), ctypes.byref(fb)) == 0
    assert o["status"].tolist() == [0, 0, 0, 0]
    assert (o["idx"] == cc.FILL).all() and (o["pk"] == cc.FILL).all()
    second = ("chunk_base", "cnt", "cnt_host", "p1", "p1_host", "density", "flag")
    assert_same(side, cc.fin2_reference(c, first["chunk_tot"], first["fold"]), second, name)
    assert_same(side, two, second, name + " against two launches")


def test_refused_calls(lib, handle):
    """a call that breaks a precondition is refused and never launched"""
    c = cc.k2_case_named("one_marked_among_four")
    t = cc.k1_model(c)
    assert c["ntiles"] < c["tstride"]

    def rc_of(tables=t, **over):
        keep = []
        k, o = k2_block(dict(c, **{f: v for f, v in over.items() if f in c}), tables, keep, True, 0)
        for f, v in over.items():
            if f not in c:
                setattr(k, f, v)
        return lib.compact_k2(handle.h, ctypes.byref(k), None)

    assert rc_of() == 0
    assert rc_of(tstride=c["tstride"] + 8) == HIP_INVALID_VALUE
    assert rc_of(chunk_super=0) == HIP_INVALID_VALUE
    assert rc_of(nkeys=61) == HIP_INVALID_VALUE
    assert rc_of(cap=cc.H["cap"] + 1) == HIP_INVALID_VALUE
    bad = dict(t, tile_tot=t["tile_tot"].copy())
    bad["tile_tot"][0, c["ntiles"]] = 1                      # a total behind ntiles
    assert rc_of(bad) == HIP_INVALID_VALUE
    bad = dict(t, tile_tot=t["tile_tot"].copy())
    bad["tile_tot"][0, 0] += 1                               # the stash knows of one record less
    assert rc_of(bad) == HIP_INVALID_VALUE
    assert rc_of(seg=(0, 5, 5, c["n"])) == HIP_INVALID_VALUE
    assert rc_of(seg=(0, 5, c["n"] - 1)) == HIP_INVALID_VALUE
    f = cc.fin_case_named("ntiles_5")
    keep = []
    fb, o = fin_block(dict(f, chunk_super=4095), keep)
    assert lib.compact_finalize(handle.h, ctypes.byref(fb)) == HIP_INVALID_VALUE
    mono = f["tile_mono"].copy()
    mono[0, 0]["ft"], mono[0, 0]["fp"] = -1, 3               # an absent file's record that is not 0xFF
    fb, o = fin_block(dict(f, tile_mono=mono), keep)
    assert lib.compact_finalize(handle.h, ctypes.byref(fb)) == HIP_INVALID_VALUE


# ---- K1's model against K1 ----------------------------------------------------------------------------------------------------------------------------

CHAIN = [("one-library", "table", 0), ("one-library", "spread", 0), ("uniform", "spread", 0), ("uniform", "perm", 0), ("mixed", "spread", 0), ("mixed", "table", 0),
         ("mixed-two-keys", "spread", 1), ("mixed-two-keys", "perm", 1), ("nine-libraries", "spread", 0), ("two-files", "spread", 0), ("two-files", "perm", 0),
         ("tail-1", "perm", 0), ("tail-129", "perm", 0), ("tail-255", "table", 0)]


CHAIN_CAP = 40960


@pytest.fixture(scope="module")
def chain_handle(lib):
    h = Handle(lib, n_cap=620000, cap=CHAIN_CAP, with_seg=0)
    yield h
    h.close()


@pytest.mark.parametrize("layout,order,cn_lib", CHAIN)
def test_the_model_of_k1_is_k1(lib, chain_handle, layout, order, cn_lib):
    """launch_k1 -> launch_finalize -> launch_k2 on a layout of tests/classify_cases.py: cls, tile_tot and the written stash slots are the model's,
    and the chain's Compact is compact_k2's on the model's tables"""
    spec = kc.LAYOUTS[layout]
    d = kc.store(layout, order)
    n = len(d["tid"])
    libs = kc.lib_params(spec)
    nlibs, nbams = len(libs), kc.nbams(spec)
    lib_key = list(range(nlibs)) if cn_lib else list(spec["files"])
    nkeys = nlibs if cn_lib else nbams
    use_stash = nkeys <= cc.STASH_KEYS
    cls = kc.restate(d, libs, nbams=nbams)["cls"]
    name = d["name_id"].astype(np.uint64)
    c = dict(name="%s-%s" % (layout, order), n=n, nkeys=nkeys, nlibs=nlibs, lib_key=np.asarray(lib_key, np.int32), seg=None, fills=((3, 1), (0, 0), (0, 0), (5, 2)),
             has_check=True, hcap=CHAIN_CAP, ntiles=(n + cc.TILE - 1) // cc.TILE, cls=cls, tid=d["tid"], pos=d["pos"], isize=d["isize"], flag=d["flag"], qlen=d["qlen"].astype(np.uint16),
             lib=d["lib"].astype(np.uint8), key=name * np.uint64(0x9E3779B97F4A7C15), check=name * np.uint64(0xC2B2AE3D27D4EB4F))
    c["tstride"], c["nsuper"] = cc.row16(c["ntiles"]), (c["ntiles"] + cc.SUB - 1) // cc.SUB
    rounds = max(1, (c["nsuper"] + cc.ROUND - 1) // cc.ROUND)
    c["chunk_super"] = cc.ROUND * ((rounds + cc.MAX_CHUNKS - 1) // cc.MAX_CHUNKS)
    c["pre_off"] = c["chunk_off"] = np.zeros(2 + nkeys, np.uint32)
    c["count"] = int(cc.masks(c)["anom"].sum())
    c["cap"] = c["count"]
    assert 0 < c["count"] <= CHAIN_CAP
    model = cc.k1_model(c)
    h = chain_handle
    keep = []
    k, o = k2_block(c, None, keep, use_stash, 0)
    ncols, ts, nt = 2 + nkeys, c["tstride"], c["ntiles"]
    co = dict(cls=np.zeros(n, np.uint8), tile_tot=np.zeros((ncols, ts), np.uint32), stash=np.zeros((nt, cc.STASH_CAP, cc.STASH_WORDS), np.uint32),
              tile_pre=np.zeros((ncols, ts), np.uint32), chunk_tot=np.zeros((ncols, cc.MAX_CHUNKS), np.uint32), chunk_base=np.zeros((ncols, cc.MAX_CHUNKS), np.uint32),
              dims=np.zeros(4, np.uint32))
    ci = dict(mtid=np.ascontiguousarray(d["mtid"]), mpos=np.ascontiguousarray(d["mpos"]), mapq=np.ascontiguousarray(d["bdqual"]), bam=np.ascontiguousarray(d["bam"], np.uint8),
              upper=np.asarray([l[1] for l in libs], np.float32), lower=np.asarray([l[0] for l in libs], np.float32), min_mapq=np.asarray([l[2] for l in libs], np.int32))
    ch = Chain()
    for f, a in ci.items():
        setattr(ch, f, ptr(a))
    for f, a in co.items():
        setattr(ch, "o_" + f, ptr(a))
    ch.nbams, ch.max_sd, ch.opt_t, ch.opt_l, ch.use_stash, ch.w0 = nbams, kc.MAX_SD_DEFAULT, 0, 0, int(use_stash), 1000
    fin = dict(ntiles=nt, tstride=ts, nkeys=nkeys, nlibs=nlibs, nbams=nbams, ncols=ncols, ncnt=nlibs * 12 + nbams, chunk_super=c["chunk_super"], nchunk=1,
               nfold=max(1, min(64, (nt + 1023) // 1024)), w0=1000, cn_lib=cn_lib, na_cap=0, stamp=3, tile_tot=model["tile_tot"],
               tile_mono=np.zeros((nbams, ts), cc.MONO), blk_cnt=np.zeros((cc.CNT_COPIES, nlibs * 12 + nbams), np.uint32), lib_key=c["lib_key"])
    fb, fo = fin_block(fin, keep)
    assert lib.compact_chain(h.h, ctypes.byref(k), ctypes.byref(ch), ctypes.byref(fb)) == 0
    assert o["status"].tolist() == [0, 0, 0, 0]
    assert co["dims"].tolist() == [nt, ts, c["chunk_super"], 1]
    np.testing.assert_array_equal(co["cls"], cls)
    np.testing.assert_array_equal(co["tile_tot"], model["tile_tot"])
    if use_stash:
        np.testing.assert_array_equal(co["stash"], model["stash"])
    else:
        assert (co["stash"] == cc.FILL).all()
    np.testing.assert_array_equal(co["tile_pre"][:, :c["nsuper"]], model["tile_pre"][:, :c["nsuper"]])
    np.testing.assert_array_equal(co["chunk_tot"][:, 0], model["chunk_tot"][:, 0])
    np.testing.assert_array_equal(co["chunk_base"], model["chunk_base"])
    assert int(fo["p1"][2]) == c["count"]
    want = cc.k2_reference(c)
    assert_same(o, want, cc.OUT_FIELDS, c["name"] + " (chain)")
    o2 = run_k2(lib, h, c, model, use_stash, 0)
    assert_same(o2, o, cc.OUT_FIELDS, c["name"] + " (compact_k2 on the model's tables)")


def test_a_product_run_beside_the_harness(lib, handle):
    """the harness carries second copies of K1's and K2's kernels: a product run in the same process, after the harness has launched its own, is
    the oracle's as before"""
    from fuzzgen import OPTION_SETS, make_case
    from helpers import make_opts
    from runner import compare, oracle_case, product_from_oracle
    c = cc.k2_case_named("n_1025_dense")
    run_k2(lib, handle, c, cc.k1_model(c), True, 1)
    cfg, streams, targets = make_case(3)
    run = oracle_case(cfg, streams, targets, make_opts(score_threshold=-1, **OPTION_SETS[3 % len(OPTION_SETS)]))
    bd = product_from_oracle(run)
    compare(run, bd)
    bd.close()
    o = run_k2(lib, handle, c, cc.k1_model(c), True, 0)
    assert_same(o, cc.k2_reference(c), cc.OUT_FIELDS, "after the product run")
