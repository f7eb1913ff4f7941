"""K6 between the mate join and the final table on its own -- launch_k6_groups (k6_pairs_kernel, k6_label_kernel, k6_classify_kernel,
k6_emit_kernel, the counter mirror), launch_k6_walk (k6_walk_kernel, k6_walk_big_kernel with assemble_sv) and launch_k6_table behind the
host's share (k6_insert_kernel, k6_place_kernel, k6_score_kernel) -- through tests/prims/assemble.hip, against the read-level reference
and the models of tests/assemble_cases.py (held to ground truth by tests/test_assemble_cases.py).  Every comparison is exact, word for
word, but logp (runner.compare's rule: 1e-9 relative); what a launch must not touch has to come back as the 0xA5 bytes it started as,
and the guards behind every array intact.

The harness keeps the launchers' preconditions and refuses a call that would break one; no launch here is meant to fault or to spin.
What no result shows: the label of a component that has not converged, the order of g_rec, the member slot a region gets."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

import assemble_cases as ac
from helpers import oracle_lib

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TARGET = "tests/prims/libbdx_assemble.so"
HIP_INVALID_VALUE = 1
FILL = np.uint32(ac.FILL)
CAP, NKEYS, NLIBS = 1200, 17, 17

_U32 = ("n_regions", "n_host", "n_reads", "n_agg", "g_cap", "stamp", "covered_ref_len")
_I32 = ("last_maxq", "nlibs", "nkeys", "min_read_pair", "chr_restricted", "period", "force_host", "big_walk", "asm_plain", "ins_plain", "propagation_rounds",
        "mirror_in_walk", "stage", "wire_rows", "score_threshold")
_IN = ("rec", "pk", "region_of", "partner", "pair_lo", "meta", "isize", "in_groups", "in_goff", "taint", "hist", "key_density", "lib_mean")
_OUT = ("rs", "parts", "scratch", "members", "member_ids", "owners", "owners_big", "g_rec", "counts_dev", "counts_host", "counts2", "taint_out", "sv_stage",
        "lib_stage", "cn_stage", "own_nsv", "own_nacc", "own_ncn", "own_first", "slot_next", "old_key", "old_slot", "sv_out", "lib_index", "lib_pairs", "cn_key",
        "cn_value", "info")


class AsmIO(ctypes.Structure):
    _fields_ = [(k, ctypes.c_uint32) for k in _U32] + [(k, ctypes.c_int32) for k in _I32] + [(k, ctypes.c_void_p) for k in _IN + _OUT]


@pytest.fixture(scope="module")
def lib():
    path = os.path.join(ROOT, TARGET)
    if not os.path.exists(path):
        env = dict(os.environ)
        env.setdefault("HIPCC", "/opt/rocm/bin/hipcc")
        subprocess.check_call(["make", "-C", ROOT, TARGET], env=env)
    so = ctypes.CDLL(path)
    vp = ctypes.c_void_p
    so.assemble_open.argtypes = [ctypes.c_uint32, ctypes.c_int, ctypes.c_int, ctypes.POINTER(vp)]
    so.assemble_close.argtypes = [vp]
    so.assemble_close.restype = None
    so.assemble_caps.argtypes = [vp, vp]
    so.assemble_caps.restype = None
    for f in (so.assemble_groups, so.assemble_walk, so.assemble_chain):
        f.argtypes = [vp, ctypes.POINTER(AsmIO)]
    k = np.zeros(16, np.uint32)
    so.assemble_constants.argtypes = [vp]
    so.assemble_constants.restype = None
    so.assemble_constants(k.ctypes.data)
    assert k.tolist() == ac.CONSTANTS          # what the models are built on
    return so


class Harness:
    """one buffer set, kept from call to call; hands out the stamps: never the same one twice"""

    def __init__(self, so, cap=CAP, nkeys=NKEYS, nlibs=NLIBS):
        self.so, self.cap, self.stamp = so, cap, 0
        self.h = ctypes.c_void_p()
        assert so.assemble_open(cap, nkeys, nlibs, ctypes.byref(self.h)) == 0
        caps = np.zeros(6, np.uint32)
        so.assemble_caps(self.h, caps.ctypes.data)
        self.sv_cap, self.term_cap, _, _, self.p2, self.g_alloc = (int(x) for x in caps)

    def close(self):
        self.so.assemble_close(self.h)

    def run(self, c, stage=3, stamp=None, **over):
        a = dict(c)
        a.update(over)
        cap, nk = self.cap, a["nkeys"]
        stride = min(a["nlibs"], ac.LIB_STRIDE)
        cn_cap = self.sv_cap * nk
        o = dict(rs=np.zeros((cap, ac.RS_WORDS), np.uint32), parts=np.zeros((cap, 4), np.uint32), scratch=np.zeros((6, cap), np.uint32),
                 members=np.zeros((cap * ac.MAX_MEMBERS, ac.MEMBER_WORDS), np.uint32), member_ids=np.zeros((cap, ac.BIG_MEMBERS), np.uint32),
                 owners=np.zeros(cap, np.uint32), owners_big=np.zeros(cap, np.uint32), g_rec=np.zeros((self.g_alloc, 4), np.uint32),
                 counts_dev=np.zeros(ac.COUNT_WORDS, np.uint32), counts_host=np.zeros(ac.COUNT_WORDS, np.uint32), counts2=np.zeros(ac.COUNT_WORDS, np.uint32),
                 taint_out=np.zeros(cap, np.uint8), sv_stage=np.zeros((cap, ac.SV_WORDS), np.uint32), lib_stage=np.zeros((cap, stride, 4), np.uint32),
                 cn_stage=np.zeros((cap, nk, 2), np.uint32), own_nsv=np.zeros(cap, np.uint32), own_nacc=np.zeros(cap, np.uint32), own_ncn=np.zeros(cap, np.uint32),
                 own_first=np.zeros(cap, np.uint32), slot_next=np.zeros(cap, np.uint32), old_key=np.zeros(self.p2, np.uint64), old_slot=np.zeros(self.p2, np.uint32),
                 sv_out=np.zeros((self.sv_cap, ac.SV_WORDS), np.uint32), lib_index=np.zeros(self.term_cap, np.int32), lib_pairs=np.zeros(self.term_cap, np.int32),
                 cn_key=np.zeros(cn_cap, np.int32), cn_value=np.zeros(cn_cap, np.uint32), info=np.zeros(8, np.uint32))
        io = AsmIO()
        if stamp is None:
            self.stamp += 1
            stamp = self.stamp
        agg = a.get("agg")
        NR = a["n_regions"]
        io.n_regions, io.n_reads, io.n_agg = NR, (0 if agg is not None else a["n_reads"]), (len(agg) if agg is not None else 0)
        io.n_host = NR if a["n_host"] is None else a["n_host"]
        io.g_cap = self.g_alloc if a["g_cap"] is None else a["g_cap"]
        io.stamp, io.covered_ref_len, io.last_maxq = stamp, a["covered"], a["last_maxq"]
        for k in ("nlibs", "nkeys", "min_read_pair", "chr_restricted", "period", "big_walk", "asm_plain", "ins_plain", "propagation_rounds"):
            setattr(io, k, a[k])
        io.force_host, io.mirror_in_walk, io.wire_rows, io.score_threshold = a.get("force_host", 0), a.get("mirror_in_walk", 0), a.get("wire_rows", 0), ac.SCORE_THRESHOLD
        keep = dict(rec=np.ascontiguousarray(a["rec"], np.uint32), pk=np.ascontiguousarray(a["pk"], np.uint32), hist=np.ascontiguousarray(a["hist"], np.uint32),
                    key_density=np.ascontiguousarray(a["key_density"], np.float32), lib_mean=np.ascontiguousarray(a["lib_mean"], np.float32))
        if agg is not None:
            g = np.zeros((max(len(agg), 1), 4), np.uint32)
            for i, (k, p, s) in enumerate(agg):
                g[i] = [k & 0xFFFFFFFF, k >> 32, p, s]
            keep.update(in_groups=g, in_goff=np.ascontiguousarray(a["in_goff"], np.uint32))
            if a.get("taint") is not None:
                keep["taint"] = np.ascontiguousarray(a["taint"], np.uint8)
        else:
            keep.update(region_of=a["region_of"], partner=a["partner"], meta=a["meta"], isize=a["isize"])
            if a["use_pair_lo"]:
                keep["pair_lo"] = a["pair_lo"]
        for k, v in keep.items():
            setattr(io, k, v.ctypes.data)
        for k, v in o.items():
            setattr(io, k, v.ctypes.data)
        fn = {1: self.so.assemble_groups, 2: self.so.assemble_walk, 3: self.so.assemble_chain}[stage]
        o["rc"] = fn(self.h, ctypes.byref(io))
        if o["rc"] not in (0, HIP_INVALID_VALUE):          # an error of the device's: nothing more is launched in this session
            pytest.exit("HIP error %d in case %s" % (o["rc"], a["name"]), returncode=3)
        o["args"] = a
        return o


@pytest.fixture(scope="module")
def hs(lib):
    h = Harness(lib)
    yield h
    h.close()


@pytest.fixture(scope="module")
def tail():
    L = oracle_lib()

    def f(lam, k):
        p = L.bdo_poisson_upper_tail(float(lam), int(k))
        return math.log(p) if p > 0 else -math.inf
    return f


_REFS = {}


def reference(c, tail):
    if c["name"] not in _REFS:
        _REFS[c["name"]] = ac.walk_reference(c, tail=tail)
    return _REFS[c["name"]]


# ---- comparisons ------------------------------------------------------------------------------------------------------------

def check_record(w, o, what):
    """24 words of an SvOut against a record of the reference: everything but the list offsets, logp, score and printed"""
    i32 = w.view(np.int32)
    got = dict(chr=i32[0:2].tolist(), pos=i32[2:4].tolist(), fwd=i32[4:6].tolist(), rev=i32[6:8].tolist(), flag=int(i32[8]), size=int(i32[9]),
               num_reads=int(i32[11]), region=i32[13:15].tolist(), grp_mask=int(w[22]), start=int(w[23]))
    for k, v in got.items():
        assert v == o[k], (what, k, v, o[k])
    assert int(i32[16]) == len(o["terms"]) and int(i32[18]) == len(o["cn"]), (what, "counts")
    assert int(w[19]) == int(np.float32(o["af"]).view(np.uint32)), (what, "allele_frequency", hex(int(w[19])))


def check_scores(w, o, what):
    i32 = w.view(np.int32)
    lp = float(w[20:22].view(np.float64)[0])
    assert math.isnan(lp) == math.isnan(o["logp"]) and math.isinf(lp) == math.isinf(o["logp"]), (what, lp, o["logp"])
    if math.isfinite(o["logp"]):
        assert abs(lp - o["logp"]) / max(1.0, abs(o["logp"])) < 1e-9, (what, lp, o["logp"])
    assert int(i32[10]) == o["score"] and int(i32[12]) == o["printed"], (what, "score", int(i32[10]), o["score"])


def check_groups(c, o):
    """the groups stage word for word against the models"""
    NR, cap = c["n_regions"], o["rs"].shape[0]
    m = ac.groups_model(c)
    np.testing.assert_array_equal(o["rs"][:NR], m["rs"], err_msg="RegSum")
    assert (o["rs"][NR:] == FILL).all()
    want = np.full((cap, 4), FILL, np.uint32)
    for r, ps in m["parts"].items():
        f = ac.first_of(c, r)
        for i, (k, p, s) in enumerate(ps):
            want[f + i] = [k & 0xFFFFFFFF, k >> 32, p, s]
    np.testing.assert_array_equal(o["parts"], want, err_msg="parts")
    np.testing.assert_array_equal(o["scratch"][0, :NR], m["out_deg"], err_msg="out_deg")
    np.testing.assert_array_equal(o["scratch"][2, :NR], m["bad_v"], err_msg="bad_v")
    idx = np.arange(cap, dtype=np.uint32)
    np.testing.assert_array_equal(o["scratch"][1, NR:], idx[NR:])        # behind the regions: as launch_k6_scratch_init left them
    for row in (0, 2, 3, 4, 5):
        assert (o["scratch"][row, NR:] == 0).all()
    assert (o["scratch"][1, :NR] <= idx[:NR]).all()                      # a label is some region at or before its own
    assert int(o["counts_host"][3]) == int(m["rs"][:, 5].sum())           # n_pairs, mirrored with k6_emit_kernel's partial totals
    assert int(o["counts_dev"][6]) == 0 and int(o["counts_host"][6]) == 0, ("overflow", int(o["counts_dev"][6]), int(o["counts_host"][6]))
    same = [0, 1, 2, 4, 16]                                                # what no later kernel bumps: n_cand, n_regions, last_maxq, n_groups, n_owners_big
    np.testing.assert_array_equal(o["counts_host"][same], o["counts_dev"][same])
    return m


def host_rows(m, regions):
    rows = [x for r in regions for x in m["emit"].get(r, [])] + [x for r in regions for x in m["raw"].get(r, [])]
    return sorted((k & 0xFFFFFFFF, k >> 32, p, s) for k, p, s in rows)


def check_host_list(o, want_rows):
    n = int(o["counts_host"][4])
    assert int(o["counts_host"][6]) == 0
    got = sorted(tuple(int(x) for x in row) for row in o["g_rec"][:n])
    assert got == want_rows
    assert (o["g_rec"][n:] == FILL).all()


def staged(o, c):
    """the device-walked records as the walks staged them: per start vertex in emission order (own_first / slot_next), and the from-old ones in
    the order of their keys"""
    NR = c["n_regions"]
    own = {}
    for v in range(NR):
        n = int(o["own_nsv"][v])
        assert n < 4 * ac.BIG_MEMBERS, v
        slots, s = [], int(o["own_first"][v])
        for q in range(n):
            slots.append(s)
            if q + 1 < n:
                s = int(o["slot_next"][s])
        own[v] = slots
    n_old = int(o["counts_dev"][18])
    keys = o["old_key"][:n_old]
    assert len(np.unique(keys)) == n_old, "order keys that differ"
    order = np.argsort(keys, kind="stable")
    return own, [(int(keys[i]), int(o["old_slot"][i])) for i in order]


def check_staging(c, o, ref, m):
    """every staged record is the reference's record of the same pair of regions; the records of a start vertex come in the reference's order,
    the from-old ones sort into it by key; their list entries are the reference's"""
    by_regions = {tuple(x["region"]): x for x in ref}
    assert len(by_regions) == len(ref)
    own, old = staged(o, c)
    dev = set()

    def one(slot, what):
        w = o["sv_stage"][slot]
        key = tuple(w.view(np.int32)[13:15].tolist())
        assert key in by_regions, (what, key)
        x = by_regions[key]
        check_record(w, x, what)
        for i, (l, k, lam) in enumerate(x["terms"]):
            e = o["lib_stage"][slot, i]
            assert (int(e[0]), int(e[1]), float(e[2:4].view(np.float64)[0])) == (l, k, lam), (what, "term", i)
        for i, (k, v) in enumerate(x["cn"]):
            e = o["cn_stage"][slot, i]
            assert (int(e[0]), int(e[1])) == (k, int(np.float32(v).view(np.uint32))), (what, "cn", i)
        dev.add(key)
        return x

    per_start = {v: [one(s, ("own", v)) for s in slots] for v, slots in own.items()}
    for v, recs in per_start.items():
        want = [x for x in ref if x["start"] == v and not x["from_old"] and tuple(x["region"]) in dev]
        assert [x["region"] for x in recs] == [x["region"] for x in want], ("own order", v)
        if recs:
            assert int(o["own_nacc"][v]) == sum(len(x["terms"]) for x in recs) and int(o["own_ncn"][v]) == sum(len(x["cn"]) for x in recs), ("own totals", v)
    recs = []
    for key, slot in old:
        x = one(slot, ("old", hex(key)))
        assert key >> ac.SHIFT_T == x["T"] and (key >> ac.SHIFT_START) & ((1 << 26) - 1) == x["start"] and not (key >> ac.SHIFT_OWN) & 1 and x["from_old"]
        recs.append(x)
    want = [x for x in ref if x["from_old"] and tuple(x["region"]) in dev]
    assert [x["region"] for x in recs] == [x["region"] for x in want], "from-old order"
    return dev


def check_table(c, o, ref, wire):
    n = len(ref)
    assert o["rc"] == 0 and int(o["info"][0]) == 0, ("rc / guards", o["rc"], int(o["info"][0]))
    assert int(o["counts2"][6]) == 0 and int(o["counts2"][8]) == n, ("overflow, n_sv", int(o["counts2"][6]), int(o["counts2"][8]), n)
    nt, nc = sum(len(x["terms"]) for x in ref), sum(len(x["cn"]) for x in ref)
    assert (int(o["counts2"][9]), int(o["counts2"][10])) == (nt, nc)
    assert int(o["info"][2]) == sum(x["printed"] for x in ref)
    lb = cb = 0
    rows = o["sv_out"].reshape(-1)
    for i, x in enumerate(ref):
        if wire:
            w = rows[i * ac.WIRE_WORDS:(i + 1) * ac.WIRE_WORDS]
            i32 = w.view(np.int32)
            bits = int(w[11])
            got = dict(pos=i32[0:2].tolist(), region=i32[2:4].tolist(), size=int(i32[4]), num_reads=int(i32[6]), start=int(w[10]), flag=(bits >> 16) & 15,
                       grp_mask=(bits >> 20) & 7)
            for k, v in got.items():
                assert v == x[k], (i, k, v, x[k])
            assert (bits & 255, (bits >> 8) & 255, (bits >> 23) & 1) == (len(x["terms"]), len(x["cn"]), x["printed"]), (i, "bits")
            assert int(w[7]) == int(np.float32(x["af"]).view(np.uint32)) and int(i32[5]) == x["score"], (i, "af / score")
            lp = float(w[8:10].view(np.float64)[0])
            assert (lp == x["logp"]) or abs(lp - x["logp"]) / max(1.0, abs(x["logp"])) < 1e-9, (i, lp, x["logp"])
        else:
            w = rows[i * ac.SV_WORDS:(i + 1) * ac.SV_WORDS]
            check_record(w, x, i)
            check_scores(w, x, i)
            assert (int(w[15]), int(w[17])) == (lb, cb), (i, "list offsets")
        for q, (l, k, _) in enumerate(x["terms"]):
            assert (int(o["lib_index"][lb + q]), int(o["lib_pairs"][lb + q])) == (l, k), (i, "lib list", q)
        for q, (k, v) in enumerate(x["cn"]):
            assert (int(o["cn_key"][cb + q]), int(o["cn_value"][cb + q])) == (k, int(np.float32(v).view(np.uint32))), (i, "cn list", q)
        lb += len(x["terms"]); cb += len(x["cn"])
    used = n * (ac.WIRE_WORDS if wire else ac.SV_WORDS)
    assert (rows[used:] == FILL).all(), "nothing behind the table"
    assert (o["lib_index"].view(np.uint32)[nt:] == FILL).all() and (o["cn_key"].view(np.uint32)[nc:] == FILL).all()


# ---- tests ------------------------------------------------------------------------------------------------------------------

CASES = {c["name"]: c for c in ac.table_cases()}
WALKED = sorted(n for n, c in CASES.items() if not c["groups_only"])


def test_the_harness_refuses_what_breaks_a_precondition(hs):
    c = CASES["gate-r2"]
    assert hs.run(c, stage=1, stamp=0)["rc"] == HIP_INVALID_VALUE
    ok = hs.run(c, stage=1)
    assert ok["rc"] == 0
    assert hs.run(c, stage=1, stamp=hs.stamp)["rc"] == HIP_INVALID_VALUE                     # a used stamp
    assert hs.run(c, stage=1, n_host=c["n_regions"] - 1)["rc"] == HIP_INVALID_VALUE
    assert hs.run(c, stage=1, n_host=hs.cap + 1)["rc"] == HIP_INVALID_VALUE
    assert hs.run(c, stage=1, nlibs=NLIBS + 1)["rc"] == HIP_INVALID_VALUE
    assert hs.run(c, stage=1, period=0)["rc"] == HIP_INVALID_VALUE
    assert hs.run(c, stage=1, force_host=1, mirror_in_walk=1)["rc"] == HIP_INVALID_VALUE
    bad = dict(c)
    bad["partner"] = c["partner"].copy()
    bad["partner"][0] = c["n_reads"]
    assert hs.run(bad, stage=1)["rc"] == HIP_INVALID_VALUE
    bad = dict(c)
    bad["rec"] = c["rec"].copy()
    bad["rec"][-1, 3] += 1                                                                   # first + n behind the reads
    assert hs.run(bad, stage=1)["rc"] == HIP_INVALID_VALUE
    bad = ac.as_aggregates(c)
    bad["in_goff"] = bad["in_goff"].copy()
    bad["in_goff"][-1] += 1
    assert hs.run(bad, stage=1)["rc"] == HIP_INVALID_VALUE


@pytest.mark.parametrize("name", WALKED)
def test_groups_walk_and_table_against_the_reference(hs, tail, name):
    """the groups stage against the models, the walks' staging and the final table (full rows) against the reference; then the same table as
    wire rows with the counters mirrored by the walk and pair_lo derived, and once more with everything walked by the host"""
    c = CASES[name]
    ref = reference(c, tail)
    o = hs.run(c)
    assert o["rc"] == 0
    m = check_groups(c, o)
    dev = check_staging(c, o, ref, m)
    assert len(dev) + int(o["info"][1]) == len(ref), ("n_dev + n_host", len(dev), int(o["info"][1]), len(ref))
    check_table(c, o, ref, wire=False)
    # a component in which every region has a gate-passing group with the smallest one settles in the first round whatever order the atomics
    # take: which walk takes it is the model's to say
    comps = ac.components(c, m)
    settled = {L: v for L, v in comps.items() if ac.settles_at_once(c, m, v)}
    for v in settled.values():
        mine = {tuple(x["region"]) for x in ref if x["region"][0] in v}
        assert (mine <= dev) if ac.walker_of(c, m, v) != "host" else not (mine & dev), ("the device's share", v)
    if len(settled) == len(comps):
        check_host_list(o, host_rows(m, [r for v in comps.values() if ac.walker_of(c, m, v) == "host" for r in v]))
    o2 = hs.run(c, wire_rows=1, mirror_in_walk=1, use_pair_lo=False)
    check_groups(c, o2)
    check_table(c, o2, ref, wire=True)
    o3 = hs.run(c, force_host=1)
    check_groups(c, o3)
    assert int(o3["info"][1]) == len(ref) and int(o3["counts_dev"][18]) == 0
    check_host_list(o3, host_rows(m, range(c["n_regions"])))
    check_table(c, o3, ref, wire=False)


@pytest.mark.parametrize("name", ["order-key-128", "order-key-129"])
@pytest.mark.parametrize("ins_plain", [1, 2])
def test_the_order_key_keeps_candidates_of_one_window_and_start_apart(hs, tail, name, ins_plain):
    """128 and 129 candidates of one (window, start) through walk_big and the other routes of the insertion merge"""
    c = CASES[name]
    ref = reference(c, tail)
    o = hs.run(c, ins_plain=ins_plain)
    assert int(o["counts_dev"][18]) == len(ref) and int(o["info"][1]) == 0          # all of them from the earlier window's vertex, on the device
    check_staging(c, o, ref, None)
    check_table(c, o, ref, wire=False)


@pytest.mark.parametrize("big_walk", [0, 1])
@pytest.mark.parametrize("rounds", [1, 2, 3, 8])
@pytest.mark.parametrize("period", [1, 2, 3, 101])
def test_the_same_table_whatever_the_walks_and_rounds(hs, tail, big_walk, rounds, period):
    c = CASES["shapes-p%d-k2-b0" % period]
    ref = reference(c, tail)
    o = hs.run(c, big_walk=big_walk, propagation_rounds=rounds)
    check_staging(dict(c, big_walk=big_walk), o, ref, None)
    check_table(c, o, ref, wire=False)


@pytest.mark.parametrize("split", [1, 2, 5])
@pytest.mark.parametrize("name", ["shapes-p3-k2-b0", "gate-r2", "assemble-l5-k17-p0", "windows-p3", "many-parts"])
def test_the_aggregate_route_gives_the_same_table(hs, tail, name, split):
    """a group arriving in 1, 2 and 5 partial aggregates, in reverse key order"""
    c = CASES[name]
    d = ac.as_aggregates(c, split)
    o = hs.run(d)
    check_groups(d, o)
    check_table(d, o, reference(c, tail), wire=False)


def test_the_groups_stage_alone_with_both_mirrors_library_byte_255_and_holes(hs):
    """stage 1 with k6_mirror_kernel and with the walk's first wave mirroring; library bytes 0 and 255; a sharded rank's table with holes:
    taint on both regions of a group whose earlier region is a hole, nowhere else"""
    assert hs.run(CASES["lib-bytes"], stage=1, mirror_in_walk=1)["rc"] == HIP_INVALID_VALUE      # (the walk would look library 255 up)
    for name in ("lib-bytes", "shapes-p3-k2-b0", "reads-per-region"):
        for mirror in ((0,) if name == "lib-bytes" else (0, 1)):
            c = CASES[name]
            o = hs.run(c, stage=1, mirror_in_walk=mirror)
            assert o["rc"] == 0 and int(o["info"][0]) == 0
            check_groups(c, o)
            if not mirror:
                assert (o["sv_stage"] == FILL).all() and (o["own_first"] == FILL).all() and (o["old_key"] == np.uint64(0xA5A5A5A5A5A5A5A5)).all()
            assert (o["sv_out"] == FILL).all()
    d, want = ac.with_holes(CASES["shapes-p3-k2-b0"], (2, 13, 23))
    o = hs.run(d, stage=1)
    assert o["rc"] == 0 and int(o["info"][0]) == 0
    check_groups(d, o)
    np.testing.assert_array_equal(o["taint_out"][:d["n_regions"]], want)
    assert (o["taint_out"][d["n_regions"]:] == 0).all()
    bad = o["scratch"][3]
    for r in np.flatnonzero(want):
        assert bad[o["scratch"][1, r]] == 1, ("a tainted region's component goes to the host", r)


def test_launch_sizes_capacity_reuse_and_empties(hs, tail):
    """a host count well above the device's; g_cap at the count and one below it (the overflow word is set, nothing behind the capacity
    is written); four calls of shrinking size on the one handle; no regions at all"""
    c = CASES["shapes-p3-k2-b0"]
    ref = reference(c, tail)
    o = hs.run(c, n_host=hs.cap)
    check_groups(c, o)
    check_table(c, o, ref, wire=False)
    full = hs.run(c, stage=1, force_host=1)
    n = int(full["counts_host"][4])
    at = hs.run(c, stage=1, force_host=1, g_cap=n)
    assert int(at["counts_host"][6]) == 0 and (at["g_rec"][n:] == FILL).all() and not (at["g_rec"][:n] == FILL).all(axis=1).any()
    below = hs.run(c, stage=1, force_host=1, g_cap=n - 1)
    assert int(below["counts_host"][6]) == 1 and (below["g_rec"][n - 1:] == FILL).all() and int(below["info"][0]) == 0
    for name in ("big-64-in3", "shapes-p3-k2-b0", "gate-r2", "no-normal-reads"):
        d = CASES[name]
        o = hs.run(d)
        check_groups(d, o)
        check_table(d, o, reference(d, tail), wire=False)
    e = dict(CASES["gate-r2"], n_regions=0, n_reads=0, rec=np.zeros((0, 9), np.uint32), pk=np.zeros((0, 2), np.uint32), region_of=np.zeros(0, np.int32),
             partner=np.zeros(0, np.int32), pair_lo=np.zeros(0, np.int32), meta=np.zeros(0, np.uint32), isize=np.zeros(0, np.int32), names=[])
    for n_host in (0, 64):
        o = hs.run(e, n_host=n_host)
        assert o["rc"] == 0 and int(o["info"][0]) == 0 and (o["rs"] == FILL).all() and (o["sv_out"] == FILL).all()
        assert int(o["counts2"][8]) == 0 and int(o["counts2"][6]) == 0


STREAMS = [(seed, o) for seed in (1, 2) for o in ac.STREAM_SETS]


@pytest.mark.parametrize("seed,optset", STREAMS, ids=["%d-%s" % (s, "-".join("%s%d" % kv for kv in sorted(o.items())) or "defaults") for s, o in STREAMS])
def test_the_stream_cases_through_the_harness_and_through_the_whole_product(hs, tail, seed, optset):
    """K6's inputs from the stream through the cut and join references; the same stream once more through the whole product against the oracle"""
    import runner
    run, c = ac.stream_case(seed, optset)
    ref = ac.walk_reference(c, tail=tail)
    assert ac.differs_from_oracle(run, ref) is None
    for big_walk in (0, 1):
        o = hs.run(c, big_walk=big_walk, propagation_rounds=8 if big_walk else 2)
        check_groups(c, o)
        dev = check_staging(c, o, ref, None)
        assert len(dev) + int(o["info"][1]) == len(ref)
        check_table(c, o, ref, wire=False)
    runner.compare(run, runner.product_from_oracle(run))
