"""GPU tests of --sites: the site counter (bdx_count_site_pairs, KS) against a numpy restatement of the rule in include/bdx.h, its
argument errors, and the CLI's --sites-vcf on the chr21 golden fixtures and on a sharded run.

The rule pinned here: a site is (tid1, pos1, tid2, pos2, flag_mask), 1-based, (tid1, pos1) <= (tid2, pos2).  A record is near P on T when
tid == T and |pos + 1 - P| <= window, its mate when mtid == T and |mpos + 1 - P| <= window.  A record counts when it passes the filters
and its ReadFlag (class byte, after the pass-2 remaps) is in flag_mask, it is its pair's lower mate ((tid, pos) < (mtid, mpos), or equal
and first in pair), and it is near pos1 with its mate near pos2, or near pos2 with its mate near pos1.

The restatement is brute force over all records of the store -- no windows, no search, no gate on the reverse route -- so it shares no
logic with the kernel.  Every comparison is exact.

About ARP_RR: the pass-2 remap turns every passing RR record into FF (BreakDancer.cpp:190), so no class byte of a passing record carries
ARP_RR and the single-bit RR mask counts nothing; the RR-oriented pairs of the stores below count under FF (and FF|RR, the INV mask).  The
stores therefore have to make FF, LARGE_INSERT, SMALL_INSERT, RF and CTX each contribute, and the FF count include reverse-reverse pairs."""
import math
import os
import subprocess

import numpy as np
import pytest

from helpers import GOLDEN, ROOT, filter_cmd_lines, load_chr21, make_opts, read_bam
from runner import oracle_case, product_from_oracle

pytestmark = pytest.mark.gpu
EXE = os.path.join(ROOT, "bin", "breakdancer-max")
CWD = os.path.join(GOLDEN, "chr21")

FF, LARGE, SMALL, RF, RR, CTX = 1, 2, 3, 4, 5, 8
SINGLE_BITS = [1 << f for f in (FF, LARGE, SMALL, RF, RR, CTX)]
INV = (1 << FF) | (1 << RR)
WMAX = 1 << 30


# ---------------------------------------------------------------------------------------------------------------------------------
# numpy restatement (brute force)
# ---------------------------------------------------------------------------------------------------------------------------------
def expected_site_counts(soa, cls, keys, nkeys, sites, window):
    t, s = soa["tid"].astype(np.int64), soa["pos"].astype(np.int64)
    mt, ms = soa["mtid"].astype(np.int64), soa["mpos"].astype(np.int64)
    first = (soa["flag"].astype(np.int64) & 0x40) != 0
    ok = (cls & 0x10) != 0
    f = (cls & 15).astype(np.int64)
    lower = (t < mt) | ((t == mt) & ((s < ms) | ((s == ms) & first)))
    k = keys.astype(np.int64) if nkeys > 1 else np.zeros(len(t), np.int64)
    k = np.where(k < nkeys, k, 0)
    w = int(window)
    out = np.zeros((len(sites), nkeys), np.uint32)
    for i, (t1, p1, t2, p2, mask) in enumerate(sites):
        in_mask = ((int(mask) >> f) & 1) != 0
        r1, r2 = (t == t1) & (np.abs(s + 1 - p1) <= w), (t == t2) & (np.abs(s + 1 - p2) <= w)
        m1, m2 = (mt == t1) & (np.abs(ms + 1 - p1) <= w), (mt == t2) & (np.abs(ms + 1 - p2) <= w)
        hit = ok & in_mask & lower & ((r1 & m2) | (r2 & m1))
        out[i] = np.bincount(k[hit], minlength=nkeys)[:nkeys]
    return out


def genotype(dr, dv):
    """the documented model: alt-read probability 0.01 / 0.5 / 0.99, PL rounded half away from zero, GQ = second-smallest PL capped at 99"""
    if dr is None or dv is None or dr + dv == 0:
        return None
    lk = [dv * math.log10(p) + dr * math.log10(1.0 - p) for p in (0.01, 0.5, 0.99)]
    best = max(lk)
    pl = []
    for x in lk:
        v = -10.0 * (x - best)
        fl = math.floor(v)
        pl.append(int(fl + 1 if v - fl >= 0.5 else fl))
    gt = min(range(3), key=lambda g: (pl[g], g))
    return ("0/0", "0/1", "1/1")[gt], min(99, sorted(pl)[1]), pl


# ---------------------------------------------------------------------------------------------------------------------------------
# hand-built stores
# ---------------------------------------------------------------------------------------------------------------------------------
TARGETS = ["c0", "c1", "c2", "c3"]          # c2 never has a read; tid 4 is beyond the header
ONE_LIB = [("rg0", "a.bam", "lib0", 400.0, 30.0)]
THREE_LIBS = [("rg0", "a.bam", "lib0", 400.0, 30.0), ("rg1", "a.bam", "lib1", 350.0, 40.0), ("rg2", "b.bam", "lib2", 500.0, 50.0)]
RL = 100
FAR = 2_000_000_000                          # c3 ends near 2^31: positions whose window arithmetic does not fit 32 bits


def config_text(libs):
    return "".join("readgroup:%s\tplatform:illumina\tmap:%s\treadlen:%d.00\tlib:%s\tlower:%.2f\tupper:%.2f\tmean:%.2f\tstd:%.2f\n"
                   % (rg, bam, RL, lib, mean - 3 * std, mean + 3 * std, mean, std) for rg, bam, lib, mean, std in libs)


class Store:
    def __init__(self, libs):
        self.libs = libs
        self.bams = sorted({l[1] for l in libs})
        self.recs = [[] for _ in self.bams]
        self.names = 0
        self.clusters = []   # (kind, ta, a, tb, b): 0-based start positions of the two ends

    def pair(self, li, ta, pa, tb, pb, ra, rb, mapq=60, both=True):
        """one read pair: the first mate at (ta, pa), the second at (tb, pb); ra / rb: on the reverse strand; both=False: the second
        mate's record is not in the store"""
        self.names += 1
        isz = (pb + RL - pa) if ta == tb else 0
        fa = 0x1 | 0x40 | (0x10 if ra else 0) | (0x20 if rb else 0)
        fb = 0x1 | 0x80 | (0x10 if rb else 0) | (0x20 if ra else 0)
        rg, bam = self.libs[li][0], self.bams.index(self.libs[li][1])
        self.recs[bam].append(dict(tid=ta, pos=pa, mtid=tb, mpos=pb, isize=isz, flag=fa, qlen=RL, bdqual=mapq, rg=rg, name=self.names))
        if both:
            self.recs[bam].append(dict(tid=tb, pos=pb, mtid=ta, mpos=pa, isize=-isz, flag=fb, qlen=RL, bdqual=mapq, rg=rg, name=self.names))

    def cluster(self, rng, kind, ta, a, tb, b, n, spread=100, mapq=60):
        """n pairs of one kind with their first mates within `spread` of (ta, a): the second mate's place follows from the kind for the
        insert-size classes (b is then the mean of where they land) and lies within `spread` of (tb, b) otherwise"""
        ends = []
        for _ in range(n):
            li = int(rng.integers(0, len(self.libs)))
            mean, std = self.libs[li][3], self.libs[li][4]
            pa = a + int(rng.integers(0, spread + 1))
            if kind in ("normal", "large", "small"):
                ins = {"normal": mean + rng.uniform(-1, 1) * std, "large": mean + rng.uniform(6, 12) * std, "small": mean - rng.uniform(5, 7) * std}[kind]
                pb = pa + max(int(ins), RL + 1) - RL
            else:
                pb = b + int(rng.integers(0, spread + 1))
            ra, rb = {"ff": (False, False), "rr": (True, True), "rf": (True, False)}.get(kind, (False, True))
            if ta == tb and pb < pa:
                pa, pb = pb, pa
            self.pair(li, ta, pa, tb, pb, ra, rb, mapq=mapq)
            ends.append(pb)
        self.clusters.append((kind, ta, a, tb, int(np.mean(ends)) if kind in ("normal", "large", "small") else b))

    def streams(self):
        out = []
        for rr in self.recs:
            rr = sorted(rr, key=lambda r: (r["tid"], r["pos"]))
            d = {k: np.array([r[k] for r in rr], dtype=dt) for k, dt in
                 (("tid", np.int32), ("pos", np.int32), ("mtid", np.int32), ("mpos", np.int32), ("isize", np.int32), ("flag", np.uint16),
                  ("qlen", np.int32), ("bdqual", np.uint8))}
            d["rg"] = [r["rg"] for r in rr]
            d["name_id"] = np.array([r["name"] for r in rr], dtype=np.uint64)
            out.append(d)
        return out

    def n_records(self):
        return sum(len(r) for r in self.recs)


KIND_MASK = dict(ff=1 << FF, rr=1 << FF, large=1 << LARGE, small=1 << SMALL, rf=1 << RF, ctx=1 << CTX, normal=1 << LARGE)


def small_store(libs, n_records, seed):
    """n_records records on c0 and c1: FF, RF and CTX pairs around two places, and -- an odd count -- one CTX record whose mate is absent"""
    rng = np.random.default_rng(seed)
    st = Store(libs)
    if n_records % 2:
        st.pair(0, 0, 1000, 1, 5000, False, True, both=False)
        st.clusters.append(("ctx", 0, 1000, 1, 5000))
    kinds = [("ff", 0, 900, 0, 3000), ("ctx", 0, 950, 1, 5000), ("rf", 1, 4000, 1, 9000), ("rr", 0, 1000, 0, 1400)]
    per = (n_records // 2 + len(kinds) - 1) // len(kinds)
    left = n_records // 2
    for kind, ta, a, tb, b in kinds:
        n = min(per, left)
        left -= n
        if n:
            st.cluster(rng, kind, ta, a, tb, b, n)
    assert st.n_records() == n_records
    return st


def big_store(libs, seed):
    """about 5,000 records on c0, c1 and c3: clusters of every anomalous class, normal and failing pairs between them, the store's first
    records within a window of position 1, its last ones near 2^31, and the special pairs of special_sites()"""
    rng = np.random.default_rng(seed)
    st = Store(libs)
    kinds = ["ff", "rr", "large", "small", "rf", "ctx"]
    st.cluster(rng, "ff", 0, 150, 0, 2500, 20)            # the store begins inside the first site's window
    lengths = {0: 3_000_000, 1: 2_000_000, 3: 1_500_000}
    for c in range(66):
        kind = kinds[c % len(kinds)]
        ta = (0, 1, 3)[int(rng.integers(0, 3))]
        a = int(rng.integers(20_000, lengths[ta] - 20_000))
        if kind == "ctx":
            tb = (0, 1, 3)[((0, 1, 3).index(ta) + 1 + int(rng.integers(0, 2))) % 3]
            b = int(rng.integers(20_000, lengths[tb] - 20_000))
            if tb < ta:
                ta, a, tb, b = tb, b, ta, a
        else:
            tb, b = ta, a + int(rng.integers(300, 5000))
        st.cluster(rng, kind, ta, a, tb, b, int(rng.integers(14, 36)))
    for kind, mapq in (("normal", 60), ("ff", 0), ("large", 0), ("ctx", 0), ("normal", 60), ("rf", 10)):   # normal pairs, and ones that fail -q
        for _ in range(6):
            ta = (0, 1, 3)[int(rng.integers(0, 3))]
            a = int(rng.integers(20_000, lengths[ta] - 20_000))
            tb = ta if kind != "ctx" else (0, 1, 3)[((0, 1, 3).index(ta) + 1) % 3]
            if tb < ta:
                ta, tb = tb, ta
            st.cluster(rng, kind, ta, a, tb, a + 2000, 20, mapq=mapq)
    # special pairs on c1, far from everything else (special_sites)
    st.pair(0, 1, 1_900_000, 1, 1_900_000, False, False)                   # both records at one (tid, pos): FF, only the first in pair counts
    st.pair(0, 1, 1_910_000, 1, 1_910_060, False, False)                   # near both ends of a short site by both routes
    for d in range(0, 8):
        st.pair(0, 1, 1_920_000 + 499 + d - 4, 1, 1_920_000 + 499 + d - 4 + (d % 3), True, False)   # tight RF pairs around where two windows meet
    st.cluster(rng, "ff", 3, FAR, 3, FAR + 3000, 12)                       # the store's last records; c3 "ends" near 2^31
    st.cluster(rng, "ctx", 1, 1_950_000, 3, FAR + 10_000, 9)
    return st


def special_sites(w):
    """the sites that go with big_store's special pairs, for window w"""
    s = [(1, 1_900_001, 1, 1_900_001, 1 << FF), (1, 1_900_001, 1, 1_900_001, INV),
         (1, 1_910_011, 1, 1_910_051, 1 << FF)]
    base = 1_920_000 + 500 - w            # pos1; the tight RF pairs start around pos1 - 1 + w
    if base >= 1:
        for gap in sorted({0, max(2 * w - 1, 0), 2 * w, 2 * w + 1}):
            for shift in (-1, 0, 1, 3):
                s.append((1, base + shift, 1, base + shift + gap, 1 << RF))
    return s


def make_sites(st, soa, cls, rng, w):
    """sites for a store at window w: every cluster with its own mask, with every other single-bit mask and FF|RR, with its ends moved by up
    to 1.4 windows; sites laid exactly on records (what window 0 can match); the special ones; chromosomes without reads"""
    sites = []
    for kind, ta, a, tb, b in st.clusters:
        own = KIND_MASK[kind]
        sites.append((ta, a + 51, tb, b + 51, own))
        sites.append((ta, a + 51, tb, b + 51, INV))
        sites.append((ta, a + 51, tb, b + 51, SINGLE_BITS[int(rng.integers(0, 6))]))
        j = max(int(1.4 * w), 2)
        sites.append((ta, max(a + 51 + int(rng.integers(-j, j)), 1), tb, max(b + 51 + int(rng.integers(-j, j)), 1), own))
    t, s, mt, ms = (soa[k].astype(np.int64) for k in ("tid", "pos", "mtid", "mpos"))
    lower = np.nonzero((t < mt) | ((t == mt) & (s <= ms)))[0]
    for i in rng.choice(lower, size=min(60, len(lower)), replace=False):
        f = int(cls[i]) & 15
        mask = (1 << f) if f in (FF, LARGE, SMALL, RF, CTX) else SINGLE_BITS[int(rng.integers(0, 6))]
        sites.append((int(t[i]), int(s[i]) + 1, int(mt[i]), int(ms[i]) + 1, mask))
        sites.append((int(t[i]), int(s[i]) + 1 + w, int(mt[i]), int(ms[i]) + 1 + w, mask))          # the window's last position ...
        sites.append((int(t[i]), int(s[i]) + 2 + w, int(mt[i]), int(ms[i]) + 1, mask))              # ... and one past it
    sites += special_sites(w)
    sites += [(2, 1, 2, 5000, 1 << LARGE), (0, 1000, 2, 5, 1 << CTX), (2, 700, 3, 5, 1 << CTX), (4, 10, 4, 20, 1 << FF), (1, 10, 4, 20, 1 << CTX),
              (0, 1, 0, 1, 1 << FF), (0, 1, 0, 2600, INV), (3, FAR + 1, 3, FAR + 3001, INV), (3, FAR + 200, 3, 2**31 - 1, 1 << FF),
              (3, 2**31 - 1, 3, 2**31 - 1, 1 << FF)]
    norm = []
    for t1, p1, t2, p2, m in sites:
        p1, p2 = min(max(p1, 1), 2**31 - 1), min(max(p2, 1), 2**31 - 1)
        norm.append((t1, p1, t2, p2, m) if (t1, p1) <= (t2, p2) else (t2, p2, t1, p1, m))
    return norm


STORES = {}


def store_case(label):
    """(oracle run, store, merged stream) of a labelled store: built and run through the oracle once, shared by the tests"""
    if label not in STORES:
        libs = ONE_LIB if label.startswith("one") else THREE_LIBS
        size = label.split("/")[1]
        st = big_store(libs, 11 + len(label)) if size == "big" else small_store(libs, int(size), 7 + int(size))
        run = oracle_case(config_text(libs), st.streams(), TARGETS, make_opts(illumina_long_insert=int(label.endswith("/l"))))
        STORES[label] = (run, st, run.merged_soa())
    return STORES[label]


def coverage(run, st, soa, w=500):
    """(share of the sites with a non-zero expected count, the class flags that contribute to one, whether a reverse-reverse pair does)"""
    rng = np.random.default_rng(5)
    sites = make_sites(st, soa, run.cls, rng, w)
    exp = expected_site_counts(soa, run.cls, soa["bam"], 1, sites, w)[:, 0]
    flags = set()
    rr_counts = False
    rr = ((soa["flag"] & 0x10) != 0) & ((soa["flag"] & 0x20) != 0)
    for f in (FF, LARGE, SMALL, RF, RR, CTX):
        only = (run.cls & 15) == f
        cls_f = np.where(only, run.cls, 0).astype(np.uint8)
        if expected_site_counts(soa, cls_f, soa["bam"], 1, sites, w).any():
            flags.add(f)
    if expected_site_counts(soa, np.where(rr, run.cls, 0).astype(np.uint8), soa["bam"], 1, sites, w).any():
        rr_counts = True
    return float((exp > 0).mean()), flags, rr_counts


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. the kernel against the restatement
# ---------------------------------------------------------------------------------------------------------------------------------
LABELS = ["one/1", "one/63", "one/64", "one/65", "one/big", "three/65", "three/big", "three/big/l"]


@pytest.mark.parametrize("label", LABELS)
def test_site_counts_equal_numpy_restatement(label):
    from breakdancer_amd import _lib
    run, st, soa = store_case(label)
    n = len(soa["tid"])
    if "big" in label:
        assert 4500 < n < 6500 and not (soa["tid"] == 2).any()
        share, flags, rr_counts = coverage(run, st, soa)
        assert share > 0.3 and rr_counts, (share, rr_counts)       # (no empty comparison: checked on the oracle alone, before the GPU is used)
        if not label.endswith("/l"):
            assert flags == {FF, LARGE, SMALL, RF, CTX}, flags     # (ARP_RR: see the module's docstring)
    else:
        assert n == int(label.split("/")[1])
    bd = product_from_oracle(run)
    np.testing.assert_array_equal(bd.read_class() & 0x3F, run.cls)   # (what K1 wrote is what the restatement reads)
    nlibs, nbams = run.nlibs, run.nbams
    rng = np.random.default_rng(len(label))
    nonzero = 0
    for w in (0, 500, WMAX):
        sites = make_sites(st, soa, run.cls, rng, w)
        arr = np.array(sites, dtype=_lib.SITE_DTYPE)
        for by_library, keys, nkeys in ((False, soa["bam"], nbams), (True, soa["lib"], nlibs)):
            exp = expected_site_counts(soa, run.cls, keys, nkeys, sites, w)
            got = bd.count_site_pairs(arr, w, by_library=by_library)
            assert got.shape == (len(sites), nkeys) and got.dtype == np.uint32
            np.testing.assert_array_equal(got, exp, err_msg="%s window=%d by_library=%s" % (label, w, by_library))
            nonzero += int((exp > 0).sum())
            for nq in (1, 4, 5):   # one block with idle waves, a full one, and one wave into the second
                order = rng.permutation(len(sites))[:nq]
                np.testing.assert_array_equal(bd.count_site_pairs(arr[order], w, by_library=by_library), exp[order])
    assert nonzero > 0
    assert bd.count_site_pairs([], 500).shape == (0, nbams)
    assert bd.count_site_pairs([(0, 1001, 1, 5001, 1 << CTX)], 500).shape == (1, nbams)   # (a sequence of tuples is taken as well)
    bd.close()


def test_site_counts_refuse_bad_calls():
    import ctypes as C
    import breakdancer_amd as bda
    from breakdancer_amd import _lib
    from breakdancer_amd.api import LibraryConfig
    from runner import product_options
    run, st, soa = store_case("one/65")
    lib = _lib.load()
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    good = np.array([(0, 1001, 1, 5001, 1 << CTX)], dtype=_lib.SITE_DTYPE)
    out = np.zeros(4, np.uint32)
    libs = [LibraryConfig(*[float(x) for x in run.lib_f[i]], min_mapping_quality=int(run.lib_i[i, 0]), bam_file_index=int(run.lib_i[i, 1]))
            for i in range(run.nlibs)]
    fresh = bda.BreakDancer(product_options(run.opts), libs, run.nbams, ntids=0, max_read_window_size=run.w0)
    assert lib.bdx_count_site_pairs(fresh.h, p(good), 1, 500, 0, p(out)) == 4          # BDX_ESTATE: no run yet
    fresh.close()
    bd = product_from_oracle(run)
    assert lib.bdx_count_site_pairs(bd.h, p(good), 1, 500, 0, p(out)) == 0
    assert lib.bdx_count_site_pairs(bd.h, None, 0, 500, 0, None) == 0                   # n == 0, null pointers
    assert lib.bdx_count_site_pairs(bd.h, None, 1, 500, 0, p(out)) == 1                 # BDX_EINVAL from here on: a null array
    assert lib.bdx_count_site_pairs(bd.h, p(good), 1, 500, 0, None) == 1
    bad_sites = [(-1, 10, 0, 10, 1 << FF), (0, 10, -1, 10, 1 << FF), (0, 0, 0, 10, 1 << FF), (0, 10, 0, 0, 1 << FF), (-2, 10, -1, 10, 1 << FF),
                 (1, 10, 0, 10, 1 << CTX), (0, 11, 0, 10, 1 << FF),                       # not normalised
                 (0, 10, 0, 10, 0), (0, 10, 0, 10, 1 << 0), (0, 10, 0, 10, 1 << 6), (0, 10, 0, 10, 1 << 7), (0, 10, 0, 10, 1 << 9),
                 (0, 10, 0, 10, 1 << 10), (0, 10, 0, 10, (1 << FF) | (1 << 11)), (0, 10, 0, 10, 1 << 31)]
    for s in bad_sites:
        a = np.array([good[0].tolist(), s], dtype=_lib.SITE_DTYPE)
        assert lib.bdx_count_site_pairs(bd.h, p(a), 2, 500, 0, p(out)) == 1, s
    for w in (-1, WMAX + 1, -2**31):
        assert lib.bdx_count_site_pairs(bd.h, p(good), 1, w, 0, p(out)) == 1, w
    assert lib.bdx_count_site_pairs(bd.h, p(good), 1, WMAX, 0, p(out)) == 0 and lib.bdx_count_site_pairs(bd.h, p(good), 1, 0, 0, p(out)) == 0
    assert lib.bdx_count_site_pairs(bd.h, p(good), 2**31 + 1, 500, 0, p(out)) == 5         # BDX_ELIMIT (checked before any site is read)
    bd.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. the CLI on the chr21 golden fixtures
# ---------------------------------------------------------------------------------------------------------------------------------
def run_cli(args, cwd=CWD, cfg="inv_del_bam_config", env=None):
    p = subprocess.run([EXE] + args + [cfg], cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       env=dict(os.environ, **env) if env else None, timeout=300)
    assert p.returncode == 0, p.stderr.decode()
    return p.stdout.decode()


def table_rows(text):
    return [l.split("\t") for l in text.split("\n") if l and not l.startswith("#")]


def vcf_parts(text):
    lines = text.rstrip("\n").split("\n")
    meta = [l for l in lines if l.startswith("##")]
    head = [l for l in lines if l.startswith("#CHROM")]
    assert lines[0] == "##fileformat=VCFv4.2" and len(head) == 1
    cols = head[0].split("\t")
    recs = [l.split("\t") for l in lines if not l.startswith("#")]
    info_ids = {l.split("ID=")[1].split(",")[0] for l in meta if l.startswith("##INFO=")}
    for r in recs:
        assert len(r) == len(cols) and r[8] == "GT:GQ:PL:DR:DV"
        assert {kv.split("=")[0] for kv in r[7].split(";")} <= info_ids
    return meta, cols[9:], recs


def without_command(text):
    return "\n".join(l for l in text.split("\n") if not l.startswith("##command="))


TYPE_MASK = dict(DEL=1 << LARGE, INS=1 << SMALL, INV=INV, ITX=1 << RF, CTX=1 << CTX)   # without -l


def default_window(run):
    return int(max(math.ceil(float(run.lib_f[i][2])) for i in range(run.nlibs)))


def check_sites_vcf(table, text, vcf_text, run, targets, by_lib, sites_file):
    rows = table_rows(table)
    meta, samples, recs = vcf_parts(text)
    assert samples == (run.lib_names if by_lib else [os.path.basename(b) for b in run.bam_names])
    w = default_window(run)
    assert "##sites=" + sites_file in meta and "##sites_window=%d" % w in meta
    assert len(recs) == len(rows) > 0
    by_id = {r[2]: r for r in recs}
    vcf_by_id = {r[2]: r for r in vcf_parts(vcf_text)[2]}
    sites = []
    for row in rows:
        a, b = (targets.index(row[0]), int(row[1])), (targets.index(row[3]), int(row[4]))
        lo, hi = min(a, b), max(a, b)
        sites.append((lo[0], lo[1], hi[0], hi[1], TYPE_MASK[row[6]]))
    soa = run.merged_soa()
    keys, nkeys = (soa["lib"], run.nlibs) if by_lib else (soa["bam"], run.nbams)
    dv_exp = expected_site_counts(soa, run.cls, keys, nkeys, sites, w)
    assert dv_exp.sum() > 0
    for k, row in enumerate(rows):
        r = by_id["SITE%d" % (k + 1)]
        assert r[0] == row[0] and r[1] == row[1] and r[3] == "N" and r[4] == "<%s>" % row[6] and r[5] == "." and r[6] == "PASS"
        info = dict(kv.split("=") if "=" in kv else (kv, None) for kv in r[7].split(";"))
        assert set(info) <= {"IMPRECISE", "SVTYPE", "CHR2", "POS2", "END", "SVLEN"}
        assert "IMPRECISE" in info and info["SVTYPE"] == row[6] and info["CHR2"] == row[3] and info["POS2"] == row[4]
        assert ("END" in info) == (row[0] == row[3] and int(row[4]) >= int(row[1])) and info.get("END", row[4]) == row[4]
        assert ("SVLEN" in info) == (row[6] in ("DEL", "INS")) and (row[6] not in ("DEL", "INS") or int(info["SVLEN"]) == -int(row[7]))
        v = vcf_by_id["BDX%d" % (k + 1)]
        for j, f in enumerate(r[9:]):
            gt, gq, pl, dr, dv = f.split(":")
            assert int(dv) == int(dv_exp[k, j]), (k, j, f)
            assert dr == v[9 + j].split(":")[3], (k, j, f, v[9 + j])     # the DR of the same run's --vcf record for that row
            g = genotype(int(dr), int(dv))
            if g is None:
                assert (gt, gq, pl) == ("./.", ".", ".")
            else:
                assert (gt, int(gq), [int(x) for x in pl.split(",")]) == g, f


@pytest.mark.parametrize("args", [[], ["-a", "-o", "21"]], ids=["per-bam", "per-library-dash-o"])
def test_cli_sites_vcf_on_the_golden_fixture(args, tmp_path):
    by_lib = "-a" in args
    plain = run_cli(args)
    sites_file = str(tmp_path / "table.txt")
    open(sites_file, "w").write(plain)                       # a run's own stdout, fed back
    out, vcf, vcf0 = str(tmp_path / "sites.vcf"), str(tmp_path / "calls.vcf"), str(tmp_path / "calls0.vcf")
    with_sites = run_cli(["--sites", sites_file, "--sites-vcf", out, "--vcf", vcf] + args)
    without = run_cli(["--vcf", vcf0] + args)
    assert filter_cmd_lines(with_sites) == filter_cmd_lines(plain) == filter_cmd_lines(without)   # (the #Command line names the options)
    assert without_command(open(vcf).read()) == without_command(open(vcf0).read())
    run = load_chr21(make_opts(cn_lib=int(by_lib), chr_tid=22 if "-o" in args else -1)).run()
    targets = read_bam(os.path.join(CWD, run.bam_names[0]))[0]
    check_sites_vcf(plain, open(out).read(), open(vcf).read(), run, targets, by_lib, sites_file)


def test_cli_sites_vcf_is_the_same_through_the_host_decode_the_cache_and_a_mask_elsewhere(tmp_path):
    """BDX_DECODE=host, -C then -R (the cache keeps the command line, -R reads FILE again) and an --exclude mask that drops nothing: the same
    records are held, so OUT is the same apart from its ##command= / ##exclude= lines"""
    sites_file, out = str(tmp_path / "table.txt"), str(tmp_path / "sites.vcf")
    open(sites_file, "w").write(run_cli(["-o", "21"]))
    sargs = ["--sites", sites_file, "--sites-vcf", out, "-o", "21"]
    body = lambda: "\n".join(l for l in open(out).read().split("\n") if not l.startswith(("##command=", "##exclude=")))
    table = run_cli(sargs)
    ref = body()
    assert any(int(f.split(":")[4]) > 0 for r in vcf_parts(open(out).read())[2] for f in r[9:])
    os.remove(out)
    assert filter_cmd_lines(run_cli(sargs, env=dict(BDX_DECODE="host"))) == filter_cmd_lines(table) and body() == ref
    os.remove(out)
    cache = str(tmp_path / "pass1.cache")
    assert filter_cmd_lines(run_cli(["-C", cache] + sargs)) == filter_cmd_lines(table) and body() == ref
    os.remove(out)
    p = subprocess.run([EXE, "-R", cache], cwd=CWD, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert p.returncode == 0, p.stderr.decode()
    assert filter_cmd_lines(p.stdout.decode()) == filter_cmd_lines(table) and body() == ref
    os.remove(out)
    mask = tmp_path / "mask.bed"
    mask.write_text("21\t0\t10\n")
    assert filter_cmd_lines(run_cli(["--exclude", str(mask)] + sargs)) == filter_cmd_lines(table) and body() == ref
    assert "##exclude=" + str(mask) in open(out).read()


def test_cli_sites_on_a_chromosome_the_run_did_not_read_are_unknown(tmp_path):
    targets = read_bam(os.path.join(CWD, "NA19238_chr21_del_inv.bam"))[0]
    other = [t for t in targets if t != "21"][0]
    sites_file = str(tmp_path / "s.txt")
    open(sites_file, "w").write("%s\t100\t1+1-\t%s\t900\t1+1-\tDEL\t800\n21\t29185056\t1+1-\t21\t29185377\t1+1-\tDEL\n" % (other, other) +
                                "21\t500\t1+0-\t%s\t700\t0+1-\tCTX\t-1\n" % other)
    out = str(tmp_path / "o.vcf")
    run_cli(["--sites", sites_file, "--sites-vcf", out, "--sites-window", "300", "-o", "21"])
    meta, samples, recs = vcf_parts(open(out).read())
    assert "##sites_window=300" in meta
    by_id = {r[2]: r for r in recs}
    assert all(f == "./.:.:.:.:." for f in by_id["SITE1"][9:]) and all(f == "./.:.:.:.:." for f in by_id["SITE3"][9:])
    assert all(f.split(":")[3] != "." and f.split(":")[4] != "." for f in by_id["SITE2"][9:])
    assert "SVLEN=-800" in by_id["SITE1"][7] and "SVLEN" not in by_id["SITE2"][7]          # (no Size column, no SVLEN)


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. a sharded run
# ---------------------------------------------------------------------------------------------------------------------------------
def test_cli_sites_vcf_sharded_equals_one_gpu(tmp_path):
    from exclude_cases import write_case
    from fuzzgen import make_case
    rng = np.random.default_rng(3)
    cfg, streams, targets = make_case(913, n_pairs=1400)
    write_case(str(tmp_path), streams, targets, rng)
    (tmp_path / "cfg").write_text(cfg)
    d = str(tmp_path)
    args = ["-y", "-1", "-r", "1"]
    table = run_cli(args, cwd=d, cfg="cfg")
    # (the fuzz input is messy enough for the walk to join regions of two sequences under a same-chromosome type; --sites calls such a line
    # malformed, so the table goes back without them)
    kept = [l for l in table.split("\n") if l.startswith("#") or not l or (l.split("\t")[6] == "CTX") == (l.split("\t")[0] != l.split("\t")[3])]
    assert len(table_rows("\n".join(kept))) > 0
    table = "\n".join(kept)
    (tmp_path / "table.txt").write_text(table)
    sargs = ["--sites", "table.txt", "--sites-vcf", "sites.vcf", "--vcf", "calls.vcf"] + args
    one = run_cli(sargs, cwd=d, cfg="cfg")
    assert filter_cmd_lines(one) == filter_cmd_lines(run_cli(args, cwd=d, cfg="cfg"))
    ref, ref_calls = open(os.path.join(d, "sites.vcf")).read(), open(os.path.join(d, "calls.vcf")).read()
    meta, samples, recs = vcf_parts(ref)
    assert len(recs) == len(table_rows(table))
    ctx = [r for r in recs if r[4] == "<CTX>"]
    assert ctx and any(int(f.split(":")[4]) > 0 for r in ctx for f in r[9:])           # a CTX site with support, counted on tid1's rank
    assert any(int(f.split(":")[3]) > 0 for r in recs for f in r[9:])
    for gpus in ("0,0", "0,0,0"):
        out = run_cli(sargs, cwd=d, cfg="cfg", env=dict(BDX_GPUS=gpus))
        assert filter_cmd_lines(out) == filter_cmd_lines(one)
        assert open(os.path.join(d, "sites.vcf")).read() == ref, gpus
        assert open(os.path.join(d, "calls.vcf")).read() == ref_calls, gpus
