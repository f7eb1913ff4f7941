"""Python mirror of the reference's interface for the clustering path.

Names follow the reference: `Options` (common/Options.hpp:24-45, same field names), `LibraryConfig`
(io/LibraryConfig.hpp:11-24) and `BreakDancer` (breakdancer/BreakDancer.hpp:30-99: construct, feed reads, run).
Errors surface as `BdxError` the way the reference's exceptions surface as "ERROR: ..." in main()."""
import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _lib as L

FLAG_NAMES = ["NA", "ARP_FF", "ARP_LARGE_INSERT", "ARP_SMALL_INSERT", "ARP_RF", "ARP_RR", "NORMAL_FR", "NORMAL_RF",
              "ARP_CTX", "MATE_UNMAPPED", "UNMAPPED"]


class BdxError(RuntimeError):
    pass


@dataclass
class Options:
    """common/Options.cpp:27-41 defaults"""
    min_len: int = 7
    cut_sd: int = 3
    max_sd: int = 1000000000
    min_map_qual: int = 35
    min_read_pair: int = 2
    seq_coverage_lim: int = 1000
    buffer_size: int = 100
    transchr_rearrange: bool = False
    fisher: bool = False
    Illumina_long_insert: bool = False
    CN_lib: bool = False
    print_AF: bool = False
    score_threshold: int = 30
    chr: str = ""

    def to_c(self):
        o = L.bdx_opts()
        o.min_len, o.cut_sd, o.max_sd, o.min_map_qual = self.min_len, self.cut_sd, self.max_sd, self.min_map_qual
        o.min_read_pair, o.seq_coverage_lim, o.buffer_size = self.min_read_pair, self.seq_coverage_lim, self.buffer_size
        o.transchr_rearrange, o.fisher = int(self.transchr_rearrange), int(self.fisher)
        o.illumina_long_insert, o.cn_lib, o.print_af = int(self.Illumina_long_insert), int(self.CN_lib), int(self.print_AF)
        o.score_threshold = self.score_threshold
        o.chr_restricted = 1 if self.chr else 0
        return o


@dataclass
class LibraryConfig:
    mean_insertsize: float
    std_insertsize: float
    uppercutoff: float
    lowercutoff: float
    readlens: float
    min_mapping_quality: int = -1
    bam_file_index: int = 0
    name: str = ""


BATCH_FIELDS = (("tid", np.int32), ("pos", np.int32), ("mtid", np.int32), ("mpos", np.int32), ("isize", np.int32),
                ("flag", np.uint16), ("qlen", np.uint16), ("mapq", np.uint8), ("lib", np.uint8), ("bam", np.uint8),
                ("name_key", np.uint64))


def make_batch(arrs):
    """dict of numpy arrays -> (bdx_batch, keepalive list).  Accepts 'bdqual' for mapq and 'name_id' for name_key."""
    b = L.bdx_batch()
    keep = []
    n = None
    for k, dt in BATCH_FIELDS:
        src = arrs.get(k)
        if src is None and k == "mapq":
            src = arrs.get("bdqual")
        if src is None and k == "name_key":
            src = arrs.get("name_id")
        if src is None:
            raise KeyError(k)
        a = np.ascontiguousarray(src, dtype=dt)
        if n is None:
            n = len(a)
        elif len(a) != n:
            raise ValueError("ragged batch: %s has %d rows, expected %d" % (k, len(a), n))
        keep.append(a)
        setattr(b, k, a.ctypes.data_as(C.c_void_p))
    if arrs.get("name_check") is not None:  # the second name hash (looked at after use_name_check() only)
        a = np.ascontiguousarray(arrs["name_check"], dtype=np.uint64)
        if len(a) != (n or 0):
            raise ValueError("ragged batch: name_check has %d rows, expected %d" % (len(a), n or 0))
        keep.append(a)
        b.name_check = a.ctypes.data_as(C.c_void_p)
    b.n = n or 0
    return b, keep


def lib_array(libs):
    """list of LibraryConfig -> ctypes array of bdx_lib"""
    arr = (L.bdx_lib * len(libs))()
    for i, l in enumerate(libs):
        arr[i].mean_insertsize, arr[i].std_insertsize = l.mean_insertsize, l.std_insertsize
        arr[i].uppercutoff, arr[i].lowercutoff, arr[i].readlens = l.uppercutoff, l.lowercutoff, l.readlens
        arr[i].min_mapping_quality, arr[i].bam_index = l.min_mapping_quality, l.bam_file_index
    return arr


def run_many(contexts, in_flight=3):
    """bdx_run_many: every context of the list runs, `in_flight` of them at a time (the native driver for one context per chromosome)"""
    lib = L.load()
    arr = (C.c_void_p * len(contexts))(*[c.h for c in contexts])
    rc = lib.bdx_run_many(arr, len(contexts), in_flight)
    if rc != 0:
        msgs = [lib.bdx_last_error(c.h).decode() for c in contexts]
        raise BdxError("bdx_run_many: %s (%s)" % (lib.bdx_strerror(rc).decode(), "; ".join(m for m in msgs if m)))
    for c in contexts:
        c._keep.clear()
    return contexts


class BreakDancer:
    """One clustering context on one GPU (reference: BreakDancer::BreakDancer / run, BreakDancer.cpp:87-144)."""

    def __init__(self, opts, libs, nbams, ntids=0, max_read_window_size=100000000, device=0):
        self.lib = L.load()
        self.opts = opts
        self.libs = list(libs)
        self.nlibs, self.nbams = len(self.libs), nbams
        co = opts.to_c()
        arr = lib_array(self.libs)
        self.h = C.c_void_p()
        rc = self.lib.bdx_create(C.byref(self.h), C.byref(co), arr, self.nlibs, nbams, ntids, max_read_window_size, device)
        if rc != 0:
            self.h = C.c_void_p()
            raise BdxError("bdx_create: %s" % self.lib.bdx_strerror(rc).decode())
        self._keep = []
        self._n_held = 0   # records pushed or streamed through this object since the last reset_reads (get_clips' default row count)

    @classmethod
    def borrow(cls, handle, opts, libs, nbams):
        """wrap a context that somebody else owns (a chromosome or the result of a sharded run, dist.py): never destroyed here"""
        self = cls.__new__(cls)
        self.lib = L.load()
        self.opts, self.libs = opts, list(libs)
        self.nlibs, self.nbams = len(self.libs), nbams
        self.h = C.c_void_p(handle)
        self._keep = []
        self._n_held = 0
        self._borrowed = True
        return self

    def _chk(self, rc, what):
        if rc != 0:
            raise BdxError("%s: %s (%s)" % (what, self.lib.bdx_strerror(rc).decode(),
                                           self.lib.bdx_last_error(self.h).decode()))

    def close(self):
        if getattr(self, "_borrowed", False):
            self.h = C.c_void_p()
            return
        if getattr(self, "h", None) is not None and self.h.value:
            self.lib.bdx_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def use_name_check(self, on=True):
        """every batch carries 'name_check', a second hash of the read name: mates must agree in it as well (bdx_use_name_check)"""
        self._chk(self.lib.bdx_use_name_check(self.h, 1 if on else 0), "bdx_use_name_check")
        return self

    def mark_duplicates(self, on=True):
        """duplicate read pairs get SAM flag 0x400 on the GPU before the classifier reads the flags (bdx_set_mark_duplicates; the rule is in
        include/bdx.h); while the context holds no reads"""
        self._chk(self.lib.bdx_set_mark_duplicates(self.h, 1 if on else 0), "bdx_set_mark_duplicates")
        return self

    def duplicates(self):
        """(records marked, groups of two or more) of the last run (bdx_get_duplicates)"""
        m, g = C.c_uint64(0), C.c_uint64(0)
        self._chk(self.lib.bdx_get_duplicates(self.h, C.byref(m), C.byref(g)), "bdx_get_duplicates")
        return m.value, g.value

    def insert_size_histogram(self):
        """(hist[nlibs][ISIZE_BINS], n_over[nlibs]) as uint64: the insert sizes of the proper, well-mapped pairs the store holds, per library
        (bdx_insert_size_histogram; the rule is in include/bdx.h); before or after a run"""
        hist = np.empty((self.nlibs, L.ISIZE_BINS), dtype=np.uint64)
        over = np.empty(self.nlibs, dtype=np.uint64)
        self._chk(self.lib.bdx_insert_size_histogram(self.h, hist.ctypes.data_as(C.c_void_p), over.ctypes.data_as(C.c_void_p)), "bdx_insert_size_histogram")
        return hist, over

    def set_libs(self, libs, max_read_window_size):
        """the libraries and the initial window of the runs that follow (bdx_set_libs): same number, same BAM indices; the next run classifies
        the store again"""
        libs = list(libs)
        self._chk(self.lib.bdx_set_libs(self.h, lib_array(libs), len(libs), int(max_read_window_size)), "bdx_set_libs")
        self.libs = libs
        return self

    def use_clips(self, on=True):
        """the store gets a column of clip words (bdx_use_clips; the word is in include/bdx.h, bdx_clip_word): what site_clip_peaks reads;
        while the context holds no reads"""
        self._chk(self.lib.bdx_use_clips(self.h, 1 if on else 0), "bdx_use_clips")
        return self

    def put_clips(self, first, clip):
        """clip words of the records [first, first + len(clip)) the context already holds (bdx_put_clips); rows never put stay 0"""
        a = np.ascontiguousarray(clip, dtype=np.uint32)
        self._chk(self.lib.bdx_put_clips(self.h, int(first), a.ctypes.data_as(C.c_void_p), len(a)), "bdx_put_clips")
        return self

    def get_clips(self, n=None):
        """the clip column's first n rows as uint32 (bdx_get_clips).  The default n counts only what push_reads / stream_reads of THIS object
        put into the store since the last reset_reads: it is wrong (too small) for a store that a decoder or merge_decoded filled -- give
        that store's own record count"""
        n = int(self._n_held if n is None else n)
        out = np.zeros(n, np.uint32)
        self._chk(self.lib.bdx_get_clips(self.h, out.ctypes.data_as(C.c_void_p), n), "bdx_get_clips")
        return out

    def push_reads(self, arrs, clip=None):
        """clip: the batch's clip words (after use_clips), put behind the push"""
        b, keep = make_batch(arrs)
        if clip is not None and len(clip) != b.n:
            raise ValueError("ragged batch: clip has %d rows, expected %d" % (len(clip), b.n))
        self._keep.append(keep)  # the H2D copies are asynchronous: the arrays must outlive them (released by run())
        self._chk(self.lib.bdx_push(self.h, C.byref(b)), "bdx_push")
        first = self._n_held
        self._n_held = first + b.n
        if clip is not None:
            self.put_clips(first, clip)

    def stream_reads(self, arrs, batch=1 << 20, clip=None):
        """The streaming producer's path: fill the context's pinned staging buffers batch by batch (bdx_acquire_batch /
        bdx_submit_batch); copies and the classifier overlap the filling of the next buffer.  clip: the records' clip words (after
        use_clips), put behind each batch."""
        n = len(arrs["tid"])
        if clip is not None and len(clip) != n:
            raise ValueError("ragged batch: clip has %d rows, expected %d" % (len(clip), n))
        cols = {}
        for k, dt in BATCH_FIELDS:
            src = arrs.get(k)
            if src is None and k == "mapq":
                src = arrs.get("bdqual")
            if src is None and k == "name_key":
                src = arrs.get("name_id")
            cols[k] = np.ascontiguousarray(src, dtype=dt)
        fields = list(BATCH_FIELDS)
        if arrs.get("name_check") is not None:
            cols["name_check"] = np.ascontiguousarray(arrs["name_check"], dtype=np.uint64)
            fields.append(("name_check", np.uint64))
        for lo in range(0, n, batch):
            m = min(batch, n - lo)
            buf = L.bdx_batch_buf()
            self._chk(self.lib.bdx_acquire_batch(self.h, m, C.byref(buf)), "bdx_acquire_batch")
            for k, dt in fields:
                C.memmove(getattr(buf, k), cols[k][lo:lo + m].ctypes.data, m * np.dtype(dt).itemsize)
            self._chk(self.lib.bdx_submit_batch(self.h, m), "bdx_submit_batch")
            first = self._n_held
            self._n_held = first + m
            if clip is not None:
                self.put_clips(first, clip[lo:lo + m])

    def reset_reads(self):
        self._chk(self.lib.bdx_reset_reads(self.h), "bdx_reset_reads")
        self._keep.clear()
        self._n_held = 0
        return self

    def set_device_reads(self, ptrs, n):
        """ptrs: dict field -> device pointer (int); arrays stay owned by the caller."""
        b = L.bdx_batch()
        for k, _ in BATCH_FIELDS:
            setattr(b, k, C.c_void_p(int(ptrs[k])))
        if ptrs.get("name_check"):
            b.name_check = C.c_void_p(int(ptrs["name_check"]))
        b.n = n
        self._chk(self.lib.bdx_set_device_reads(self.h, C.byref(b)), "bdx_set_device_reads")

    def run(self):
        self._chk(self.lib.bdx_run(self.h), "bdx_run")
        self._keep.clear()  # bdx_run has waited for the stream: every pushed batch is in HBM
        return self

    # ---- results ----------------------------------------------------------------------------------------
    def summary(self):
        s = L.bdx_summary()
        self._chk(self.lib.bdx_get_summary(self.h, C.byref(s)), "bdx_get_summary")
        return {k: getattr(s, k) for k, _ in s._fields_}

    def counters(self):
        lib_cnt = np.zeros(self.nlibs, np.uint32)
        bam_cnt = np.zeros(self.nbams, np.uint32)
        hist = np.zeros((self.nlibs, 11), np.uint32)
        seqcov = np.zeros(self.nlibs, np.float32)
        dens = np.zeros(self.nlibs, np.float32)
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        self._chk(self.lib.bdx_get_counters(self.h, p(lib_cnt), p(bam_cnt), p(hist), p(seqcov), p(dens)), "bdx_get_counters")
        return dict(lib_read_count=lib_cnt, bam_read_count=bam_cnt, flag_hist=hist, seqcov=seqcov, density=dens)

    def regions(self):
        n = self.summary()["n_regions"]
        out = np.zeros(n, dtype=L.REGION_DTYPE)
        self._chk(self.lib.bdx_get_regions(self.h, out.ctypes.data_as(C.c_void_p), n), "bdx_get_regions")
        return out

    def svs(self):
        n = self.summary()["n_svs"]
        out = np.zeros(n, dtype=L.SV_DTYPE)
        assert L.SV_DTYPE.itemsize == 88
        self._chk(self.lib.bdx_get_svs(self.h, out.ctypes.data_as(C.c_void_p), n), "bdx_get_svs")
        nl = int((out["lib_begin"] + out["lib_count"]).max()) if n else 0
        nc = int((out["cn_begin"] + out["cn_count"]).max()) if n else 0
        li, lp = np.zeros(nl, np.int32), np.zeros(nl, np.int32)
        ck, cv = np.zeros(nc, np.int32), np.zeros(nc, np.float32)
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        self._chk(self.lib.bdx_get_sv_lists(self.h, p(li), p(lp), nl, p(ck), p(cv), nc), "bdx_get_sv_lists")
        return out, (li, lp), (ck, cv)

    def collect_support(self, on=True):
        self._chk(self.lib.bdx_set_collect_support(self.h, int(on)), "bdx_set_collect_support")

    def sv_support(self):
        """(offsets[n_svs+1], read_index, read_flag): supporting reads per SV in the reference's order"""
        n = self.summary()["n_svs"]
        off = np.zeros(n + 1, np.uint32)
        tot = C.c_size_t()
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        self._chk(self.lib.bdx_get_sv_support(self.h, p(off), None, None, 0, C.byref(tot)), "bdx_get_sv_support")
        idx, flg = np.zeros(tot.value, np.uint64), np.zeros(tot.value, np.uint8)
        self._chk(self.lib.bdx_get_sv_support(self.h, p(off), p(idx), p(flg), tot.value, C.byref(tot)), "bdx_get_sv_support")
        return off, idx, flg

    def read_class(self):
        n = self.summary()["n_reads"]
        out = np.zeros(n, np.uint8)
        self._chk(self.lib.bdx_get_read_class(self.h, out.ctypes.data_as(C.c_void_p), n), "bdx_get_read_class")
        return out

    def count_junction_pairs(self, tid, pos_a, pos_b, by_library=False):
        """Normal read pairs of the last run whose fragment covers a junction (bdx_count_junction_pairs): query i is chromosome
        tid[i] with the junctions pos_a[i] <= pos_b[i] (1-based; the boundary between base p and p + 1), a pair counts once if it covers
        at least one of them.  Returns an (n, nkeys) uint32 array: per library with by_library, else per BAM file."""
        t = np.ascontiguousarray(tid, dtype=np.int32)
        a = np.ascontiguousarray(pos_a, dtype=np.int32)
        b = np.ascontiguousarray(pos_b, dtype=np.int32)
        if not (len(t) == len(a) == len(b)):
            raise ValueError("tid, pos_a and pos_b differ in length")
        nkeys = self.nlibs if by_library else self.nbams
        out = np.zeros((len(t), nkeys), np.uint32)
        p = lambda x: x.ctypes.data_as(C.c_void_p)
        self._chk(self.lib.bdx_count_junction_pairs(self.h, p(t), p(a), p(b), len(t), int(bool(by_library)), p(out)),
                  "bdx_count_junction_pairs")
        return out

    def count_site_pairs(self, sites, window, by_library=False):
        """Alternate-supporting read pairs of the last run at given SV sites (bdx_count_site_pairs; the rule is in include/bdx.h):
        `sites` is an array of _lib.SITE_DTYPE, or a sequence of (tid1, pos1, tid2, pos2, flag_mask) with 1-based positions,
        (tid1, pos1) <= (tid2, pos2) and bit f of flag_mask set when ReadFlag f supports the site.  A passing record whose flag is in the
        mask counts, once per pair by its lower mate, when it starts within `window` of one end and its mate within `window` of the
        other.  Returns an (n, nkeys) uint32 array: per library with by_library, else per BAM file."""
        if isinstance(sites, np.ndarray) and sites.dtype == L.SITE_DTYPE:
            s = np.ascontiguousarray(sites)
        else:
            rows = [tuple(int(v) for v in r) for r in sites]
            s = np.array(rows, dtype=L.SITE_DTYPE) if rows else np.zeros(0, dtype=L.SITE_DTYPE)
        nkeys = self.nlibs if by_library else self.nbams
        out = np.zeros((len(s), nkeys), np.uint32)
        p = lambda x: x.ctypes.data_as(C.c_void_p)
        self._chk(self.lib.bdx_count_site_pairs(self.h, p(s), len(s), int(window), int(bool(by_library)), p(out)), "bdx_count_site_pairs")
        return out

    def site_breakpoint_bounds(self, sites, window):
        """Breakpoint intervals of given SV sites from the supporting pairs of the last run (bdx_site_breakpoint_bounds; the rule is in
        include/bdx.h): `sites` and `window` as for count_site_pairs, whose records -- all keys pooled -- are the ones that count.  Each
        bounds the breakpoint at either end by where its read there starts, its strand and its library's uppercutoff.  Returns an array
        of _lib.SITE_BOUNDS_DTYPE: n, and per end the largest lower bound lo and the smallest upper bound hi (1-based; lo > hi when the
        pairs contradict each other; all 0 with n == 0)."""
        if isinstance(sites, np.ndarray) and sites.dtype == L.SITE_DTYPE:
            s = np.ascontiguousarray(sites)
        else:
            rows = [tuple(int(v) for v in r) for r in sites]
            s = np.array(rows, dtype=L.SITE_DTYPE) if rows else np.zeros(0, dtype=L.SITE_DTYPE)
        out = np.zeros(len(s), dtype=L.SITE_BOUNDS_DTYPE)
        p = lambda x: x.ctypes.data_as(C.c_void_p)
        self._chk(self.lib.bdx_site_breakpoint_bounds(self.h, p(s), len(s), int(window), p(out)), "bdx_site_breakpoint_bounds")
        return out

    def site_end_quality(self, sites, ends, window):
        """Mapping quality at one end of given SV sites (bdx_site_end_quality; the rule is in include/bdx.h): `sites` and `window` as for
        count_site_pairs, `ends` one 1 or 2 per site -- the end that is asked.  A passing record whose flag is in the mask supports the end
        when it starts within `window` of it and its mate within `window` of the other end (no lower-mate condition: each mate counts at
        its own end); a mapped record that starts within `window` of the end is around it, and low when its quality does not exceed its
        library's minimum.  Returns an array of _lib.SITE_QUALITY_DTYPE: n, n_all, n_low, and over the supporters' qualities qmin, q1
        (lower quartile), median (lower median) and qmax (all 0 with n == 0)."""
        if isinstance(sites, np.ndarray) and sites.dtype == L.SITE_DTYPE:
            s = np.ascontiguousarray(sites)
        else:
            rows = [tuple(int(v) for v in r) for r in sites]
            s = np.array(rows, dtype=L.SITE_DTYPE) if rows else np.zeros(0, dtype=L.SITE_DTYPE)
        e = np.ascontiguousarray(np.asarray(ends).reshape(-1), dtype=np.uint8)
        if len(e) != len(s):
            raise ValueError("sites and ends differ in length")
        out = np.zeros(len(s), dtype=L.SITE_QUALITY_DTYPE)
        p = lambda x: x.ctypes.data_as(C.c_void_p)
        self._chk(self.lib.bdx_site_end_quality(self.h, p(s), p(e), len(s), int(window), p(out)), "bdx_site_end_quality")
        return out

    def site_clip_peaks(self, sites, ends, window, min_clip=10):
        """Where the clipped reads pile up around one end of given SV sites (bdx_site_clip_peaks; the rule is in include/bdx.h), after
        use_clips: `sites` and `ends` as for site_end_quality (the flag mask is not used), window 0 .. _lib.CLIP_WINDOW_MAX, min_clip
        1 .. 255.  A passing record clipped by min_clip or more on its left gives an observation at its first aligned base, one clipped on
        its right at its last.  Returns an array of _lib.CLIP_PEAKS_DTYPE: per side the observations within `window` of the end, the
        position most of them share and how many do (ties: nearer to the end, then smaller; all 0 with n == 0)."""
        if isinstance(sites, np.ndarray) and sites.dtype == L.SITE_DTYPE:
            s = np.ascontiguousarray(sites)
        else:
            rows = [tuple(int(v) for v in r) for r in sites]
            s = np.array(rows, dtype=L.SITE_DTYPE) if rows else np.zeros(0, dtype=L.SITE_DTYPE)
        e = np.ascontiguousarray(np.asarray(ends).reshape(-1), dtype=np.uint8)
        if len(e) != len(s):
            raise ValueError("sites and ends differ in length")
        out = np.zeros(len(s), dtype=L.CLIP_PEAKS_DTYPE)
        p = lambda x: x.ctypes.data_as(C.c_void_p)
        self._chk(self.lib.bdx_site_clip_peaks(self.h, p(s), p(e), len(s), int(window), int(min_clip), p(out)), "bdx_site_clip_peaks")
        return out

    def count_interval_reads(self, intervals, by_library=False):
        """Passing read starts of the last run inside given intervals (bdx_count_interval_reads; the rule is in include/bdx.h):
        `intervals` is an array of _lib.INTERVAL_DTYPE, or a sequence of (tid, beg, end), 0-based and half-open.  A record counts when it
        lies on tid, beg <= pos < end and K1 let it pass the filter chain -- a density of read starts, not a per-base pileup.  Returns an
        (n, nkeys) uint32 array: per library with by_library, else per BAM file."""
        if isinstance(intervals, np.ndarray) and intervals.dtype == L.INTERVAL_DTYPE:
            iv = np.ascontiguousarray(intervals)
        else:
            rows = [tuple(int(v) for v in r) for r in intervals]
            iv = np.array(rows, dtype=L.INTERVAL_DTYPE) if rows else np.zeros(0, dtype=L.INTERVAL_DTYPE)
        nkeys = self.nlibs if by_library else self.nbams
        out = np.zeros((len(iv), nkeys), np.uint32)
        p = lambda x: x.ctypes.data_as(C.c_void_p)
        self._chk(self.lib.bdx_count_interval_reads(self.h, p(iv), len(iv), int(bool(by_library)), p(out)), "bdx_count_interval_reads")
        return out

    def set_insert_null(self, hist):
        """the null distribution of window_insert_shift (bdx_set_insert_null): hist[nlibs][ISIZE_BINS] as insert_size_histogram gives it
        (ranks summed by the caller), kept on the device as cumulative counts until the next call; None frees it"""
        if hist is None:
            self._chk(self.lib.bdx_set_insert_null(self.h, None), "bdx_set_insert_null")
            return self
        h = np.ascontiguousarray(hist, dtype=np.uint64)
        if h.shape != (self.nlibs, L.ISIZE_BINS):
            raise ValueError("hist is not [nlibs][ISIZE_BINS]")
        self._chk(self.lib.bdx_set_insert_null(self.h, h.ctypes.data_as(C.c_void_p)), "bdx_set_insert_null")
        return self

    def window_insert_shift(self, intervals):
        """Insert-size shift of the pairs of the last run that start inside given windows (bdx_window_insert_shift; the rule is in
        include/bdx.h): `intervals` as for count_interval_reads.  A passing record of a same-chromosome class whose only anomaly can be its
        insert size, the lower mate of its pair, is an observation |isize| of its library.  Returns an (n, nlibs) array of
        _lib.INSERT_SHIFT_DTYPE: n, n_over, saturated, sum, and t_plus / t_minus = n N times the one-sided Kolmogorov-Smirnov distances
        against the null set with set_insert_null; a window of more than _lib.MINI_CAP observations is saturated and has no t."""
        if isinstance(intervals, np.ndarray) and intervals.dtype == L.INTERVAL_DTYPE:
            iv = np.ascontiguousarray(intervals)
        else:
            rows = [tuple(int(v) for v in r) for r in intervals]
            iv = np.array(rows, dtype=L.INTERVAL_DTYPE) if rows else np.zeros(0, dtype=L.INTERVAL_DTYPE)
        out = np.zeros((len(iv), self.nlibs), dtype=L.INSERT_SHIFT_DTYPE)
        p = lambda x: x.ctypes.data_as(C.c_void_p)
        self._chk(self.lib.bdx_window_insert_shift(self.h, p(iv), len(iv), p(out)), "bdx_window_insert_shift")
        return out

    def window_anchor_split(self, intervals, min_qual=-1):
        """The one-end-anchored reads of the last run that start inside given windows, and the position that best splits them
        (bdx_window_anchor_split; the rule is in include/bdx.h): `intervals` as for count_interval_reads.  A record of class
        MATE_UNMAPPED whose quality passes -- above its library's minimum with min_qual = -1, at least min_qual otherwise -- is an anchor
        and points right on the forward strand (left under -l).  Returns an (n,) array of _lib.ANCHOR_SPLIT_DTYPE."""
        if isinstance(intervals, np.ndarray) and intervals.dtype == L.INTERVAL_DTYPE:
            iv = np.ascontiguousarray(intervals)
        else:
            rows = [tuple(int(v) for v in r) for r in intervals]
            iv = np.array(rows, dtype=L.INTERVAL_DTYPE) if rows else np.zeros(0, dtype=L.INTERVAL_DTYPE)
        out = np.zeros(len(iv), dtype=L.ANCHOR_SPLIT_DTYPE)
        p = lambda x: x.ctypes.data_as(C.c_void_p)
        self._chk(self.lib.bdx_window_anchor_split(self.h, p(iv), len(iv), int(min_qual), p(out)), "bdx_window_anchor_split")
        return out

    def set_stage_timing(self, on=True):
        """HIP events between the stages (compact / regions / join timings); costs a few microseconds per event."""
        self._chk(self.lib.bdx_set_stage_timing(self.h, int(on)), "bdx_set_stage_timing")
        return self

    def set_enqueue_ahead(self, mode=2):
        """How the stages behind pass 1 are sized and launched (bdx_set_enqueue_ahead): 2 ahead of the pass-1 read-back, from
        the previous run of the same input or else a prior on the read count (default); 1 always from the prior (every run
        behaves like a first run); 0 only after the read-back.  True / False stand for 2 / 0."""
        mode = 2 if mode is True else (0 if mode is False else int(mode))
        self._chk(self.lib.bdx_set_enqueue_ahead(self.h, mode), "bdx_set_enqueue_ahead")
        return self

    def set_debug(self, name, value=1):
        """test / measurement switches by name (include/bdx.h bdx_set_debug); before run()"""
        self._chk(self.lib.bdx_set_debug(self.h, name.encode(), int(value)), "bdx_set_debug")
        return self

    def set_host_walk(self, on=True):
        """Send every component of the region graph through the host walk (same results as the device assembly)."""
        self._chk(self.lib.bdx_set_host_walk(self.h, int(on)), "bdx_set_host_walk")
        return self

    def walk_split(self):
        """(SVs assembled on the device, SVs from the host walk, pair groups handed to the host walk)"""
        v = [C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)]
        self._chk(self.lib.bdx_get_walk_split(self.h, C.byref(v[0]), C.byref(v[1]), C.byref(v[2])), "bdx_get_walk_split")
        return tuple(x.value for x in v)

    def was_replayed(self):
        """True if the last run met a read name more than twice and replayed the region graph read by read on the host"""
        return bool(self.lib.bdx_was_replayed(self.h))

    def cross_window_svs(self):
        """device-assembled SVs whose traversal started from a region of an earlier flush window"""
        v = C.c_uint32(0)
        self._chk(self.lib.bdx_get_cross_window_svs(self.h, C.byref(v)), "bdx_get_cross_window_svs")
        return v.value

    def timings(self):
        ms = np.zeros(12, np.float32)
        self.lib.bdx_get_timings(self.h, ms.ctypes.data_as(C.c_void_p), 12)
        return dict(zip(("classify", "compact", "regions", "join", "readback", "walk", "score", "total", "final_wait", "merge",
                         "combine_scores"), ms.tolist()))


def estimate_insert_size(hist):
    """bdx_estimate_insert_size: bam2cfg's figures of one library from its histogram hist[ISIZE_BINS] (host only, no GPU), as a dict"""
    lib = L.load()
    h = np.ascontiguousarray(hist, dtype=np.uint64)
    if h.shape != (L.ISIZE_BINS,):
        raise ValueError("a histogram of %d bins is expected" % L.ISIZE_BINS)
    out = L.bdx_insert_estimate()
    rc = lib.bdx_estimate_insert_size(h.ctypes.data_as(C.c_void_p), C.byref(out))
    if rc != 0:
        raise BdxError("bdx_estimate_insert_size: %s" % lib.bdx_strerror(rc).decode())
    return {k: getattr(out, k) for k, _ in L.bdx_insert_estimate._fields_}


def clip_word(cigar, l_seq, flag=0):
    """bdx_clip_word: the clip word of a CIGAR given as a sequence of (length, operation) with the operation a letter of MIDNSHP=X or its
    BAM code (host only, no GPU)"""
    lib = L.load()
    code = lambda op: "MIDNSHP=X".index(op) if isinstance(op, str) else int(op)
    w = np.array([(int(n) << 4) | code(op) for n, op in cigar], dtype=np.uint32)
    return int(lib.bdx_clip_word(w.ctypes.data_as(C.c_void_p) if len(w) else None, len(w), int(l_seq), int(flag)))


def insert_shift_score(row, N):
    """bdx_insert_shift_score: (score, D) of one row of window_insert_shift against a null of N observations (host only, no GPU)"""
    lib = L.load()
    r = np.zeros(1, dtype=L.INSERT_SHIFT_DTYPE)
    r[0] = row
    score, d = C.c_double(), C.c_double()
    rc = lib.bdx_insert_shift_score(r.ctypes.data_as(C.c_void_p), int(N), C.byref(score), C.byref(d))
    if rc != 0:
        raise BdxError("bdx_insert_shift_score: %s" % lib.bdx_strerror(rc).decode())
    return score.value, d.value


def mark_duplicates(tid, pos, mtid, mpos, flag, lib, name_key, device=0):
    """bdx_mark_duplicates on host arrays: (bool mask of the records the rule marks, groups of two or more)"""
    lb = L.load()
    cols = [np.ascontiguousarray(a, dtype=dt) for a, dt in ((tid, np.int32), (pos, np.int32), (mtid, np.int32), (mpos, np.int32),
                                                            (flag, np.uint16), (lib, np.uint8), (name_key, np.uint64))]
    n = len(cols[0])
    if any(len(c) != n for c in cols):
        raise ValueError("the columns differ in length")
    out = np.zeros(n, np.uint8)
    groups = C.c_uint64(0)
    rc = lb.bdx_mark_duplicates(device, *[c.ctypes.data_as(C.c_void_p) for c in cols], n, out.ctypes.data_as(C.c_void_p), C.byref(groups))
    if rc != 0:
        raise BdxError("bdx_mark_duplicates: %s" % lb.bdx_strerror(rc).decode())
    return out.astype(bool), groups.value


def classify(opts, libs, arrs, device=0):
    """bdx_classify on host arrays: the class byte of every record of the batch `arrs` (as for push_reads) under `opts` and `libs`, from a
    context of its own; the number of source files is the larger of what the libraries and the batch's file indices say"""
    lb = L.load()
    co = opts.to_c()
    libs = list(libs)
    arr = lib_array(libs)
    b, keep = make_batch(arrs)
    out = np.zeros(b.n, np.uint8)
    rc = lb.bdx_classify(C.byref(co), arr, len(libs), C.byref(b), out.ctypes.data_as(C.c_void_p), device)
    del keep
    if rc != 0:
        raise BdxError("bdx_classify: %s" % lb.bdx_strerror(rc).decode())
    return out


def poisson_log_upper_tail(lam, k, device=0):
    lib = L.load()
    lam = np.ascontiguousarray(lam, np.float64)
    k = np.ascontiguousarray(k, np.int32)
    out = np.zeros(len(lam), np.float64)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    rc = lib.bdx_poisson_log_upper_tail(p(lam), p(k), p(out), len(lam), device)
    if rc != 0:
        raise BdxError("bdx_poisson_log_upper_tail: %s" % lib.bdx_strerror(rc).decode())
    return out
