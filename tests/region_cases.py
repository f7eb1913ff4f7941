"""Cases, references and models for the region cut (K3, csrc/k3_regions.hip) and the mate join (K4, csrc/k4_join.hip) on their own
(tests/test_gpu_regions.py through tests/prims/stages.hip; held to ground truth by tests/test_region_cases.py).  No GPU is needed here.

References -- plain statements of the operation, sharing nothing with the kernels' way of computing it:
  cut_reference    one read at a time, as BreakDancer.cpp:202-264 and the oracle's push_read / process_breakpoint do it
  cut_vectorised   the same table in O(n) numpy, sharing no code with the loop (the large cases are held to it)
  join_reference   a dictionary from (key, check) to the entries that carry it
  join_all_pairs   the same statement as an O(n^2) comparison of every entry with every other
Models -- restatements of HOW the kernels do it, so that a case's purpose can be asserted (which lane starts a run, which bucket takes
which table, which probe wraps) and so that a slip applied to a copy must fail a case:
  headout_model    HeadOut's segmented running maximum over the lanes of a wave
  direct_model     the direct join's table, entries arriving in index order
  bucket_routes    the bucketed join's LDS / HBM choice per bucket
  forward_model    forward_quads' turns, partial last turn and tail words

What no result can show: whether partner[] of a name seen three times or more holds one mate or another (any is right: irregular = 1 sends
the run to the host replay), and the order in which the entries of a concurrent join arrive -- the models take index order, the
references take none."""
import functools
from fractions import Fraction

import numpy as np

FILL = 0xA5A5A5A5
F_FF, F_CTX = 1, 8
W0 = 50                      # the window of every case that is also a read stream (one library, mean 300, reads of 50: min(200, 50))
SCAN_BLOCK = 256             # lanes of a scan workgroup (csrc/bdx_scan.h)
TWO_PER_LANE = 1 << 19       # launch_k3: above this many reads (the host's count) a lane takes two
JOIN_LDS_SLOTS = 8192        # a bucket of up to half as many entries is joined in LDS
MAX_BUCKETS = 8192
MAX_PROBES = 4096
REC_WORDS = 9                # tid, start, end, n, rev, nonctx, nnormal, maxq, first
FWD_BLOCKS, FWD_AHEAD = 32, 4
FWD_TURN_QUADS = FWD_BLOCKS * 256 * FWD_AHEAD
M64 = (1 << 64) - 1
STREAM_MAX = 1 << 16

# ---------------------------------------------------------------------------------------------------------------------------------
# the cut
# ---------------------------------------------------------------------------------------------------------------------------------


def cut_case(name, tid, pos, qlen, rev=None, flag=None, nn=None, pk=None, nkeys=1, W=W0, n_normal=None, min_len=7, lim=1000, tail=None,
             n_host=None, stream=None):
    n = len(tid)
    tid = np.asarray(tid, np.int32)
    pos = np.asarray(pos, np.int32)
    qlen = np.asarray(qlen, np.int64)
    assert len(pos) == n and len(qlen) == n and n >= 1 and qlen.min() >= 0 and qlen.max() <= 65535
    j = np.arange(n, dtype=np.int64)
    rev = ((j * 7 // 3) & 1).astype(np.uint32) if rev is None else np.asarray(rev, np.uint32)
    flag = np.where(j % 5 == 2, F_CTX, F_FF).astype(np.uint32) if flag is None else np.asarray(flag, np.uint32)
    if nn is None:
        nn = (j // 3).astype(np.uint32)
    nn = np.asarray(nn, np.uint32)
    if n_normal is None:
        n_normal = (int(nn[-1]) + 2) & 0xFFFFFFFF
    if pk is None:
        pk = np.stack([((nn.astype(np.int64) * (k + 1) + 5 * k + j // (k + 2)) & 0xFFFFFFFF).astype(np.uint32) for k in range(nkeys)])
    pk = np.ascontiguousarray(pk, np.uint32)
    assert pk.shape == (nkeys, n)
    meta = (flag | (rev << np.uint32(4)) | (qlen.astype(np.uint32) << np.uint32(16))).astype(np.uint32)
    if tail is not None:
        tail = np.ascontiguousarray(tail, np.uint32)
        assert tail.ndim == 2 and tail.shape[1] == 4 and tid.min() >= 0 and tid.max() < len(tail)
    if stream is None:
        stream = tail is None and W == W0 and n < STREAM_MAX and nkeys == 1
    if stream:   # a read stream can say it: sorted, counts that only grow from the stream's start
        d = np.diff(nn.astype(np.int64))
        assert W == W0 and tail is None and (d >= 0).all() and n_normal >= int(nn[-1])
        assert ((np.diff(tid) > 0) | ((np.diff(tid) == 0) & (np.diff(pos) >= 0))).all(), name
    c = dict(name=name, n=n, tid=tid, pos=pos, qlen=qlen, rev=rev, flag=flag, meta=meta, nn=nn, pk=pk, nkeys=nkeys, W=int(W), n_normal=int(n_normal),
             min_len=int(min_len), lim=int(lim), tail=tail, n_host=int(n if n_host is None else n_host), stream=bool(stream))
    assert c["n_host"] >= n
    for a in (tid, pos, qlen, rev, flag, meta, nn, pk):
        a.setflags(write=False)
    return c


def accept_f32(qsum, den, lim):
    """the verdict as the reference and the kernel compute it: float32 operands, one correctly rounded float32 division"""
    return bool(np.float32(qsum) / np.float32(den) < np.float32(lim))


def cut_reference(c, slip=None):
    """One read at a time.  The state is BreakDancer's: region start / end, `collecting`, the nucleotide sum and the largest read length of
    the reads that came while collecting.  A candidate is closed by the read that breaks it (counted before the break test), by the tail
    table's read where the list holds several chromosomes of a sharded run, or by the end of the stream."""
    tid, pos, q, nn, tail = c["tid"].tolist(), c["pos"].tolist(), c["qlen"].tolist(), c["nn"].tolist(), c["tail"]
    rev, flag = c["rev"].tolist(), c["flag"].tolist()
    n, W, min_len, lim = c["n"], c["W"], c["min_len"], c["lim"]
    cand, c_first, c_maxq, c_rid, recs, pks = [], [], [], [], [], []
    state = dict(collecting=False, qsum=0, maxq=0)
    last_maxq = 0

    def close(f, l, closer_nn, tail_row):
        """candidate of reads f .. l; closer_nn: the normal-pair count it ends with"""
        nonlocal last_maxq
        qsum, maxq = state["qsum"], state["maxq"]
        c_maxq.append(maxq)
        if tail_row is not None and tail_row[0]:
            qsum += int(tail_row[1])
            if slip != "maxq_without_tail":
                maxq = max(maxq, int(tail_row[1]))
        span = pos[l] - pos[f]
        den = span + 1 + maxq
        if slip == "div_double":
            below = float(qsum) / float(den) < float(lim)
        elif slip == "div_exact":
            below = Fraction(qsum, den) < lim
        elif slip == "cov_le":
            below = bool(np.float32(qsum) / np.float32(den) <= np.float32(lim))
        else:
            below = accept_f32(qsum, den, lim)
        long_enough = span >= min_len if slip == "min_len_ge" else span > min_len
        last_maxq = maxq
        if long_enough and below:
            c_rid.append(len(recs))
            recs.append([tid[f], pos[f], pos[l], l - f + 1, sum(rev[f:l + 1]), sum(1 for x in flag[f:l + 1] if x != F_CTX), (closer_nn - nn[f]) & 0xFFFFFFFF, maxq, f])
            pks.append([int(c["pk"][k, f]) for k in range(c["nkeys"])] + [int(c["pk"][k, l]) for k in range(c["nkeys"])])
        else:
            c_rid.append(-1)

    first = 0
    for j in range(n):
        if j == 0:
            brk = True
        else:
            gap = pos[j] - pos[j - 1]
            far = gap >= W if slip == "gap_ge" else gap > W
            brk = far if slip == "tid_ignored" else (tid[j] != tid[j - 1] or far)
        other = j > 0 and tid[j] != tid[j - 1]
        # (BreakDancer.cpp:209-212 runs before the break test at :216: the breaking read counts for the candidate it closes -- unless
        # the list holds several chromosomes of a sharded run: then another chromosome's read is not the one that closed it in the genome)
        counts_here = state["collecting"] and not (brk and slip == "breaking_not_counted")
        if tail is not None and brk and other and slip != "tail_other_chrom_counted":
            counts_here = False
        if counts_here:
            state["qsum"] += q[j]
            state["maxq"] = max(state["maxq"], q[j])
        if brk:
            if j > 0:
                row = tail[tid[first]] if tail is not None and other else None
                close(first, j - 1, int(row[2]) if row is not None else nn[j], row)
            first = j
            state.update(collecting=False, qsum=0, maxq=0)
            c_first.append(j)
            if slip == "first_counted":
                state.update(qsum=q[j], maxq=q[j])
        cand.append(len(c_first) - 1)
        state["collecting"] = True
    row = tail[tid[first]] if tail is not None else None
    close(first, n - 1, int(row[2]) if row is not None else c["n_normal"], row)
    return _cut_result(c, cand, c_first, c_maxq, c_rid, recs, pks, last_maxq)


def _cut_result(c, cand, c_first, c_maxq, c_rid, recs, pks, last_maxq):
    c_rid = np.asarray(c_rid, np.int32)
    cand = np.asarray(cand, np.int32)
    return dict(cand=cand, c_first=np.asarray(c_first, np.uint32), c_maxq=np.asarray(c_maxq, np.int32), c_rid=c_rid, region_of=c_rid[cand],
                rec=np.asarray(recs, np.int64).reshape(-1, REC_WORDS).astype(np.uint32), pk=np.asarray(pks, np.int64).reshape(-1, 2 * c["nkeys"]).astype(np.uint32),
                n_cand=len(c_first), n_regions=len(recs), last_maxq=int(last_maxq))


def cut_vectorised(c):
    """The same table from whole-array operations: heads, a running count of them, sums as differences of running sums, the maxima by
    scattering every read's length at the candidate it counts for."""
    tid, pos, q, nn, tail = c["tid"].astype(np.int64), c["pos"].astype(np.int64), c["qlen"], c["nn"].astype(np.int64), c["tail"]
    n, W = c["n"], c["W"]
    other = np.zeros(n, bool)
    other[1:] = tid[1:] != tid[:-1]
    head = other.copy()
    head[0] = True
    head[1:] |= (pos[1:] - pos[:-1]) > W
    cand = np.cumsum(head) - 1
    first = np.flatnonzero(head)
    nc = len(first)
    nxt = np.append(first[1:], n)
    last = nxt - 1
    csum = np.concatenate([[0], np.cumsum(q)])                      # csum[j] = lengths of reads before j
    closed_by_next = np.arange(nc) + 1 < nc
    if tail is not None:
        chrom_last = ~closed_by_next | other[np.minimum(nxt, n - 1)]
        closed_by_next &= ~chrom_last
    upto = np.where(closed_by_next, nxt, last)                      # the last read that counts
    qsum = csum[upto + 1] - csum[first + 1]
    target = np.where(head, cand - 1, cand)
    counted = target >= 0
    if tail is not None:
        counted &= ~(head & other)
    c_maxq = np.zeros(nc, np.int64)
    np.maximum.at(c_maxq, target[counted], q[counted])
    maxq = c_maxq.copy()
    nn_end = np.where(np.arange(nc) + 1 < nc, nn[np.minimum(nxt, n - 1)], c["n_normal"])
    if tail is not None:
        rows = tail[tid[first]].astype(np.int64)
        closes = chrom_last & (rows[:, 0] != 0)
        qsum = qsum + np.where(closes, rows[:, 1], 0)
        maxq = np.where(closes, np.maximum(maxq, rows[:, 1]), maxq)
        nn_end = np.where(chrom_last, rows[:, 2], nn_end)
    span = pos[last] - pos[first]
    cov = qsum.astype(np.float32) / (span + 1 + maxq).astype(np.float32)
    ok = (span > c["min_len"]) & (cov < np.float32(c["lim"]))
    c_rid = np.where(ok, np.cumsum(ok) - 1, -1)
    f, l = first[ok], last[ok]
    crev = np.concatenate([[0], np.cumsum(c["rev"].astype(np.int64))])
    cnon = np.concatenate([[0], np.cumsum(c["flag"] != F_CTX)])
    rec = np.stack([tid[f], pos[f], pos[l], l - f + 1, crev[l + 1] - crev[f], cnon[l + 1] - cnon[f], (nn_end[ok] - nn[f]) & 0xFFFFFFFF, maxq[ok], f], axis=1)
    pk = np.concatenate([c["pk"][:, f].T, c["pk"][:, l].T], axis=1)
    return dict(cand=cand.astype(np.int32), c_first=first.astype(np.uint32), c_maxq=c_maxq.astype(np.int32), c_rid=c_rid.astype(np.int32),
                region_of=c_rid[cand].astype(np.int32), rec=(rec & 0xFFFFFFFF).astype(np.uint32).reshape(-1, REC_WORDS), pk=pk.astype(np.uint32).reshape(-1, 2 * c["nkeys"]),
                n_cand=nc, n_regions=int(ok.sum()), last_maxq=int(maxq[-1]))


CUT_FIELDS = ("cand", "c_first", "c_maxq", "c_rid", "region_of", "rec", "pk")


def cut_differs(a, b):
    """the first field two cut results differ in, or None"""
    for k in ("n_cand", "n_regions", "last_maxq"):
        if a[k] != b[k]:
            return k
    for k in CUT_FIELDS:
        if a[k].shape != b[k].shape or (a[k] != b[k]).any():
            return k
    return None


def head_targets(c):
    """per read: is it a head, the candidate it counts for (-1: none) and whether its length is left out (another chromosome's read under a
    tail table) -- HeadOut's inputs, from the case alone"""
    tid, pos = c["tid"].astype(np.int64), c["pos"].astype(np.int64)
    other = np.zeros(c["n"], bool)
    other[1:] = tid[1:] != tid[:-1]
    head = other.copy()
    head[0] = True
    head[1:] |= (pos[1:] - pos[:-1]) > c["W"]
    cand = np.cumsum(head) - 1
    target = np.where(head, cand - 1, cand)
    left_out = head & other if c["tail"] is not None else np.zeros(c["n"], bool)
    return head, target, left_out


def headout_model(c, slip=None):
    """c_maxq as HeadOut computes it: the lanes of a wave hold 64 consecutive reads (both instantiations: a lane's second read lies 256
    further on, a multiple of 64); a segmented running maximum over the lanes below, and the last lane of a target's run in the wave
    reports it with one atomicMax.  Returns (c_maxq, lanes at which runs start, lanes at which they end)."""
    n = c["n"]
    head, target, left_out = head_targets(c)
    nw = (n + 63) // 64
    INT_MIN = -(1 << 31)
    t = np.full(nw * 64, -2, np.int64)
    t[:n] = target
    here = np.zeros(nw * 64, bool)
    here[:n] = True
    v = np.full(nw * 64, INT_MIN, np.int64)
    v[:n] = np.where((target >= 0) & ~left_out, c["qlen"], INT_MIN)
    t, v, here = t.reshape(nw, 64), v.reshape(nw, 64), here.reshape(nw, 64)
    lane = np.arange(64)
    o = 1
    while o < 64:
        pv = np.roll(v, o, axis=1)
        pt = np.roll(t, o, axis=1)
        take = (lane >= o)[None, :] if slip == "segmax_no_reset" else (lane >= o)[None, :] & (pt == t)
        v = np.where(take, np.maximum(v, pv), v)
        o <<= 1
    nt = np.roll(t, -1, axis=1)
    nt[:, 63] = t[:, 63]                       # (a shuffle from beyond the wave hands back the lane's own)
    jn = np.arange(nw * 64).reshape(nw, 64)
    last_of_run = (jn == n - 1) | (nt != t)
    if slip != "lane63_no_report":
        last_of_run |= (lane == 63)[None, :]
    prev_t = np.roll(t, 1, axis=1)
    first_of_run = (lane == 0)[None, :] | (prev_t != t)
    rep = here & last_of_run & (t >= 0) & (v != INT_MIN)
    out = np.zeros(int(target.max()) + 2, np.int64)
    np.maximum.at(out, t[rep], v[rep])
    live = here & (t >= 0)
    return out[:int(head.sum())].astype(np.int32), set(np.nonzero(live & first_of_run)[1].tolist()), set(np.nonzero(live & last_of_run)[1].tolist())


def instantiation(c):
    """reads per workgroup of the head scan launch_k3 picks for the case"""
    return 2 * SCAN_BLOCK if c["n_host"] > TWO_PER_LANE else SCAN_BLOCK


# ---- builders -------------------------------------------------------------------------------------------------------------------

def runs(lengths, lead=0, step=3, W=W0, tid0=0, pos0=100):
    """(tid, pos) of `lead` single-read candidates and then candidates of the given lengths on one chromosome: reads `step` apart, candidates
    W + 1 apart"""
    L = np.concatenate([np.ones(lead, np.int64), np.asarray(lengths, np.int64)])
    n = int(L.sum())
    first = np.concatenate([[0], np.cumsum(L)[:-1]])
    head = np.zeros(n, bool)
    head[first] = True
    d = np.where(head, W + 1, step)
    d[0] = pos0
    return np.full(n, tid0, np.int32), np.cumsum(d)


def qlens(n, seed, lo=30, hi=150):
    return np.random.default_rng(seed).integers(lo, hi + 1, n)


MIX = (1, 2, 5, 3, 8, 1, 1, 70, 4, 2, 130, 6)
RUN_LAYOUTS = ("lane0", "end63", "straddle", "straddle512")


def run_lead(L, how):
    """single-read candidates in front of a candidate of L reads so that it starts on lane 0, ends on lane 63, or lies (or, a single read:
    is broken) across the boundary of the second wave and first 256-read workgroup, or of the first 512-read workgroup"""
    return {"lane0": 64, "end63": 64 + (63 - (L - 1)) % 64, "straddle": 256 - min(max(1, L // 2), 200), "straddle512": 512 - min(max(1, L // 2), 200)}[how]


def mixed_lengths(n):
    reps = n // sum(MIX) + 1
    L = np.tile(np.asarray(MIX, np.int64), reps)
    cs = np.cumsum(L)
    k = int(np.searchsorted(cs, n))
    L = L[:k + 1].copy()
    L[k] -= cs[k] - n
    return L[L > 0]


def cov_reads(qsum, den, lim_w=W0, span=10):
    """(positions from 0, read lengths) of a candidate whose nucleotide sum is qsum and whose denominator is den, and the length its breaking
    read has to have: the first read (not counted) has length 1; the counted ones are as long as the denominator lets them be"""
    maxq = min(den - 1 - span, 65535)
    assert maxq >= 1 and qsum >= maxq
    span = den - 1 - maxq
    k, r = divmod(qsum, maxq)
    ql = [maxq] * k + ([r] if r else [])
    brk = ql.pop()                      # the breaking read carries the last share (the remainder, or a whole maxq)
    m = len(ql)
    assert m >= 1 and span <= m * lim_w, (qsum, den, m, span)
    p = [0] + [int(round(span * (i + 1) / m)) for i in range(m)]
    return np.asarray(p, np.int64), np.asarray([1] + ql, np.int64), brk


def chain(cands, final_q=40, **kw):
    """candidates from cov_reads, one chromosome each: the first read of the next one breaks, and carries the length asked for"""
    tid, pos, q = [], [], []
    want = 1
    for t, (p, ql, brk) in enumerate(cands):
        ql = ql.copy()
        ql[0] = want
        tid.append(np.full(len(p), t, np.int32)); pos.append(p + 1000); q.append(ql)
        want = brk
    tid.append(np.asarray([len(cands)], np.int32)); pos.append(np.asarray([1000])); q.append(np.asarray([want]))
    return dict(tid=np.concatenate(tid), pos=np.concatenate(pos), qlen=np.concatenate(q), **kw)


@functools.lru_cache(maxsize=None)
def verdict_pairs(lim):
    """(qsum, den) whose float32 verdict differs from the exact one, by a seeded search: two where float32 says "not below" and exact
    arithmetic "below", two the other way round where there are any.  With lim 1 and 1000 there are none: lim x den is a float32 there
    (den itself, or a multiple of 8 below 2^26), rounding is monotone, so qsum >= lim x den stays float(qsum) >= lim x den and the
    quotient rounds to lim or above.  With lim 3 both happen.  Read lengths of at most 65,535 can say each of them."""
    rng = np.random.default_rng(1000 + lim)
    strict, loose = [], []        # float32 not below / exact below; float32 below / exact not below
    for _ in range(400000):
        if len(strict) >= 2 and (len(loose) >= 2 or lim != 3):
            break
        den = int(rng.integers((1 << 24) // lim + 2, (1 << 26) // lim))
        qsum = lim * den + int(rng.integers(-3, 4))
        if qsum <= (1 << 24) or den < 12:
            continue
        f, e = accept_f32(qsum, den, lim), Fraction(qsum, den) < lim
        if f == e:
            continue
        side = loose if f else strict
        if len(side) < 2:
            side.append((qsum, den))
    assert len(strict) == 2 and len(loose) == (2 if lim == 3 else 0), (lim, strict, loose)
    return strict, loose


def _tail_case(name, lim, rows, q_by_chrom, **kw):
    """chromosomes 2, 5 and 9 of a genome of 12 in one list: candidates of 5 reads 4 apart (span 16), one per chromosome but two on 5"""
    tid, pos, q = [], [], []
    for t, n_c in ((2, 1), (5, 2), (9, 1)):
        for k in range(n_c):
            tid += [t] * 5
            pos += [500 + 400 * k + 4 * i for i in range(5)]
            q += q_by_chrom[t]
    tail = np.zeros((12, 4), np.uint32)
    for t, r in rows.items():
        tail[t] = r
    return cut_case(name, tid, pos, q, tail=tail, lim=lim, nn=np.arange(len(tid)) * 2, n_normal=10 ** 6, **kw)


@functools.lru_cache(maxsize=None)
def cut_cases():
    out = []

    def add(name, tid, pos, qlen, **kw):
        out.append(cut_case(name, tid, pos, qlen, **kw))

    for n in (1, 2, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1025):
        t, p = runs(mixed_lengths(n))
        add("n%d" % n, t, p, qlens(n, n))
    for n in (TWO_PER_LANE - 1, TWO_PER_LANE, TWO_PER_LANE + 1, TWO_PER_LANE + 513):
        t, p = runs(mixed_lengths(n))
        add("n%d" % n, t, p, qlens(n, n % 1000))
    t, p = runs(mixed_lengths(300))
    add("host_count_above_300_700", t, p, qlens(300, 1), n_host=700)
    n = TWO_PER_LANE - 100
    t, p = runs(mixed_lengths(n))
    add("host_count_above_two_per_lane", t, p, qlens(n, 2), n_host=TWO_PER_LANE + 513)
    t, p = runs(np.ones(600, np.int64))
    add("every_read_its_own", t, p, qlens(600, 3))
    t, p = runs([600], step=1)
    add("one_candidate", t, p, qlens(600, 4))
    t, p = runs([TWO_PER_LANE + 513], step=1)
    add("one_candidate_two_per_lane", t, p, qlens(TWO_PER_LANE + 513, 5, 30, 100))
    for L in (1, 2, 64, 65, 257, 600):
        for how in RUN_LAYOUTS:
            lead = run_lead(L, how)
            t, p = runs([L, 3, 9, 1], lead=lead)
            add("run%d_%s" % (L, how), t, p, qlens(len(t), 10 * L + lead))
    # the largest read length, in turn: candidate of 70 reads from index 60 on (it straddles a wave), then one of 6, then singles
    t, p = runs([70, 6, 1, 3], lead=60)
    for where, idx in (("first", 60), ("second", 61), ("last", 129), ("breaking", 130), ("last_of_list", len(t) - 1)):
        q = qlens(len(t), 77, 30, 90)
        q[idx] = 60000
        add("maxq_" + where, t, p, q)
    t, p = runs([65], step=1)
    q = qlens(65, 78, 30, 90)
    q[64] = 60000
    add("maxq_alone_in_its_wave", t, p, q)
    t, p = runs([10, 10, 1], lead=4)
    t = t.copy()
    t[14:] = 1
    q = qlens(len(t), 79, 30, 90)
    q[14] = 60000
    add("maxq_breaking_on_another_chromosome", t, p, q)
    # gaps and chromosome changes
    add("gaps_W-1_W_W+1", [0] * 8, np.cumsum([100, 20, W0 - 1, 20, W0, 20, W0 + 1, 20]), qlens(8, 80))
    add("chromosome_change_+1_0_negative_far", [0, 0, 1, 1, 2, 2, 3, 3, 4, 4], [100, 120, 121, 140, 140, 160, 30, 50, 50 + W0 + 1, 90 + W0], qlens(10, 81))
    for ml in (-1, 0, 7):
        d = [100, max(ml, 0), W0 + 1, ml + 1, W0 + 1, ml + 2, W0 + 1]
        add("min_len_%d" % ml, [0] * 7, np.cumsum(d), qlens(7, 82), min_len=ml)
    for lim in (1, 3, 1000):
        den = 2000 if lim == 1 else 40
        add("coverage_at_lim_%d" % lim, **chain([cov_reads(lim * den + e, den) for e in (-1, 0, 1)], lim=lim))
        strict, loose = verdict_pairs(lim)
        wide = lim < 1000       # the denominators are 2^24 / lim and more: reads a window of 50 cannot chain
        add("float32_verdict_lim_%d" % lim, **chain([cov_reads(qs, dn, lim_w=1 << 20 if wide else W0) for qs, dn in strict + loose], lim=lim, W=1 << 20 if wide else W0))
    t, p = runs(np.ones(70000, np.int64))
    qs, dn = verdict_pairs(1000)[0][0]
    cp, cq, brk = cov_reads(qs, dn)
    cq[0] = 65535
    add("running_sum_past_2^32", np.concatenate([t, np.full(len(cp) + 1, 1, np.int32)]), np.concatenate([p, cp + 1000, [cp[-1] + 1000 + W0 + 1]]),
        np.concatenate([np.full(70000, 65535), cq, [brk]]))
    for nk in (1, 2, 3):
        t, p = runs(mixed_lengths(300))
        j = np.arange(300, dtype=np.int64)
        nn = ((1 << 32) - 40 + j // 2) & 0xFFFFFFFF
        pk = np.stack([((1 << 32) - 100 * (k + 1) + j * (k + 1)) & 0xFFFFFFFF for k in range(nk)])
        add("counts_wrap_%d_keys" % nk, t, p, qlens(300, 83), nn=nn, pk=pk, nkeys=nk, n_normal=200, stream=False)
    # tid_tail: several chromosomes of a sharded run in one list
    plain = {2: [40] * 5, 5: [40] * 5, 9: [40] * 5}
    out.append(_tail_case("tail_raises_maxq", 1000, {2: [1, 500, 77, 0], 5: [1, 30, 99, 0], 9: [1, 45, 123, 0]}, plain))
    # span 16, four counted reads of 40: 160 / (17 + 40) = 2.8 < 3; with the tail's 12 more: 172 / 57 = 3.02
    out.append(_tail_case("tail_tips_coverage", 3, {2: [1, 12, 77, 0], 5: [1, 12, 99, 0], 9: [0, 12, 123, 0]}, plain))
    out.append(_tail_case("tail_absent_for_the_last", 1000, {2: [1, 60, 77, 0], 5: [1, 70, 99, 0], 9: [0, 60000, 123, 0]}, plain))
    out.append(_tail_case("tail_next_chromosome_read_is_long", 1000, {2: [1, 41, 77, 0], 5: [1, 42, 99, 0], 9: [1, 43, 123, 0]},
                          {2: [40] * 5, 5: [50000] + [40] * 4, 9: [60000] + [40] * 4}))
    names = [c["name"] for c in out]
    assert len(set(names)) == len(names)
    for c in out:
        assert int(c["qlen"].sum()) < (1 << 31) or c["name"] == "running_sum_past_2^32"      # (a candidate's own sum always is)
    return out


def cut_case_named(name):
    return next(c for c in cut_cases() if c["name"] == name)


CUT_SLIPS = ("gap_ge", "tid_ignored", "first_counted", "breaking_not_counted", "tail_other_chrom_counted", "min_len_ge", "cov_le", "div_double", "div_exact",
             "maxq_without_tail")
HEADOUT_SLIPS = ("segmax_no_reset", "lane63_no_report")

# ---- a cut case as a read stream ------------------------------------------------------------------------------------------------

STREAM_CONFIG = "readgroup:rg1\tplatform:illumina\tmap:a.bam\treadlen:50.00\tlib:libA\tnum:10001\tlower:240.00\tupper:360.00\tmean:300.00\tstd:20.00\n"


def stream_of(c):
    """One BAM's records that make the oracle (and the product) see the case: an FF / RR or an inter-chromosomal read per anomalous read
    (mapping quality 60, its name seen once), and in front of read j as many leftmost reads of normal pairs as nn says.  The window
    comes out as W0: min(mean - 2 x read length, 50 where no pair has a wrong insert size)."""
    assert c["stream"]
    n = c["n"]
    nn = c["nn"].astype(np.int64)
    before = np.diff(np.concatenate([[0], nn]))
    after = c["n_normal"] - int(nn[-1])
    reps = before + 1
    reps[-1] += after
    idx = np.repeat(np.arange(n), reps)
    is_anom = np.zeros(len(idx), bool)
    is_anom[np.cumsum(reps) - reps + before] = True
    tid, pos = c["tid"][idx], c["pos"][idx]
    ctx = c["flag"][idx] == F_CTX
    rev = c["rev"][idx] != 0
    ntid = int(c["tid"].max()) + 2
    sam_anom = 0x1 | 0x40 | np.where(rev, 0x10, 0) | np.where(rev & ~ctx, 0x20, 0)
    d = dict(tid=tid.astype(np.int32), pos=pos.astype(np.int32),
             mtid=np.where(is_anom & ctx, (tid + 1) % ntid, tid).astype(np.int32),
             mpos=np.where(is_anom, pos, pos + 250).astype(np.int32),
             isize=np.where(is_anom, 0, 300).astype(np.int32),
             flag=np.where(is_anom, sam_anom, 0x1 | 0x2 | 0x40 | 0x20).astype(np.uint16),
             qlen=np.where(is_anom, c["qlen"][idx], 50).astype(np.int32),
             bdqual=np.full(len(idx), 60, np.uint8))
    d["rg"] = ["rg1"] * len(idx)
    d["name_id"] = np.arange(1, len(idx) + 1, dtype=np.uint64)
    return STREAM_CONFIG, [d], ["c%d" % (i + 1) for i in range(ntid)]


# ---------------------------------------------------------------------------------------------------------------------------------
# the join
# ---------------------------------------------------------------------------------------------------------------------------------
_C1, _C2 = 0xff51afd7ed558ccd, 0xc4ceb9fe1a85ec53
_I1, _I2 = pow(_C1, -1, 1 << 64), pow(_C2, -1, 1 << 64)


def mix64(k):
    k = np.asarray(k, np.uint64)
    with np.errstate(over="ignore"):
        h = k ^ (k >> np.uint64(33))
        h = h * np.uint64(_C1)
        h = h ^ (h >> np.uint64(33))
        h = h * np.uint64(_C2)
        h = h ^ (h >> np.uint64(33))
    return h


def unmix64(h):
    """the key whose mix64 is h (every step of the finaliser can be undone): how the builders aim a key at a slot, a tag or a bucket"""
    h = int(h)
    h ^= h >> 33
    h = (h * _I2) & M64
    h ^= h >> 33
    h = (h * _I1) & M64
    h ^= h >> 33
    return h


def bucket_of(h, log2b):
    h = np.asarray(h, np.uint64)
    return (h >> np.uint64(64 - log2b)).astype(np.int64) if log2b else np.zeros(h.shape, np.int64)


def join_case(name, key, region, check=None, fkey=None, fregion=None, fcheck=None, n_host=None, direct=True, bucketed=True, slots=None, nbuckets=(1,),
              routes=None, expect=None):
    key = np.ascontiguousarray(key, np.uint64)
    n = len(key)
    region = np.ascontiguousarray(region, np.int32)
    assert len(region) == n
    nf = 0 if fkey is None else len(fkey)
    if fkey is not None:
        fkey, fregion = np.ascontiguousarray(fkey, np.uint64), np.ascontiguousarray(fregion, np.int32)
        bucketed = False                     # foreign entries always take the direct table (sharded runs force it)
    if check is not None:
        check = np.ascontiguousarray(check, np.uint64)
        fcheck = None if fkey is None else np.ascontiguousarray(fcheck, np.uint64)
    if slots is None:
        slots = 1024
        while slots < 4 * (n + nf):
            slots <<= 1
    assert 2 * (n + nf) <= slots <= (1 << 20)
    return dict(name=name, n=n, nf=nf, key=key, region=region, check=check, fkey=fkey, fregion=fregion, fcheck=fcheck, n_host=int(n + nf if n_host is None else n_host),
                direct=direct, bucketed=bucketed, slots=slots, nbuckets=tuple(nbuckets), routes=routes, expect=expect or {})


def _names(c):
    key = c["key"].tolist() + (c["fkey"].tolist() if c["nf"] else [])
    if c["check"] is not None:
        chk = c["check"].tolist() + (c["fcheck"].tolist() if c["nf"] else [])
    else:
        chk = [0] * len(key)
    reg = c["region"].tolist() + (c["fregion"].tolist() if c["nf"] else [])
    return key, chk, reg


def join_reference(c):
    """partner and pair_lo of the own entries, irregular, and the own entries whose partner no result pins (names seen three times or more)"""
    key, chk, reg = _names(c)
    n = c["n"]
    table = {}
    for i, nm in enumerate(zip(key, chk)):
        table.setdefault(nm, []).append(i)
    partner = np.full(n, -1, np.int32)
    pair_lo = np.full(n, -1, np.int32)
    loose = np.zeros(n, bool)
    irregular = 0
    for idx in table.values():
        if len(idx) == 1:
            continue
        if len(idx) > 2:
            irregular = 1
            for i in idx:
                if i < n:
                    loose[i] = True
            continue
        a, b = idx
        alive = reg[a] >= 0 and reg[b] >= 0
        for x, y in ((a, b), (b, a)):
            if x < n:
                partner[x] = y if alive else -2
        if alive and a < n:                   # (b >= n: the foreign entry is the earlier one whatever its index)
            later, earlier = (b, a) if b < n else (a, b)
            pair_lo[later] = reg[earlier]
        # (two foreign entries: neither has a partner[] or pair_lo[] entry)
    return dict(partner=partner, pair_lo=pair_lo, irregular=irregular, loose=loose)


def join_all_pairs(c):
    """every entry against every other"""
    key, chk, reg = (np.asarray(x) for x in _names(c))
    key, chk = key.astype(np.uint64), chk.astype(np.uint64)
    n, tot = c["n"], c["n"] + c["nf"]
    same = (key[:, None] == key[None, :]) & (chk[:, None] == chk[None, :]) & ~np.eye(tot, dtype=bool)
    cnt = same.sum(axis=1)
    other = same.argmax(axis=1)
    partner = np.full(n, -1, np.int32)
    pair_lo = np.full(n, -1, np.int32)
    for i in range(n):
        if cnt[i] != 1:
            continue
        o = int(other[i])
        alive = reg[i] >= 0 and reg[o] >= 0
        partner[i] = o if alive else -2
        if alive and (o >= n or o < i):
            pair_lo[i] = reg[o]
    return dict(partner=partner, pair_lo=pair_lo, irregular=int((cnt > 1).any()), loose=(cnt > 1)[:n])


def join_differs(got, ref):
    if got["irregular"] != ref["irregular"]:
        return "irregular"
    keep = ~ref["loose"]
    for k in ("partner", "pair_lo"):
        if k in got and got[k] is not None and (got[k][keep] != ref[k][keep]).any():
            return k
    return None


def direct_model(c, slip=None):
    """The direct table with the entries arriving in index order (own ones, then foreign ones).  Also says what happened on the way: a probe
    that went from the last slot to slot 0, an equal tag on another key, a check that told two equal keys apart."""
    key, chk, reg = _names(c)
    n, mask = c["n"], c["slots"] - 1
    h = mix64(np.asarray(key, np.uint64)).tolist()
    table = {}
    partner = np.full(n, -1, np.int32)
    pair_lo = np.full(n, -1, np.int32)
    seen = dict(wrap=0, tag_clash=0, check_split=0, irregular=0)
    for j in range(len(key)):
        tag, s = h[j] >> 32, h[j] & mask
        jf = j >= n
        for probes in range(MAX_PROBES + 1):
            if s not in table:
                table[s] = (tag, j)
                break
            otag, o = table[s]
            if otag == tag:
                same_key = key[o] == key[j]
                if not same_key:
                    seen["tag_clash"] += 1
                if same_key and chk[o] != chk[j]:
                    seen["check_split"] += 1
                if (same_key or slip == "tag_is_key") and (chk[o] == chk[j] or slip == "check_ignored"):
                    of = o >= n
                    alive = reg[j] >= 0 and reg[o] >= 0
                    pj = int(o) if (alive or (slip == "minus2_own_only" and reg[j] >= 0)) else -2
                    po = int(j) if (alive or (slip == "minus2_own_only" and reg[o] >= 0)) else -2
                    if not jf:
                        partner[j] = pj
                    if not of:
                        third = partner[o] != -1
                        if slip == "third_adjacent_only":
                            third = third and abs(j - o) == 1
                        if third:
                            seen["irregular"] = 1
                        partner[o] = po
                    if alive:
                        if jf != of:
                            if jf:
                                pair_lo[o] = reg[j]
                            else:
                                pair_lo[j] = reg[o]
                        elif not jf:
                            lo, hi = (o, j) if o < j else (j, o)
                            if slip == "pair_lo_earlier":
                                pair_lo[lo] = reg[hi]
                            else:
                                pair_lo[hi] = reg[lo]
                    break
            if s == mask:
                seen["wrap"] += 1
            s = (s + 1) & mask
        else:
            seen["irregular"] = 1
    return dict(partner=partner, pair_lo=pair_lo, irregular=seen["irregular"]), seen


def bucket_routes(c, nbuckets, slip=None):
    """per bucket that holds entries: (entries, "lds" or "hbm") -- k4_join_kernel's choice"""
    log2b = nbuckets.bit_length() - 1
    cnt = np.bincount(bucket_of(mix64(c["key"]), log2b), minlength=nbuckets)
    out = {}
    for b in np.flatnonzero(cnt).tolist():
        k = int(cnt[b])
        lds = 2 * k < JOIN_LDS_SLOTS if slip == "bucket_route_ge" else 2 * k <= JOIN_LDS_SLOTS
        out[b] = (k, "lds" if lds else "hbm")
    return out


def bucket_offsets(c, nbuckets):
    log2b = nbuckets.bit_length() - 1
    cnt = np.bincount(bucket_of(mix64(c["key"]), log2b), minlength=nbuckets)
    return np.concatenate([[0], np.cumsum(cnt)]).astype(np.uint32)


def forward_model(words, slip=None):
    """dst after forward_quads and the tail words, for a table of `words` 32-bit words numbered 1 ..: 0 where nothing was stored"""
    src = np.arange(1, words + 1, dtype=np.int64)
    dst = np.zeros(words, np.int64)
    quads = words // 4
    gsz = FWD_BLOCKS * 256
    t = np.arange(gsz, dtype=np.int64)

    def store(q):
        q = q[q < quads]
        for w in range(4):
            dst[4 * q + w] = src[4 * q + w]

    i = t.copy()
    if quads:
        while True:
            whole = i + 3 * gsz < quads
            if not whole.any():
                break
            for u in range(4):
                store(i[whole] + u * gsz)
            i = np.where(whole, i + 4 * gsz, i)
        if slip != "forward_last_turn_dropped":
            for u in range(3):
                store(i + u * gsz)
    if slip != "forward_no_tail_words":
        for w in range(quads * 4, words):
            dst[w] = src[w]
    return dst, src


def rng_keys(n, seed):
    return np.random.default_rng(seed).integers(1, 1 << 63, n, dtype=np.uint64)


def paired(n, seed, apart=1):
    """n entries: entry i and i + apart carry one name, in blocks of 2 x apart; what is left over is seen once"""
    key = rng_keys(n, seed)
    i = np.arange(n)
    blk = i // (2 * apart)
    full = (blk + 1) * 2 * apart <= n
    mate = np.where(full & (i % (2 * apart) >= apart), i - apart, i)
    return key[mate]


def key_at(slot_bits=None, tag=None, top=None, top_bits=0, salt=0):
    """a key whose hash has the given low bits (slot), tag (upper 32 bits) or top bits (bucket); the rest comes from the salt"""
    h = int(mix64(np.uint64(0x9E3779B97F4A7C15 * (salt + 1) & M64)))
    if tag is not None:
        h = (h & 0xFFFFFFFF) | (tag << 32)
    if top_bits:
        h = (h & ((1 << (64 - top_bits)) - 1)) | (top << (64 - top_bits))
    if slot_bits is not None:
        bits, val = slot_bits
        h = (h & ~((1 << bits) - 1)) | val
    k = unmix64(h)
    assert int(mix64(np.uint64(k))) == h
    return k


@functools.lru_cache(maxsize=None)
def join_cases():
    out = []

    def add(name, key, region=None, **kw):
        region = np.arange(len(key)) // 3 if region is None else region
        out.append(join_case(name, key, region, **kw))

    for n in (1, 2, 255, 256, 257, 511, 512, 513):
        add("n%d" % n, paired(n, n), nbuckets=(1, 2))
    add("host_count_above", paired(300, 9), n_host=900, slots=4096, nbuckets=(2,))
    add("mates_64_apart", paired(1024, 10, apart=64), nbuckets=(2,))
    add("mates_in_different_workgroups", paired(2048, 11, apart=512), nbuckets=(1024, 2048, 8192))
    k = paired(600, 12)
    add("both_in_one_region", k, region=np.arange(600) // 2)
    r = np.arange(600) // 2
    r1 = r.copy(); r1[::4] = -1            # one mate of every second pair rejected
    add("one_mate_rejected", k, region=r1)
    r2 = r.copy(); r2[(np.arange(600) // 2) % 2 == 0] = -1
    add("both_mates_rejected", k, region=r2)
    add("names_seen_once", rng_keys(700, 13), nbuckets=(1, 1024))
    for name, idx, rej in (("third_sighting_in_one_wave", (3, 4, 5), None), ("third_sighting_in_three_workgroups", (10, 300, 700), None),
                           ("third_sighting_one_rejected", (10, 300, 700), 300), ("four_sightings", (5, 6, 400, 800), None)):
        k = paired(900, 14)
        k[list(idx)] = np.uint64(0x1234567890ABCDEF)
        # (their former mates are now seen once)
        r = np.arange(900) // 3
        if rej is not None:
            r[rej] = -1
        add(name, k, region=r, nbuckets=(1, 2), expect=dict(irregular=1))
    k = paired(400, 15)
    chk = rng_keys(400, 16)[np.arange(400) // 2 * 2]        # mates agree
    k2, c2 = k.copy(), chk.copy()
    k2[10] = k2[20]; c2[10] = np.uint64(111); c2[20] = np.uint64(222)       # one key, two names seen once (their old mates as well)
    add("equal_key_two_names", k2, check=c2, nbuckets=(1, 2), expect=dict(check_split=True))
    k3, c3 = k.copy(), chk.copy()
    k3[30:32] = k3[40]; k3[41] = k3[40]                      # entries 30, 31, 40, 41: one key, two pairs
    c3[30:32] = np.uint64(333); c3[40:42] = np.uint64(444)
    add("equal_key_two_pairs", k3, check=c3, nbuckets=(1, 2), expect=dict(check_split=True))
    k = rng_keys(4300, 17)
    k[100:4200] = np.uint64(0x0FEDCBA987654321)
    add("name_carried_by_4100", k, nbuckets=(1, 2), expect=dict(irregular=1))
    own = paired(500, 18)
    fk = rng_keys(40, 19)
    own2 = own.copy()
    solo = np.arange(20) * 22 + 1
    own2[solo] = rng_keys(20, 20)                            # 20 own reads (and their former mates) seen once ...
    fk[:20] = own2[solo]                                     # ... of which these get a foreign mate
    fr = np.arange(40, dtype=np.int32) + 1000
    fr[5] = -1
    fk[39] = fk[38]                                          # two foreign entries with one name: no entry of theirs anywhere
    add("foreign_entries", own2, fkey=fk, fregion=fr)
    add("foreign_entries_with_check", own2, check=own2 ^ np.uint64(0xABCDEF), fkey=fk, fregion=fr, fcheck=fk ^ np.uint64(0xABCDEF))
    # direct only
    add("table_1023_half_full", paired(512, 21), slots=1024, bucketed=False)
    keys, slot, tag = [], 700, 0xDEADBEEF
    for s in range(4):                                       # four different keys with one tag on one slot, each carried twice
        keys += [key_at(slot_bits=(10, slot), tag=tag, salt=s)]
    keys = keys + keys
    fillers = [key_at(slot_bits=(10, slot + 1 + i % 3), salt=100 + i) for i in range(6)]
    add("equal_tags_on_one_probe_run", np.asarray(keys + fillers + fillers, np.uint64), region=np.arange(20), slots=1024, bucketed=False, expect=dict(tag_clash=True))
    keys = [key_at(slot_bits=(10, 1023), salt=200 + i) for i in range(5)] + [key_at(slot_bits=(10, 1022), salt=300 + i) for i in range(3)]
    add("wrap_from_the_last_slot", np.asarray(keys + keys, np.uint64), region=np.arange(16), slots=1024, bucketed=False, expect=dict(wrap=True))
    # bucketed only
    def in_bucket(b, log2b, count, salt):
        ks = [key_at(top=b, top_bits=log2b, salt=salt + i) for i in range(count // 2)]
        return ks + ks + ([key_at(top=b, top_bits=log2b, salt=salt + count)] if count % 2 else [])

    add("all_in_one_bucket_of_8", np.asarray(in_bucket(5, 3, 600, 1000), np.uint64), direct=False, nbuckets=(8,), routes={8: {5: (600, "lds")}})
    for cnt, route in ((4096, "lds"), (4097, "hbm"), (10000, "hbm")):
        ks = np.asarray(in_bucket(1, 1, cnt, 2000) + in_bucket(0, 1, 300, 40000), np.uint64)
        add("bucket_of_%d" % cnt, ks, direct=False, nbuckets=(2,), routes={2: {1: (cnt, route), 0: (300, "lds")}})
    names = [c["name"] for c in out]
    assert len(set(names)) == len(names)
    return out


def join_case_named(name):
    return next(c for c in join_cases() if c["name"] == name)


DIRECT_SLIPS = ("minus2_own_only", "pair_lo_earlier", "third_adjacent_only", "tag_is_key", "check_ignored")
FORWARD_REGIONS = (0, 1, 2, 3, 4, 5, 14563, 14564, 29127, 29128)      # 9 words a region: every words mod 4; either side of one and of two whole turns
FORWARD_NKEYS2 = (2, 4, 6)


def forward_table(n_regions, nkeys2, seed=0):
    rng = np.random.default_rng(500 + seed + n_regions)
    return rng.integers(0, 1 << 32, (n_regions, REC_WORDS), dtype=np.uint32), rng.integers(0, 1 << 32, (n_regions, nkeys2), dtype=np.uint32)
