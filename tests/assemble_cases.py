"""Cases, reference and models for K6 between the mate join and the final table (csrc/k6_assemble.hip: k6_pairs_kernel, k6_label_kernel,
k6_classify_kernel, k6_emit_kernel, k6_walk_kernel, k6_walk_big_kernel with assemble_sv, k6_place_kernel behind them), run on their own
by tests/test_gpu_assemble.py through tests/prims/assemble.hip and held to ground truth by tests/test_assemble_cases.py.  No GPU is
needed here.

A case is a table of regions and the anomalous reads of those regions in stream order, each read with a name: what the region cut and
the mate join hand to K6 (region table, region_of, partner, pair_lo, meta, isize) is derived from the names by a dictionary.

The reference (walk_reference) is a read-level restatement of BreakDancer.cpp:266-497 and SvBuilder.cpp:18-118: one read at a time, a
name -> regions dictionary, a dict-of-dicts graph, flushes of buffer_size + 1 regions, start vertices ascending, the frontier, neighbours
ascending, paired reads leaving their regions before any gate, regions cleared once final, the stale _max_readlen, process_sv in numpy
float32 in the reference's operation order (float64 for lambda).  It shares nothing with bdx_walk.cpp or K6: it knows no pair group.

The models restate what the groups stage leaves (RegSum with its part order, the kWeakPart marks, e_lo / e_w / e_off / e_cnt, out_deg,
the hub and bad_v verdicts, the host list as a multiset) and, where the order of the atomics cannot matter, which walk takes a
component.

What no result can show: which label a component carries whose labels have not converged (it goes to the host whatever they are), the
order of g_rec (wave-aggregated reservations in arrival order), and which member slot of its label a region gets (atomicAdd order)."""
import numpy as np

FILL = 0xA5A5A5A5
NA, FF, LARGE, SMALL, RF, RR, NORMAL_FR, NORMAL_RF, CTX, MATE_UNMAPPED, UNMAPPED = range(11)
NUM_FLAGS = 11
# what the classifier emits for a read that reaches the region cut (BreakDancer.cpp:194-207: RR has become FF, the normal classes have left)
EMITTED_FLAGS = (FF, LARGE, SMALL, RF, CTX, MATE_UNMAPPED)
MAX_MEMBERS, MAX_IN, BIG_MEMBERS, LIB_STRIDE = 4, 3, 64, 16                     # kK6MaxMembers, kK6MaxIn, kK6BigMembers, kK6LibStride
SHIFT_T, SHIFT_OWN, SHIFT_START, SEQ_MASK = 35, 34, 8, 255                     # the order key (csrc/bdx_k3.h)
RS_WORDS, SV_WORDS, WIRE_WORDS, MEMBER_WORDS, COUNT_WORDS, REC_WORDS = 20, 24, 12, 28, 22, 9
MAX_CAP = 4094
CONSTANTS = [MAX_MEMBERS, MAX_IN, BIG_MEMBERS, LIB_STRIDE, SHIFT_T, SHIFT_OWN, SHIFT_START, SEQ_MASK, RS_WORDS, SV_WORDS, WIRE_WORDS, MEMBER_WORDS, COUNT_WORDS,
             NUM_FLAGS, REC_WORDS, MAX_CAP]
WEAK = 1 << 63
INT_MIN = -(1 << 31)
COVERED = 3_000_000
SCORE_THRESHOLD = 30


# ---------------------------------------------------------------------------------------------------------------------------------
# a case: regions and named reads
# ---------------------------------------------------------------------------------------------------------------------------------

class Table:
    """regions 0 .. n - 1 on one chromosome (or as tid says), 1,000 bases apart; reads are added region by region, pairs by name"""

    def __init__(self, n, tid=None, maxq=None):
        self.n = n
        self.tid = [0] * n if tid is None else list(tid)
        self.start = [1000 * (r + 1) for r in range(n)]
        self.end = [1000 * (r + 1) + 100 + 7 * (r % 5) for r in range(n)]
        self.maxq = [40 + (r * 5) % 23 for r in range(n)] if maxq is None else list(maxq)
        self.reads = [[] for _ in range(n)]        # per region: (name, flag, lib, isize, rev)
        self.loose = []                            # reads of rejected candidates: (region they follow, name)
        self.names = 0

    def _name(self):
        self.names += 1
        return self.names

    def single(self, r, flag=FF, lib=0, isize=100, rev=0):
        """a read whose mate is nowhere (partner -1)"""
        self.reads[r].append((self._name(), flag, lib, isize, rev))

    def pair(self, a, b, flag=FF, lib=0, isize=100, n=1, flag_first=None):
        """n pairs: the first-observed mate in region a, the second-observed one -- whose flag, library and insert size count -- in b >= a"""
        assert a <= b
        for i in range(n):
            nm = self._name()
            self.reads[a].append((nm, flag if flag_first is None else flag_first, lib, isize + 3 * i, i & 1))
            self.reads[b].append((nm, flag, lib, isize + 3 * i, (i + 1) & 1))

    def pairs_with(self, a, b, isizes, flag=FF, lib=0):
        for isz in isizes:
            nm = self._name()
            self.reads[a].append((nm, flag, lib, isz, 0))
            self.reads[b].append((nm, flag, lib, isz, 1))

    def rejected_mate(self, r, flag=FF, lib=0, isize=100, later=True):
        """a read of region r whose mate lies in a rejected candidate behind it (partner -2: ReadRegionData.cpp:177-199 forgets the name)"""
        nm = self._name()
        self.reads[r].append((nm, flag, lib, isize, 0))
        self.loose.append((r, nm))


def make_case(name, t, nlibs=1, nkeys=1, min_read_pair=2, chr_restricted=0, period=101, last_maxq=55, pk=None, why_no_stream=None, **kw):
    """the case as K6 gets it.  Reads are numbered in stream order, region by region; the reads of rejected candidates (region -1) follow
    the region they were added behind"""
    rec = np.zeros((t.n, REC_WORDS), np.int64)
    region_of, names, meta, isize = [], [], [], []
    for r in range(t.n):
        rd = t.reads[r]
        rec[r] = [t.tid[r], t.start[r], t.end[r], len(rd), sum(x[4] for x in rd), sum(1 for x in rd if x[1] != CTX), 3 * r, t.maxq[r], len(region_of)]
        for nm, flag, lib, isz, rev in rd:
            region_of.append(r); names.append(nm); meta.append(flag | (rev << 4) | (lib << 8) | (50 << 16)); isize.append(isz)
        for rr, nm in t.loose:
            if rr == r:
                region_of.append(-1); names.append(nm); meta.append(FF | (50 << 16)); isize.append(0)
    n = len(region_of)
    seen = {}
    partner = np.full(n, -1, np.int32)
    pair_lo = np.full(n, -1, np.int32)
    for j, nm in enumerate(names):
        if nm in seen:
            i = seen[nm]
            alive = region_of[i] >= 0 and region_of[j] >= 0
            partner[i], partner[j] = (j, i) if alive else (-2, -2)
            if alive:
                pair_lo[j] = region_of[i]
        else:
            seen[nm] = j
    if pk is None:
        pk = default_pk(t.n, nkeys)
    pk = np.ascontiguousarray(pk, np.uint32)
    assert pk.shape == (t.n, 2 * nkeys)
    c = dict(name=name, n_regions=t.n, n_reads=n, rec=rec.astype(np.uint32), region_of=np.asarray(region_of, np.int32).reshape(n), partner=partner, pair_lo=pair_lo,
             meta=np.asarray(meta, np.uint32).reshape(n), isize=np.asarray(isize, np.int32).reshape(n), names=names, pk=pk, nlibs=nlibs, nkeys=nkeys,
             min_read_pair=min_read_pair, chr_restricted=chr_restricted, period=period, last_maxq=last_maxq, why_no_stream=why_no_stream,
             lib_mean=(300 + 10 * np.arange(nlibs) + 0.25).astype(np.float32), key_density=(0.001 * (np.arange(nkeys) + 1)).astype(np.float32),
             hist=(1000 * (np.arange(nlibs)[:, None] + 1) + 37 * np.arange(NUM_FLAGS)[None, :]).astype(np.uint32), covered=COVERED,
             big_walk=0, asm_plain=0, ins_plain=0, propagation_rounds=2, n_host=None, g_cap=None, use_pair_lo=True, groups_only=False, expect={})
    c.update(kw)
    return c


def default_pk(n, nkeys):
    """proper-read prefix samples that only grow along the stream: at a region's first read, at its last; some keys without a read in between"""
    pk = np.zeros((n, 2 * nkeys), np.int64)
    cur = np.array([11 * k for k in range(nkeys)], np.int64)
    for r in range(n):
        cur = cur + np.array([(r * 7 + k * 3) % 5 if k % 3 != 2 else 0 for k in range(nkeys)])
        pk[r, :nkeys] = cur
        cur = cur + np.array([(r + k) % 3 for k in range(nkeys)])
        pk[r, nkeys:] = cur
    return (pk & 0xFFFFFFFF).astype(np.uint32)


# ---------------------------------------------------------------------------------------------------------------------------------
# the reference: BreakDancer.cpp:266-497, SvBuilder.cpp:18-118, one read at a time
# ---------------------------------------------------------------------------------------------------------------------------------

def _to_int(x):
    """int(double) as cvttsd2si does it: truncation toward zero, INT_MIN for a NaN or a value out of range"""
    x = float(x)
    if x != x or x >= 2147483648.0 or x <= -2147483649.0:
        return INT_MIN
    return int(x)


def poisson_logp(terms, tail):
    """ComputeProbScore's Kahan-compensated sum (BreakDancer.cpp:52-69); tail(lambda, k) = log of the Poisson upper tail"""
    logp, err = 0.0, 0.0
    for lam, k in terms:
        a = tail(lam, k) - err
        b = logp + a
        err = (b - logp) - a
        logp = b
    return logp


def walk_reference(c, slip=None, tail=None):
    """the reference's table in output order: one dict per record, with the start vertex of its traversal, whether that vertex belongs to an
    earlier flush window, and the (lib, pairs, lambda) and (key, copy number) entries"""
    f32 = np.float32
    NR, mrp, nk, period = c["n_regions"], c["min_read_pair"], c["nkeys"], c["period"]
    rec = c["rec"].astype(np.int64)
    rec[:, :3] = c["rec"][:, :3].view(np.int32)
    flags = (c["meta"] & 15).tolist()
    libs = ((c["meta"] >> 8) & 255).tolist()
    isz = c["isize"].tolist()
    names, region_of = c["names"], c["region_of"].tolist()
    read_regions = {}             # name -> regions it was seen in (ReadRegionData::_read_regions)
    graph = {}                    # vertex -> {neighbour: pairs}
    region_reads = {}             # region -> indices of its stored reads; absent: deleted
    out = []
    first_seen = {}               # library -> order of first appearance (a slip)

    def exists(j):
        return names[j] in read_regions

    def process_sv(snodes, max_readlen, start, from_old, T):
        observed, cnt, rc, span, pairs_at = {}, [0] * NUM_FLAGS, {}, {}, []
        kept = {r: [j for j in region_reads[r] if exists(j)] for r in snodes}
        for r in snodes:
            for j in kept[r]:
                nm = names[j]
                if nm in observed:
                    i = observed.pop(nm)
                    cnt[flags[j]] += 1
                    rc.setdefault(flags[j], {}); span.setdefault(flags[j], {})
                    rc[flags[j]][libs[j]] = rc[flags[j]].get(libs[j], 0) + 1
                    span[flags[j]][libs[j]] = span[flags[j]].get(libs[j], 0) + isz[j]
                    first_seen.setdefault(libs[j], len(first_seen))
                    pairs_at.append((region_of[i], region_of[j], nm))
                else:
                    observed[nm] = j
        num_pairs = sum(cnt)
        best = max(cnt)
        flag = NA
        if best > 0:
            flag = max(f for f in range(NUM_FLAGS) if cnt[f] == best) if slip == "tie_highest" else cnt.index(best)
        passes = num_pairs >= mrp and cnt[flag] >= mrp
        stay = set(observed)
        if not passes and slip == "rejected_keeps":
            stay |= {nm for _, _, nm in pairs_at}
        if not passes and slip == "self_after_gates":
            stay |= {nm for a, b, nm in pairs_at if a == b}
        for r in snodes:                          # paired reads leave their regions before any gate (BreakDancer.cpp:363-368)
            region_reads[r] = [j for j in kept[r] if names[j] in stay]
        if num_pairs < mrp:
            return
        if cnt[flag] < mrp:
            return
        A = snodes[0]
        B = snodes[1] if len(snodes) == 2 else -1
        ra = rec[A]
        chr_, pos = [int(ra[0]), int(ra[0])], [int(ra[1]), int(ra[2])]
        fwd, rev = [int(ra[3] - ra[4])] * 2, [int(ra[4])] * 2
        size = int(ra[2] - ra[1] + 1)
        cn = []
        if B >= 0:
            rb = rec[B]
            fwd[1], rev[1] = int(rb[3] - rb[4]), int(rb[4])
            if flag == RF:
                pos[1] = int(rb[2]) + max_readlen - 5
            elif flag == FF:
                pos[0] = pos[1]
                pos[1] = int(rb[2]) + max_readlen - 5
            elif flag == RR:
                pos[1] = int(rb[1])
            else:
                pos[0] = pos[1]
                pos[1] = int(rb[1])
            chr_[1] = int(rb[0])
            size += int(rb[2] - rb[1] + 1)
            dist = f32(pos[1] - pos[0])
            for k in range(nk):
                n_between = (int(c["pk"][B, k]) - int(c["pk"][A, nk + k])) & 0xFFFFFFFF
                if n_between:
                    cn.append((k, f32(f32(f32(n_between) / f32(c["key_density"][k] * dist)) * f32(2.0))))
        with np.errstate(invalid="ignore", divide="ignore"):
            if slip == "cn_sum_double":
                total = f32(sum(float(v) for _, v in cn))
            else:
                total = f32(0.0)
                for _, v in cn:
                    total = f32(total + v)
            total = f32(total / f32(f32(2.0) * f32(len(cn))))
            af = f32(f32(1) - total)
        if flag != RF and flag != RR and pos[0] + max_readlen - 5 < pos[1]:
            pos[0] += max_readlen - 5
        by_lib = sorted(rc.get(flag, {}))
        if slip == "lib_first_seen":
            by_lib = sorted(by_lib, key=lambda l: first_seen[l])
        diff = f32(0.0)
        terms = []
        for l in by_lib:
            diff = f32(diff + f32(f32(span[flag][l]) - f32(f32(rc[flag][l]) * c["lib_mean"][l])))
            lam = float(size) * (float(c["hist"][l, flag]) / float(c["covered"]))
            if slip != "no_lambda_floor":
                lam = max(1.0e-10, lam)
            terms.append((l, rc[flag][l], lam))
        with np.errstate(invalid="ignore", divide="ignore"):
            q = f32(diff / f32(cnt[flag]))
        if slip == "size_quotient_double" and cnt[flag]:
            q = float(diff) / cnt[flag]
        diffspan = _to_int(np.floor(float(q) + 0.5)) if slip == "size_nearest" else _to_int(float(q) + 0.5)
        mask = 0
        for a, b, _ in pairs_at:
            mask |= 2 if a != b else (1 if a == A else 4)
        o = dict(chr=chr_, pos=[pos[0] + 1, pos[1] + 1], fwd=fwd, rev=rev, flag=flag, size=diffspan, num_reads=cnt[flag], region=[A, B], af=af, cn=cn,
                 terms=terms, grp_mask=mask, start=start, from_old=from_old, T=T)
        if tail is not None:
            o["logp"] = poisson_logp([(lam, k) for _, k, lam in terms], tail)
            ph = -10.0 * o["logp"] / np.log(10.0)
            o["score"] = 99 if ph > 99 else _to_int(ph + 0.5)
            o["printed"] = 1 if o["score"] > SCORE_THRESHOLD else 0
        out.append(o)

    def build_connection(max_readlen, first_new):
        active = sorted(graph)
        v = min(graph) if graph else None
        while v is not None:
            tails = [v]
            from_old = v < first_new
            if slip == "old_self_again" and from_old and v in region_reads:
                graph[v].setdefault(v, mrp)
            while tails:
                newtails = []
                for tl in tails:
                    if tl not in region_reads or tl not in graph:
                        continue
                    edges = graph[tl]
                    for s1 in sorted(edges, reverse=(slip == "neighbours_descending")):
                        nlinks = edges.pop(s1)
                        too_few = nlinks <= mrp if slip == "gate_gt" else nlinks < mrp
                        if too_few or s1 not in region_reads:
                            continue
                        if tl != s1:
                            graph.get(s1, {}).pop(tl, None)
                            sn = [min(s1, tl), max(s1, tl)]
                        else:
                            sn = [s1]
                        newtails.append(s1)
                        process_sv(sn, max_readlen, v, from_old, first_new if from_old else v)
                    del graph[tl]
                tails = newtails
            later = [x for x in graph if x > v]
            v = min(later) if later else None
        for r in active:                              # ReadRegionData::is_region_final / clear_region
            if r not in region_reads or r == last_region[0]:
                continue
            if all((c["chr_restricted"] and flags[j] == CTX) or len(read_regions.get(names[j], ())) == 2 for j in region_reads[r]):
                for j in region_reads[r]:
                    left = [x for x in read_regions.get(names[j], ()) if x != r]
                    if left:
                        read_regions[names[j]] = left
                    else:
                        read_regions.pop(names[j], None)
                del region_reads[r]
        graph.clear()

    def flush(closing):
        """_max_readlen is the value of the candidate that closes at the flush (BreakDancer.cpp:254-259), the last candidate's at the end"""
        at = closing
        if slip == "own_window_maxq" and graph:
            at = (min(graph) // period + 1) * period - 1
            at = at if at < NR else None
        build_connection(int(rec[at, 7]) if at is not None else c["last_maxq"], first_new[0])

    last_region = [-1]
    in_buffer, first_new = 0, [0]
    j = 0
    n = c["n_reads"]
    for r in range(NR):
        mine = []
        while j < n and region_of[j] in (r, -1):
            if region_of[j] == -1:                    # a rejected candidate: its reads' names are forgotten (ReadRegionData.cpp:177-199)
                read_regions.pop(names[j], None)
            else:
                mine.append(j)
            j += 1
        last_region[0] = r
        for i in mine:                                # ReadRegionData::add_region
            rl = read_regions.setdefault(names[i], [])
            rl.append(r)
            if len(rl) == 2:
                a, b = rl
                graph.setdefault(a, {})
                graph[a][b] = graph[a].get(b, 0) + 1
                if a != b:
                    graph.setdefault(b, {})
                    graph[b][a] = graph[b].get(a, 0) + 1
        valid = int(rec[r, 3]) if (not c["chr_restricted"] or slip == "stored_from_n") else int(rec[r, 5])
        region_reads[r] = mine if valid >= mrp else []
        in_buffer += 1
        if in_buffer > period - 1:
            flush(r)
            in_buffer = 0
            first_new[0] = r + 1
    while j < n:                                      # rejected candidates behind the last region
        read_regions.pop(names[j], None)
        j += 1
    flush(None)
    return out


def reference_keys(ref, seq_bits=None):
    """the order keys of the reference's from-old records with the sequence number counted per (T, start) and kept to seq_bits bits: the
    device's count runs on over the start vertices of a component, so two records share a key there exactly when two share one here"""
    seq = {}
    keys = []
    for o in ref:
        if not o["from_old"]:
            keys.append(None)
            continue
        s = seq.get((o["T"], o["start"]), 0)
        seq[(o["T"], o["start"])] = s + 1
        mask = SEQ_MASK if seq_bits is None else (1 << seq_bits) - 1
        keys.append((o["T"] << SHIFT_T) | (o["start"] << SHIFT_START) | (s & mask))
    return keys


# ---------------------------------------------------------------------------------------------------------------------------------
# models of what the groups stage leaves
# ---------------------------------------------------------------------------------------------------------------------------------

def second_mates(c, r):
    """(lo, lib, flag, isize) of the reads of region r that are the second-observed mate of a pair, in read order, with their chunk of 64"""
    first, n = int(c["rec"][r, 8]), int(c["rec"][r, 3])
    out = []
    for i in range(n):
        j = first + i
        p = int(c["partner"][j])
        lo = int(c["region_of"][p]) if 0 <= p < j else -1
        if lo >= 0:
            out.append((lo, (int(c["meta"][j]) >> 8) & 255, int(c["meta"][j]) & 15, int(c["isize"][j]), i // 64))
    return out


def _merge(items):
    """items (key, pairs, sum) -> parts sorted by key, equal keys added up"""
    acc = {}
    for k, p, s in items:
        a = acc.setdefault(k, [0, 0])
        a[0] += p; a[1] += s
    return [(k, acc[k][0], acc[k][1]) for k in sorted(acc)]


def as_aggregates(c, split=1, name=None):
    """the same case as a sharded run's rank 0 gets it: every region's pair groups as aggregates of (lo, r, library, flag), a part arriving in
    up to `split` partial aggregates (its pairs dealt round robin), in reverse key order; a region's `first` is its place among them"""
    agg, goff = [], [0]
    for r in range(c["n_regions"]):
        per = {}
        for lo, lib, flag, isz, _ in second_mates(c, r):
            per.setdefault((lo, lib, flag), []).append(isz)
        for (lo, lib, flag) in sorted(per, reverse=True):
            v = per[(lo, lib, flag)]
            for q in range(min(split, len(v))):
                sub = v[q::split]
                agg.append(((lo << 38) | (r << 12) | (lib << 4) | flag, len(sub), sum(sub)))
        goff.append(len(agg))
    d = dict(c)
    d.update(name=name or "%s-agg%d" % (c["name"], split), agg=agg, in_goff=np.asarray(goff, np.uint32), taint=None)
    return d


def region_items(c, r):
    """(part key, pairs, sum, chunk of 64) of what k6_pairs_kernel merges for region r, and whether the chunk route takes it"""
    if c.get("agg") is not None:
        g0, g1 = int(c["in_goff"][r]), int(c["in_goff"][r + 1])
        return [(((k >> 38) << 12) | (k & 0xFFF), p, s, i // 64) for i, (k, p, s) in enumerate(c["agg"][g0:g1])], g1 - g0 > 64
    return [((lo << 12) | (lib << 4) | flag, 1, isz, ch) for lo, lib, flag, isz, ch in second_mates(c, r)], int(c["rec"][r, 3]) > 64


def first_of(c, r):
    return int(c["in_goff"][r]) if c.get("agg") is not None else int(c["rec"][r, 8])


def groups_model(c, slip=None):
    """RegSum per region with the part order, the parts with their kWeakPart marks, out_deg, bad_v, the hub verdict, the route every
    region takes through k6_pairs_kernel, and every part the host would get (as GroupRec words) by region"""
    NR = c["n_regions"]
    mrp = max(c["min_read_pair"], 0)
    rs = np.zeros((NR, RS_WORDS), np.uint32)
    parts = {}
    out_deg = np.zeros(NR, np.int64)
    bad_v = np.zeros(NR, np.uint32)
    hub = np.zeros(NR, bool)
    route, emit, raw = [], {}, {}
    for r in range(NR):
        its, chunked = region_items(c, r)
        items = [(k, p, q) for k, p, q, _ in its]     # in lane order: a wave's lanes take the reads (aggregates) as they come
        big = False
        if not chunked:
            route.append("wave" if items else "none")
        else:
            chunks = sorted({ch for *_, ch in its})
            per_chunk = [_merge([(k, p, q) for k, p, q, ch2 in its if ch2 == ch]) for ch in chunks]
            npx, fits = 0, c.get("agg") is None       # (more than 64 aggregates always go to the host as they are)
            for pc in per_chunk:
                if not fits or npx + len(pc) > 64:
                    fits = False
                    break
                npx += len(pc)
            items = [x for pc in per_chunk for x in pc]   # the stash: every chunk's parts in key order, chunk after chunk
            big = not fits
            route.append("big" if big else ("fits" if items else "none"))
            if big:
                raw[r] = [((k >> 12) << 38 | r << 12 | (k & 0xFFF), p, s) for pc in per_chunk for k, p, s in pc]
                rs[r, 5] = sum(p for pc in per_chunk for _, p, _ in pc)
                rs[r, 3] = sum(p for pc in per_chunk for k, p, _ in pc if k >> 12 == r)
                rs[r, 7] = 1
                bad_v[r] = 1
                hub[r] = True
                for pc in per_chunk:
                    for lo in sorted({k >> 12 for k, _, _ in pc}):
                        if lo < r:
                            out_deg[lo] += 1
                            bad_v[lo] = 1
                continue
        if not items:
            continue
        merged = _merge(items)
        gw = {}
        for k, p, _ in merged:
            gw[k >> 12] = gw.get(k >> 12, 0) + p
        if slip == "weight_per_part":
            strong = {lo: any(p >= mrp for k, p, _ in merged if k >> 12 == lo) for lo in gw}
        else:
            strong = {lo: gw[lo] >= mrp for lo in gw}
        rs[r, 0] = len(merged)
        rs[r, 2] = sum(1 for k, _, _ in merged if k >> 12 == r)
        rs[r, 1] = sum(1 for k, _, _ in merged if k >> 12 == r or strong[k >> 12])
        rs[r, 3] = gw.get(r, 0)
        # the incoming gate-passing groups in the order of the lanes that lead them: the first lane holding the group's smallest part key
        lead = {lo: min(i for i, (k, _, _) in enumerate(items) if k == min(k2 for k2, _, _ in items if k2 >> 12 == lo)) for lo in gw}
        ins = sorted((lo for lo in gw if lo < r and strong[lo]), key=lambda lo: lead[lo])
        rs[r, 4] = len(ins)
        rs[r, 5] = sum(gw.values())
        rs[r, 6] = sum(1 for lo in gw if lo < r and not strong[lo])
        if len(ins) > MAX_IN:
            hub[r] = True
            bad_v[r] = 1
            for lo in ins:
                bad_v[lo] = 1
        else:
            for e, lo in enumerate(ins):
                rank = [i for i, (k, _, _) in enumerate(merged) if k >> 12 == lo]
                rs[r, 8 + e], rs[r, 11 + e], rs[r, 14 + e], rs[r, 17 + e] = lo, gw[lo], rank[0], len(rank)
        for lo in ins:
            out_deg[lo] += 1
        parts[r] = [((k | WEAK) if (k >> 12) < r and not strong[k >> 12] else k, p, s) for k, p, s in merged]
        emit[r] = [((k >> 12) << 38 | r << 12 | (k & 0xFFF), p, s) for k, p, s in merged if (k >> 12) == r or strong[k >> 12]]
    return dict(rs=rs, parts=parts, out_deg=out_deg.astype(np.uint32), bad_v=bad_v, hub=hub, route=route, emit=emit, raw=raw)


def components(c, m):
    """the components of the graph of gate-passing groups: label -> sorted members.  A region is registered when it has a group that could
    ever be consumed (k6_classify_kernel)"""
    NR = c["n_regions"]
    parent = list(range(NR))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    reg = np.zeros(NR, bool)
    for r in range(NR):
        n_in = int(m["rs"][r, 4])
        reg[r] = m["hub"][r] or n_in > 0 or m["out_deg"][r] > 0 or m["rs"][r, 2] > 0
    for r in range(NR):
        for k, _, _ in m["emit"].get(r, []):
            lo = k >> 38
            if lo < r:
                a, b = find(lo), find(r)
                parent[max(a, b)] = min(a, b)
        for k, _, _ in m["raw"].get(r, []):
            lo = k >> 38
            if lo < r:
                a, b = find(lo), find(r)
                parent[max(a, b)] = min(a, b)
    comp = {}
    for r in range(NR):
        if reg[r]:
            comp.setdefault(find(r), []).append(r)
    return comp


def settles_at_once(c, m, members):
    """every region has a gate-passing group with the component's smallest region: whatever order the atomics take, each label is the
    smallest region's after the first round"""
    root = members[0]
    for r in members[1:]:
        if root not in [int(x) for x in m["rs"][r, 8:8 + min(int(m["rs"][r, 4]), MAX_IN)]]:
            return False
    return True


def walker_of(c, m, members):
    """'lane', 'wave' or 'host' for a component whose labels have converged"""
    if any(m["hub"][r] or m["bad_v"][r] for r in members):
        return "host"
    pcount = sum(int(m["rs"][r, 1]) for r in members)
    if min(c["nlibs"], pcount) > min(c["nlibs"], LIB_STRIDE):
        return "host"
    if len(members) <= MAX_MEMBERS:
        return "lane"
    if c["big_walk"] and len(members) <= BIG_MEMBERS:
        return "wave"
    return "host"


# ---------------------------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------------------------

def _reads_per_region():
    """1, 63, 64, 65, 128 and 129 reads in a region, all of them self pairs but the odd one; library bytes 0 and 16; equal part keys in
    different chunks; reads that are no second-observed mate (partner -1, -2, pointing forward)"""
    sizes = (1, 63, 64, 65, 128, 129)
    t = Table(len(sizes) + 2)
    for r, n in enumerate(sizes):
        for i in range(n // 2):
            t.pair(r, r, flag=EMITTED_FLAGS[i % 3], lib=(i % 2) * 16, isize=90 + i)
        if n & 1:
            t.single(r)
    t.rejected_mate(6)
    t.pair(6, 7, n=3)          # (region 6's mates point forward)
    t.pair(6, 6, n=2)
    return make_case("reads-per-region", t, nlibs=17, why_no_stream="library 16 of 17 with reads of one flag each would need seventeen read groups")


def _chunk_parts(total):
    """a region of 130 reads on the chunk route whose chunks hold `total` parts between them -- 63 or 64 in the first chunk and one in the
    second, with a key the first chunk holds too: 64 fit the second merge (equal keys of different chunks become one part), 65 do not (raw
    chunk parts in g_rec, bad_v on the region and on every earlier one it has a group with)"""
    t = Table(70)
    r = 69
    first = total - 1
    for lo in range(first):
        t.pair(lo, r, n=1, isize=80 + lo)
    for _ in range(64 - first):
        t.single(r)
    t.pair(0, r, n=1, isize=200)
    while len(t.reads[r]) < 130:
        t.single(r)
    return make_case("chunk-parts-%d" % total, t, min_read_pair=1, why_no_stream="130 reads of one region with 63 or 64 distinct earlier regions, a chunk boundary between them")


def _gate(mrp):
    """group weights at -r - 1, -r and -r + 1, spread over several (flag, library) parts; a weak group next to a strong one"""
    t = Table(8)
    for hi, w in ((1, mrp - 1), (3, mrp), (5, mrp + 1)):
        for i in range(max(w, 0)):
            t.pair(hi - 1, hi, flag=(FF, RF, LARGE)[i % 3], lib=i % 2, isize=150 + i)
    # region 7: a weak group from 5 next to a strong one from 6
    for i in range(max(mrp - 1, 0)):
        t.pair(5, 7, lib=i % 2)
    t.pair(6, 7, n=max(mrp, 1) + 1, flag=RF)
    t.pair(7, 7, n=max(mrp, 1))
    return make_case("gate-r%d" % mrp, t, nlibs=2, min_read_pair=mrp)


def _shapes(period=101, rounds=2, big_walk=0, name=None):
    """components of 1 .. 5 regions: self group only, chain, star, triangle, complete graph, a chain linked so that labels need more than two
    rounds, 3 and 4 incoming groups"""
    t = Table(40)
    t.pair(0, 0, n=3, flag=SMALL)                                              # 1 region, self group only
    t.pair(2, 3, n=2, flag=RF); t.pair(3, 3, n=2)                               # 2 regions
    t.pair(5, 6, n=2); t.pair(6, 7, n=3, flag=LARGE); t.pair(5, 5, n=2)        # chain of 3
    t.pair(9, 10, n=2); t.pair(9, 11, n=2); t.pair(10, 11, n=2, flag=RF); t.pair(11, 11, n=2)      # triangle: the third group is reached from either side
    t.pair(13, 14, n=2); t.pair(13, 15, n=2); t.pair(13, 16, n=2, flag=CTX)    # star of 4
    for a in range(18, 22):                                                   # complete graph of 4
        for b in range(a + 1, 22):
            t.pair(a, b, n=2, flag=(FF, RF)[(a + b) & 1], lib=(a + b) & 1)
    t.pair(23, 24, n=2); t.pair(24, 25, n=2); t.pair(25, 26, n=2); t.pair(26, 27, n=2)             # chain of 5: the host's, the wave walk's with big_walk
    t.pair(29, 31, n=2); t.pair(30, 32, n=2); t.pair(31, 32, n=2); t.pair(29, 30, n=2, flag=RF)    # 4 regions whose labels meet late
    t.pair(34, 38, n=2); t.pair(35, 38, n=2); t.pair(36, 38, n=2); t.pair(37, 38, n=2)             # 4 incoming groups: a hub
    t.pair(34, 37, n=2); t.pair(35, 37, n=2); t.pair(36, 37, n=2)                                  # 3 incoming groups
    t.pair(39, 39, n=1)                                                        # a self group below the gate
    t.single(39)
    return make_case(name or "shapes-p%d-k%d-b%d" % (period, rounds, big_walk), t, nlibs=2, nkeys=2, period=period, propagation_rounds=rounds, big_walk=big_walk)


def _rejected():
    """calls rejected by num_pairs and by the dominant flag's count that still consume their groups and self groups; a region with fewer
    reads than -r; with -o one whose non-CTX reads are fewer than -r while n is not"""
    t = Table(12)
    # 0 - 1: weight 3 in flags 1 + 1 + 1, and 1's self group of one pair: the dominant flag's count is below -r = 2: rejected; 1 - 2 must not see 1's self group again
    t.pair(0, 1, flag=FF); t.pair(0, 1, flag=RF); t.pair(0, 1, flag=LARGE)
    t.pair(1, 1, n=1, flag=SMALL)
    t.pair(1, 2, n=2, flag=RF)
    # 4 (one read: not stored) - 5: the group's reads are never seen
    t.pair(4, 5, n=1); t.pair(5, 5, n=2); t.single(5)
    # 7 - 8 with -o: region 7 holds three reads, two of them CTX: not stored.  The call sees 8's self group of one pair alone: rejected by num_pairs; 8 - 9 must not see it again
    t.pair(7, 8, n=2, flag=LARGE, flag_first=CTX); t.single(7, flag=LARGE)
    t.pair(8, 8, n=1, flag=SMALL)
    t.pair(8, 9, n=2, flag=RF)
    t.pair(10, 11, n=2, flag=RF); t.pair(10, 10, n=2); t.pair(11, 11, n=2, flag=SMALL)
    return make_case("rejected-calls", t, chr_restricted=1, why_no_stream="with -o a CTX read has no mate in the stream; the table pairs two to hold nonctx < -r <= n")


def _assemble(nlibs, nkeys, asm_plain, maxq=None, name=None):
    """each flag as the dominant one with its position rule, ties between flags, parts over nlibs libraries, nkeys counter keys, a negative
    size, a histogram entry of 0 (lambda at its floor), prefix differences that wrap"""
    flags = (FF, LARGE, SMALL, RF, RR, CTX, MATE_UNMAPPED)
    t = Table(3 * len(flags) + 6, maxq=maxq)
    for i, f in enumerate(flags):
        a = 3 * i
        for l in reversed(range(nlibs)):       # (first seen in descending order: the output's is ascending)
            t.pair(a, a + 1, flag=f, lib=l, isize=20 + 31 * l + i, n=1 + (l + i) % 3)
        t.pair(a, a + 1, flag=flags[(i + 1) % len(flags)], lib=0, n=1)
    a = 3 * len(flags)
    t.pair(a, a + 1, flag=RF, n=2); t.pair(a, a + 1, flag=FF, n=2); t.pair(a, a + 1, flag=CTX, n=2)     # a three-way tie: the lowest flag
    t.pair(a + 3, a + 4, flag=SMALL, lib=nlibs - 1, isize=1, n=3)                                       # a negative size
    t.pair(a + 4, a + 4, flag=LARGE, n=2, isize=5000)
    c = make_case(name or "assemble-l%d-k%d-p%d" % (nlibs, nkeys, asm_plain), t, nlibs=nlibs, nkeys=nkeys, asm_plain=asm_plain,
                  why_no_stream="ARP_RR and MATE_UNMAPPED never reach the region cut from a stream (RR becomes FF, an unmapped mate is filtered): the walk's rules for them are held here")
    hist = c["hist"].copy()
    hist[0, SMALL] = 0
    hist[nlibs - 1, SMALL] = 0
    c["hist"] = hist
    pk = c["pk"].astype(np.int64)
    pk[:, 0] = (pk[:, 0] + 0xFFFFFFF0) & 0xFFFFFFFF
    pk[:, nkeys] = (pk[:, nkeys] + 0xFFFFFFF0) & 0xFFFFFFFF
    c["pk"] = pk.astype(np.uint32)
    return c


def _no_normal_reads():
    t = Table(4)
    t.pair(0, 1, n=3); t.pair(2, 3, n=2, flag=RF)
    return make_case("no-normal-reads", t, nkeys=3, pk=np.full((4, 6), 0xFFFFFFFE, np.uint32))


def _pos_rule():
    """pos[0] + max_readlen - 5 one below, at and one above pos[1] (flag LARGE: pos[0] = end of A, pos[1] = start of B)"""
    t = Table(6, maxq=[45] * 6)
    for i, d in enumerate((39, 40, 41)):
        a, b = 2 * i, 2 * i + 1
        t.end[a] = t.start[a] + 50
        t.start[b] = t.end[a] + d
        t.end[b] = t.start[b] + 60
        t.pair(a, b, flag=LARGE, n=2)
    return make_case("pos-rule", t, last_maxq=45)


def _order_key(n_new, name, last_self=True):
    """one region in a window, n_new in the next, each of these with its self group and up to three incoming groups (one and two for the
    first two), -r 0 so that every call passes the gates: 4 n_new - 3 candidates of one (T, start), all through walk_big"""
    period = 40
    t = Table(period + n_new)
    old = period - 1
    new = list(range(period, period + n_new))
    for i, r in enumerate(new):
        if last_self or r != new[-1]:
            t.pair(r, r, n=1, flag=SMALL)
        los = [old] + new[max(0, i - 2):i]
        for lo in los[:3] if i >= 2 else los:
            t.pair(lo, r, n=1, flag=(FF, RF, LARGE)[(lo + r) % 3])
    return make_case(name, t, min_read_pair=0, period=period, big_walk=1, propagation_rounds=8,
                     why_no_stream="-r 0 and thirty-odd regions with exactly three earlier neighbours each")


def _big(n, incoming=1):
    """n regions in one component for the wave walk, every one with a group from the smallest (the labels settle in the first round, so the
    walk that takes it is the model's to say): a star, or (incoming = 3) also linked to the two regions before it, with a self group"""
    t = Table(n + 2)
    for r in range(2, n + 1):
        if incoming == 3:
            t.pair(r, r, n=2, flag=SMALL)
        for lo in sorted({1} | set(range(max(2, r - incoming + 1), r))):
            t.pair(lo, r, n=2, flag=(FF, RF)[(lo + r) & 1])
    if incoming == 3:
        t.pair(1, 1, n=2, flag=SMALL)
    return make_case("big-%d-in%d" % (n, incoming), t, big_walk=1, propagation_rounds=8, period=1000)


def launch_grids(n_host):
    """(waves of k6_pairs_kernel's grid, walking lanes of k6_walk_kernel's) as launch_k6_pairs and launch_k6_walk size them"""
    return 4 * min((n_host // 8 + 3) // 4 + 1, 16384), 32 * min(n_host // 32 // 4 + 1, 8192)


def _windows():
    """members on both sides of one boundary and over three windows (period 3), a traversal from an earlier window's vertex whose self
    group must not be taken again, max_readlen from the window's last region and from last_maxq when that region lies behind the table"""
    t = Table(11)
    t.pair(1, 1, n=2, flag=SMALL); t.pair(1, 4, n=2); t.pair(4, 7, n=2, flag=RF); t.pair(4, 4, n=2); t.pair(7, 7, n=2)
    t.pair(2, 3, n=2, flag=LARGE); t.pair(2, 2, n=3)
    t.pair(8, 9, n=2); t.pair(9, 10, n=2, flag=RF); t.pair(10, 10, n=2)
    return make_case("windows-p3", t, period=3, last_maxq=77)


def _many_parts():
    """regions with 64 and 65 distinct parts (three earlier regions and the region itself over 16 libraries, and one part more): as
    aggregates, 64 are merged by the wave and 65 go to the host as they are"""
    t = Table(24)
    for r, extra in ((20, 0), (22, 1)):
        for lo in (0, 1, 2, r):
            for lib in range(16):
                t.pair(lo, r, lib=lib, isize=100 + lib + lo)
        if extra:
            t.pair(0, r, lib=0, flag=RF)
    t.pair(5, 5, n=1)                 # one aggregate; the regions between have none
    return make_case("many-parts", t, nlibs=16, min_read_pair=1, why_no_stream="sixteen libraries with one pair each from each of three regions")


def _lib_bytes():
    """library bytes 0 and 255 in a part key (the groups stage alone: no walk has 256 libraries to look up)"""
    t = Table(3)
    t.pair(0, 1, lib=255, n=2); t.pair(0, 1, lib=0, n=1); t.pair(1, 1, lib=255, n=1); t.pair(1, 2, lib=255, flag=CTX, n=2)
    return make_case("lib-bytes", t, nlibs=1, groups_only=True, why_no_stream="a library index of 255 needs a configuration of 256 libraries")


def quotient_search(seed=7):
    """(pairs, insert sizes) of one library whose diff / flag_count, rounded to float32 as the reference rounds it, lands on the other side
    of a half than the quotient in double: found by a seeded search, as tests/region_cases.py finds its verdict pairs"""
    rng = np.random.default_rng(seed)
    mean = np.float32(300.25)
    rc = rng.integers(3, 60, 2_000_000)
    span = rc * 700_000 + rng.integers(0, 900_000, len(rc)) * rc + rng.integers(0, 60, len(rc))   # (quotients near 2^20: float32 keeps eighths there)
    diff = (span.astype(np.float32) - rc.astype(np.float32) * mean).astype(np.float32)
    q32 = (diff / rc.astype(np.float32)).astype(np.float32)
    a = np.trunc(q32.astype(np.float64) + 0.5)
    b = np.trunc(diff.astype(np.float64) / rc + 0.5)
    i = int(np.flatnonzero(a != b)[0])
    n, total = int(rc[i]), int(span[i])
    sizes = [total // n] * n
    sizes[-1] += total - sum(sizes)
    return sizes


def _quotient():
    t = Table(2)
    t.pairs_with(0, 1, quotient_search(), flag=LARGE)
    return make_case("quotient-f32", t)


def table_cases():
    out = [_many_parts(), _lib_bytes(), _quotient(), _reads_per_region(), _chunk_parts(64), _chunk_parts(65), _gate(2), _gate(1), _gate(0), _gate(-1), _rejected(), _no_normal_reads(), _pos_rule(), _windows()]
    out += [_shapes(period=p) for p in (1, 2, 3, 101)]
    out += [_shapes(rounds=k, name="shapes-rounds-%d" % k) for k in (1, 3, 8)]
    out += [_shapes(big_walk=1, rounds=8, name="shapes-big")]
    out += [_assemble(nl, nk, ap) for nl, nk, ap in ((1, 1, 0), (2, 2, 0), (2, 2, 1), (4, 16, 0), (4, 16, 1), (1, 1, 1), (5, 17, 0), (5, 17, 1), (16, 1, 0), (17, 1, 0), (17, 1, 1))]
    out += [_order_key(33, "order-key-128", last_self=False), _order_key(33, "order-key-129"), _big(64), _big(65), _big(64, incoming=3)]
    return out


def with_holes(c, holes):
    """the aggregate form of a case as one rank of a sharded run holds it: the regions in `holes` are another rank's (n == 0 in this rank's
    table; they must be the later region of no group).  Returns the case and the taint bytes the groups stage must leave: both regions of
    every gate-passing group whose earlier region is a hole"""
    d = as_aggregates(c, 1, name=c["name"] + "-holes")
    rec = d["rec"].copy()
    rec[list(holes), 3:6] = 0
    d["rec"] = rec
    m = groups_model(d)
    want = np.zeros(c["n_regions"], np.uint8)
    for r in range(c["n_regions"]):
        assert not (r in holes and m["rs"][r, 5])
        for k, _, _ in m["emit"].get(r, []):
            if k >> 38 in holes:
                want[k >> 38] = want[r] = 1
    d["taint"] = np.zeros(MAX_CAP, np.uint8)
    return d, want


def case_named(name):
    return next(c for c in table_cases() if c["name"] == name)


WALK_SLIPS = ("gate_gt", "neighbours_descending", "rejected_keeps", "self_after_gates", "own_window_maxq", "old_self_again", "stored_from_n", "tie_highest",
              "cn_sum_double", "size_nearest", "size_quotient_double", "no_lambda_floor", "lib_first_seen")
MODEL_SLIPS = ("weight_per_part",)


def differs(a, b):
    """do two tables of the reference differ anywhere a result shows?"""
    if len(a) != len(b):
        return True
    for x, y in zip(a, b):
        for k in ("chr", "pos", "fwd", "rev", "flag", "size", "num_reads", "region", "grp_mask", "start"):
            if x[k] != y[k]:
                return True
        if np.float32(x["af"]).view(np.uint32) != np.float32(y["af"]).view(np.uint32):
            return True
        if [(k, np.float32(v).view(np.uint32)) for k, v in x["cn"]] != [(k, np.float32(v).view(np.uint32)) for k, v in y["cn"]] or x["terms"] != y["terms"]:
            return True
    return False


# ---------------------------------------------------------------------------------------------------------------------------------
# cases a read stream can say: K6's inputs from the stream through the cut and join references of tests/region_cases.py
# ---------------------------------------------------------------------------------------------------------------------------------

STREAM_SETS = [dict(), dict(min_read_pair=1), dict(min_read_pair=3), dict(buffer_size=1), dict(buffer_size=2), dict(buffer_size=3, min_read_pair=1),
               dict(cn_lib=1, print_af=1), dict(chr_tid=0), dict(min_read_pair=0, buffer_size=2)]


def stream_case(seed, optset, n_slots=60):
    """(oracle run, case): fuzzgen's graph case through the oracle; the reads the oracle let pass as anomalous, cut into regions by
    region_cases.cut_reference and joined by region_cases.join_reference; the run constants as the oracle's header computes them"""
    import fuzzgen
    import region_cases as rc
    from helpers import OracleRun, make_opts
    config, streams, targets = fuzzgen.make_graph_case(seed, n_slots=n_slots)
    opts = make_opts(**optset)
    run = OracleRun(config, opts)
    run.set_targets(targets)
    for b, st in enumerate(streams):
        d = dict(st)
        d["lib"] = np.array([run.lib_of_rg(g) for g in st["rg"]], dtype=np.int32)
        run.set_stream(b, d)
    run.run()
    soa = run.merged_soa()
    flag = (run.cls & 15).astype(np.uint32)
    passed = (run.cls & 0x10) != 0
    anom = passed & (flag != NORMAL_FR) & (flag != NORMAL_RF)
    proper = passed & ((soa["flag"] & 0x2) != 0)
    by_lib = bool(opts["cn_lib"])
    nkeys = run.nlibs if by_lib else run.nbams
    key_of = soa["lib"].astype(np.int64) if by_lib else run.lib_i[soa["lib"], 1].astype(np.int64)
    at = np.flatnonzero(anom)
    pk = np.stack([np.cumsum(proper & (key_of == k))[at] for k in range(nkeys)]).astype(np.uint32) if len(at) else np.zeros((nkeys, 0), np.uint32)
    rev = ((soa["flag"][at] & 0x10) != 0).astype(np.uint32)
    cut = rc.cut_case("stream-%d" % seed, soa["tid"][at], soa["pos"][at], soa["qlen"][at], rev=rev, flag=flag[at], nn=np.zeros(len(at), np.uint32), pk=pk,
                      nkeys=nkeys, W=run.W, n_normal=0, min_len=opts["min_len"], lim=opts["seq_coverage_lim"], stream=False)
    res = rc.cut_reference(cut)
    join = rc.join_reference(rc.join_case("stream-%d" % seed, soa["name_id"][at], res["region_of"]))
    assert not join["irregular"]
    lib = soa["lib"][at].astype(np.uint32)
    dens = np.zeros(nkeys, np.float32)
    for k in range(nkeys):
        cnt = int(run.lib_cnt[k]) if by_lib else int(run.bam_cnt[k])
        dens[k] = np.float32(cnt) / np.float32(run.ref_len) if (cnt or not by_lib) else np.float32(0.000001)
    name = "stream-%d-%s" % (seed, "-".join("%s%d" % (k[:3], v) for k, v in sorted(optset.items())) or "defaults")
    c = dict(name=name, n_regions=res["n_regions"], n_reads=len(at), rec=res["rec"], region_of=res["region_of"].astype(np.int32), partner=join["partner"],
             pair_lo=join["pair_lo"], meta=(flag[at] | (rev << 4) | (lib << 8) | (soa["qlen"][at].astype(np.uint32) << 16)).astype(np.uint32),
             isize=np.abs(soa["isize"][at]).astype(np.int32), names=soa["name_id"][at].tolist(), pk=res["pk"], nlibs=run.nlibs, nkeys=nkeys,
             min_read_pair=opts["min_read_pair"], chr_restricted=1 if opts["chr_tid"] >= 0 else 0, period=max(1, opts["buffer_size"] + 1), last_maxq=res["last_maxq"],
             why_no_stream=None, lib_mean=run.lib_f[:, 0].astype(np.float32), key_density=dens, hist=run.hist.astype(np.uint32), covered=int(run.ref_len),
             big_walk=0, asm_plain=0, ins_plain=0, propagation_rounds=2, n_host=None, g_cap=None, use_pair_lo=True, expect={})
    return run, c


def differs_from_oracle(run, ref):
    """the reference's table against the oracle's, field by field as runner.compare takes them; None when they agree"""
    if len(ref) != run.n_svs:
        return "count %d / %d" % (len(ref), run.n_svs)
    oi, od = run.sv_i, run.sv_d
    lb = cb = 0
    for i, x in enumerate(ref):
        got = x["chr"][:1] + x["pos"][:1] + x["fwd"][:1] + x["rev"][:1] + x["chr"][1:] + x["pos"][1:] + x["fwd"][1:] + x["rev"][1:] + [x["flag"], x["size"]]
        if got != oi[i, :10].tolist() or x["num_reads"] != oi[i, 11] or (len(x["terms"]), len(x["cn"])) != (oi[i, 13], oi[i, 14]):
            return "record %d: %r / %r" % (i, got, oi[i].tolist())
        af = np.float32(od[i, 1])
        if np.isnan(af) != np.isnan(x["af"]) or (not np.isnan(af) and af.view(np.uint32) != np.float32(x["af"]).view(np.uint32)):
            return "record %d: allele frequency" % i
        if [(l, k) for l, k, _ in x["terms"]] != [tuple(r) for r in run.sv_lib[lb:lb + len(x["terms"])].tolist()]:
            return "record %d: library list" % i
        if [k for k, _ in x["cn"]] != run.sv_cn_key[cb:cb + len(x["cn"])].tolist() or \
                [int(np.float32(v).view(np.uint32)) for _, v in x["cn"]] != run.sv_cn_val[cb:cb + len(x["cn"])].view(np.uint32).tolist():
            return "record %d: copy numbers" % i
        if "logp" in x:
            if np.isfinite(od[i, 0]) and abs(x["logp"] - od[i, 0]) / max(1.0, abs(od[i, 0])) >= 1e-9:
                return "record %d: logp" % i
            if x["score"] != oi[i, 10] or x["printed"] != oi[i, 12]:
                return "record %d: score" % i
        lb += len(x["terms"]); cb += len(x["cn"])
    return None
