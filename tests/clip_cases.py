"""What the --clip tests share: the clip word and the pile rule restated in plain Python / numpy (include/bdx.h: bdx_clip_word,
bdx_site_clip_peaks), a plain parse of a BAM's CIGARs, and the CIGAR table both test files mix into their inputs.  Nothing here is imported
by the product, and nothing here shares code with it."""
import gzip
import os
import struct

import numpy as np

OPS = "MIDNSHP=X"
SPAN_MAX = 4096          # BDX_CLIP_SPAN_MAX
WINDOW_MAX = 1023        # BDX_CLIP_WINDOW_MAX


def cigar_of(text):
    """'5S85M' -> [(5, 'S'), (85, 'M')]"""
    out, num = [], ""
    for ch in text:
        if ch.isdigit():
            num += ch
        else:
            out.append((int(num), ch))
            num = ""
    assert num == ""
    return out


def word_of(cigar, l_seq, flag=0):
    """the clip word by the rule's words: cigar a list of (length, letter)"""
    if not cigar or (flag & 0x4):
        return 0
    if len(cigar) == 2 and cigar[0] == (l_seq, "S") and cigar[1][1] == "N":
        return 0                                                     # htslib's long-CIGAR placeholder
    clip = [op in "SH" for _, op in cigar]
    lead = 0
    while lead < len(cigar) and clip[lead]:
        lead += 1
    left = sum(n for n, _ in cigar[:lead])
    trail = 0
    while trail < len(cigar) - lead and clip[len(cigar) - 1 - trail]:
        trail += 1
    right = sum(n for n, _ in cigar[len(cigar) - trail:]) if trail else 0
    span = sum(n for n, op in cigar if op in "MDN=X")
    if span > 65535:
        span, right = 65535, 0
    return min(left, 255) | (min(right, 255) << 8) | (span << 16)


# the table of the issue: (CIGAR, l_seq, flag, left, right, span) -- the expectation written out by hand, not computed
TABLE = [
    ("", 90, 0, 0, 0, 0),
    ("90M", 90, 0, 0, 0, 90),
    ("5S85M", 90, 0, 5, 0, 85),
    ("85M5S", 90, 0, 0, 5, 85),
    ("3H2S80M5S", 87, 0, 5, 5, 80),
    ("300S90M", 390, 0, 255, 0, 90),
    ("90M300S", 390, 0, 0, 255, 90),
    ("90S", 90, 0, 90, 0, 0),
    ("40H50S", 50, 0, 90, 0, 0),
    ("10S80M10S", 100, 0x4, 0, 0, 0),
    ("10S80M10S", 100, 0, 10, 10, 80),
    ("40M5I45M", 90, 0, 0, 0, 85),
    ("40M10D40M2N8M", 88, 0, 0, 0, 100),
    ("10S30=2X28=20S", 90, 0, 10, 20, 60),
    ("10S40M5P40M10H", 90, 0, 10, 10, 80),
    ("5S65534M7S", 65546, 0, 5, 7, 65534),
    ("5S65535M7S", 65547, 0, 5, 7, 65535),
    ("5S65536M7S", 65548, 0, 5, 0, 65535),
    ("5S60000M10000N60000M7S", 120012, 0, 5, 0, 65535),
    ("90S4000N", 90, 0, 0, 0, 0),                                    # the long-CIGAR placeholder ...
    ("89S4000N", 90, 0, 89, 0, 4000),                                # ... and what only looks like it
    ("90S4000M", 90, 0, 90, 0, 4000),
]


def table_word(row):
    return row[3] | (row[4] << 8) | (row[5] << 16)


def parse_bam_cigars(path):
    """every record of a BAM, in file order: dict of tid, pos, flag, l_seq (numpy) and cigar (list of lists of (length, letter))"""
    d = gzip.decompress(open(path, "rb").read())
    assert d[:4] == b"BAM\1"
    l_text, = struct.unpack_from("<i", d, 4)
    o = 8 + l_text
    n_ref, = struct.unpack_from("<i", d, o)
    o += 4
    for _ in range(n_ref):
        l, = struct.unpack_from("<i", d, o)
        o += 8 + l
    tid, pos, flag, l_seq, cigars = [], [], [], [], []
    while o < len(d):
        bs, = struct.unpack_from("<i", d, o)
        t, p, l_rn, _mq, _bin, n_cig, fl, ls = struct.unpack_from("<iiBBHHHi", d, o + 4)
        cg = struct.unpack_from("<%dI" % n_cig, d, o + 36 + l_rn)
        tid.append(t); pos.append(p); flag.append(fl); l_seq.append(ls)
        cigars.append([(w >> 4, OPS[w & 15]) for w in cg])
        o += 4 + bs
    return dict(tid=np.array(tid, np.int32), pos=np.array(pos, np.int32), flag=np.array(flag, np.uint16), l_seq=np.array(l_seq, np.int64),
                cigar=cigars)


def words_of_bam(recs):
    return np.array([word_of(c, int(l), int(f)) for c, l, f in zip(recs["cigar"], recs["l_seq"], recs["flag"])], dtype=np.uint32)


# ---- the pile rule, brute force over all records: no window walk, no histogram, a sort instead ----
PEAKS_DTYPE = np.dtype([("n_left", "<u4"), ("n_right", "<u4"), ("pos_left", "<i4"), ("pos_right", "<i4"), ("peak_left", "<u4"), ("peak_right", "<u4")])


def observations(tid, pos, cls, clip, min_clip):
    """(tid, X) of the left and of the right observations the store gives, whatever the query"""
    t, s = np.asarray(tid).astype(np.int64), np.asarray(pos).astype(np.int64)
    w = np.asarray(clip).astype(np.int64)
    ok = (np.asarray(cls) & 0x10) != 0
    left, right, span = w & 255, (w >> 8) & 255, w >> 16
    xl, xr = s + 1, s + span
    rep = lambda x: (x >= 1) & (x <= 2**31 - 1)
    ml = ok & (left >= min_clip) & rep(xl)
    mr = ok & (right >= min_clip) & (span >= 1) & (span <= SPAN_MAX) & rep(xr)
    return (t[ml], xl[ml]), (t[mr], xr[mr])


def pile(t, x, T, P, window):
    """(n, pos, peak) of one side"""
    m = (t == T) & (np.abs(x - P) <= window)
    if not m.any():
        return 0, 0, 0
    vals, counts = np.unique(x[m], return_counts=True)
    best = sorted(zip((-counts).tolist(), np.abs(vals - P).tolist(), vals.tolist()))[0]
    return int(m.sum()), int(best[2]), int(-best[0])


def expected_peaks(tid, pos, cls, clip, queries, window, min_clip):
    """queries: (T, P) per query"""
    (tl, xl), (tr, xr) = observations(tid, pos, cls, clip, min_clip)
    out = np.zeros(len(queries), dtype=PEAKS_DTYPE)
    for i, (T, P) in enumerate(queries):
        nl, pl, kl = pile(tl, xl, int(T), int(P), int(window))
        nr, pr, kr = pile(tr, xr, int(T), int(P), int(window))
        out[i] = (nl, nr, pl, pr, kl, kr)
    return out


# ---- stores of pushed records, and a synthetic BAM whose records carry the CIGAR table ----
TOP = 2**31 - 1


def word(left=0, right=0, span=100):
    return left | (right << 8) | (span << 16)


class Store:
    """records given one by one, sorted by (tid, pos) when built"""

    def __init__(self):
        self.rows = []

    def add(self, tid, pos, w, kind="ok", times=1):
        for _ in range(times):
            self.rows.append((tid, pos, w, kind))
        return self

    def left(self, tid, X, clip=20, **kw):
        return self.add(tid, X - 1, word(left=clip), **kw)

    def right(self, tid, X, clip=20, span=100, **kw):
        return self.add(tid, X - span, word(right=clip, span=span), **kw)

    def build(self):
        rows = sorted(self.rows, key=lambda r: (r[0], r[1]))     # (stable: equal positions keep the order they were given in)
        n = len(rows)
        tid = np.array([r[0] for r in rows], np.int32).reshape(n)
        pos = np.array([r[1] for r in rows], np.int64).reshape(n)
        assert n == 0 or (pos.min() >= 0 and pos.max() <= TOP)
        high = pos > TOP - 1000                                  # the mate in front where there is no room behind
        kind = [r[3] for r in rows]
        flag = np.where(high, 0x1 | 0x2 | 0x10 | 0x80, 0x1 | 0x2 | 0x20 | 0x40).astype(np.uint16)
        flag |= np.array([0x400 if k == "dup" else 0 for k in kind], np.uint16).reshape(n)
        soa = dict(tid=tid, pos=pos.astype(np.int32), mtid=tid.copy(), mpos=np.where(high, pos - 300, pos + 300).astype(np.int32),
                   isize=np.where(high, -400, 400).astype(np.int32), flag=flag, qlen=np.full(n, 100, np.uint16),
                   mapq=np.array([10 if k == "lowq" else 60 for k in kind], np.uint8).reshape(n), lib=np.zeros(n, np.uint8), bam=np.zeros(n, np.uint8),
                   name_key=(np.arange(1, n + 1, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)))
        clip = np.array([r[2] for r in rows], np.uint32).reshape(n)
        return soa, clip, kind


READLEN = 100
SYN_TARGETS = ["c0", "c1", "c2"]


def synthetic_bam(path, n=3000, seed=4, index=False, parity=None):
    """(the records' columns, their CIGARs, the words the rule gives them) of a position-sorted BAM whose records carry the table's CIGARs
    (the placeholder with this file's read length), the fixture's commonest shapes and random clips, a few of them unmapped"""
    from breakdancer_amd.bamwrite import write_bam, write_bam_records
    rng = np.random.default_rng(seed)
    texts = [r[0] for r in TABLE if r[0]] + ["%dS4000N" % READLEN, "100M", "100M", "30S70M", "70M30S", "12S76M12S"]
    st = Store()
    for i in range(n):
        pos = int(rng.integers(0, 200_000)) if parity is None else 2 * int(rng.integers(0, 100_000)) + parity   # (parity: two files share no position)
        st.add(int(rng.integers(0, 3)), pos, 0, kind="ok" if rng.random() < 0.9 else "lowq")
    soa, _, kind = st.build()
    cigars = []
    for i in range(n):
        if rng.random() < 0.5:
            cigars.append(texts[int(rng.integers(0, len(texts)))])
        else:
            a, b = int(rng.choice([0, 0, 3, 10, 25])), int(rng.choice([0, 0, 3, 10, 25]))
            cigars.append(("%dS" % a if a else "") + "%dM" % (READLEN - a - b) + ("%dS" % b if b else ""))
    soa["flag"] = soa["flag"] | np.where(rng.random(n) < 0.02, 0x4, 0).astype(np.uint16)
    soa["qlen"] = np.full(n, READLEN, np.uint16)
    if index:   # (the writer of records one by one: it has the index)
        recs = [dict(tid=int(soa["tid"][i]), pos=int(soa["pos"][i]), mtid=int(soa["mtid"][i]), mpos=int(soa["mpos"][i]), isize=int(soa["isize"][i]),
                     flag=int(soa["flag"][i]), qlen=READLEN, mapq=int(soa["mapq"][i]), name="r%07d" % i, rg="rg1", cigar=cigars[i]) for i in range(n)]
        write_bam_records(path, recs, SYN_TARGETS, rgs=("rg1",), index=True)
    else:
        write_bam(path, soa, SYN_TARGETS, rg="rg1", readlen=READLEN, cigars=cigars, threads=2)
    words = np.array([word_of(cigar_of(c), READLEN, int(f)) for c, f in zip(cigars, soa["flag"])], dtype=np.uint32)
    return soa, cigars, words
