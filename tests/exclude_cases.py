"""Shared by test_exclude.py and test_gpu_exclude.py: the --exclude rule restated in numpy (independent of csrc/bdx_exclude.h:
a union of intervals per sequence, looked up with searchsorted), BED files written the messy way, and fuzz cases written as BAMs."""
import os

import numpy as np


def merge_intervals(intervals):
    """rows of (tid, beg, end), any order, overlapping or touching -> {tid: (begs, ends)} sorted, disjoint, non-touching; empty ones dropped"""
    by_tid = {}
    for t, b, e in sorted((int(t), int(b), int(e)) for t, b, e in intervals):
        if b >= e:
            continue
        cur = by_tid.setdefault(t, [])
        if cur and b <= cur[-1][1]:
            cur[-1][1] = max(cur[-1][1], e)
        else:
            cur.append([b, e])
    return {t: (np.array([x[0] for x in v], np.int64), np.array([x[1] for x in v], np.int64)) for t, v in by_tid.items()}


def n_merged(intervals):
    return sum(len(b) for b, _ in merge_intervals(intervals).values())


def _hit(tid, pos, merged):
    tid = np.asarray(tid, np.int64)
    pos = np.asarray(pos, np.int64)
    out = np.zeros(len(tid), bool)
    for t, (begs, ends) in merged.items():
        m = tid == t
        if not m.any():
            continue
        k = np.searchsorted(begs, pos[m], side="right")   # intervals that begin at or before pos
        inside = np.zeros(int(m.sum()), bool)
        ok = k > 0
        inside[ok] = pos[m][ok] < ends[k[ok] - 1]
        out[m] = inside
    return out


def rule_mask(tid, pos, mtid, mpos, intervals):
    """True where the rule drops the record: its own start in an interval of tid, or its mate's start in an interval of mtid"""
    merged = merge_intervals(intervals)
    return _hit(tid, pos, merged) | _hit(mtid, mpos, merged)


def merge_two_files(rows_a, rows_b):
    """BamMerger's order (io/BamMerger.cpp:40-126) for two files, restated: rows are (tid, pos, flag, payload) in file order; the file
    that emitted last goes on only while its next record is strictly below the other file's on (tid, pos, strand) -- a tie goes to the
    file that has been waiting, and the very first one to file 0"""
    key = lambda r: (r[0], r[1], (r[2] >> 4) & 1)
    out, i, j, last = [], 0, 0, 1
    while i < len(rows_a) and j < len(rows_b):
        ka, kb = key(rows_a[i]), key(rows_b[j])
        take_a = ka < kb if last == 0 else not kb < ka
        if take_a:
            out.append(rows_a[i][3]); i += 1; last = 0
        else:
            out.append(rows_b[j][3]); j += 1; last = 1
    out += [r[3] for r in rows_a[i:]] + [r[3] for r in rows_b[j:]]
    return out


def masked_dump(plain_rows, intervals):
    """What bdx-dump-reads must print for the masked files, from its unmasked rows (text lines of twelve tab-separated columns): the rows
    the rule marks removed PER FILE, the files merged again.  Removing rows from the merged dump itself is the same thing except where
    the two files tie on (tid, pos, strand): who wins a tie depends on which file emitted last, hence on what was removed in front of it.
    Returns (expected rows, marked rows)"""
    f = np.array([[int(x) for x in l.split("\t")[:10]] for l in plain_rows], dtype=np.int64).reshape(-1, 10)
    drop = rule_mask(f[:, 0], f[:, 1], f[:, 2], f[:, 3], intervals)
    files = sorted(set(f[:, 9].tolist()))
    assert len(files) <= 2
    per = [[(int(f[i, 0]), int(f[i, 1]), int(f[i, 5]), plain_rows[i]) for i in range(len(plain_rows)) if f[i, 9] == b and not drop[i]] for b in (0, 1)]
    return merge_two_files(per[0], per[1]), drop


def write_bed(path, intervals, names, rng=None, extra_lines=()):
    """intervals (tid, beg, end) as BED lines, shuffled when rng is given, fields separated by tabs or (every third line) spaces"""
    lines = ["%s\t%d\t%d" % (names[t], b, e) if i % 3 else "%s %d  %d extra_field" % (names[t], b, e) for i, (t, b, e) in enumerate(intervals)]
    lines += list(extra_lines)
    if rng is not None:
        lines = [lines[i] for i in rng.permutation(len(lines))]
    with open(path, "w") as f:
        f.write("".join(l + "\n" for l in lines))


def write_case(tmp, streams, targets, rng, index=False, files=("a.bam", "b.bam")):
    """the streams of fuzzgen.make_case as BAM files (test_gpu_cli_fuzz.write_case restated): bdqual through AM or MAPQ, and secondary /
    supplementary copies the reader filter drops"""
    from breakdancer_amd.bamwrite import write_bam_records
    for b, (fn, st) in enumerate(zip(files, streams)):
        recs = []
        for i in range(len(st["tid"])):
            bq, q = int(st["bdqual"][i]), int(st["bdqual"][i])
            am = None
            if rng.random() < 0.5:
                am, q = bq, int(rng.integers(0, 61))
            recs.append(dict(tid=st["tid"][i], pos=st["pos"][i], mtid=st["mtid"][i], mpos=st["mpos"][i], isize=st["isize"][i],
                             flag=st["flag"][i], qlen=st["qlen"][i], mapq=q, am=am, rg=st["rg"][i], name="read%d" % int(st["name_id"][i])))
            if rng.random() < 0.02:
                extra = dict(recs[-1])
                extra["flag"] = int(extra["flag"]) | (0x100 if rng.random() < 0.5 else 0x800)
                recs.append(extra)
        write_bam_records(os.path.join(tmp, fn), recs, targets, rgs=("rg1", "rg2", "rg3"), seed=b, index=index)


def without(stream, drop):
    """a make_case stream with the marked records removed"""
    keep = ~np.asarray(drop, bool)
    out = {}
    for k, v in stream.items():
        out[k] = [x for x, kk in zip(v, keep) if kk] if isinstance(v, list) else np.asarray(v)[keep]
    return out


def excluded_count(stderr_text):
    """R, M, K of the BDX_TIMING line"""
    import re
    m = re.findall(r"excluded (\d+) records in (\d+) intervals \((\d+) BED lines on unknown sequences ignored\)", stderr_text)
    assert len(m) == 1, stderr_text
    return tuple(int(x) for x in m[0])


def table_rows(text):
    return [l for l in text.splitlines() if l and not l.startswith("#")]


def mask_from_table(text, targets, rng):
    """the CLI tests' mask, built from a printed table: +-400 bases around Pos1 of every third row, one interval that holds no read
    (c3:0-500), and one overlapping duplicate; returned in shuffled order"""
    iv = []
    for l in table_rows(text)[::3]:
        f = l.split("\t")
        p = int(f[1])
        iv.append((targets.index(f[0]), max(0, p - 400), p + 400))
    iv.append((targets.index("c3"), 0, 500))
    if len(iv) > 1:
        t, b, e = iv[0]
        iv.append((t, b + 100, e + 100))
    return [iv[i] for i in rng.permutation(len(iv))]


def mask_streams(streams, intervals):
    """(the make_case streams without the records the rule marks, the number of marked records per stream)"""
    out, removed = [], []
    for st in streams:
        drop = rule_mask(st["tid"], st["pos"], st["mtid"], st["mpos"], intervals)
        out.append(without(st, drop))
        removed.append(int(drop.sum()))
    return out, removed


def rewrite_bam_without(src, dst, intervals):
    """the BAM `src` written again as `dst` without the records the rule marks: every other record byte for byte (names, bases,
    qualities and tags included), blocked into fresh BGZF members.  Returns the number of records left out."""
    import gzip
    import struct
    from breakdancer_amd.bamwrite import _EOF, _bgzf_block
    d = gzip.decompress(open(src, "rb").read())
    l_text, = struct.unpack_from("<i", d, 4)
    o = 8 + l_text
    n_ref, = struct.unpack_from("<i", d, o)
    o += 4
    for _ in range(n_ref):
        l, = struct.unpack_from("<i", d, o)
        o += 8 + l
    starts, cols = [], []
    while o < len(d):
        bs, = struct.unpack_from("<i", d, o)
        tid, pos = struct.unpack_from("<ii", d, o + 4)
        mtid, mpos = struct.unpack_from("<ii", d, o + 24)
        starts.append((o, o + 4 + bs))
        cols.append((tid, pos, mtid, mpos))
        o += 4 + bs
    c = np.array(cols, dtype=np.int64).reshape(-1, 4)
    drop = rule_mask(c[:, 0], c[:, 1], c[:, 2], c[:, 3], intervals)
    raw = d[:starts[0][0] if starts else len(d)] + b"".join(d[a:b] for (a, b), x in zip(starts, drop) if not x)
    with open(dst, "wb") as f:
        for i in range(0, len(raw), 65280):
            f.write(_bgzf_block(raw[i:i + 65280], 1))
        f.write(_EOF)
    return int(drop.sum())
