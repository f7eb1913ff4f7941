"""Shared by test_markdup.py and test_gpu_markdup.py: the duplicate-marking rule of include/bdx.h restated in numpy (one sort and a scan
over group boundaries -- independent of csrc/kd_markdup.hip, which compares neighbours and hashes), duplicates planted in fuzz cases, and
BAMs written again with 0x400 set on the marked records."""
import re

import numpy as np

from namehash import hash_name

NOT_CANDIDATE = 0x4 | 0x8 | 0x100 | 0x400 | 0x800


def _groups(tid, pos, mtid, mpos, flag, lib, name_key):
    """(order, first): the candidates' indices sorted by (run, K, name_key, index), and a mask over that order that is True where a
    group begins"""
    tid, pos, mtid, mpos = (np.asarray(a, np.int64) for a in (tid, pos, mtid, mpos))
    flag = np.asarray(flag, np.int64)
    lib = np.asarray(lib, np.int64)
    key = np.asarray(name_key, np.uint64)
    n = len(tid)
    if n == 0:
        return np.zeros(0, np.int64), np.zeros(0, bool)
    new_run = np.ones(n, bool)
    new_run[1:] = (tid[1:] != tid[:-1]) | (pos[1:] != pos[:-1])
    run = np.cumsum(new_run)   # runs: maximal stretches of CONSECUTIVE records with equal (tid, pos)
    cand = ((flag & 0x1) != 0) & ((flag & NOT_CANDIDATE) == 0) & (tid >= 0) & (mtid >= 0)
    idx = np.nonzero(cand)[0]
    k = [run[idx], lib[idx], flag[idx] & 0x10, mtid[idx], mpos[idx], flag[idx] & 0x20, flag[idx] & 0x40]   # (tid, pos) are the run's
    order = np.lexsort([idx, key[idx]] + k[::-1])   # (last key first: run, ..., name_key, index)
    first = np.ones(len(idx), bool)
    if len(idx) > 1:
        same = np.ones(len(idx) - 1, bool)
        for c in k:
            s = c[order]
            same &= s[1:] == s[:-1]
        first[1:] = ~same
    return idx[order], first


def rule_marks(tid, pos, mtid, mpos, flag, lib, name_key):
    """True where the rule gives the record 0x400: every candidate of a group of two or more except the one with the smallest
    (name_key, index)"""
    order, first = _groups(tid, pos, mtid, mpos, flag, lib, name_key)
    out = np.zeros(len(np.asarray(tid)), bool)
    out[order[~first]] = True
    return out


def rule_group_count(tid, pos, mtid, mpos, flag, lib, name_key):
    """groups of two or more"""
    order, first = _groups(tid, pos, mtid, mpos, flag, lib, name_key)
    if len(order) == 0:
        return 0
    sizes = np.diff(np.append(np.nonzero(first)[0], len(order)))
    return int((sizes >= 2).sum())


def sort_stream(st):
    """a make_case stream sorted again by (tid, pos), stable"""
    order = np.lexsort((np.asarray(st["pos"]), np.asarray(st["tid"])))
    return {k: ([v[i] for i in order] if isinstance(v, list) else np.asarray(v)[order]) for k, v in st.items()}


def plant_duplicates(streams, seed, anomalous_share=0.35, other_share=0.05):
    """fuzzgen.make_case streams with PCR copies: both mates of chosen pairs are written again, one to three times, under new names (every
    record of the pair lives in one stream).  Pairs that are not flagged proper -- the anomalous ones are among them -- are chosen more
    often, so that the copies inflate calls.  Returns the new streams, sorted by (tid, pos)."""
    rng = np.random.default_rng(55_000 + seed)
    next_name = int(max(int(np.asarray(s["name_id"]).max()) for s in streams if len(s["name_id"]))) + 1
    out = []
    for st in streams:
        ids = np.asarray(st["name_id"])
        flag = np.asarray(st["flag"])
        names = np.unique(ids)
        proper = {int(x) for x in ids[(flag & 0x2) != 0]}
        extra = []
        for nm in names:
            p = other_share if int(nm) in proper else anomalous_share
            if rng.random() >= p:
                continue
            rows = np.nonzero(ids == nm)[0]
            for _ in range(int(rng.integers(1, 4))):
                extra.append((rows, next_name))
                next_name += 1
        d = {k: (list(v) if isinstance(v, list) else np.asarray(v).copy()) for k, v in st.items()}
        for rows, nm in extra:
            for k in d:
                if k == "name_id":
                    d[k] = np.append(d[k], np.full(len(rows), nm, np.uint64))
                elif isinstance(d[k], list):
                    d[k] = d[k] + [d[k][i] for i in rows]
                else:
                    d[k] = np.append(d[k], d[k][rows])
        out.append(sort_stream(d))
    return out


def cli_name_keys(st):
    """the name keys the readers give the records that exclude_cases.write_case writes for a stream"""
    return np.array([hash_name(b"read%d" % int(x)) for x in st["name_id"]], dtype=np.uint64)


def stream_marks(streams, libs, keys=None):
    """The rule over the merged store of several position-sorted streams, per stream.  libs[b]: library index of every record of stream
    b; keys[b]: its name keys (default: name_id).  The store's order among records of one (tid, pos) does not matter as long as no two
    records of a group share a name key: the streams are concatenated and sorted stably."""
    cat = lambda k: np.concatenate([np.asarray(s[k]) for s in streams])
    tid, pos = cat("tid"), cat("pos")
    key = np.concatenate([np.asarray(k, np.uint64) for k in (keys if keys is not None else [s["name_id"] for s in streams])])
    lib = np.concatenate([np.asarray(l) for l in libs])
    order = np.lexsort((pos, tid))
    m = rule_marks(tid[order], pos[order], cat("mtid")[order], cat("mpos")[order], cat("flag")[order], lib[order], key[order])
    g = rule_group_count(tid[order], pos[order], cat("mtid")[order], cat("mpos")[order], cat("flag")[order], lib[order], key[order])
    back = np.zeros(len(tid), bool)
    back[order] = m
    cuts = np.cumsum([len(s["tid"]) for s in streams])[:-1]
    return np.split(back, cuts), g


def with_marks(stream, marks):
    """a stream whose marked records carry 0x400"""
    d = dict(stream)
    d["flag"] = np.where(marks, np.asarray(stream["flag"]) | 0x400, np.asarray(stream["flag"])).astype(np.uint16)
    return d


def marked_count(stderr_text):
    """D, G of the BDX_TIMING line"""
    m = re.findall(r"marked (\d+) duplicate records in (\d+) groups", stderr_text)
    assert len(m) == 1, stderr_text
    return int(m[0][0]), int(m[0][1])


def rewrite_bam_marked(src, dst, marks):
    """The BAM `src` written again as `dst`, every record byte for byte (names, bases, qualities and tags included) except that 0x400 is
    set in the flag of the marked ones, blocked into fresh BGZF members.  marks: one entry per record of the file that passes the reader
    filter (primary, placed), in file order -- the file's share of the store.  Returns the number of flags changed."""
    import gzip
    import struct
    from breakdancer_amd.bamwrite import _EOF, _bgzf_block
    d = bytearray(gzip.decompress(open(src, "rb").read()))
    l_text, = struct.unpack_from("<i", d, 4)
    o = 8 + l_text
    n_ref, = struct.unpack_from("<i", d, o)
    o += 4
    for _ in range(n_ref):
        l, = struct.unpack_from("<i", d, o)
        o += 8 + l
    marks = np.asarray(marks, bool)
    k = changed = 0
    while o < len(d):
        bs, = struct.unpack_from("<i", d, o)
        tid, = struct.unpack_from("<i", d, o + 4)
        flag, = struct.unpack_from("<H", d, o + 18)   # (flag_nc: the flag is its upper half)
        if tid >= 0 and not flag & 0x900:
            if marks[k]:
                struct.pack_into("<H", d, o + 18, flag | 0x400)
                changed += 1
            k += 1
        o += 4 + bs
    assert k == len(marks), (k, len(marks))
    raw = bytes(d)
    with open(dst, "wb") as f:
        for i in range(0, len(raw), 65280):
            f.write(_bgzf_block(raw[i:i + 65280], 1))
        f.write(_EOF)
    return changed
