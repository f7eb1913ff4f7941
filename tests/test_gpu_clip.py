"""GPU tests of --clip: the piles of clipped reads around one end of given sites (bdx_site_clip_peaks, KP) against a numpy restatement of
the rule in include/bdx.h, and the clip column (bdx_use_clips / bdx_put_clips / bdx_get_clips) beside the store.

The rule pinned here: a query is (site, end); (T, P) the asked end.  A record with clip word w gives a LEFT observation at X = pos + 1 when
left(w) >= min_clip and a RIGHT one at X = pos + span(w) when right(w) >= min_clip and 1 <= span <= 4096; one counts when the record passes
(class byte 0x10), tid == T and |X - P| <= window.  Per side: n the observations, pos the X most of them share, peak that number; ties go to
the smaller |X - P|, then the smaller X; n == 0: all 0.

The restatement (clip_cases.py) is brute force over all records -- no window, no search, no histogram -- so it shares no logic with the
kernel.  The class bytes are the run's own (bdx_get_read_class).  Every comparison is exact.

The stores are pushed records, each a mate of a pair whose other mate is not in the store: K1 judges a record by what it carries itself,
so most pass, those with 0x400 or a low quality do not, and the tests check on the class bytes that both kinds are there."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from clip_cases import PEAKS_DTYPE, READLEN, SPAN_MAX, SYN_TARGETS, TOP, WINDOW_MAX, Store, expected_peaks, observations, synthetic_bam, word
from helpers import context

pytestmark = pytest.mark.gpu
MASK = 1 << 2           # a valid flag mask: the rule does not look at it


def run_store(soa, clip, batches=1):
    bd = context().use_clips()
    n = len(clip)
    if n:
        cut = [n * k // batches for k in range(batches + 1)]
        for lo, hi in zip(cut, cut[1:]):
            bd.push_reads({k: v[lo:hi] for k, v in soa.items()}, clip=clip[lo:hi])
    bd.run()
    cls = bd.read_class() if n else np.zeros(0, np.uint8)
    return bd, cls


def check_classes(cls, kind):
    """the run let the ordinary records pass and turned the marked ones away: both kinds are really there"""
    ok = (cls & 0x10) != 0
    kind = np.array(kind)
    assert ok[kind == "ok"].all() and not ok[kind != "ok"].any()


def ask(bd, queries, window, min_clip):
    """queries (T, P): each as end 1 of a site of its own"""
    sites = [(T, P, T, P, MASK) for T, P in queries]
    return bd.site_clip_peaks(sites, [1] * len(sites), window, min_clip)


def same(got, exp, msg=""):
    assert got.dtype == PEAKS_DTYPE and got.shape == exp.shape
    for k in PEAKS_DTYPE.names:
        np.testing.assert_array_equal(got[k], exp[k], err_msg="%s %s" % (msg, k))


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. KP against the restatement
# ---------------------------------------------------------------------------------------------------------------------------------
EDGE_WINDOWS = (0, 1, 7, 100, WINDOW_MAX)
B = {w: 100_000 + 20_000 * i for i, w in enumerate(EDGE_WINDOWS)}    # one P per window on sequence 1, far from each other
SPANP = 300_000                                                       # the span scenario's P
TIES = (400_000, 420_000)
STEPS = {63: 500_000, 64: 520_000, 65: 540_000, 129: 560_000}
PILE = 600_000
MINP = 620_000
MIN_CLIP = 12


def edge_store():
    st = Store()
    for w, P in B.items():
        # observations at P - w and P + w (in) and one beyond either way (out), both sides; the neighbouring sequences hold the same
        # piles, larger, and records that do not pass stand on the piles
        for tid, times in ((0, 5), (1, 1), (2, 7)):
            st.left(tid, P - w, times=2 * times).left(tid, P + w, times=times).left(tid, P - w - 1, times=3 * times).left(tid, P + w + 1, times=4 * times)
            st.right(tid, P - w, times=times).right(tid, P + w, times=3 * times).right(tid, P - w - 1, times=4 * times).right(tid, P + w + 1, times=5 * times)
        st.left(1, P + w, kind="dup", times=4).left(1, P - w, kind="lowq", times=4).right(1, P - w, kind="dup", times=6).right(1, P + w, kind="lowq")
    # the longest span: in at 4096 -- with w = WINDOW_MAX its read starts at the first position the walk visits --, out at 4097; and a read
    # of span 4096 one base in front of the walk's first position, whose X is one in front of the window
    for w in (0, WINDOW_MAX):
        P = SPANP + 10_000 * (w > 0)
        st.right(1, P - w, span=SPAN_MAX, times=2).add(1, P - w - SPAN_MAX, word(right=20, span=SPAN_MAX + 1), times=3)
        st.right(1, P - w - 1, span=SPAN_MAX, times=4).right(1, P + w, span=1).right(1, P + w, span=0, times=5)
    # ties: equal piles at P - 3 and P + 3 (the smaller X), at P - 2 and P + 1 (the nearer); a smaller pile, nearer or at P itself, wins neither
    for side in (st.left, st.right):
        side(1, TIES[0] - 3, times=3); side(1, TIES[0] + 3, times=3); side(1, TIES[0] + 5, times=2)
        side(1, TIES[1] - 2, times=3); side(1, TIES[1] + 1, times=3); side(1, TIES[1], times=2)
    # 63, 64, 65 and 129 records in the walk's window: the walk's steps
    rng = np.random.default_rng(5)
    for k, P in STEPS.items():
        for j in range(k):
            x = P - 400 + int(rng.integers(0, 800))
            (st.left if j % 2 else st.right)(1, x, clip=int(rng.integers(MIN_CLIP, 60)))
    st.left(1, PILE, times=300).right(1, PILE + 2, times=299).left(1, PILE + 1, times=7)
    # the clip length: min_clip is in, one less is out; 255 stands for anything longer
    st.left(1, MINP, clip=MIN_CLIP, times=2).left(1, MINP + 1, clip=MIN_CLIP - 1, times=3).right(1, MINP + 2, clip=MIN_CLIP, times=2)
    st.right(1, MINP + 3, clip=MIN_CLIP - 1, times=3).left(1, MINP + 4, clip=255).right(1, MINP + 5, clip=255)
    st.add(1, MINP + 10, word(left=30, right=30, span=50))          # one record, both observations
    # P = 1: the first base of a sequence
    st.left(1, 1, times=2).left(1, 2).right(1, 1, span=1, times=3).right(1, 3, span=2)
    return st.build()


def edge_queries(w):
    q = [(1, B[w]), (0, B[w]), (2, B[w]), (3, B[w]), (1, B[w] + 1), (1, B[w] - 1), (1, 50_000)]     # (3: no such records; 50,000: a window holding none)
    q += [(1, SPANP), (1, SPANP + 10_000), (1, TIES[0]), (1, TIES[1])] + [(1, P) for P in STEPS.values()]
    q += [(1, PILE), (1, PILE + 1), (1, MINP), (1, MINP + 5), (1, 1), (1, 2), (1, TOP)]
    return q


@pytest.fixture(scope="module")
def edge():
    soa, clip, kind = edge_store()
    bd, cls = run_store(soa, clip)
    check_classes(cls, kind)
    yield bd, soa, cls, clip
    bd.close()


def test_clip_peaks_equal_the_restatement_on_the_edges(edge):
    bd, soa, cls, clip = edge
    for w in EDGE_WINDOWS:
        q = edge_queries(w)
        for m in (MIN_CLIP, 1, 255):
            exp = expected_peaks(soa["tid"], soa["pos"], cls, clip, q, w, m)
            same(ask(bd, q, w, m), exp, "window=%d min=%d" % (w, m))
        exp = expected_peaks(soa["tid"], soa["pos"], cls, clip, q, w, MIN_CLIP)
        # what the scenarios are there for, on the restatement: the piles at the window's edges count, those beyond do not
        at = exp[0]
        assert (at["n_left"], at["n_right"]) == (3, 4), (w, at)
        if w:
            assert (at["pos_left"], at["peak_left"], at["pos_right"], at["peak_right"]) == (B[w] - w, 2, B[w] + w, 3)
    big, none = WINDOW_MAX, 0
    e0 = expected_peaks(soa["tid"], soa["pos"], cls, clip, [(1, SPANP)], none, MIN_CLIP)[0]
    e1 = expected_peaks(soa["tid"], soa["pos"], cls, clip, [(1, SPANP + 10_000)], big, MIN_CLIP)[0]
    assert (e0["n_right"], e0["pos_right"], e0["peak_right"]) == (3, SPANP, 3)                         # span 4096 and span 1; 4097 and 0 are out
    assert e1["n_right"] == 3 and e1["peak_right"] == 2 and e1["pos_right"] == SPANP + 10_000 - big
    t0 = expected_peaks(soa["tid"], soa["pos"], cls, clip, [(1, TIES[0]), (1, TIES[1])], 10, MIN_CLIP)
    assert t0["pos_left"].tolist() == [TIES[0] - 3, TIES[1] + 1] and t0["pos_right"].tolist() == [TIES[0] - 3, TIES[1] + 1]
    assert t0["peak_left"].tolist() == [3, 3]
    p = expected_peaks(soa["tid"], soa["pos"], cls, clip, [(1, PILE)], 5, MIN_CLIP)[0]
    assert (p["pos_left"], p["peak_left"], p["pos_right"], p["peak_right"], p["n_left"]) == (PILE, 300, PILE + 2, 299, 307)
    mn = expected_peaks(soa["tid"], soa["pos"], cls, clip, [(1, MINP)], 3, MIN_CLIP)[0]
    assert (mn["n_left"], mn["n_right"]) == (2, 2)
    first = expected_peaks(soa["tid"], soa["pos"], cls, clip, [(1, 1)], 1, MIN_CLIP)[0]
    assert (first["n_left"], first["pos_left"], first["n_right"], first["pos_right"]) == (3, 1, 3, 1)
    for k, P in STEPS.items():
        e = expected_peaks(soa["tid"], soa["pos"], cls, clip, [(1, P)], WINDOW_MAX, MIN_CLIP)[0]
        assert e["n_left"] + e["n_right"] == k


def test_clip_peaks_with_idle_waves_and_both_ends_of_a_site(edge):
    bd, soa, cls, clip = edge
    q = edge_queries(100)
    exp = expected_peaks(soa["tid"], soa["pos"], cls, clip, q, 100, MIN_CLIP)
    rng = np.random.default_rng(2)
    for nq in (1, 4, 5, 9):      # one block with idle waves, a full one, one wave into the second, one into the third
        order = rng.permutation(len(q))[:nq]
        same(ask(bd, [q[i] for i in order], 100, MIN_CLIP), exp[order], "nq=%d" % nq)
    assert bd.site_clip_peaks([], [], 100).shape == (0,)
    # both ends of one site, on one sequence and on two: the asked end alone decides
    sites = [(1, TIES[0], 1, PILE, MASK), (0, B[100], 1, PILE, MASK), (1, PILE, 2, B[100], MASK)]
    pts = [(1, TIES[0]), (1, PILE), (0, B[100]), (1, PILE), (1, PILE), (2, B[100])]
    arr = [s for s in sites for _ in (1, 2)]
    got = bd.site_clip_peaks(arr, [1, 2] * len(sites), 100, MIN_CLIP)
    e = expected_peaks(soa["tid"], soa["pos"], cls, clip, pts, 100, MIN_CLIP)
    same(got, e, "both ends")
    assert got[0] != got[1] and got[2] != got[3]


def test_clip_peaks_on_an_empty_store_and_at_the_last_position():
    bd, cls = run_store(*Store().build()[:2])
    got = ask(bd, [(0, 1), (1, 500), (0, TOP)], WINDOW_MAX, 1)
    assert got.tobytes() == bytes(24 * 3)
    bd.close()
    # P = 2^31 - 1: X is 64-bit inside, an observation at 2^31 is no position and does not exist
    st = Store()
    st.left(0, TOP, times=2).left(0, TOP - 1).right(0, TOP, span=50, times=3).right(0, TOP - WINDOW_MAX, span=SPAN_MAX)
    st.add(0, TOP, word(left=20))                                    # X = 2^31
    st.add(0, TOP - 10, word(right=20, span=10)).add(0, TOP - 10, word(right=20, span=11))      # X = 2^31 - 1, and 2^31
    st.left(0, 5000)
    soa, clip, kind = st.build()
    bd, cls = run_store(soa, clip)
    check_classes(cls, kind)
    for w in (0, 1, WINDOW_MAX):
        q = [(0, TOP), (0, TOP - 1), (0, TOP - w), (0, 5000)]
        exp = expected_peaks(soa["tid"], soa["pos"], cls, clip, q, w, 10)
        same(ask(bd, q, w, 10), exp, "window=%d" % w)
    top = expected_peaks(soa["tid"], soa["pos"], cls, clip, [(0, TOP)], 0, 10)[0]
    assert (top["n_left"], top["n_right"], top["pos_left"], top["pos_right"]) == (2, 4, TOP, TOP)
    bd.close()


def fuzz_store(rng, n=5000):
    st = Store()
    centres = [(int(rng.integers(0, 3)), int(rng.integers(5000, 58_000))) for _ in range(30)]
    while len(st.rows) < n:
        kind = "ok" if rng.random() < 0.88 else ("dup" if rng.random() < 0.5 else "lowq")
        if rng.random() < 0.6:                                       # a member of a pile, now and then a base off
            tid, X = centres[int(rng.integers(0, len(centres)))]
            X += int(rng.choice([0, 0, 0, 0, 1, -1, 2, -3]))
            clip = int(rng.choice([3, 9, 10, 11, 25, 80, 255]))
            if rng.random() < 0.5:
                st.left(tid, X, clip=clip, kind=kind)
            else:
                st.right(tid, X, clip=clip, span=int(rng.choice([1, 36, 100, 151, 4000, SPAN_MAX, SPAN_MAX + 1])), kind=kind)
        else:
            w = word(left=int(rng.choice([0, 0, 0, 4, 10, 30])), right=int(rng.choice([0, 0, 0, 4, 10, 30])), span=int(rng.integers(0, 300)))
            st.add(int(rng.integers(0, 3)), int(rng.integers(0, 60_000)), w, kind=kind)
    return st.build(), centres


def test_clip_peaks_fuzz():
    rng = np.random.default_rng(77)
    (soa, clip, kind), centres = fuzz_store(rng)
    assert len(clip) == 5000
    bd, cls = run_store(soa, clip, batches=3)                        # (three pushes: the second and third grow the store, the column with it)
    check_classes(cls, kind)
    np.testing.assert_array_equal(bd.get_clips(), clip)
    hits = 0
    for w, m in ((0, 10), (5, 10), (300, 1), (WINDOW_MAX, 11), (60, 255)):
        q = []
        for _ in range(40):
            if rng.random() < 0.8:
                tid, X = centres[int(rng.integers(0, len(centres)))]
                q.append((tid, max(1, X + int(rng.integers(-w - 2, w + 3)))))
            else:
                q.append((int(rng.integers(0, 4)), int(rng.integers(1, 70_000))))
        exp = expected_peaks(soa["tid"], soa["pos"], cls, clip, q, w, m)
        same(ask(bd, q, w, m), exp, "window=%d min=%d" % (w, m))
        hits += int(((exp["n_left"] > 0) & (exp["n_right"] > 0)).sum())
    assert hits > 20
    (tl, xl), (tr, xr) = observations(soa["tid"], soa["pos"], cls, clip, 10)
    assert len(xl) > 500 and len(xr) > 500
    bd.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. the column beside the store
# ---------------------------------------------------------------------------------------------------------------------------------
def test_clip_column_growth_reset_and_rows_never_put():
    rng = np.random.default_rng(9)
    st = Store()
    for i in range(3000):
        st.add(0, 10 * i, int(rng.integers(0, 2**32)))
    soa, clip, _ = st.build()
    part = lambda lo, hi: {k: v[lo:hi] for k, v in soa.items()}
    bd = context().use_clips()
    bd.push_reads(part(0, 1000), clip=clip[:1000])                   # capacity 1024
    bd.push_reads(part(1000, 1500))                                  # no words: these rows stay 0 through the growth
    bd.push_reads(part(1500, 3000), clip=clip[1500:])
    exp = clip.copy()
    exp[1000:1500] = 0
    np.testing.assert_array_equal(bd.get_clips(), exp)
    bd.put_clips(1200, clip[1200:1300])                              # rows of records already held, later
    exp[1200:1300] = clip[1200:1300]
    np.testing.assert_array_equal(bd.get_clips(), exp)
    with pytest.raises(Exception, match="invalid argument"):
        bd.put_clips(2999, clip[:2])                                 # one row too many
    bd.run()
    np.testing.assert_array_equal(bd.get_clips(), exp)
    with pytest.raises(Exception, match="call out of order"):
        bd.use_clips(False)                                          # not while reads are held
    bd.reset_reads()
    assert bd.get_clips().shape == (0,)
    bd.stream_reads(part(0, 2000), batch=700, clip=clip[:2000])      # the staged route; the column was emptied: nothing of the old load shows
    bd.push_reads(part(2000, 2500))
    exp = np.concatenate([clip[:2000], np.zeros(500, np.uint32)])
    np.testing.assert_array_equal(bd.get_clips(), exp)
    bd.close()


def test_without_use_clips_there_is_no_column_and_bad_calls_are_refused(edge):
    from breakdancer_amd import _lib
    from breakdancer_amd.api import BATCH_FIELDS
    lib = _lib.load()
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    good = np.array([(1, PILE, 1, PILE, MASK)], dtype=_lib.SITE_DTYPE)
    e1 = np.array([1], np.uint8)
    mark = np.frombuffer(b"\xA5" * 48, dtype=_lib.CLIP_PEAKS_DTYPE).copy()
    out = mark.copy()
    words = np.zeros(4, np.uint32)
    call = lib.bdx_site_clip_peaks
    soa, clip, _ = Store().left(0, 100).left(0, 200).build()
    off = context()
    off.push_reads(soa)
    off.run()
    assert call(off.h, p(good), p(e1), 1, 100, 10, p(out)) == 4      # BDX_ESTATE: no column
    assert lib.bdx_get_clips(off.h, p(words), 4) == 4 and lib.bdx_put_clips(off.h, 0, p(words), 1) == 4
    assert lib.bdx_use_clips(off.h, 1) == 4                          # ... and none while reads are held
    off.close()
    fresh = context().use_clips()
    fresh.push_reads(soa, clip=clip)
    assert call(fresh.h, p(good), p(e1), 1, 100, 10, p(out)) == 4    # BDX_ESTATE: no run yet
    fresh.reset_reads()
    with pytest.raises(Exception, match="call out of order"):
        fresh.set_device_reads({k: 4096 for k, _ in BATCH_FIELDS}, 0)   # an adopted store with clips on
    fresh.close()
    bd = edge[0]
    assert call(bd.h, None, None, 0, 100, 10, None) == 0             # n == 0, null pointers
    assert call(bd.h, None, p(e1), 1, 100, 10, p(out)) == 1          # BDX_EINVAL from here on
    assert call(bd.h, p(good), None, 1, 100, 10, p(out)) == 1 and call(bd.h, p(good), p(e1), 1, 100, 10, None) == 1
    for w in (-1, WINDOW_MAX + 1, 2**30, -2**31):
        assert call(bd.h, p(good), p(e1), 1, w, 10, p(out)) == 1, w
    for m in (0, 256, -1, 2**31 - 1):
        assert call(bd.h, p(good), p(e1), 1, 100, m, p(out)) == 1, m
    for end in (0, 3):
        assert call(bd.h, p(good), p(np.array([end], np.uint8)), 1, 100, 10, p(out)) == 1
    assert out.tobytes() == mark.tobytes()                           # no refused call wrote a result
    assert call(bd.h, p(good), p(e1), 1, WINDOW_MAX, 255, p(out)) == 0 and call(bd.h, p(good), p(e1), 1, 0, 1, p(out)) == 0
    assert out[:1].tobytes() != mark[:1].tobytes() and out[1:].tobytes() == mark[1:].tobytes()


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. the column through the readers: a synthetic BAM with the CIGAR table mixed in, and the fixture's two BAMs merged
# ---------------------------------------------------------------------------------------------------------------------------------
def test_device_decode_fills_the_column_like_the_python_parse(tmp_path):
    from breakdancer_amd import bamdec
    path = str(tmp_path / "syn.bam")
    soa, cigars, words = synthetic_bam(path)
    n = len(words)
    # into a context's store (a sink): the sink's own switch decides
    bd = context().use_clips()
    cols, names, stats = bamdec.decode_file(path, rg_ids=["rg1"], rg_lib=[0], sink=bd, piece_blocks=2, batch_blocks=3)
    assert names == SYN_TARGETS
    np.testing.assert_array_equal(bd.get_clips(n), words)
    bd.run()
    np.testing.assert_array_equal(bd.get_clips(n), words)
    cls = bd.read_class()
    q = [(int(t), int(p) + 1) for t, p in zip(soa["tid"][::97], soa["pos"][::97])]
    same(ask(bd, q, 200, 10), expected_peaks(soa["tid"], soa["pos"], cls, words, q, 200, 10), "decoded store")
    bd.close()
    # the decoder's own columns, whole and with an --exclude mask that drops some records
    cols, _, _ = bamdec.decode_file(path, rg_ids=["rg1"], rg_lib=[0], clips=True)
    np.testing.assert_array_equal(cols["clip"], words)
    mask = [(0, 50_000, 90_000), (2, 0, 20_000)]
    cols, _, stats = bamdec.decode_file(path, rg_ids=["rg1"], rg_lib=[0], clips=True, exclude=mask)
    t, s, mt, ms = (soa[k].astype(np.int64) for k in ("tid", "pos", "mtid", "mpos"))
    drop = np.zeros(n, bool)
    for tid, beg, end in mask:
        drop |= ((t == tid) & (s >= beg) & (s < end)) | ((mt == tid) & (ms >= beg) & (ms < end))
    assert 100 < drop.sum() < n // 2 and stats["excluded"] == drop.sum()
    np.testing.assert_array_equal(cols["pos"], soa["pos"][~drop])
    np.testing.assert_array_equal(cols["clip"], words[~drop])
    # a region: the records that overlap it
    region = (1, 60_000, 120_000)
    cols, _, _ = bamdec.decode_file(path, rg_ids=["rg1"], rg_lib=[0], clips=True, region=region)
    from clip_cases import cigar_of
    end_pos = s + np.array([sum(k for k, op in cigar_of(c) if op in "MDN=X") for c in cigars], np.int64)
    keep = (t == region[0]) & (end_pos > region[1]) & (s < region[2])
    assert 100 < keep.sum() < n and (end_pos[keep] - s[keep] > 65535).any()
    np.testing.assert_array_equal(cols["pos"], soa["pos"][keep])
    np.testing.assert_array_equal(cols["clip"], words[keep])
    # without clips the decoder keeps none
    d = bamdec.decode_file(path, rg_ids=["rg1"], rg_lib=[0])[0]
    assert "clip" not in d


def test_two_decoders_merged_keep_their_clip_words():
    """the fixture's two BAMs (689 soft clips), each through a decoder of its own, gathered in the oracle's merge order"""
    import breakdancer_amd as bda
    from breakdancer_amd import bamdec
    from breakdancer_amd.api import LibraryConfig
    from clip_cases import parse_bam_cigars, words_of_bam
    from helpers import GOLDEN, load_chr21, make_opts
    from runner import product_options
    from test_gpu_bamdec import config_read_groups
    chr21 = os.path.join(GOLDEN, "chr21")
    run = load_chr21(make_opts()).run()
    rows, libs = config_read_groups(os.path.join(chr21, "inv_del_bam_config"))
    rg_ids, rg_lib = [r[0] for r in rows], [libs.index(r[1]) for r in rows]
    merged = merged_words(run, chr21)

    def decoders(clips):
        out = []
        for b, fn in enumerate(run.bam_names):
            data = np.fromfile(os.path.join(chr21, fn), dtype=np.uint8)
            members = bamdec.scan_bgzf(data)
            names, lens, k, off = bamdec.bam_header(data, members)
            d = bamdec.BamDecoder(len(names), bam_index=b, rg_ids=rg_ids, rg_lib=rg_lib, fallback_lib=0, first_record_offset=off, clips=clips)
            d.feed(data, members[k:], 3)
            d.finish()
            out.append(d)
        return out

    lcfg = [LibraryConfig(*[float(x) for x in run.lib_f[i]], min_mapping_quality=int(run.lib_i[i, 0]), bam_file_index=int(run.lib_i[i, 1]),
                          name=run.lib_names[i]) for i in range(run.nlibs)]
    bd = bda.BreakDancer(product_options(run.opts), lcfg, run.nbams, ntids=0, max_read_window_size=run.w0).use_clips()
    with_clips, without = decoders(True), decoders(False)
    with pytest.raises(RuntimeError, match="invalid argument"):
        bamdec.merge_decoded(bd, without, run.m_bam.astype(np.uint8), run.m_src.astype(np.uint32))     # a decoder without clip words
    bamdec.merge_decoded(bd, with_clips, run.m_bam.astype(np.uint8), run.m_src.astype(np.uint32))
    np.testing.assert_array_equal(bd.get_clips(len(merged)), merged)
    assert ((merged & 255) >= 5).sum() > 100
    bd.close()
    for d in with_clips + without:
        d.close()


def merged_words(run, chr21):
    """the clip words of the oracle run's merged stream: a plain parse of each BAM, the reader filter, the merge order"""
    from clip_cases import parse_bam_cigars, words_of_bam
    per = []
    for fn in run.bam_names:
        recs = parse_bam_cigars(os.path.join(chr21, fn))
        kept = ((recs["flag"] & (0x100 | 0x800)) == 0) & (recs["tid"] >= 0)
        per.append(words_of_bam(recs)[kept])
    out = np.zeros(run.n_merged, np.uint32)
    for b in range(run.nbams):
        m = run.m_bam == b
        out[m] = per[b][run.m_src[m]]
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. the CLI
# ---------------------------------------------------------------------------------------------------------------------------------
CL_KEYS = ("CLN", "CLPOS", "CLSUP", "CLSIDE")


def run_cli(args, cwd, cfg="inv_del_bam_config", env=None):
    from helpers import ROOT
    p = subprocess.run([os.path.join(ROOT, "bin", "breakdancer-max")] + args + ([cfg] if cfg else []), cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       env=dict(os.environ, **env) if env else None, timeout=300)
    assert p.returncode == 0, p.stderr.decode()
    return p.stdout.decode(), p.stderr.decode()


def strip_clip(text):
    """a VCF minus what --clip adds: the three ##clip_ lines, the four ##INFO lines and the records' keys (and minus its ##command= line)"""
    out = []
    for l in text.split("\n"):
        if l.startswith(("##clip_window=", "##clip_min=", "##clip_support=", "##command=")) or any(l.startswith("##INFO=<ID=%s," % k) for k in CL_KEYS):
            continue
        if l and not l.startswith("#"):
            c = l.split("\t")
            c[7] = ";".join(kv for kv in c[7].split(";") if kv.split("=")[0] not in CL_KEYS)
            l = "\t".join(c)
        out.append(l)
    return "\n".join(out)


def clip_keys(text):
    """per record ID (the record's fields, its --clip keys as printed and in their order)"""
    recs = [l.split("\t") for l in text.split("\n") if l and not l.startswith("#")]
    return {r[2]: (r, [kv for kv in r[7].split(";") if kv.split("=")[0] in CL_KEYS]) for r in recs}


def check_clip_records(text, soa, cls, words, targets, window, min_clip, support):
    """every record's four keys against the rule over the given records; returns {record ID: the peaks of its two printed ends}"""
    from test_clip import restated
    meta = [l for l in text.split("\n") if l.startswith("##")]
    for line in ("##clip_window=%d" % window, "##clip_min=%d" % min_clip, "##clip_support=%d" % support):
        assert line in meta, line
    for k in CL_KEYS:
        line = [l for l in meta if l.startswith("##INFO=<ID=%s," % k)]
        assert len(line) == 1 and ",Number=2,Type=%s," % ("String" if k == "CLSIDE" else "Integer") in line[0], k
    got = clip_keys(text)
    assert len(got) > 0
    peaks = {}
    for rid, (r, keys) in got.items():
        info = dict(kv.split("=") for kv in r[7].split(";") if "=" in kv)
        ends = [(targets.index(r[0]), int(r[1])), (targets.index(info["CHR2"]), int(info["POS2"]))]
        e = expected_peaks(soa["tid"], soa["pos"], cls, words, ends, window, min_clip)
        peaks[rid] = e
        rows = [(1, ends[j][1]) + tuple(int(e[j][name]) for name in ("n_left", "n_right", "pos_left", "pos_right", "peak_left", "peak_right")) for j in (0, 1)]
        assert ";" + ";".join(keys) == restated(rows[0], rows[1], 0, support), (rid, keys, rows)
        assert [kv.split("=")[0] for kv in r[7].split(";")][-4:] == list(CL_KEYS)                   # behind the existing keys
    return peaks


def test_cli_vcf_clip_on_the_golden_fixture(tmp_path):
    import test_gpu_sites as T
    from helpers import GOLDEN, filter_cmd_lines, load_chr21, make_opts, read_bam
    cwd = os.path.join(GOLDEN, "chr21")
    run = load_chr21(make_opts()).run()
    targets = read_bam(os.path.join(cwd, run.bam_names[0]))[0]
    soa, words = run.merged_soa(), merged_words(run, cwd)
    golden = filter_cmd_lines(open(os.path.join(cwd, "expected_output")).read())
    f0, f1, f2, fh = (str(tmp_path / n) for n in ("plain.vcf", "clip.vcf", "clip5.vcf", "host.vcf"))
    out0, _ = run_cli(["--vcf", f0], cwd)
    out1, err1 = run_cli(["--vcf", f1, "--clip"], cwd, env=dict(BDX_TIMING="1"))
    assert filter_cmd_lines(out0) == golden and filter_cmd_lines(out1) == golden
    assert len([l for l in err1.split("\n") if l.startswith("[bdx timing] --clip:")]) == 1
    plain, with_clip = open(f0).read(), open(f1).read()
    assert not any(k + "=" in plain for k in CL_KEYS) and "##clip_" not in plain              # (without --clip nothing of it appears)
    assert strip_clip(plain) == T.without_command(plain)
    assert strip_clip(with_clip) == T.without_command(plain)                                  # the header lines and the four keys alone
    assert T.default_window(run) == 533
    peaks = check_clip_records(with_clip, soa, run.cls, words, targets, 533, 10, 2)
    # the DEL at 29185462: its first end's left clips pile up at 29185119
    rid = [k for k, (r, _) in clip_keys(with_clip).items() if r[0] == "21" and r[1] == "29185462" and r[4] == "<DEL>"]
    assert len(rid) == 1
    e = peaks[rid[0]][0]
    # (measured: 25 left observations, 13 of them at 29185119; 2 right ones, 1 at 29185361)
    assert e["pos_left"] == 29185119 and e["peak_left"] > e["peak_right"] and e["peak_left"] >= 2
    entries = dict(kv.split("=") for kv in clip_keys(with_clip)[rid[0]][1])
    assert entries["CLPOS"].split(",")[0] == "29185119" and entries["CLSIDE"].split(",")[0] == "L"
    assert entries["CLSUP"].split(",")[0] == str(int(e["peak_left"]))
    # the same VCF from the host reader; other values of the three options, again the rule's
    outh, _ = run_cli(["--vcf", fh, "--clip"], cwd, env=dict(BDX_DECODE="host"))
    assert filter_cmd_lines(outh) == golden and T.without_command(open(fh).read()) == T.without_command(with_clip)
    out2, _ = run_cli(["--vcf", f2, "--clip", "--clip-window", "40", "--clip-min", "5", "--clip-support", "4", "--mapq", "--ci", "--depth"], cwd)
    other = open(f2).read()
    assert filter_cmd_lines(out2) == golden
    check_clip_records(other, soa, run.cls, words, targets, 40, 5, 4)
    assert {k: v[1] for k, v in clip_keys(other).items()} != {k: v[1] for k, v in clip_keys(with_clip).items()}


def test_cli_clip_of_one_sequence_through_the_index(tmp_path):
    """-o with a .bai, on a BAM whose records carry the CIGAR table: the device decode seeks through the index, the host reader reads the
    region; both print the rule's keys for given sites (the records' classes: those of quality 60 that are mapped pass, as the stores above show)"""
    path = str(tmp_path / "syn.bam")
    soa, cigars, words = synthetic_bam(path, n=2500, seed=8, index=True)
    (tmp_path / "cfg").write_text("readgroup:rg1\tplatform:illumina\tmap:syn.bam\treadlen:100.00\tlib:lib1\tlower:310.00\tupper:490.00\tmean:400.00\tstd:30.00\n")
    cls = np.where((soa["mapq"] == 60) & ((soa["flag"] & 0x4) == 0), 0x10, 0).astype(np.uint8)
    on1 = soa["tid"] == 1
    rng = np.random.default_rng(1)
    starts = np.sort(rng.choice(np.unique(soa["pos"][on1 & ((words & 255) >= 10) & (cls != 0)]), size=12, replace=False)).tolist()   # (passing, left-clipped)
    sites = [["c1", str(a + 1), "1+1-", "c1", str(a + 1 + 700 * (i + 1)), "1+1-", "DEL", str(700 * (i + 1))] for i, a in enumerate(starts)]
    (tmp_path / "sites.txt").write_text("".join("\t".join(r) + "\n" for r in sites))
    texts = []
    for env in (None, dict(BDX_DECODE="host")):
        run_cli(["-o", "c1", "--sites", "sites.txt", "--sites-vcf", "s.vcf", "--clip", "--clip-window", "300"], str(tmp_path), cfg="cfg", env=env)
        texts.append("\n".join(l for l in open(str(tmp_path / "s.vcf")).read().split("\n") if not l.startswith("##command=")))
    assert texts[0] == texts[1]
    peaks = check_clip_records(texts[0], soa, cls, words, SYN_TARGETS, 300, 10, 2)
    assert len(peaks) == 12 and all(int(e[0]["n_left"]) >= 1 for e in peaks.values()) and any(int(e[0]["n_right"]) for e in peaks.values())


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. the column as the CLI's own feeding leaves it, route by route (bin/bdx-clip-store), and sharded runs
# ---------------------------------------------------------------------------------------------------------------------------------
CFG_LINE = "readgroup:%s\tplatform:illumina\tmap:%s\treadlen:100.00\tlib:%s\tlower:310.00\tupper:490.00\tmean:400.00\tstd:30.00\n"


@pytest.fixture(scope="module")
def two_bams(tmp_path_factory):
    """two indexed BAMs with the CIGAR table mixed in that share no position (no tie between the files: the merged order is the sorted one),
    their configurations, and per file (columns, words)"""
    d = tmp_path_factory.mktemp("two")
    files = []
    for k, name in enumerate(("a.bam", "b.bam")):
        soa, cigars, words = synthetic_bam(str(d / name), n=1500, seed=20 + k, index=True, parity=k)
        files.append((soa, cigars, words))
    (d / "one.cfg").write_text(CFG_LINE % ("rg1", "a.bam", "lib1"))
    (d / "two.cfg").write_text(CFG_LINE % ("rg1", "a.bam", "lib1") + CFG_LINE % ("rg2", "b.bam", "lib2"))
    (d / "mask.bed").write_text("c0\t50000\t90000\nc2\t0\t20000\n")
    return str(d), files


def merged_of(files):
    """(tid, pos, mtid, mpos, end_pos, mapq, flag, words) of the files' records in the merged order"""
    from clip_cases import cigar_of
    cols = {k: np.concatenate([f[0][k] for f in files]).astype(np.int64) for k in ("tid", "pos", "mtid", "mpos", "mapq", "flag")}
    cols["end"] = cols["pos"] + np.concatenate([[sum(n for n, op in cigar_of(c) if op in "MDN=X") for c in f[1]] for f in files]).astype(np.int64)
    cols["word"] = np.concatenate([f[2] for f in files])
    order = np.lexsort((cols["pos"], cols["tid"]))          # (stable; the files share no position)
    return {k: v[order] for k, v in cols.items()}


def clip_store(d, args, cfg, env):
    from helpers import ROOT
    p = subprocess.run([os.path.join(ROOT, "bin", "bdx-clip-store"), "--vcf", "store.vcf", "--clip"] + args + [cfg], cwd=d, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, env=dict(os.environ, **env), timeout=120)
    assert p.returncode == 0, p.stderr.decode()
    route, rank_of, contexts = None, None, {}
    cur = None
    for l in p.stdout.decode().split("\n"):
        if l.startswith("#route"):
            route = l.split()[1]
        elif l.startswith("#rank_of"):
            rank_of = [int(v) for v in l.split()[1:]]
        elif l.startswith("#context"):
            cur = contexts.setdefault(int(l.split()[1]), [])
            want = int(l.split()[2])
        elif l:
            cur.append(int(l))
    assert all(isinstance(v, list) for v in contexts.values()) and want >= 0
    return route, rank_of, {k: np.array(v, np.uint32) for k, v in contexts.items()}


ROUTES = [("host, one file, batches of 700", "one.cfg", [], dict(BDX_DECODE="host", BDX_BATCH_RECORDS="700"), "host"),
          ("host, two files merged, batches of 700", "two.cfg", [], dict(BDX_DECODE="host", BDX_BATCH_RECORDS="700"), "host"),
          ("host, two files, --exclude", "two.cfg", ["--exclude", "mask.bed"], dict(BDX_DECODE="host", BDX_BATCH_RECORDS="333"), "host"),
          ("host, -o through the index", "two.cfg", ["-o", "c1:60000-120000"], dict(BDX_DECODE="host", BDX_BATCH_RECORDS="100"), "host"),
          ("device, one file", "one.cfg", [], {}, "device"),
          ("device, two files gathered", "two.cfg", [], {}, "device"),
          ("device, two files, --exclude", "two.cfg", ["--exclude", "mask.bed"], {}, "device"),
          ("device, -o through the index", "two.cfg", ["-o", "c1:60000-120000"], {}, "device"),
          ("sharded, host producer routed to two ranks, batches of 300", "two.cfg", [], dict(BDX_GPUS="0,0", BDX_DECODE="host", BDX_BATCH_RECORDS="300"), "host"),
          ("sharded, three ranks decode through the index", "two.cfg", [], dict(BDX_GPUS="0,0,0"), "device"),
          ("sharded, --exclude, two ranks decode through the index", "two.cfg", ["--exclude", "mask.bed"], dict(BDX_GPUS="0,0"), "device")]


@pytest.mark.parametrize("label,cfg,args,env,route", ROUTES, ids=[r[0] for r in ROUTES])
def test_the_clis_feeding_leaves_the_parsed_words_in_store_order(two_bams, label, cfg, args, env, route):
    d, files = two_bams
    m = merged_of(files[:1] if cfg == "one.cfg" else files)
    keep = np.ones(len(m["word"]), bool)
    if "--exclude" in args:
        for tid, beg, end in ((0, 50_000, 90_000), (2, 0, 20_000)):
            keep &= ~(((m["tid"] == tid) & (m["pos"] >= beg) & (m["pos"] < end)) | ((m["mtid"] == tid) & (m["mpos"] >= beg) & (m["mpos"] < end)))
    if "-o" in args:            # samtools' region c1:60000-120000 is [59999, 120000) 0-based; the records that overlap it
        keep &= (m["tid"] == 1) & (m["end"] > 59_999) & (m["pos"] < 120_000)
    assert 100 < keep.sum() and (keep.sum() < len(keep)) == bool(args)
    got_route, rank_of, contexts = clip_store(d, args, cfg, env)
    assert got_route == route, label
    if rank_of is None:
        assert list(contexts) == [0]
        np.testing.assert_array_equal(contexts[0], m["word"][keep], err_msg=label)
        assert (contexts[0] != 0).sum() > 200
        return
    assert len(set(rank_of[:3])) >= 2                        # the three sequences lie on two ranks at least
    for r, words in contexts.items():
        mine = keep & np.isin(m["tid"], [t for t in range(3) if rank_of[t] == r])
        np.testing.assert_array_equal(words, m["word"][mine], err_msg="%s, rank %d" % (label, r))
    assert sum(len(w) for w in contexts.values()) == keep.sum()


def test_cli_clip_sharded_equals_one_gpu_and_the_rule(two_bams):
    """given sites on all three sequences and one between two of them (its ends are answered by two ranks), over reads with clipped CIGARs:
    the sharded runs print what one GPU prints, and that is the rule's"""
    d, files = two_bams
    m = merged_of(files)
    cls = np.where((m["mapq"] == 60) & ((m["flag"] & 0x4) == 0), 0x10, 0).astype(np.uint8)
    rng = np.random.default_rng(6)
    sites = []
    for t in range(3):
        ok = (m["tid"] == t) & (cls != 0) & (((m["word"] & 255) >= 10) | (((m["word"] >> 8) & 255) >= 10))
        for a in np.sort(rng.choice(np.unique(m["pos"][ok]), size=5, replace=False)).tolist():
            sites.append(["c%d" % t, str(a + 1), "1+1-", "c%d" % t, str(a + 900), "1+1-", "DEL", "899"])
    sites.append(["c0", sites[0][1], "1+0-", "c2", sites[-1][1], "0+1-", "CTX", "-1"])
    open(os.path.join(d, "sites.txt"), "w").write("".join("\t".join(r) + "\n" for r in sites))
    args = ["--sites", "sites.txt", "--sites-vcf", "s.vcf", "--clip", "--clip-window", "200", "--clip-support", "1"]   # (scattered reads: piles of one)
    text = lambda: "\n".join(l for l in open(os.path.join(d, "s.vcf")).read().split("\n") if not l.startswith("##command="))
    run_cli(args, d, cfg="two.cfg")
    one = text()
    soa = dict(tid=m["tid"], pos=m["pos"])
    peaks = check_clip_records(one, soa, cls, m["word"], SYN_TARGETS, 200, 10, 1)
    assert len(peaks) == 16 and sum(int(e[j]["n_left"]) + int(e[j]["n_right"]) > 0 for e in peaks.values() for j in (0, 1)) >= 16
    sides = [kv.split("=")[1] for v in clip_keys(one).values() for kv in v[1] if kv.startswith("CLSIDE=")]
    assert len(sides) == 16 and any("L" in x for x in sides) and any("R" in x for x in sides) and sum("." not in x for x in sides) >= 10
    for env in (dict(BDX_GPUS="0,0"), dict(BDX_GPUS="0,0,0"), dict(BDX_GPUS="0,0", BDX_DECODE="host", BDX_BATCH_RECORDS="300")):
        run_cli(args, d, cfg="two.cfg", env=env)
        assert text() == one, env


def test_ranks_with_and_without_the_column_are_refused_and_ranks_with_it_answer():
    from breakdancer_amd import dist as D
    from breakdancer_amd.api import BdxError, LibraryConfig, Options
    from breakdancer_amd.synth import LIB_C2
    st = Store()
    for t in (0, 1):
        st.left(t, 5000, times=4).right(t, 5003, times=3).left(t, 5001, kind="dup", times=9)
    soa, clip, kind = st.build()
    part = lambda t: ({k: v[soa["tid"] == t] for k, v in soa.items()}, clip[soa["tid"] == t])

    def ranks_fed(with_clips):
        ranks = D.DistRun.threads(Options(), [LibraryConfig(**LIB_C2)], 1, 2, 200, [0, 0])
        for r, t in enumerate((0, 1)):
            c = ranks[r].chromosome(t)
            if with_clips[r]:
                c.use_clips().push_reads(part(t)[0], clip=part(t)[1])
            else:
                c.push_reads(part(t)[0])
        return ranks
    ranks = ranks_fed((True, False))
    with pytest.raises(BdxError, match="bdx_use_clips is set on some ranks"):
        D.run_threads(ranks)
    for r in ranks:
        r.close()
    ranks = ranks_fed((True, True))
    D.run_threads(ranks)
    for r, t in enumerate((0, 1)):
        c = ranks[r].chromosome(t)
        np.testing.assert_array_equal(c.get_clips(), part(t)[1])
        got = ask(c, [(t, 5000), (1 - t, 5000)], 10, 10)
        assert got[0].tolist() == (4, 3, 5000, 5003, 4, 3) and got[1].tolist() == (0, 0, 0, 0, 0, 0)     # (the other sequence's reads are on the other rank)
    for r in ranks:
        r.close()
