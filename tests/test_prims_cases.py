"""tests/prims_cases.py on its own: the references against plain loops, and the case tables against the edges that
tests/test_gpu_prims.py relies on them to hold (a table that lost an edge would let the GPU tests pass for nothing)."""
import numpy as np
import pytest

import prims_cases as pc


# ---- references ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cols", [1, 4])
@pytest.mark.parametrize("family", pc.FAMILIES)
def test_scan_reference_is_the_running_sum_modulo_2_32(family, cols):
    for n in (0, 1, 2, 5, 64, 257, 700):
        v = pc.values(family, n, cols)
        assert v.dtype == np.uint32 and v.shape == ((n,) if cols == 1 else (n, cols))
        rows = v.reshape(n, cols).tolist()
        acc, want_incl, want_excl = [0] * cols, [], []
        for row in rows:
            want_excl.append(list(acc))
            acc = [(a + x) & 0xFFFFFFFF for a, x in zip(acc, row)]
            want_incl.append(list(acc))
        assert pc.scan_reference(v).reshape(n, cols).tolist() == want_incl
        assert pc.exclusive_reference(v).reshape(n, cols).tolist() == want_excl
        assert pc.scan_reference(v).dtype == np.uint32


def test_value_families_are_what_they_say():
    for cols in (1, 4):
        f, s, w = (pc.values(k, 70_000, cols) for k in pc.FAMILIES)
        assert set(np.unique(f)) == {0, 1}
        assert s.max() <= 65_535 and s.max() > 60_000
        assert (w >> 31).mean() > 0.4 and w.reshape(-1, cols)[0].tolist() == [0xFFFFFFFF] * cols
        # a workgroup's total and the prefixes wrap 2^32 several times over
        assert w.reshape(-1, cols)[:256].astype(np.uint64).sum(axis=0).min() >> 32 >= 4
        # ... and the other two never do at these sizes, so the three differ in kind
        assert int(s.astype(np.uint64).sum(axis=0).max()) < 1 << 32
    assert np.array_equal(pc.values("full", 1000, 4), pc.values("full", 1000, 4))
    # a shorter draw is a prefix of a longer one: the GPU tests slice one pool and one reference
    assert np.array_equal(pc.values("full", 100, 4), pc.values("full", 1000, 4)[:100])
    assert np.array_equal(pc.values("small", 100, 1), pc.values("small", 1000, 1)[:100])


def naive_lower_bound(tid, pos, n, t, p):
    for i in range(n):
        if not (tid[i] < t or (tid[i] == t and pos[i] < p)):
            return i
    return n


@pytest.mark.parametrize("family", pc.SEARCH_FAMILIES)
def test_search_reference_is_the_first_record_not_below(family):
    for n in (0, 1, 2, 63, 64, 65, 66, 700):
        tid, pos = pc.store(family, n)
        qt, qp = pc.queries(tid, pos, extra=pc.run_ends(n))
        want = [naive_lower_bound(tid.tolist(), pos.tolist(), n, int(t), int(p)) for t, p in zip(qt, qp)]
        assert pc.search_reference(pc.keys_of(tid, pos), qt, qp).tolist() == want
        assert pc.search_reference(pc.keys_of(tid, pos, as_view=True), qt, qp).tolist() == want
        if n > 10:  # a prefix of the store
            want = [naive_lower_bound(tid.tolist(), pos.tolist(), n - 7, int(t), int(p)) for t, p in zip(qt, qp)]
            assert pc.search_reference(pc.keys_of(tid, pos), qt, qp, n - 7).tolist() == want


def naive_walk(tid, pos, n, t, wlo, whi):
    L = R = naive_lower_bound(tid, pos, n, t, wlo)
    while R < n and tid[R] == t and pos[R] <= whi:
        R += 1
    return L, R, (R - L) // 64 + 1


def test_walk_reference_is_the_plain_loop():
    for label, family, n_upper, n, queries in pc.walk_cases():
        tid, pos = pc.store(family, n_upper)
        qt, qlo, qhi = pc.walk_arrays(queries)
        L, R, steps = pc.walk_reference(tid, pos, qt, qlo, qhi, n)
        want = [naive_walk(tid.tolist(), pos.tolist(), n, t, lo, hi) for t, lo, hi in queries]
        assert list(zip(L.tolist(), R.tolist(), steps.tolist())) == want, label
    # a grid of windows over a store with runs, and bounds far outside 32 bits on a store whose positions reach both ends of the int32 range
    tid, pos = pc.store("runs", 700)
    pos = pos.copy()
    pos[0], pos[-1] = -2**31, 2**31 - 1
    far = 1 << 40
    q = [(7, int(p) + d, int(p2) + e) for p in pos[::37] for p2 in pos[5::91] for d in (-1, 0, 1) for e in (-1, 0, 1)]
    q += [(7, -far, far), (7, -2**31, 2**31 - 1), (7, -2**31 - 1, -2**31), (7, 2**31 - 1, pc.WHI_WIDE), (7, 2**31, far), (6, -far, far), (8, -far, far)]
    L, R, steps = pc.walk_reference(tid, pos, *pc.walk_arrays(q))
    assert list(zip(L.tolist(), R.tolist(), steps.tolist())) == [naive_walk(tid.tolist(), pos.tolist(), 700, *x) for x in q]


def test_count_reference_is_the_plain_loop():
    tid, pos, hit, key = pc.count_store()
    queries = pc.count_queries(tid, pos)
    qt, qlo, qhi = pc.walk_arrays(queries)
    for nkeys in pc.COUNT_NKEYS:
        want = []
        for t, lo, hi in queries:
            L, R, _ = naive_walk(tid.tolist(), pos.tolist(), len(tid), t, lo, hi)
            row = [0] * nkeys
            for i in range(L, R):
                if hit[i]:
                    row[int(key[i]) if key[i] < nkeys else 0] += 1
            want.append(row)
        got = pc.count_reference(tid, pos, hit, key, qt, qlo, qhi, nkeys)
        assert got.dtype == np.uint32 and got.tolist() == want


# ---- the tables ------------------------------------------------------------------------------------------------------------

def test_three_launch_sizes_reach_every_route():
    s = set(pc.SCAN3_SIZES)
    assert {1, 511, 512, 513} <= s
    assert {512 * 255 - 1, 512 * 255 + 1, 512 * 256 - 1, 512 * 256 + 1, 512 * 257, 512 * 1024, 512 * 1024 + 1, 512 * 2048 + 1} <= s
    grids = {pc.grid3(n) for n in s}
    assert 1 in grids and pc.SELF_SUM_MAX in grids and pc.SELF_SUM_MAX + 1 in grids
    assert any(256 < g <= pc.SELF_SUM_MAX for g in grids)            # phase 3's strided sum makes a second trip (workgroups 257 and up)
    assert any(1024 < g <= 2048 for g in grids) and any(2048 < g <= 3072 for g in grids)   # phase 2's loop: two trips, three trips
    assert not pc.scan3_has_total(512 * 1024) and pc.scan3_has_total(512 * 1024 + 1)
    assert (0, 512 * 1024 + 1) in pc.SCAN3_NPTR and (700, 512 * 1024 + 1) in pc.SCAN3_NPTR
    assert any(n == 0 and pc.grid3(up) == 1 and up > 0 for n, up in pc.SCAN3_NPTR)
    assert all(n <= up for n, up in pc.SCAN3_NPTR)
    assert max(s) <= pc.LB_MAX_N   # (one pool of values serves every scan)


def test_look_back_sizes_hold_every_block_count_and_tail():
    assert pc.LB_BLOCKS[4] == [0, 1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 300]
    assert pc.LB_BLOCKS[1] == [0, 1, 63, 64, 65, 255, 256, 257, 513]
    assert pc.LB_TAILS == [0, 1, 63, 64, 65, 255]
    assert pc.lb_window_edges(4) == {15, 16, 17, 63, 64, 65} and pc.lb_window_edges(1) == {63, 64, 65, 255, 256, 257}
    assert set(pc.LB_VARIANTS.values()) == {(1, 1), (4, 1), (4, 2)}
    for variant, (cols, iters) in pc.LB_VARIANTS.items():
        sizes = pc.lb_sizes(variant)
        assert {B for B, _, _ in sizes} == set(pc.LB_BLOCKS[cols]) and {r for _, r, _ in sizes} == set(pc.LB_TAILS)
        assert pc.lb_window_edges(cols) <= set(pc.LB_BLOCKS[cols])
        for B in pc.lb_window_edges(cols):       # a tail behind every window edge: the workgroup with exactly B predecessors exists and is partial
            assert any(b == B and r != 0 for b, r, _ in sizes) and any(b == B and r == 0 for b, r, _ in sizes)
        for B, r, n in sizes:
            assert n == 256 * iters * B + r and n <= pc.LB_MAX_N
            assert (n + 256 * iters - 1) // (256 * iters) == B + (r != 0)
    assert pc.LB_MAX_N == (1 << 20) + 1
    assert pc.LB_STALE_SEQUENCE == [(1 << 20) + 1, 300, 70_000] and pc.LB_LAST_STAMP == 0x3FFFFFFF
    n, up = pc.LB_NPTR
    assert n * 10 <= up <= pc.LB_MAX_N
    assert {B for B, _ in pc.HEAD_CASES} == set(pc.LB_BLOCKS[4]) and {r for _, r in pc.HEAD_CASES} >= {0, 1, 255}
    assert all(pc.head_workgroups(256 * B + r) == B + (r != 0) for B, r in pc.HEAD_CASES)


def test_search_sizes_sit_on_the_round_boundaries():
    s = pc.SEARCH_SIZES
    for edge in (64, 65, 64 * 65, 65 ** 2, 65 ** 3):
        assert {edge - 1, edge, edge + 1} <= set(s), edge
    assert {0, 1, 2, (1 << 20) + 3} <= set(s)
    assert pc.SEARCH_LARGE == (1 << 26) + (1 << 20) + 1
    assert pc.SEARCH_LARGE * 64 >= 1 << 32 and max(s) * 64 < 1 << 32   # len * (lane + 1) leaves 32 bits in the large case alone
    assert set(pc.QUERY_COUNTS) == {1, 4, 5}


def test_runs_lie_across_first_round_probe_points():
    seen = set()
    for n in pc.SEARCH_SIZES:
        tid, pos = pc.store("runs", n)
        assert (np.diff(pos.astype(np.int64)) >= 0).all() and (tid == 7).all()
        points = {pc.probe_point(n, lane) for lane in range(64)} if n > 64 else set()
        for length, start in pc.runs_layout(n):
            run = pos[start:start + length]
            assert (run == run[0]).all() and (start == 0 or pos[start - 1] < run[0]) and (start + length == n or pos[start + length] > run[0])
            inside = [p for p in points if start <= p < start + length]
            assert inside
            if length >= 64:  # records of the run on both sides of the probe point
                assert any(start < p < start + length - 1 for p in inside)
            seen.add(length)
    assert seen == set(pc.RUN_LENGTHS)
    assert len(pc.runs_layout((1 << 20) + 3)) == len(pc.RUN_LENGTHS) and len(pc.runs_layout(274_625)) == len(pc.RUN_LENGTHS)


def test_stores_are_sorted_and_hold_what_the_families_promise():
    for n in (1, 2, 65, 4161, 274_625):
        for family in pc.SEARCH_FAMILIES:
            tid, pos = pc.store(family, n)
            assert tid.dtype == np.int32 and pos.dtype == np.int32 and len(tid) == len(pos) == n
            k = tid.astype(np.int64) * (1 << 32) + pos
            assert (np.diff(k) >= 0).all(), (family, n)
            if family == "distinct":
                assert (np.diff(k) > 0).all()
            if family == "equal":
                assert (np.diff(k) == 0).all()
    tid, pos = pc.store("tids", 4161)
    assert set(tid.tolist()) == set(pc.TIDS) and (pos == -1).sum() == 2 * len(pc.TIDS)
    assert set(range(min(pc.TIDS), max(pc.TIDS))) - set(pc.TIDS)   # a tid absent in the middle


def test_queries_hold_every_kind():
    far = 1 << 40
    tid, pos = pc.store("tids", 700)
    qt, qp = pc.queries(tid, pos)
    q = set(zip(qt.tolist(), qp.tolist()))
    for t, p in set(zip(tid.tolist(), pos.tolist())):
        assert {(t, p - 1), (t, p), (t, p + 1)} <= q
    assert any(t < tid[0] for t, _ in q) and any(t > tid[-1] for t, _ in q)
    absent = set(range(int(tid[0]), int(tid[-1]))) - set(tid.tolist())
    assert any(t in absent for t, _ in q)
    assert any(p == far for _, p in q) and any(p == -far for _, p in q)
    assert any((t, p) < (tid[0], pos[0]) and t == tid[0] for t, p in q) and any((t, p) > (tid[-1], pos[-1]) and t == tid[-1] for t, p in q)
    assert qp.dtype == np.int64 and qt.dtype == np.int32
    # a large store is sampled, with the ends of its runs in the sample
    n = 274_625
    tid, pos = pc.store("runs", n)
    qt, qp = pc.queries(tid, pos, extra=pc.run_ends(n))
    assert 3 * pc.SAMPLE * 0.9 <= len(qt) <= 3 * (pc.SAMPLE + 40) + 40
    q = set(zip(qt.tolist(), qp.tolist()))
    for length, start in pc.runs_layout(n):
        assert (7, int(pos[start])) in q and (7, int(pos[start + length - 1]) + 1) in q and (7, int(pos[start - 1])) in q


def test_large_store_is_a_formula_over_the_index():
    n = (1 << 24) * 2 + 77   # (the formula at a size the CPU suite can afford; the GPU test builds SEARCH_LARGE records)
    tid, pos = pc.large_store(n)
    assert tid.dtype == np.int32 and pos.dtype == np.int32 and len(tid) == n
    for i in (0, 1, 2, 3, (1 << 24) - 1, 1 << 24, (1 << 24) + 1, n - 1):
        assert tid[i] == (i >> 24) * 2 + 1 and pos[i] == ((i & ((1 << 24) - 1)) >> 1) * 3 - 1
    k = tid.astype(np.int64) * (1 << 32) + pos
    assert (np.diff(k) >= 0).all() and pos[0] == -1 and pos[1 << 24] == -1


def walk_table():
    """every case of walk_cases with its store and reference: (label, tid, pos, n, queries, L, R, steps)"""
    for label, family, n_upper, n, queries in pc.walk_cases():
        tid, pos = pc.store(family, n_upper)
        yield (label, tid, pos, n, queries) + pc.walk_reference(tid, pos, *pc.walk_arrays(queries), n)


def test_walk_cases_hold_every_store_count_and_place():
    assert pc.WALK_STORES == [0, 1, 63, 64, 65, 128, 129, 64 * 65] and pc.WALK_COUNTS == [0, 1, 63, 64, 65, 128]
    assert pc.WHI_WIDE == 2**31 - 2 + 2**30 and pc.WHI_WIDE >= 1 << 31
    table = {row[0]: row for row in walk_table()}
    assert {"distinct-%d" % n for n in pc.WALK_STORES} <= set(table)
    for n in pc.WALK_STORES:
        _, tid, pos, m, queries, L, R, steps = table["distinct-%d" % n]
        assert m == n == len(tid)
        on7 = np.array([t == 7 for t, _, _ in queries])
        for k in pc.WALK_COUNTS:
            if k > n:
                continue
            has = (R - L == k) & on7
            assert (has & (L == 0)).any(), (n, k, "at the first record")
            assert (has & (R == n)).any(), (n, k, "ending at the last record")
            if n - k >= 2 and k:
                assert (has & (L > 0) & (R < n)).any(), (n, k, "in the middle")
        assert any(lo < 0 for _, lo, _ in queries) and any(hi == pc.WHI_WIDE for _, _, hi in queries) and any(lo > hi for _, lo, hi in queries)
        assert any(t < 7 for t, _, _ in queries) and any(t > 7 for t, _, _ in queries)
        assert (steps == (R - L) // 64 + 1).all() and (R >= L).all()
    # the extra step wholly behind n: whole steps of records that end with the store
    _, _, _, _, _, L, R, steps = table["distinct-%d" % (64 * 65)]
    assert ((R == 64 * 65) & (R - L == 64)).any() and ((R == 64 * 65) & (R - L == 128)).any() and (steps == 66).any()
    # a store that ends inside the window while records that would lie inside follow it in memory
    _, tid, pos, n, queries, L, R, _ = table["prefix-128"]
    assert n == 128 < len(tid) and (R == n).any() and any(hi >= pos[n] and lo <= pos[n] for _, lo, hi in queries) and (R <= n).all()
    assert table["prefix-0"][3] == 0 and (table["prefix-0"][7] == 1).all()


def test_walk_cases_stop_on_the_chromosome_and_cut_runs_whole():
    table = {row[0]: row for row in walk_table()}
    counts = set()
    for n in pc.WALK_TID_STORES:
        _, tid, pos, _, queries, L, R, _ = table["tids-%d" % n]
        for (t, lo, hi), a, b in zip(queries, L.tolist(), R.tolist()):
            # the window's last record is the chromosome's last and the next chromosome starts at a position <= whi
            if a < b < n and tid[b] != t and tid[b - 1] == t and pos[b] <= hi:
                counts.add(b - a)
        present = set(tid.tolist())
        assert any(t not in present and min(present) < t < max(present) and a == b for (t, _, _), a, b in zip(queries, L, R))   # absent
        assert any(t > max(present) and a == b == n for (t, _, _), a, b in zip(queries, L, R))                               # behind the last
        assert any(t < min(present) and a == b == 0 for (t, _, _), a, b in zip(queries, L, R))
    assert {1, 2, 63, 64, 65, 66, 128} <= counts, counts
    _, tid, pos, n, queries, L, R, _ = table["runs-%d" % pc.WALK_RUN_STORE]
    layout = pc.runs_layout(n)
    assert {length for length, _ in layout} == {1, 64, 65}
    got = set(zip(L.tolist(), R.tolist()))
    for length, start in layout:
        end = start + length
        assert (start, end) in got                                  # wlo == whi == the run's position: all of it, nothing else
        assert any(a == end for a, _ in got)                        # the run at wlo - 1: none of it
        assert any(b == end and a < start for a, b in got)          # the run at whi: all of it
        assert any(b == start and a < start for a, b in got)        # the run at whi + 1: none of it
        assert not any(start < a < end or start < b < end for a, b in got), "a window cuts a run of equal positions"


def test_count_cases_hold_every_key_count_and_out_of_range_keys():
    assert pc.COUNT_NKEYS == [1, 2, 64, 65, 255]
    tid, pos, hit, key = pc.count_store()
    assert hit.dtype == np.uint8 and key.dtype == np.uint8 and len(hit) == len(key) == len(tid) == pc.COUNT_STORE
    assert set(np.unique(hit)) == {0, 1, 2, 255} and 0.6 < (hit != 0).mean() < 0.9 and (key < 4).mean() > 0.4 and (key >= 65).mean() > 0.3
    queries = pc.count_queries(tid, pos)
    assert len(queries) == 5       # one, four and five queries are its first one, four and all
    qt, qlo, qhi = pc.walk_arrays(queries)
    L, R, _ = pc.walk_reference(tid, pos, qt, qlo, qhi)
    assert (R - L)[1] == 0 and 64 in (R - L).tolist() and (R == len(tid)).any() and (L == 0).any()
    for nkeys in pc.COUNT_NKEYS:
        ref = pc.count_reference(tid, pos, hit, key, qt, qlo, qhi, nkeys)
        assert ref.shape == (5, nkeys) and ref[1].sum() == 0 and ref[0].sum() > 0
        for q in (0, 2, 3, 4):
            sl = slice(L[q], R[q])
            assert ref[q].sum() == (hit[sl] != 0).sum()
            if q == 0 or nkeys < 255:                                # hits with a key out of range: key 255 in the first window, whatever nkeys
                assert ((key[sl] >= nkeys) & (hit[sl] != 0)).any()
            assert ref[q, 0] == (((key[sl] >= nkeys) | (key[sl] == 0)) & (hit[sl] != 0)).sum()
        if nkeys > 1:
            assert np.count_nonzero(ref[:, 1:].sum(axis=0)) >= min(nkeys - 1, 16)   # (the counts are spread over the keys ...
            assert ref[0, nkeys - 1] > 0                                             # ... and the first query has the last one)
