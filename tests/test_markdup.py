"""CPU tests of --mark-dup: the rule's numpy restatement (markdup_cases.rule_marks, what the GPU tests hold the kernel to) on cases
placed by hand, the planting and rewriting helpers, and the option's presence in the usage text, the header and the bindings."""
import os
import re
import subprocess

import numpy as np

from helpers import ROOT
from markdup_cases import plant_duplicates, rewrite_bam_marked, rule_group_count, rule_marks, stream_marks, with_marks

PAIRED, REV, MREV, FIRST, SECOND = 0x1, 0x10, 0x20, 0x40, 0x80
F1 = PAIRED | MREV | FIRST   # a forward first mate whose mate is reverse


def marks(rows):
    """rows of (tid, pos, mtid, mpos, flag, lib, name_key)"""
    a = np.array(rows, dtype=np.int64).reshape(-1, 7)
    cols = [a[:, i] for i in range(6)] + [a[:, 6].astype(np.uint64)]
    return rule_marks(*cols).tolist(), rule_group_count(*cols)


def test_group_of_three_keeps_the_smallest_key():
    m, g = marks([(0, 100, 0, 400, F1, 0, 7), (0, 100, 0, 400, F1, 0, 3), (0, 100, 0, 400, F1, 0, 9)])
    assert m == [True, False, True] and g == 1


def test_equal_keys_keep_the_lower_index():
    m, g = marks([(0, 100, 0, 400, F1, 0, 5), (0, 100, 0, 400, F1, 0, 5), (0, 100, 0, 400, F1, 0, 5)])
    assert m == [False, True, True] and g == 1


def test_every_part_of_the_key_splits_a_group():
    base = (0, 100, 0, 400, F1, 0, 1)
    assert marks([base, (0, 100, 0, 400, F1, 0, 2)]) == ([False, True], 1)
    for other in [(0, 100, 0, 400, F1 | REV, 0, 2),                       # strand
                  (0, 100, 0, 400, F1 & ~MREV, 0, 2),                     # mate strand
                  (0, 100, 0, 400, (F1 & ~FIRST) | SECOND, 0, 2),         # first in pair
                  (0, 100, 0, 400, F1, 1, 2),                             # library
                  (0, 100, 1, 400, F1, 0, 2),                             # mtid
                  (0, 100, 0, 401, F1, 0, 2)]:                            # mpos
        assert marks([base, other]) == ([False, False], 0), other
    # bits outside the key do not split: proper pair, second in pair (0x80 follows 0x40 in real data; alone it is not looked at)
    assert marks([base, (0, 100, 0, 400, F1 | 0x2 | 0x200, 0, 2)]) == ([False, True], 1)


def test_a_record_already_marked_is_neither_marked_again_nor_a_competitor():
    m, g = marks([(0, 100, 0, 400, F1 | 0x400, 0, 1), (0, 100, 0, 400, F1, 0, 2)])
    assert m == [False, False] and g == 0
    m, g = marks([(0, 100, 0, 400, F1 | 0x400, 0, 1), (0, 100, 0, 400, F1, 0, 5), (0, 100, 0, 400, F1, 0, 2)])
    assert m == [False, True, False] and g == 1


def test_unpaired_unmapped_and_mate_unmapped_records_are_never_marked():
    for flag, tid, mtid in [(F1 & ~PAIRED, 0, 0), (F1 | 0x4, 0, 0), (F1 | 0x8, 0, 0), (F1 | 0x100, 0, 0), (F1 | 0x800, 0, 0), (F1, 0, -1), (F1, -1, 0)]:
        rows = [(tid, 100, mtid, 400, flag, 0, k) for k in (3, 1, 2)]
        assert marks(rows) == ([False, False, False], 0), (flag, tid, mtid)
    # ... and do not compete with the candidates beside them
    m, g = marks([(0, 100, 0, 400, F1 | 0x8, 0, 1), (0, 100, 0, 400, F1, 0, 3), (0, 100, 0, 400, F1, 0, 2)])
    assert m == [False, True, False] and g == 1


def test_two_mates_at_one_position_with_one_strand_both_survive():
    a = (0, 100, 0, 100, PAIRED | FIRST, 0, 4)
    b = (0, 100, 0, 100, PAIRED | SECOND, 0, 4)
    assert marks([a, b]) == ([False, False], 0)


def test_both_ends_of_duplicated_pairs_keep_the_same_pair():
    # three copies of one pair: first mates at 100, second mates at 400; keys 8, 2, 5 -> the pair with key 2 survives at both ends
    first = [(0, 100, 0, 400, PAIRED | MREV | FIRST, 0, k) for k in (8, 2, 5)]
    second = [(0, 400, 0, 100, PAIRED | REV | SECOND, 0, k) for k in (5, 8, 2)]   # (another order at the far end)
    m, g = marks(first + second)
    assert m == [True, False, True, True, True, False] and g == 2
    keys = [r[6] for r, x in zip(first + second, m) if not x]
    assert keys == [2, 2]


def test_equal_positions_that_are_not_contiguous_form_separate_runs():
    rows = [(0, 100, 0, 400, F1, 0, 5), (0, 200, 0, 500, F1, 0, 9), (0, 100, 0, 400, F1, 0, 1)]
    assert marks(rows) == ([False, False, False], 0)
    assert marks([rows[0], rows[2], rows[1]]) == ([True, False, False], 1)


def test_planted_duplicates_are_found_and_rewritten(tmp_path):
    """plant_duplicates adds whole pairs, anomalous ones among them; stream_marks marks exactly one record less than every group holds;
    rewrite_bam_marked changes the marked flags and nothing else"""
    from breakdancer_amd.bamwrite import write_bam_records
    from fuzzgen import make_case
    from helpers import read_bam
    cfg, streams, targets = make_case(1500)
    planted = plant_duplicates(streams, 1500)
    assert all(len(p["tid"]) > len(s["tid"]) for p, s in zip(planted, streams))
    for p in planted:
        assert (np.diff(p["tid"].astype(np.int64) * (1 << 32) + p["pos"]) >= 0).all()
    libs = [np.zeros(len(p["tid"]), np.int64) for p in planted]
    per, groups = stream_marks(planted, libs)
    n_marked = sum(int(m.sum()) for m in per)
    assert groups > 20 and n_marked >= groups
    anomalous = np.concatenate([(np.asarray(p["flag"]) & 0x2) == 0 for p in planted])
    assert (np.concatenate(per) & anomalous).any()
    # marking twice changes nothing more
    again, g2 = stream_marks([with_marks(p, m) for p, m in zip(planted, per)], libs)
    assert g2 == 0 and not np.concatenate(again).any()
    # both mates of a marked record are marked (the pairs are consistent and whole)
    st, m = planted[0], per[0]
    two = np.array([np.count_nonzero(st["name_id"] == x) == 2 for x in st["name_id"]])
    by_name = {}
    for nm, x in zip(st["name_id"][two], m[two]):
        by_name.setdefault(int(nm), []).append(bool(x))
    assert all(v[0] == v[1] for v in by_name.values())
    # the rewritten file
    recs = [dict(tid=st["tid"][i], pos=st["pos"][i], mtid=st["mtid"][i], mpos=st["mpos"][i], isize=st["isize"][i], flag=st["flag"][i], qlen=st["qlen"][i],
                 mapq=int(st["bdqual"][i]), am=None, rg=st["rg"][i], name="read%d" % int(st["name_id"][i])) for i in range(len(st["tid"]))]
    extra = dict(recs[5])
    extra["flag"] = int(extra["flag"]) | 0x100   # (a secondary copy: not part of the store, never marked)
    recs.insert(6, extra)
    write_bam_records(str(tmp_path / "a.bam"), recs, targets, rgs=("rg1", "rg2", "rg3"), seed=1)
    assert rewrite_bam_marked(str(tmp_path / "a.bam"), str(tmp_path / "b.bam"), m) == int(m.sum())
    _, a = read_bam(str(tmp_path / "a.bam"), keep_all=True)
    _, b = read_bam(str(tmp_path / "b.bam"), keep_all=True)
    want = np.insert(m, 6, False)
    for k in a:
        if k == "flag":
            np.testing.assert_array_equal(np.asarray(b[k]), np.where(want, np.asarray(a[k]) | 0x400, np.asarray(a[k])))
        elif isinstance(a[k], np.ndarray):
            np.testing.assert_array_equal(a[k], b[k], err_msg=k)
        else:
            assert a[k] == b[k], k


def test_usage_names_the_option():
    exe = os.path.join(ROOT, "bin", "breakdancer-max")
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert p.returncode == 1
    assert re.search(r"^\s+--mark-dup\s", p.stderr.decode(), re.M), p.stderr.decode()


def test_header_and_bindings_declare_the_new_symbols():
    from breakdancer_amd import _lib
    names = ["bdx_set_mark_duplicates", "bdx_get_duplicates", "bdx_dist_set_mark_duplicates", "bdx_dist_get_duplicates", "bdx_mark_duplicates"]
    header = open(os.path.join(ROOT, "include", "bdx.h")).read()
    for n in names:
        assert n in _lib.EXPORTS, n
        assert re.search(r"^int %s\(" % n, header, re.M), n
    assert _lib.DUP_T >= 1
    dev = open(os.path.join(ROOT, "breakdancer_amd", "csrc", "bdx_dev.h")).read()
    assert int(re.search(r"constexpr int kDupT = (\d+);", dev).group(1)) == _lib.DUP_T   # (the mirror the GPU tests size their runs by)
