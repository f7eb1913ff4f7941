"""CPU tests of --exclude: the BED parser and its errors through bin/bdx-dump-reads and bin/breakdancer-max, and the two host
readers (ColumnReader behind produce / produce_merged_by_columns) against a numpy restatement of the rule on the unmasked dump's own
columns.  Every comparison is exact."""
import os
import subprocess

import numpy as np
import pytest

from exclude_cases import excluded_count, masked_dump, merge_intervals, n_merged, rule_mask, write_bed, write_case
from fuzzgen import make_case
from helpers import GOLDEN, ROOT

DUMP = os.path.join(ROOT, "bin", "bdx-dump-reads")
EXE = os.path.join(ROOT, "bin", "breakdancer-max")
CHR21 = os.path.join(GOLDEN, "chr21")


def run_tool(exe, args, cwd, env=None):
    if not os.path.exists(exe):
        import __graft_entry__ as g
        g.build()
    return subprocess.run([exe] + args, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=dict(os.environ, **(env or {})))


def dump_rows(args, cwd, env=None):
    """(rows of the twelve columns as text, stderr)"""
    p = run_tool(DUMP, args, cwd, dict(env or {}, BDX_TIMING="1"))
    assert p.returncode == 0, p.stderr.decode()
    return [l for l in p.stdout.decode().splitlines() if not l.startswith("#")], p.stderr.decode()


def columns(rows):
    a = np.array([[int(x) for x in l.split("\t")[:4]] for l in rows], dtype=np.int64).reshape(-1, 4)
    return a[:, 0], a[:, 1], a[:, 2], a[:, 3]


MALFORMED = [("fewer-fields", "21\t100\n", 2), ("one-field", "21\n", 2), ("not-an-integer", "21\t100\t2x0\n", 2), ("float", "21\t1e3\t2000\n", 2),
             ("empty-coordinate-sign", "21\t+\t20\n", 2), ("negative-begin", "21\t-5\t20\n", 2), ("negative-end", "21\t5\t-20\n", 2),
             ("end-before-begin", "21\t300\t200\n", 2)]


@pytest.mark.parametrize("exe", [DUMP, EXE], ids=["bdx-dump-reads", "breakdancer-max"])
@pytest.mark.parametrize("label,line,lineno", MALFORMED, ids=[m[0] for m in MALFORMED])
def test_malformed_bed_lines_exit_1_with_file_and_line(tmp_path, exe, label, line, lineno):
    bed = tmp_path / "m.bed"
    bed.write_text("21\t10\t20\n" + line + "21\t30\t40\n")
    p = run_tool(exe, ["--exclude", str(bed), "inv_del_bam_config"], CHR21)
    assert p.returncode == 1, (p.stdout.decode()[-300:], p.stderr.decode())
    assert ("%s:%d" % (str(bed), lineno)) in p.stderr.decode(), p.stderr.decode()
    assert not p.stdout.decode().strip()   # (nothing was printed: the file is read before any work is done, and before the GPU is touched)


@pytest.mark.parametrize("exe", [DUMP, EXE], ids=["bdx-dump-reads", "breakdancer-max"])
def test_unreadable_bed_file_exits_1_naming_the_file(tmp_path, exe):
    missing = str(tmp_path / "no_such.bed")
    p = run_tool(exe, ["--exclude", missing, "inv_del_bam_config"], CHR21)
    assert p.returncode == 1 and missing in p.stderr.decode(), p.stderr.decode()
    assert not p.stdout.decode().strip()


def test_usage_text_names_the_option():
    p = run_tool(EXE, [], CHR21)
    assert p.returncode == 1 and "--exclude FILE" in p.stderr.decode() and "--vcf FILE" in p.stderr.decode()


def chr21_targets():
    from helpers import read_bam
    return read_bam(os.path.join(CHR21, "NA19238_chr21_del_inv.bam"))[0]


def test_comments_unknown_names_and_messy_intervals_behave_as_their_union(tmp_path):
    """comment, track and browser lines and blank lines are skipped; lines on sequences the header does not have are ignored and counted;
    unsorted, overlapping, touching and empty intervals act as their union"""
    base, _ = dump_rows(["inv_del_bam_config"], CHR21)
    tid, pos, mtid, mpos = columns(base)
    t = int(tid[0])
    name = chr21_targets()[t]
    ps = np.sort(pos)
    a, b, c = int(ps[len(ps) // 5]), int(ps[len(ps) // 2]), int(ps[4 * len(ps) // 5])
    messy = tmp_path / "messy.bed"
    messy.write_text("# a comment\ntrack name=mask\nbrowser position %s:1-2\n\n" % name +
                     "%s\t%d\t%d\n" % (name, b, b + 500) +          # out of order
                     "%s %d %d name 0 +\n" % (name, a, a + 300) +    # spaces, further fields
                     "chrUn_gl000220\t0\t1000\n" +                   # unknown: ignored, counted
                     "%s\t%d\t%d\n" % (name, a + 200, a + 400) +     # overlaps
                     "%s\t%d\t%d\n" % (name, a + 400, a + 450) +     # touches
                     "%s\t%d\t%d\n" % (name, c, c) +                 # empty: ignored
                     "%s\t%d\t4000000000\n" % (name, c + 10_000_000) +   # end clamped to 2^31 - 1 (nothing lies there)
                     "chrUn_gl000222\t5\t6\r\n")
    clean = tmp_path / "clean.bed"
    clean.write_text("%s\t%d\t%d\n%s\t%d\t%d\n" % (name, a, a + 450, name, b, b + 500))
    got_messy, err_messy = dump_rows(["--exclude", str(messy), "inv_del_bam_config"], CHR21)
    got_clean, err_clean = dump_rows(["--exclude", str(clean), "inv_del_bam_config"], CHR21)
    want, drop = masked_dump(base, [(t, a, a + 450), (t, b, b + 500)])
    assert 0 < drop.sum() < len(base) and len(want) == len(base) - drop.sum()
    assert got_messy == want and got_clean == want
    assert excluded_count(err_messy) == (int(drop.sum()), 3, 2)
    assert excluded_count(err_clean) == (int(drop.sum()), 2, 0)


def case_intervals(rows, rng, targets):
    """a mask made from the dump itself: windows around some records' own positions, one interval that holds no read, one on a
    sequence without any other interval ... and overlapping / touching duplicates"""
    tid, pos, mtid, mpos = columns(rows)
    iv = []
    for i in rng.choice(len(rows), size=max(4, len(rows) // 60), replace=False):
        iv.append((int(tid[i]), max(0, int(pos[i]) - int(rng.integers(0, 200))), int(pos[i]) + int(rng.integers(1, 200))))
    i = int(rng.integers(0, len(rows)))
    iv.append((int(tid[i]), int(pos[i]), int(pos[i]) + 1))           # pos == beg == end - 1
    iv.append((int(tid[i]), int(pos[i]) + 1, int(pos[i]) + 40))      # touches it
    iv.append((len(targets) - 1, 0, 500))                            # holds no read (positions start at 1,000 / cluster centres at 2,000)
    iv.append(iv[0])                                                 # a duplicate
    return iv


@pytest.mark.parametrize("seed", [1210, 1211, 1212])
def test_host_readers_drop_exactly_the_records_the_rule_marks(tmp_path, seed):
    """bdx-dump-reads --exclude == the dump without the option minus the rows numpy marks (removed per file, the files merged again:
    exclude_cases.masked_dump says why), through produce (the k-way merge of
    ColumnReader's chunks), through produce_merged_by_columns (BDX_DUMP_MERGE=1), with -o c2, and with pieces of one BGZF block (every piece
    decoded from a guessed boundary, many of them a second time); the count on stderr is the number of rows removed"""
    rng = np.random.default_rng(seed)
    cfg, streams, targets = make_case(seed)
    write_case(str(tmp_path), streams, targets, rng, index=bool(seed % 2))
    (tmp_path / "cfg").write_text(cfg)
    base, _ = dump_rows(["cfg"], str(tmp_path))
    iv = case_intervals(base, rng, targets)
    write_bed(str(tmp_path / "m.bed"), iv, targets, rng, extra_lines=["chrUn_x\t0\t10", "# comment"])
    for args, env in (([], {}), ([], {"BDX_DUMP_MERGE": "1"}), (["-o", "c2"], {}), (["-o", "c2"], {"BDX_DUMP_MERGE": "1"}),
                      ([], {"BDX_BAM_PIECE_BLOCKS": "1"}), (["-o", "c2:9000-21000"], {"BDX_BAM_PIECE_BLOCKS": "1"})):
        plain, _ = dump_rows(args + ["cfg"], str(tmp_path), env)
        want, drop = masked_dump(plain, iv)
        assert drop.any() and not drop.all(), (args, env)          # the mask drops at least one record and keeps at least one
        masked, err = dump_rows(args + ["--exclude", "m.bed", "cfg"], str(tmp_path), env)
        assert masked == want, (args, env)
        removed = [l for l, d in zip(plain, drop) if not d]
        assert sorted(masked) == sorted(removed)                   # the unmasked dump with the marked rows removed, up to the order of ties
        assert excluded_count(err) == (int(drop.sum()), n_merged(iv), 1), (args, env)
    # a hit through the mate alone is among them: a record outside every interval whose mate starts in one
    tid, pos, mtid, mpos = columns(base)
    merged = merge_intervals(iv)
    own = rule_mask(tid, pos, np.full(len(tid), -1), mpos, iv)
    assert (rule_mask(tid, pos, mtid, mpos, iv) & ~own).any() and merged


def test_a_mask_on_no_known_sequence_changes_nothing(tmp_path):
    (tmp_path / "m.bed").write_text("chrUn_a\t0\t100000000\nchrUn_b\t5\t6\n")
    base, _ = dump_rows(["inv_del_bam_config"], CHR21)
    got, err = dump_rows(["--exclude", str(tmp_path / "m.bed"), "inv_del_bam_config"], CHR21)
    assert got == base and excluded_count(err) == (0, 0, 2)
