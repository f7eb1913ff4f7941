"""GPU tests of --exclude: the standalone kernel (bdx_exclude_mask) against numpy, the decoder's fused test (bdx_bamdec_set_exclude /
bdx_bamdec_excluded) against the unmasked decode with the marked rows removed, and bin/breakdancer-max --exclude on every route against
the oracle's rendering of the streams WITHOUT the marked records -- the run with the mask must print what the run prints on files from
which those records were removed.  Every comparison is exact."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from exclude_cases import (excluded_count, mask_from_table, mask_streams, n_merged, rewrite_bam_without, rule_mask, table_rows, write_bed,
                           write_case)
from fuzzgen import make_case
from helpers import ROOT, filter_cmd_lines, make_opts
from runner import oracle_case

pytestmark = pytest.mark.gpu
EXE = os.path.join(ROOT, "bin", "breakdancer-max")
BDX_EINVAL, BDX_ESTATE, BDX_ELIMIT = 1, 4, 5


# ---- 1. kernel level ----
def intervals_with(m, rng):
    """a list of intervals on sequences 0 and 2 (1 has none) whose union is exactly m intervals: m disjoint, non-touching ones, given
    out of order together with overlapping, touching, contained and empty extras"""
    base = []
    at = [50, 50]
    for k in range(m):
        s = int(rng.integers(0, 2))
        b = at[s] + int(rng.integers(2, 40))
        e = b + int(rng.integers(1, 60))
        base.append((0 if s == 0 else 2, b, e))
        at[s] = e
    extra = []
    for t, b, e in base[::3]:
        mid = (b + e) // 2
        extra += [(t, b, mid), (t, mid, e), (t, b, e), (t, b, b)]   # two that touch, a duplicate, an empty one -- the union is unchanged
    if base and base[-1][2] - base[-1][1] > 2:
        extra.append((base[-1][0], base[-1][1] + 1, base[-1][2] - 1))   # one inside another
    extra.append((1, 7, 7))   # an empty one on the sequence that has none
    iv = base + extra
    iv = [iv[i] for i in rng.permutation(len(iv))]
    assert n_merged(iv) == m
    return iv


def records_near(iv, n, rng):
    """n records over tids -1 .. 4 (the mask knows 0 .. 2), positions around the intervals' edges and elsewhere, sorted like a BAM"""
    edges = np.array(sorted({x for _, b, e in iv for x in (b - 1, b, b + 1, e - 1, e, e + 1)} | {0, 1, 49}), dtype=np.int64)
    def col():
        tid = rng.integers(-1, 5, n)
        pos = np.where(rng.random(n) < 0.6, rng.choice(edges, n), rng.integers(-1, int(edges.max()) + 200, n))
        return tid.astype(np.int32), pos.astype(np.int32)
    tid, pos = col()
    order = np.lexsort((pos, tid))
    mtid, mpos = col()
    return tid[order], pos[order], mtid, mpos


@pytest.mark.parametrize("m", [0, 1, 2, 3, 64, 65, 1000])
def test_exclude_mask_kernel_equals_numpy(m):
    from breakdancer_amd import bamdec
    rng = np.random.default_rng(100 + m)
    iv = intervals_with(m, rng)
    for n in (0, 1, 63, 64, 65, 5000):
        tid, pos, mtid, mpos = records_near(iv, n, rng)
        got = bamdec.exclude_mask(tid, pos, mtid, mpos, iv)
        want = rule_mask(tid, pos, mtid, mpos, iv)
        assert got.dtype == np.uint8 and got.shape == (n,)
        np.testing.assert_array_equal(got.astype(bool), want, err_msg="m=%d n=%d" % (m, n))
        if m >= 3 and n == 5000:
            assert want.any() and not want.all()


def test_exclude_mask_edges_placed_by_hand():
    from breakdancer_amd import bamdec
    # sequence 0: [100, 200) given as two overlapping and one touching piece, [300, 301); sequence 1: nothing; sequence 2: [0, 10) and the
    # slice's last interval [5000, 2^31 - 1)
    iv = [(0, 150, 200), (2, 5000, 0x7FFFFFFF), (0, 100, 160), (0, 300, 301), (2, 0, 10), (0, 120, 150), (0, 400, 400)]
    cases = [  # tid, pos, mtid, mpos, dropped
        (0, 100, -1, -1, 1),        # pos == beg
        (0, 199, -1, -1, 1),        # pos == end - 1
        (0, 200, -1, -1, 0),        # pos == end
        (0, 99, -1, -1, 0),         # pos == beg - 1
        (0, 160, -1, -1, 1),        # where two input intervals overlap
        (0, 150, -1, -1, 1),        # where two input intervals touch
        (0, 300, 0, 301, 1),        # an interval of one base, the first ... (mate just behind it)
        (0, 301, 0, 299, 0),        # ... and both sides of it
        (0, 400, 0, 400, 0),        # an empty interval drops nothing
        (1, 150, 1, 150, 0),        # a sequence without intervals
        (1, 150, 0, 150, 1),        # a hit through the mate only
        (0, 50, 2, 9, 1),           # the mate in the first interval of its slice
        (0, 50, 2, 10, 0),
        (0, 50, 2, 5000, 1),        # ... and in the last
        (2, 0x7FFFFFFE, -1, 0, 1),  # the last base a clamped end covers
        (2, 4999, -1, 5000, 0),     # mtid == -1: the mate's position is not looked at
        (-1, 150, -1, 150, 0),
        (3, 150, 7, 150, 0),        # tid / mtid beyond the mask's sequences
        (3, 150, 0, 150, 1),
        (0, -1, 0, -1, 0),          # a position of -1
    ]
    a = np.array(cases, dtype=np.int64)
    got = bamdec.exclude_mask(a[:, 0], a[:, 1], a[:, 2], a[:, 3], iv)
    np.testing.assert_array_equal(got, a[:, 4].astype(np.uint8))
    np.testing.assert_array_equal(rule_mask(a[:, 0], a[:, 1], a[:, 2], a[:, 3], iv), a[:, 4].astype(bool))   # (the restatement agrees)
    # no interval at all: nothing is dropped
    assert not bamdec.exclude_mask(a[:, 0], a[:, 1], a[:, 2], a[:, 3], []).any()


def test_exclude_mask_argument_errors():
    from breakdancer_amd import bamdec
    lib = bamdec._lib()
    col = np.zeros(4, np.int32)
    out = np.zeros(4, np.uint8)
    cp = col.ctypes.data

    def call(iv, niv=None, cols=(cp, cp, cp, cp), mask=out.ctypes.data, n=4):
        a = bamdec.intervals_array(iv)
        return lib.bdx_exclude_mask(0, *cols, n, a.ctypes.data if len(a) else None, len(a) if niv is None else niv, mask)
    assert call([(0, 1, 2)]) == 0
    assert call([], niv=3) == BDX_EINVAL                      # a null array with a count
    assert call([(0, 1, 2), (-1, 1, 2)]) == BDX_EINVAL        # tid < 0
    assert call([(0, -1, 2)]) == BDX_EINVAL                   # beg < 0
    assert call([(0, 5, 4)]) == BDX_EINVAL                    # end < beg
    assert call([(0, 5, 5)]) == 0                             # (empty, not an error)
    assert call([(0, 1, 2)], cols=(cp, None, cp, cp)) == BDX_EINVAL
    assert call([(0, 1, 2)], mask=None) == BDX_EINVAL
    assert call([(1 << 24, 1, 2)]) == BDX_ELIMIT              # a table's first[] spans at most 2^24 sequences


# ---- 2. decoder level ----
COLS = ("tid", "pos", "mtid", "mpos", "isize", "flag", "qlen", "mapq", "lib", "bam", "name_key")   # the eleven columns (+ the second name hash)
RG = dict(rg_ids=["rg1", "rg2", "rg3"], rg_lib=[0, 1, 2], fallback_lib=2)


@pytest.fixture(scope="module")
def one_bam(tmp_path_factory):
    """~3,000 records over three sequences with secondary and supplementary copies among them, the unmasked decode and a mask"""
    from breakdancer_amd import bamdec
    d = tmp_path_factory.mktemp("exclude_dec")
    rng = np.random.default_rng(31)
    cfg, streams, targets = make_case(1231, n_pairs=2200)
    write_case(str(d), streams[:1], targets, rng)
    path = str(d / "a.bam")
    plain, names, _ = bamdec.decode_file(path, **RG)
    n = len(plain["tid"])
    assert names == targets and 2500 < n < 3500 and len(bamdec.scan_bgzf(np.fromfile(path, np.uint8))) > 6
    iv = [(int(plain["tid"][i]), max(0, int(plain["pos"][i]) - 150), int(plain["pos"][i]) + 150) for i in rng.choice(n, 40, replace=False)]
    iv += [(2, 0, 500), iv[0], (iv[1][0], iv[1][2], iv[1][2] + 30)]
    return path, plain, iv


def assert_rows_removed(got, plain, drop):
    assert len(got["tid"]) == int((~drop).sum())
    for k in COLS + ("name_check",):
        np.testing.assert_array_equal(got[k], plain[k][~drop], err_msg=k)


@pytest.mark.parametrize("piece_blocks,batch_blocks", [(512, 0), (2, 2), (3, 4)])
def test_decoder_drops_the_marked_records(one_bam, piece_blocks, batch_blocks):
    from breakdancer_amd import bamdec
    path, plain, iv = one_bam
    drop = rule_mask(plain["tid"], plain["pos"], plain["mtid"], plain["mpos"], iv)
    assert 50 < drop.sum() < len(drop) - 50
    own = rule_mask(plain["tid"], plain["pos"], np.full(len(drop), -1), plain["mpos"], iv)
    assert (drop & ~own).any()   # hits through the mate alone are among them
    got, _, stats = bamdec.decode_file(path, piece_blocks=piece_blocks, batch_blocks=batch_blocks, exclude=iv, **RG)
    if batch_blocks:
        assert stats["pieces"] >= 2   # several batches ran
    assert_rows_removed(got, plain, drop)
    assert stats["excluded"] == int(drop.sum())


def test_decoder_mask_survives_rearm_and_can_be_removed(one_bam):
    from breakdancer_amd import bamdec
    path, plain, iv = one_bam
    data = np.fromfile(path, dtype=np.uint8)
    members = bamdec.scan_bgzf(data)
    names, lens, k, off = bamdec.bam_header(data, members)
    lib = bamdec._lib()
    d = bamdec.BamDecoder(len(names), first_record_offset=off, region=(1, 0, 1 << 29), batch_blocks=3, exclude=iv, **RG)
    try:
        for t in (1, 2):
            if t == 2:
                d.rearm(region=(2, 0, 1 << 29), first_record_offset=off)
            d.feed(data, members[k:], 2)
            a = bamdec.intervals_array(iv)
            assert lib.bdx_bamdec_set_exclude(d.h, a.ctypes.data, len(a)) == BDX_ESTATE   # a setter after the first submit
            d.finish()
            on_t = plain["tid"] == t   # (every record has a CIGAR that covers bases: the whole sequence is the region)
            drop = rule_mask(plain["tid"], plain["pos"], plain["mtid"], plain["mpos"], iv)
            assert (drop & on_t).any() and (~drop & on_t).any()
            got = d.fetch()
            sub = {c: plain[c][on_t] for c in plain}
            assert_rows_removed(got, sub, drop[on_t])
            assert d.excluded() == int((drop & on_t).sum())   # the count starts over with the re-arming
        # n == 0 removes the mask: armed again, the decoder gives the unmasked records
        d.rearm(first_record_offset=off)
        d.set_exclude([])
        d.feed(data, members[k:], 512)
        d.finish()
        assert_rows_removed(d.fetch(), plain, np.zeros(len(plain["tid"]), bool))
        assert d.excluded() == 0
    finally:
        d.close()
    # the setter's argument errors
    d = bamdec.BamDecoder(len(names), first_record_offset=off, **RG)
    try:
        bad = bamdec.intervals_array([(0, 5, 4)])
        assert lib.bdx_bamdec_set_exclude(d.h, bad.ctypes.data, 1) == BDX_EINVAL
        assert lib.bdx_bamdec_set_exclude(d.h, None, 2) == BDX_EINVAL
        assert lib.bdx_bamdec_set_exclude(d.h, bamdec.intervals_array([(-1, 1, 2)]).ctypes.data, 1) == BDX_EINVAL
        assert lib.bdx_bamdec_set_exclude(d.h, bamdec.intervals_array([(0, -1, 2)]).ctypes.data, 1) == BDX_EINVAL
        n = C.c_uint64(0)
        assert lib.bdx_bamdec_excluded(d.h, C.byref(n)) == BDX_ESTATE   # before bdx_bamdec_finish
    finally:
        d.close()


# ---- 3. the CLI against the oracle on masked input ----
ROUTES = [("device", dict()), ("device-small-pieces", dict(BDX_BAM_PIECE_BYTES="50000", BDX_BAM_BATCH_BLOCKS="2")), ("host", dict(BDX_DECODE="host")),
          ("two-ranks", dict(BDX_GPUS="0,0"))]
FLAGS = [([], dict()), (["-o", "c2"], dict(chr_tid=1)), (["-a", "-h"], dict(cn_lib=1, print_af=1))]


def run_cli(args, cwd, env=None):
    p = subprocess.run([EXE] + args, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=dict(os.environ, BDX_TIMING="1", **(env or {})))
    return p.returncode, p.stdout.decode(), p.stderr.decode()


@pytest.mark.parametrize("flags", range(len(FLAGS)), ids=["default", "o-c2", "a-h"])
@pytest.mark.parametrize("seed", [1200, 1201, 1203])
def test_cli_with_exclude_equals_oracle_on_masked_streams(tmp_path, seed, flags):
    rng = np.random.default_rng(seed)
    cfg, streams, targets = make_case(seed)
    indexed = seed != 1201   # (without .bai files -o reads the whole file, and a sharded run is fed by the host reader)
    write_case(str(tmp_path), streams, targets, rng, index=indexed)
    (tmp_path / "cfg").write_text(cfg)
    unmasked = oracle_case(cfg, streams, targets, make_opts(score_threshold=-1))
    iv = mask_from_table(unmasked.text, targets, rng)
    write_bed(str(tmp_path / "m.bed"), iv, targets, rng, extra_lines=["chrUn_gl000220\t0\t90000"])
    masked, removed = mask_streams(streams, iv)
    args, kw = FLAGS[flags]
    opts = make_opts(score_threshold=-1, **kw)
    want = oracle_case(cfg, masked, targets, opts).text
    plain = oracle_case(cfg, streams, targets, opts).text
    # the mask is not vacuous: it changes the text (the library statistics among it) and leaves rows
    stats = lambda t: [l for l in t.splitlines() if l.startswith("#") and "mean:" in l]
    assert filter_cmd_lines(want) != filter_cmd_lines(plain) and stats(want) != stats(plain) and table_rows(want)
    # R: the records that passed the reader filter and the -o test and were then dropped
    in_region = lambda st: np.ones(len(st["tid"]), bool) if "-o" not in args else np.asarray(st["tid"]) == 1
    r_want = sum(int((rule_mask(st["tid"], st["pos"], st["mtid"], st["mpos"], iv) & in_region(st)).sum()) for st in streams)
    assert 0 < r_want <= sum(removed) < sum(len(st["tid"]) for st in streams)
    print("seed %d %s: %d of %d records removed, %d of %d rows left" % (seed, args, sum(removed), sum(len(st["tid"]) for st in streams),
                                                                       len(table_rows(want)), len(table_rows(plain))))
    for label, env in ROUTES:
        rc, out, err = run_cli(["-y", "-1"] + args + ["--exclude", "m.bed", "cfg"], str(tmp_path), env)
        assert rc == 0, (label, err)
        on_gpu = label != "host" and (indexed or label != "two-ranks" or "-o" in args)
        assert ("on the GPU" in err or "on its own GPU" in err) == on_gpu, (label, err)   # (no silent hand-over to the host reader)
        assert filter_cmd_lines(out) == filter_cmd_lines(want), (label, args, err)
        assert excluded_count(err) == (r_want, n_merged(iv), 1), (label, args)
    # without the option nothing changes
    rc, out, err = run_cli(["-y", "-1"] + args + ["cfg"], str(tmp_path))
    assert rc == 0 and filter_cmd_lines(out) == filter_cmd_lines(plain) and "excluded" not in err


def test_cli_file_the_device_path_gives_up_is_masked_by_the_host_reader(tmp_path):
    """one secondary record of 4.5 MB among ordinary ones: the device decode gives the file up after its record stages have counted
    dropped records; the host reader takes it from the start -- the oracle's text on the masked stream, and R counted once"""
    from breakdancer_amd.bamwrite import write_bam_records
    seed = 1205
    rng = np.random.default_rng(seed)
    cfg, streams, targets = make_case(seed)
    cfg1 = "".join(l + "\n" for l in cfg.splitlines() if "map:a.bam" in l)
    st = streams[0]
    recs = [dict(tid=st["tid"][i], pos=st["pos"][i], mtid=st["mtid"][i], mpos=st["mpos"][i], isize=st["isize"][i], flag=st["flag"][i], qlen=st["qlen"][i],
                 mapq=int(st["bdqual"][i]), am=None, rg=st["rg"][i], name="read%d" % int(st["name_id"][i])) for i in range(len(st["tid"]))]
    big = dict(recs[2 * len(recs) // 3])
    big["qlen"] = 3_000_000
    big["flag"] = int(big["flag"]) | 0x100   # (secondary: the reader filter drops it)
    recs.insert(2 * len(recs) // 3, big)
    write_bam_records(str(tmp_path / "a.bam"), recs, targets, rgs=("rg1", "rg2", "rg3"), seed=1)
    (tmp_path / "cfg").write_text(cfg1)
    unmasked = oracle_case(cfg1, streams[:1], targets, make_opts(score_threshold=-1))
    iv = mask_from_table(unmasked.text, targets, rng)
    write_bed(str(tmp_path / "m.bed"), iv, targets, rng)
    masked, removed = mask_streams(streams[:1], iv)
    want = oracle_case(cfg1, masked, targets, make_opts(score_threshold=-1)).text
    assert removed[0] > 0 and table_rows(want) and filter_cmd_lines(want) != filter_cmd_lines(unmasked.text)
    for label, env in (("default", dict()), ("host", dict(BDX_DECODE="host"))):
        rc, out, err = run_cli(["-y", "-1", "--exclude", "m.bed", "cfg"], str(tmp_path), env)
        assert rc == 0, (label, err[-600:])
        assert "host decode threads" in err, (label, err[-600:])
        assert filter_cmd_lines(out) == filter_cmd_lines(want), label
        assert excluded_count(err)[0] == removed[0], label


# ---- 4. dumps and cache, 5. --vcf ----
@pytest.fixture()
def one_bam_case(tmp_path):
    """one BAM of a fuzz case, a mask from the oracle's unmasked table, and the same BAM written again without the marked records"""
    seed = 1204
    rng = np.random.default_rng(seed)
    cfg, streams, targets = make_case(seed)
    cfg1 = "".join(l + "\n" for l in cfg.splitlines() if "map:a.bam" in l)
    write_case(str(tmp_path), streams[:1], targets, rng)
    (tmp_path / "cfg").write_text(cfg1)
    unmasked = oracle_case(cfg1, streams[:1], targets, make_opts(score_threshold=-1))
    iv = mask_from_table(unmasked.text, targets, rng)
    write_bed(str(tmp_path / "m.bed"), iv, targets, rng)
    rew = tmp_path / "rewritten"
    rew.mkdir()
    left_out = rewrite_bam_without(str(tmp_path / "a.bam"), str(rew / "a.bam"), iv)
    (rew / "cfg").write_text(cfg1)
    masked, removed = mask_streams(streams[:1], iv)
    assert left_out >= removed[0] > 0   # (the secondary / supplementary copies of marked records go as well)
    want = oracle_case(cfg1, masked, targets, make_opts(score_threshold=-1)).text
    assert table_rows(want) and filter_cmd_lines(want) != filter_cmd_lines(unmasked.text)
    return tmp_path, rew, want


def dump_files(args, cwd, out_dir, env):
    out_dir.mkdir()
    rc, out, err = run_cli(["-y", "-1", "-g", str(out_dir / "out.bed"), "-d", str(out_dir / "fq")] + args + ["cfg"], str(cwd), env)
    assert rc == 0, err
    return filter_cmd_lines(out), {f: open(os.path.join(str(out_dir), f), "rb").read() for f in sorted(os.listdir(str(out_dir)))}


def test_dumps_and_cache_with_exclude(one_bam_case):
    tmp, rew, want = one_bam_case
    dev = dump_files(["--exclude", "m.bed"], tmp, tmp / "dev", dict())
    host = dump_files(["--exclude", "m.bed"], tmp, tmp / "host", dict(BDX_DECODE="host"))
    ref = dump_files([], rew, tmp / "ref", dict())   # no mask, the file without the marked records
    assert dev[0] == host[0] == ref[0] == filter_cmd_lines(want)
    assert dev[1] == host[1] == ref[1] and dev[1] and any(len(v) for v in dev[1].values())
    # -C writes the command line into the cache; -R parses --exclude from it and reads the file again
    rc, out_c, err = run_cli(["-y", "-1", "-C", "c", "--exclude", "m.bed", "cfg"], str(tmp))
    assert rc == 0, err
    rc, out_r, err = run_cli(["-R", "c"], str(tmp))
    assert rc == 0, err
    assert filter_cmd_lines(out_c) == filter_cmd_lines(out_r) == filter_cmd_lines(want)
    assert excluded_count(err)[0] > 0
    os.rename(str(tmp / "m.bed"), str(tmp / "gone.bed"))   # a missing file is the ordinary error
    rc, out_r, err = run_cli(["-R", "c"], str(tmp))
    assert rc == 1 and "m.bed" in err


def test_vcf_with_exclude(one_bam_case):
    tmp, rew, want = one_bam_case
    rc, out, err = run_cli(["-y", "-1", "--vcf", "out.vcf", "--exclude", "m.bed", "cfg"], str(tmp))
    assert rc == 0 and filter_cmd_lines(out) == filter_cmd_lines(want), err
    rc, out, err = run_cli(["-y", "-1", "--vcf", "out.vcf", "cfg"], str(rew))
    assert rc == 0 and filter_cmd_lines(out) == filter_cmd_lines(want), err
    got = (tmp / "out.vcf").read_text().splitlines()
    ref = (rew / "out.vcf").read_text().splitlines()
    assert "##exclude=m.bed" in got and not [l for l in ref if l.startswith("##exclude")]
    body = lambda ls: [l for l in ls if not l.startswith("##")]
    assert body(got) == body(ref) and len(body(got)) > 1        # every record, DR and DV of every sample included
    assert any(f.split(":")[3] not in (".", "0") for l in body(got)[1:] for f in l.split("\t")[9:])   # (some DR is a count)
    meta = lambda ls: [l for l in ls if l.startswith("##") and not l.startswith(("##command=", "##exclude="))]
    assert meta(got) == meta(ref)
