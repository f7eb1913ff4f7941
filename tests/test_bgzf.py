"""CPU tests of the host's one BGZF/BAM container parser (breakdancer_amd/host/bgzf.h) through `bin/bdx-inflate-check --members`
and the two command-line tools that read whole files with it (bin/bdx-dump-reads, bin/bam2cfg): the members it finds against the
independent Python parser (breakdancer_amd/bamdec.py scan_bgzf), that nothing behind the bytes it may look at changes what it says,
what the tools do with files cut at every kind of place, and the walk of the BAM header to the first record."""
import os
import struct
import subprocess
import sys
import zlib

import numpy as np
import pytest

from helpers import GOLDEN, ROOT, read_bam

CHECK = os.path.join(ROOT, "bin", "bdx-inflate-check")
DUMP = os.path.join(ROOT, "bin", "bdx-dump-reads")
BAM2CFG = os.path.join(ROOT, "bin", "bam2cfg")
EOF_MARKER = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
# a gzip header with FEXTRA whose 8-byte extra field holds an empty subfield and then the first four bytes of a BC subfield: the two
# bytes of its BSIZE would lie behind the extra field (and here behind the header)
CRAFTED = bytes.fromhex("1f8b08040000000000ff0800") + b"XX\0\0" + b"BC\x02\0"
RGS = [("rgA", "libA", "illumina"), ("rgB", "libB", "illumina")]
CFG = "".join("readgroup:%s\tplatform:illumina\tmap:h.bam\treadlen:100.00\tlib:%s\tnum:10001\tlower:200.00\tupper:600.00\tmean:400.00\tstd:30.00\n" % (r, l)
              for r, l, _ in RGS)
MESSAGES = ("truncated BGZF file", "truncated BAM record", "is not a valid bam file", "corrupt")


def member(data, pad=None, level=1):
    """one BGZF member; pad: an extra subfield of that many bytes in front of BC (the member grows by 4 + pad bytes)"""
    co = zlib.compressobj(level, zlib.DEFLATED, -15)
    comp = co.compress(data) + co.flush()
    extra = b"" if pad is None else b"XX" + struct.pack("<H", pad) + bytes(pad)
    xlen = len(extra) + 6
    total = 12 + xlen + len(comp) + 8
    assert total <= 65536
    return (b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff" + struct.pack("<H", xlen) + extra + b"BC\x02\x00" + struct.pack("<H", total - 1) + comp +
            struct.pack("<II", zlib.crc32(data) & 0xFFFFFFFF, len(data)))


def members_of(raw, chunk=65280):
    return [member(raw[i:i + chunk]) for i in range(0, len(raw), chunk)]


def bam_header(targets):
    text = "@HD\tVN:1.0\tSO:coordinate\n" + "".join("@SQ\tSN:%s\tLN:%d\n" % (t, 300000000) for t in targets) + \
           "".join("@RG\tID:%s\tPL:%s\tLB:%s\tSM:s\n" % (r, p, l) for r, l, p in RGS)
    out = b"BAM\1" + struct.pack("<i", len(text)) + text.encode() + struct.pack("<i", len(targets))
    for t in targets:
        out += struct.pack("<i", len(t) + 1) + t.encode() + b"\0" + struct.pack("<i", 300000000)
    return out


@pytest.fixture(scope="module")
def records(tmp_path_factory):
    """the records of the two-library case of tests/test_bam2cfg.py as BAM record bytes, one bytes object per record"""
    import gzip
    sys.path.insert(0, GOLDEN)
    from make_bam2cfg_vectors import two_library_records
    from breakdancer_amd.bamwrite import write_bam_records
    recs, rgs = two_library_records()
    assert rgs == RGS
    path = str(tmp_path_factory.mktemp("bgzf") / "two.bam")
    write_bam_records(path, recs, ["c1"], rgs=rgs)
    raw = gzip.decompress(open(path, "rb").read())
    o = len(bam_header(["c1"]))
    out = []
    while o < len(raw):
        n = 4 + struct.unpack_from("<i", raw, o)[0]
        out.append(raw[o:o + n])
        o += n
    assert o == len(raw) and len(out) == len(recs)
    return out


def run_members(path, avail=None):
    p = subprocess.run([CHECK, "--members", path] + ([str(avail)] if avail is not None else []), capture_output=True, text=True)
    assert p.returncode == 0, (p.returncode, p.stderr)
    lines = p.stdout.splitlines()
    assert lines and lines[-1].startswith("end ")
    end = lines[-1].split()
    return [tuple(int(x) for x in l.split()) for l in lines[:-1]], int(end[1]), end[2], p.stdout


def dump_reads(directory):
    """bin/bdx-dump-reads on directory/cfg -> (return code, stderr, the first eight columns and the library column of every record)"""
    p = subprocess.run([DUMP, "cfg"], cwd=directory, capture_output=True, text=True)
    rows = [[int(x) for x in l.split("\t")[:9]] for l in p.stdout.splitlines() if not l.startswith("#")]
    return p.returncode, p.stderr, np.array(rows, dtype=np.int64).reshape(-1, 9), p.stdout


def expected_rows(path):
    """the same columns from the independent Python decode (helpers.read_bam: the reader filter applied)"""
    _, r = read_bam(path)
    lib = np.array([[g for g, _, _ in RGS].index(g) for g in r["rg"]], dtype=np.int64)
    cols = [r[k].astype(np.int64) for k in ("tid", "pos", "mtid", "mpos", "isize", "flag", "qlen", "bdqual")] + [lib]
    return np.stack(cols, axis=1).reshape(-1, 9)


def last_record_is_whole(path):
    """does the chain of block_size words end with the inflated bytes?  (helpers.read_bam slices, and would decode a cut record)"""
    import gzip
    raw = gzip.decompress(open(path, "rb").read())
    o = len(bam_header(["c1"]))
    while o + 4 <= len(raw):
        o += 4 + struct.unpack_from("<i", raw, o)[0]
    return o == len(raw)


def write_case(directory, image):
    os.makedirs(directory, exist_ok=True)
    open(os.path.join(directory, "h.bam"), "wb").write(image)
    open(os.path.join(directory, "cfg"), "w").write(CFG)
    return os.path.join(directory, "h.bam")


# ---- 1. the same members as the independent parser ------------------------------------------------------------------------------------

def check_against_scan_bgzf(path):
    from breakdancer_amd.bamdec import scan_bgzf
    image = open(path, "rb").read()
    want = scan_bgzf(image)
    got, end, status, _ = run_members(path)
    assert len(got) == len(want) and len(got) > 1
    for (off, total, payload_off, payload_len, ulen), w, nxt in zip(got, want, [int(x) for x in want["member"][1:]] + [len(image)]):
        assert (off, off + payload_off, payload_len, ulen) == (int(w["member"]), int(w["payload"]), int(w["payload_len"]), int(w["inflated_len"]))
        assert off + total == nxt and total == payload_off + payload_len + 8
    assert (end, status) == (len(image), "end")
    assert got[-1][4] == 0 and image[got[-1][0]:] == EOF_MARKER   # (the EOF marker is a member like any other)


@pytest.mark.parametrize("name", ["NA19238_chr21_del_inv.bam", "NA19240_chr21_del_inv.bam"])
def test_members_of_the_golden_bams_equal_the_python_parser(name):
    check_against_scan_bgzf(os.path.join(GOLDEN, "chr21", name))


def test_members_of_a_synthetic_bam_equal_the_python_parser(tmp_path):
    from breakdancer_amd.bamwrite import write_bam
    from breakdancer_amd.synth import make_chromosome
    path = write_bam(str(tmp_path / "syn.bam"), make_chromosome(length=40000, seed=7), ["chrS"], seed=2)
    assert os.path.getsize(path) > 3 * 65536
    check_against_scan_bgzf(path)


def test_members_with_a_longer_extra_field(tmp_path):
    """a subfield in front of BC, of 0 and of 300 bytes: the walk skips it (scan_bgzf agrees)"""
    path = str(tmp_path / "x.bgzf")
    open(path, "wb").write(member(b"abc" * 1000, pad=0) + member(b"defg" * 500, pad=300) + member(b"h" * 70) + EOF_MARKER)
    check_against_scan_bgzf(path)
    assert [m[2] for m in run_members(path)[0]] == [22, 322, 18, 18]


# ---- 2. nothing behind `avail` matters ---------------------------------------------------------------------------------------------------

def cuts_in(off, image_member):
    """every byte position of a member's header and footer, a stride through its payload; relative to the file"""
    n = len(image_member)
    inside = set(range(1, min(n, 40))) | set(range(40, n, 997)) | set(range(max(1, n - 10), n))
    return sorted(off + c for c in inside)


@pytest.fixture(scope="module")
def cut_case(records):
    """header | records, whole | records, the last one cut | the rest | EOF marker -- the second member of records carries a subfield that
    makes the file offset 14 bytes into the header of the third a multiple of 4096"""
    a, last = b"".join(records[:200]), records[399]
    b = b"".join(records[200:399]) + last[:len(last) // 2]
    c = last[len(last) // 2:] + b"".join(records[400:600])
    parts = [member(bam_header(["c1"])), member(a)]
    before = sum(len(x) for x in parts) + len(member(b, pad=0))
    grow = (-(before + 14)) % 4096
    parts += [member(b, pad=grow), member(c), EOF_MARKER]
    offs = np.concatenate([[0], np.cumsum([len(x) for x in parts])]).tolist()
    assert (offs[3] + 14) % 4096 == 0
    cuts = offs[1:5] + cuts_in(offs[3], parts[3]) + cuts_in(offs[4], parts[4])
    return b"".join(parts), offs, cuts


TAILS = (bytes(64), b"BC\x02\x00" + b"\xff" * 60)


def test_bytes_behind_avail_do_not_change_the_parse(tmp_path, cut_case):
    image, offs, cuts = cut_case
    assert len(cuts) > 100 and any(n % 4096 == 0 for n in cuts)
    for n in cuts:
        outs = []
        for i, tail in enumerate(TAILS):
            path = str(tmp_path / ("t%d" % i))
            open(path, "wb").write(image[:n] + tail)
            outs.append(run_members(path, n))
        assert outs[0][3] == outs[1][3], n
        got, end, status, _ = outs[0]
        whole = [o for o in offs if o <= n]   # the members that lie in front of the cut, and nothing else
        assert [m[0] for m in got] == whole[:-1] and end == whole[-1] and all(m[0] + m[1] <= n for m in got), n
        assert status == ("end" if n in offs else "need-bytes"), (n, status)


def test_crafted_header_behind_avail(tmp_path):
    """a BC subfield whose BSIZE lies behind the extra field is no BC subfield, whatever stands there"""
    first = member(b"x" * 100)
    for k in range(len(CRAFTED) + 1):
        n = len(first) + k
        outs = []
        for i, tail in enumerate(TAILS):
            path = str(tmp_path / ("t%d" % i))
            open(path, "wb").write(first + CRAFTED + tail)
            outs.append(run_members(path, n))
        assert outs[0][3] == outs[1][3], k
        got, end, status, _ = outs[0]
        assert [m[:2] for m in got] == [(0, len(first))] and end == len(first)
        assert status == ("end" if k == 0 else "need-bytes" if k < len(CRAFTED) else "no-bc-field"), (k, status)


# ---- 3. the tools say so, and never die of a signal --------------------------------------------------------------------------------------

def test_cut_files_are_reported_not_crashed_on(tmp_path, cut_case):
    image, offs, cuts = cut_case
    d = str(tmp_path)
    for n in cuts:
        path = write_case(d, image[:n])
        rc, err, rows, _ = dump_reads(d)
        b2c = subprocess.run([BAM2CFG, "h.bam"], cwd=d, capture_output=True, text=True)
        assert b2c.returncode in (0, 1) and (b2c.returncode == 0 or any(m in b2c.stderr for m in MESSAGES)), (n, b2c.returncode, b2c.stderr)
        if n not in offs:
            assert rc == 1 and any(m in err for m in MESSAGES), (n, rc, err)
            continue
        # between two members: a well-formed BGZF file without its EOF marker -- all records that end before the cut, or a record cut
        want = expected_rows(path) if last_record_is_whole(path) else None
        assert (want is None) == (n == offs[3]), n
        if want is None:
            assert rc == 1 and "truncated BAM record" in err, (n, rc, err)
        else:
            assert rc == 0 and np.array_equal(rows, want) and len(rows) == {offs[1]: 0, offs[2]: 200, offs[4]: 600}[n], (n, rc, err)


def test_crafted_header_at_the_end_of_the_last_page(tmp_path, records):
    """the file ends with the crafted header and with a page of the mapping: the two bytes behind it are not there to be read"""
    parts = [member(bam_header(["c1"])), member(b"".join(records[:100]), pad=0)]
    grow = (-(sum(len(x) for x in parts) + len(CRAFTED))) % 4096
    parts[1] = member(b"".join(records[:100]), pad=grow)
    image = b"".join(parts) + CRAFTED
    assert len(image) % 4096 == 0
    d = str(tmp_path)
    write_case(d, image)
    rc, err, _, _ = dump_reads(d)
    assert rc == 1 and "BGZF block without BC field" in err, (rc, err)
    p = subprocess.run([BAM2CFG, "h.bam"], cwd=d, capture_output=True, text=True)
    assert p.returncode == 1 and "BGZF block without BC field" in p.stderr, (p.returncode, p.stderr)


# ---- 4. the header walk ------------------------------------------------------------------------------------------------------------------

# what the tools printed for these files before the container parser became one (commit ddf0b3b), with exit status 0: for the two
# header-only files the same, and for the three shapes of header the same
HEADER_ONLY_DUMP = ("#w0=200 nlibs=2 nbams=1 n=0\n#lib\t0\tlibA\th.bam\t0\t400\t30\t600\t200\t100\t-1\n"
                    "#lib\t1\tlibB\th.bam\t0\t400\t30\t600\t200\t100\t-1\n")
HEADER_ONLY_BAM2CFG = ""
THREE_SHAPES_BAM2CFG = ("readgroup:rgA\tplatform:illumina\tmap:h.bam\treadlen:100.00\tlib:libA\tnum:3736\tlower:219.23\tupper:381.46\tmean:300.08\tstd:20.28"
                        "\tSWnormality:-0.71\texe:samtools view\n"
                        "readgroup:rgB\tplatform:illumina\tmap:h.bam\treadlen:100.00\tlib:libB\tnum:3738\tlower:306.98\tupper:593.35\tmean:449.99\tstd:35.79"
                        "\tSWnormality:-0.19\texe:samtools view\n")


@pytest.mark.parametrize("eof_marker", [False, True])
def test_a_bam_that_is_only_a_header(tmp_path, eof_marker):
    d = str(tmp_path)
    write_case(d, member(bam_header(["c1"])) + (EOF_MARKER if eof_marker else b""))
    rc, err, rows, out = dump_reads(d)
    assert (rc, out, len(rows)) == (0, HEADER_ONLY_DUMP, 0), (rc, err, out)
    p = subprocess.run([BAM2CFG, "h.bam"], cwd=d, capture_output=True, text=True)
    assert (p.returncode, p.stdout) == (0, HEADER_ONLY_BAM2CFG), (p.returncode, p.stderr)


def header_shapes(records):
    body = b"".join(records)
    short, long_ = bam_header(["c1"]), bam_header(["c1"] + ["contig_%05d_of_a_fragmented_assembly" % i for i in range(1450)])
    assert 2 * 65280 < len(long_) < 3 * 65280
    return {"at_a_member_boundary": members_of(short) + members_of(body),
            "inside_a_member": members_of(short + body),
            "three_members": members_of(long_ + body)}


@pytest.mark.parametrize("shape", ["at_a_member_boundary", "inside_a_member", "three_members"])
def test_where_the_header_ends(tmp_path, records, shape):
    d = str(tmp_path)
    path = write_case(d, b"".join(header_shapes(records)[shape]) + EOF_MARKER)
    rc, err, rows, _ = dump_reads(d)
    want = expected_rows(path)
    assert rc == 0 and len(want) == len(records) and np.array_equal(rows, want), (rc, err)
    p = subprocess.run([BAM2CFG, "h.bam"], cwd=d, capture_output=True, text=True)
    assert (p.returncode, p.stdout) == (0, THREE_SHAPES_BAM2CFG), (p.returncode, p.stderr)
