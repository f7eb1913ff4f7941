"""CPU tests of the device decode's feeder, its pure parts (host/feed_plan.h) through bin/bdx-feed-check: the cut of a file into pieces of
whole BGZF members against the independent Python parser (breakdancer_amd.bamdec.scan_bgzf), the decoder's sizing plan against results
recorded from the code it was split out of (tests/golden/feed_plan.json), and the two-file tie rule at a chromosome's first position
against the reasoning of its comment.  Everything runs twice: on the Makefile's tool and on one built here with the address and
undefined-behaviour sanitizers (a stand-alone program: nothing is preloaded)."""
import json
import os
import struct
import subprocess

import numpy as np
import pytest

from helpers import GOLDEN, ROOT
from test_bgzf import EOF_MARKER, member

HOST = os.path.join(ROOT, "breakdancer_amd", "host")
GOLDEN_BAMS = [os.path.join(GOLDEN, "chr21", n) for n in ("NA19238_chr21_del_inv.bam", "NA19240_chr21_del_inv.bam")]
LEAD = 65536          # feed_plan.h's kLead: a piece begins at most that far in front of its own read offset
MAX_BLOCKS = 8 * 1024 * 1024 // 512 + 4096   # plan_decoder's piece_blocks at the default piece size


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def exe(request, tmp_path_factory):
    if request.param == "plain":
        plain = os.path.join(ROOT, "bin", "bdx-feed-check")
        if not os.path.exists(plain):
            subprocess.check_call(["make", "-C", ROOT, "bin/bdx-feed-check"], stdout=subprocess.DEVNULL)
        return plain
    san = str(tmp_path_factory.mktemp("san") / "bdx-feed-check-san")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                           "-I" + os.path.join(ROOT, "include"), "-o", san, os.path.join(HOST, "feed_check_main.cpp")])
    return san


def run(exe, args, env=None):
    e = {k: v for k, v in os.environ.items() if not k.startswith("BDX_")}
    e.update(ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    e.update(env or {})
    p = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, env=e)
    assert "Sanitizer" not in p.stderr and "runtime error" not in p.stderr, p.stderr
    return p


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """label -> path: the golden chr21 BAMs, test_producer.py's synthetic BAM, an indexed three-sequence BAM, and hand-built members with a
    longer extra field and empty members (flush blocks) in the middle"""
    from breakdancer_amd.bamwrite import write_bam
    from breakdancer_amd.synth import make_chromosome, make_genome
    d = tmp_path_factory.mktemp("feed")
    out = {"golden0": GOLDEN_BAMS[0], "golden1": GOLDEN_BAMS[1]}
    out["synthetic"] = write_bam(str(d / "syn.bam"), make_chromosome(length=300000, seed=5), ["chrS"], seed=1)
    out["indexed"] = write_bam(str(d / "three.bam"), make_genome([60000, 90000, 50000], coverage=30.0, seed=3), ["c1", "c2", "c3"], seed=2, index=True)
    rng = np.random.default_rng(7)
    noise = lambda n: rng.integers(0, 256, n, dtype=np.uint8).tobytes()   # (incompressible: the members are as large as their data)
    image = b"".join([member(noise(30000), pad=300), member(b"abc" * 1000, pad=0), member(b""), member(b"", pad=40), member(noise(60000)),
                      member(b"", pad=300), member(b"defg" * 500, pad=300), member(noise(50000), pad=7)] * 6) + EOF_MARKER
    out["padded"] = str(d / "padded.bgzf")
    open(out["padded"], "wb").write(image)
    return out


def parse_cut(stdout):
    """[(offset, bytes, nblocks, last, [(payload, payload_len, inflated_len), ...]), ...]"""
    pieces = []
    for l in stdout.splitlines():
        w = l.split()
        if w[0] == "piece":
            pieces.append((int(w[1]), int(w[2]), int(w[3]), int(w[4]), []))
        else:
            assert w[0] == "m"
            pieces[-1][4].append((int(w[1]), int(w[2]), int(w[3])))
    return pieces


def check_cut(exe, path, piece_bytes, begin=None, end=None):
    from breakdancer_amd.bamdec import scan_bgzf
    image = open(path, "rb").read()
    p = run(exe, ["cut", path, piece_bytes, MAX_BLOCKS] + ([begin, end] if end is not None else []))
    assert p.returncode == 0, p.stderr
    pieces = parse_cut(p.stdout)
    begin, end = (0, len(image)) if end is None else (begin, min(end, len(image)))
    # the pieces tile [begin, end) without gap or overlap; each begins at most 64 KiB before its own read offset
    at = begin
    for i, (off, nbytes, nblocks, last, ms) in enumerate(pieces):
        assert off == at and nblocks == len(ms)
        assert 0 <= begin + i * piece_bytes - off <= LEAD
        assert all(off < pay and pay + plen + 8 <= off + nbytes for pay, plen, _ in ms)   # (a member lies in the piece that lists it)
        at += nbytes
    assert [pc[3] for pc in pieces] == [0] * (len(pieces) - 1) + [1 if end == len(image) else 0]   # `last`: the piece that ends the file
    # every member that inflates to something, in order, each exactly once
    scan = scan_bgzf(image)
    starts = [int(m) for m in scan["member"]] + [len(image)]
    want = [(int(w["payload"]), int(w["payload_len"]), int(w["inflated_len"])) for w, nxt in zip(scan, starts[1:])
            if int(w["inflated_len"]) > 0 and int(w["member"]) >= begin and nxt <= end]
    assert [m for pc in pieces for m in pc[4]] == want and len(want) > 1
    if end == len(image):
        assert at == end
    else:   # nothing at or behind END is submitted; what is left over in front of it is the member that straddles END, cut
        assert at == max(s for s in starts if s <= end) and end - at < 65536
    return pieces


@pytest.mark.parametrize("piece", ["70000", "131072", "65537", "default", "file"])
@pytest.mark.parametrize("label", ["golden0", "golden1", "synthetic", "padded"])
def test_cut_equals_the_python_parser(exe, files, label, piece):
    path = files[label]
    size = os.path.getsize(path)
    pieces = check_cut(exe, path, {"default": 8 << 20, "file": size}.get(piece) or int(piece))
    if label == "synthetic":
        assert sum(pc[2] for pc in pieces) > 100    # (a few hundred members)
    if piece in ("default", "file") and size <= 8 << 20:
        assert len(pieces) == 1
    if piece == "70000":
        assert len(pieces) > 3 and any(pc[0] != i * 70000 for i, pc in enumerate(pieces))   # (members were carried over)


def bai_spans(path):
    """[begin, end) of the file per sequence as the .bai says (None: nothing indexed): the first chunk's member .. a member's worth behind
    the last chunk's"""
    d = open(path + ".bai", "rb").read()
    assert d[:4] == b"BAI\1"
    n_ref, = struct.unpack_from("<i", d, 4)
    p, out = 8, []
    for _ in range(n_ref):
        n_bin, = struct.unpack_from("<i", d, p)
        p += 4
        lo, hi = None, 0
        for _ in range(n_bin):
            b, n_chunk = struct.unpack_from("<Ii", d, p)
            p += 8
            for _ in range(n_chunk):
                cb, ce = struct.unpack_from("<QQ", d, p)
                p += 16
                if b != 37450:
                    lo, hi = cb if lo is None else min(lo, cb), max(hi, ce)
        n_intv, = struct.unpack_from("<i", d, p)
        p += 4 + 8 * n_intv
        out.append(None if lo is None else (lo >> 16, min(os.path.getsize(path), (hi >> 16) + 65536 + 28)))
    return out


@pytest.mark.parametrize("piece", [70000, 131072, 65537, 8 << 20])
@pytest.mark.parametrize("label", ["golden0", "golden1", "indexed"])
def test_cut_of_a_sequences_span_stops_at_its_end(exe, files, label, piece):
    path = files[label]
    spans = [s for s in bai_spans(path) if s]
    assert len(spans) == (3 if label == "indexed" else 1)
    if label == "indexed":
        assert spans[0][1] < os.path.getsize(path) and spans[1][0] > 65536   # (a span that ends, and one that begins, inside the file)
    for begin, end in spans:
        check_cut(exe, path, piece, begin, end)


def test_cut_errors(exe, files, tmp_path):
    image = open(files["padded"], "rb").read()
    cut_file = tmp_path / "cut.bgzf"
    cut_file.write_bytes(image[:100000])    # (mid-member: the members are 30 k, 3 k, ..., 60 k)
    for piece in (70000, 8 << 20):
        p = run(exe, ["cut", cut_file, piece, MAX_BLOCKS])
        assert p.returncode == 1 and p.stderr.strip() == "truncated BGZF file: %s" % cut_file, p.stderr
    p = run(exe, ["cut", files["padded"], 20000, MAX_BLOCKS])    # the first member takes 30 k
    assert p.returncode == 1 and p.stderr.strip() == "BGZF member larger than a piece: %s" % files["padded"], p.stderr
    p = run(exe, ["cut", files["padded"], 8 << 20, 3])
    assert p.returncode == 2 and p.stdout.splitlines()[-1] == "too many members", (p.stdout, p.stderr)
    p = run(exe, ["cut", files["padded"], 70000, 2])            # ... in a later piece: the pieces before it were cut
    assert p.returncode == 2 and p.stdout.splitlines()[-1] == "too many members" and p.stdout.startswith("piece 0 ")
    assert run(exe, ["cut", files["padded"], 8 << 20, 30]).returncode == 0   # (exactly as many as the file holds: empty members do not count)
    assert run(exe, ["cut", files["padded"], 8 << 20, 29]).returncode == 2
    plain = tmp_path / "plain.txt"
    plain.write_bytes(b"no BGZF member opens like this " * 100)
    p = run(exe, ["cut", plain, 70000, MAX_BLOCKS])
    assert p.returncode == 1 and p.stderr.strip() == "not a BGZF file: %s" % plain, p.stderr
    p = run(exe, ["cut", tmp_path / "no_such.bam", 70000, MAX_BLOCKS])
    assert p.returncode == 1 and "no_such.bam" in p.stderr


def test_plan_equals_the_recorded_results(exe):
    """feed_plan.json: the sizing lines of decode_on_device as they stood before plan_decoder was split out of them, run on the grid"""
    cases = json.load(open(os.path.join(GOLDEN, "feed_plan.json")))
    assert len(cases) > 200 and {k for c in cases for k in c["env"]} == {"BDX_BAM_PIECE_BYTES", "BDX_BAM_BATCH_BLOCKS", "BDX_BAM_BATCH_ROUNDS",
                                                                         "BDX_BAM_RING_BYTES", "BDX_TIMING", "BDX_BAM_AHEAD", "BDX_READ"}
    for c in cases:
        p = run(exe, ["plan"] + c["args"], c["env"])
        assert p.returncode == 0, p.stderr
        got = {l.split("=")[0]: int(l.split("=")[1]) for l in p.stdout.splitlines()}
        assert got == c["plan"], (c["args"], c["env"])


# Two files whose first records on sequence t tie.  The reference's one queue gives the tie to the file that has been waiting at the top: the
# one that did NOT emit the last record in front of t.  `want` is the file that DID emit it (merge_order's emitted_last).
TIES = [("only file 0 emitted before", "t 2\nhas 0 0 2\nhas 1 2\n", 0),
        ("only file 1 emitted before", "t 2\nhas 0 2\nhas 1 1 2\n", 1),
        ("neither emitted before: the queue's first fill, file 0 on top", "t 2\nhas 0 2\nhas 1 2\n", 1),
        ("file 0's previous sequence is the later one", "t 4\nhas 0 0 3 4\nhas 1 1 4\nlast 0 3 5 0\nlast 1 1 900 1\n", 0),
        ("file 1's previous sequence is the later one", "t 4\nhas 0 0 4\nhas 1 0 2 4\nlast 0 0 900 1\nlast 1 2 5 0\n", 1),
        ("same previous sequence, file 0's last record lies behind", "t 3\nhas 0 1 3\nhas 1 1 3\nlast 0 1 700 0\nlast 1 1 699 1\n", 0),
        ("same previous sequence, file 1's last record lies behind", "t 3\nhas 0 1 3\nhas 1 1 3\nlast 0 1 10 1\nlast 1 1 11 0\n", 1),
        ("same last position, file 0's last record on the reverse strand: it sorts behind", "t 3\nhas 0 1 3\nhas 1 1 3\nlast 0 1 700 1\nlast 1 1 700 0\n", 0),
        ("same last position, file 1's on the reverse strand", "t 3\nhas 0 1 3\nhas 1 1 3\nlast 0 1 700 0\nlast 1 1 700 1\n", 1),
        ("equal last keys: as a queue filled afresh", "t 3\nhas 0 1 3\nhas 1 1 3\nlast 0 1 700 1\nlast 1 1 700 1\n", 1)]


@pytest.mark.parametrize("label,text,want", TIES, ids=[t[0] for t in TIES])
def test_tie_rule(exe, tmp_path, label, text, want):
    f = tmp_path / "tie.txt"
    f.write_text(text)
    p = run(exe, ["tie", f])
    assert p.returncode == 0 and p.stdout.split() == [str(want)], (p.stdout, p.stderr)
