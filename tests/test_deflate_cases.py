"""CPU tests of the hand-built DEFLATE corpus (tests/deflate_cases.py): python's zlib agrees with every label, the writer's own
bookkeeping shows that the corpus reaches the decoders' branches it was built for, and the host's decoder (host/fast_inflate.cpp,
through `bdx-inflate-check --each`, plain and built a second time with the address and undefined-behaviour sanitizers) accepts nothing
that zlib rejects and produces zlib's bytes wherever it accepts.  test_gpu_bamdec.py runs the same corpus through csrc/kz_inflate.hip."""
import os
import subprocess

import pytest

import deflate_cases as D
from helpers import ROOT

HOST = os.path.join(ROOT, "breakdancer_amd", "host")
# valid members that fast_inflate declines and its callers then hand to zlib: it allows an incomplete code only for distances
LEFT_TO_ZLIB = ["V-header/end-of-block-alone"]


@pytest.fixture(scope="module")
def cases():
    return D.corpus()


def test_labels_are_zlibs_verdicts(cases):
    labels = [c[0] for c in cases]
    assert len(set(labels)) == len(labels)
    for label, payload, ulen, want in cases:
        assert label[:2] in ("V-", "R-") and (want is not None) == label.startswith("V-")
        assert len(payload) + 26 <= 65536 and ulen <= 65536, label
        ok, got = D.judge(payload, ulen)
        assert ok == (want is not None), "%s: zlib %s it" % (label, "accepts" if ok else "rejects")
        if ok:
            assert len(want) == ulen and got == want, label
    assert sum(c[3] is not None for c in cases) >= 60 and sum(c[3] is None for c in cases) >= 60


def test_deep_members_reach_the_slow_decodes():
    deep = D.writers("deep/")
    assert len(deep) == 6
    for label, f in deep.items():
        assert len(f.data) <= 65280 and len(f.payload()) + 26 <= 65536 and len(f.data) - 34000 > 20000, label
        assert all(f.lit_bits[l] >= 1 for l in range(9, 16)), (label, f.lit_bits)      # literal/length codes of 9 (kz's table) .. 15 bits
        assert f.lit_bits[15] >= 2 and f.lit[256][1] == 15   #(end-of-block is one of the 15-bit codes)
        assert all(f.dist_bits[l] >= 1 for l in range(1, 16)), (label, f.dist_bits)    # distance codes of 1 .. 15 bits
        assert f.pairs == {(True, True), (True, False), (False, True), (False, False)}, label   # (length fast?, distance fast?) for kz
        near = [m for m in f.matches if m[3] <= D.KZ_NEAR]
        assert near and len(near) < len(f.matches)
    lens = sorted(set(D.DEEP_LIT)), sorted(set(D.DEEP_DIST))
    assert lens[0] == [0] + list(range(2, 16)) and lens[1] == list(range(16))


def huffman_header_bytes(f):
    return [bit // 8 for kind, _, bit in f.blocks if kind != "stored"]


def test_mixed_members_cross_their_stored_blocks():
    mixed = D.writers("mixed/")
    assert len(mixed) >= 20
    stored_lens, before, behind = set(), False, False
    for label, f in mixed.items():
        assert 3 <= len(f.blocks) <= 9, label
        ends = [b[1] for b in f.blocks[1:]] + [len(f.data)]
        into = across = False
        for i, (kind, start, _) in enumerate(f.blocks):
            if kind != "stored": continue
            n = ends[i] - start
            stored_lens.add(n)
            assert i + 1 < len(f.blocks) and f.blocks[i + 1][0] != "stored", label    # Huffman blocks follow every stored one
            if not n & 1: continue
            # matches of the Huffman blocks behind this odd-length stored block
            later = [(dst, length, dist) for b, dst, length, dist in f.matches if b > i]
            into |= any(start <= dst - dist < start + n for dst, length, dist in later)
            across |= any(dst - dist < start for dst, length, dist in later)
        assert into and across, label
        dists = [m[3] for m in f.matches]
        assert min(dists) <= D.KZ_NEAR < max(dists), label
        before |= any(b % 512 >= 504 for b in huffman_header_bytes(f))
        behind |= any(b % 512 <= 8 and b >= 512 for b in huffman_header_bytes(f))
    assert stored_lens >= set(D.STORED_LENS), sorted(stored_lens)
    assert before and behind      # a Huffman block's header within 8 bytes of a multiple of 512 in the payload, on either side
    kinds = {(f.blocks[i][0], f.blocks[i + 1][0]) for f in mixed.values() for i in range(len(f.blocks) - 1)}
    assert {("stored", "fixed"), ("stored", "dynamic"), ("fixed", "stored"), ("dynamic", "stored")} <= kinds


def test_headers_and_tiny_blocks_are_what_they_are_named():
    f = D.writer("tiny/0")
    assert len(f.blocks) == 300 and f.blocks[-1][0] == "stored" and {b[0] for b in f.blocks} == {"stored", "fixed"}
    head = {k: next(t for t in D.writer(k).log if t[0] == "header") for k in D.writers("header/") if D.writer(k).log}
    _, hlit, hdist, hclen, clc = head["header/hclen5-hlit257-hdist1-no-distance-code"]
    assert (hlit, hdist, hclen) == (257, 1, 5) and not D.writer("header/hclen5-hlit257-hdist1-no-distance-code").dist
    assert max(head["header/7-bit-code-length-code"][4].values()) == 7
    assert all(isinstance(t, tuple) or t in D.CLC_7BIT for t in D.writer("header/7-bit-code-length-code").cl_tokens)
    f = D.writer("header/16-across-the-boundary")
    hlit = head["header/16-across-the-boundary"][1]
    _, spans = D.expand(f.cl_tokens)
    assert any(isinstance(t, tuple) and t[0] == 16 and a < hlit < b for t, (a, b) in zip(f.cl_tokens, spans))
    assert (18, 138) in D.writer("header/18x138").cl_tokens
    for k in ("sym0", "sym4", "sym10"):
        f = D.writer("header/lone-distance-code/" + k)
        assert [n for _, n in f.dist.values()] == [1] and len(f.matches) >= 50 and len(f.pairs) == 2
    f = D.writer("header/end-of-block-alone")
    assert f.lit == {256: (0, 1)} and not f.data
    for tokens in (D.DEEP_TOKENS, D.rle(D.SEVEN_LIT + D.SEVEN_DIST, use=(16, 18))):
        assert D.expand(tokens)[0] in (D.DEEP_LIT + D.DEEP_DIST, D.SEVEN_LIT + D.SEVEN_DIST)


# ---------------------------------------------------------------------------------------------------------------------------------
# the host's decoder
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def checkers(tmp_path_factory):
    """(bin/bdx-inflate-check, the same two sources built with -fsanitize=address,undefined)"""
    plain = os.path.join(ROOT, "bin", "bdx-inflate-check")
    subprocess.check_call(["make", "-C", ROOT, "bin/bdx-inflate-check"], stdout=subprocess.DEVNULL)
    san = str(tmp_path_factory.mktemp("san") / "bdx-inflate-check-san")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                           "-o", san, os.path.join(HOST, "inflate_check_main.cpp"), os.path.join(HOST, "fast_inflate.cpp"), "-lz"])
    return plain, san


def test_fast_inflate_agrees_with_zlib_on_the_corpus(tmp_path, cases, checkers):
    path = str(tmp_path / "corpus.bgzf")
    with open(path, "wb") as out:
        for label, payload, ulen, want in cases:
            out.write(D.bgzf_member(payload, ulen))
        out.write(D.EOF_BLOCK + D.EOF_BLOCK)   # (no payload within 32 bytes of the file's end: fast_inflate gets every one)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    for exe in checkers:
        p = subprocess.run([exe, "--each", path], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env)
        err = p.stderr.decode()
        assert p.returncode == 0 and "Sanitizer" not in err and "runtime error" not in err, (exe, err[-3000:])
        rows = [[int(x) for x in line.split()] for line in p.stdout.decode().splitlines()]
        assert len(rows) == len(cases) + 2 and [r[0] for r in rows] == list(range(len(rows)))
        declined = []
        for (label, payload, ulen, want), (_, zlib_ok, fast_ok, equal) in zip(cases, rows):
            assert zlib_ok == (want is not None), "%s: the C zlib's verdict differs from python's" % label
            assert not (fast_ok and want is None), "%s: fast_inflate accepts what zlib rejects" % label
            assert equal or not fast_ok, "%s: fast_inflate's bytes differ from zlib's" % label
            if want is not None and not fast_ok: declined.append(label)
        assert declined == LEFT_TO_ZLIB, (exe, declined)
