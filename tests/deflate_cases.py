"""Shared by test_deflate_cases.py (CPU: zlib as the judge, host/fast_inflate.cpp through bdx-inflate-check) and test_gpu_bamdec.py
(csrc/kz_inflate.hip): a DEFLATE writer for chosen tokens, blocks and headers (RFC 1951), and a corpus of members built with it that
no encoder in the suite would write -- codes of every length up to 15 bits, stored blocks between Huffman blocks, headers at the edges
of what 3.2.7 allows, and streams that every decoder has to refuse.  python's zlib decides what each case is; the writer's own
bookkeeping (which code lengths it emitted, where blocks and matches lie) says what the corpus reaches, independent of any decoder."""
import functools
import struct
import zlib
from collections import Counter

import numpy as np

BGZF_HEAD = b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00BC\x02\x00"
EOF_BLOCK = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
CLC_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
FIXED_LIT = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST = [5] * 32
KZ_LIT_BITS, KZ_DIST_BITS = 9, 8   # kz_inflate.hip's primary tables (kLB, kDB): longer codes take its canonical decode
KZ_NEAR = 574                      # ... and its kNearDist: matches further back may read HBM instead of the LDS window


def bgzf_member(payload, ulen, crc=0):
    assert len(payload) + 26 <= 65536 and ulen <= 65536
    return BGZF_HEAD + struct.pack("<H", len(payload) + 25) + payload + struct.pack("<II", crc, ulen)


def judge(payload, ulen):
    """(accepted, bytes): what zlib makes of a raw deflate payload that is said to inflate to ulen bytes"""
    d = zlib.decompressobj(-15)
    try:
        got = d.decompress(payload, ulen + 1)
    except zlib.error:
        return False, b""
    return bool(d.eof and len(got) == ulen), got


class TokenDeflate:
    """a DEFLATE writer for chosen token sequences (RFC 1951): zlib picks its own matches and blocks, the tests need a match of a given
    length at a given distance right behind given tokens, in a block of a given kind with a given header.

    TokenDeflate() opens one final block in the fixed code (3.2.6), TokenDeflate(lit_lens, dist_lens) one final dynamic block (3.2.7) whose
    286 + 30 code lengths are sent without run lengths; finish() closes it and wraps the payload in a BGZF member.
    TokenDeflate(open_block=False) writes nothing: stored(), fixed() and dynamic() then open blocks of any kind one behind the other,
    end_block() closes a Huffman block, payload() pads to the byte.  bits() / code() / sym() / dsym() write anything else.

    What it keeps for the tests: `data` (the bytes the tokens stand for), `blocks` [(kind, first output byte, payload bit of the header)],
    `matches` [(block index, destination, length, distance)], `lit_bits` / `dist_bits` (how many codes of each length were emitted),
    `pairs` {(length code resolved by kz's primary table, distance code resolved by it)}, `cl_tokens` of the last dynamic header and `log`."""
    LBASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
    LEXTRA = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
    DBASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577]
    DEXTRA = [0, 0, 0, 0] + [i // 2 for i in range(2, 28)]

    @staticmethod
    def canonical(lens):   # symbol -> (code, length), RFC 1951 3.2.2
        code, out = 0, {}
        for l in range(1, 16):
            for s, x in enumerate(lens):
                if x == l:
                    out[s] = (code, l)
                    code += 1
            code <<= 1
        return out

    def __init__(self, lit_lens=None, dist_lens=None, open_block=True):
        self.acc, self.nbits, self.out, self.data = 0, 0, bytearray(), bytearray()
        self.lit, self.dist = {}, {}
        self.blocks, self.matches, self.log, self.cl_tokens = [], [], [], []
        self.lit_bits, self.dist_bits, self.pairs = Counter(), Counter(), set()
        self.valid = True   # False once a match reached back further than there is output
        if not open_block:
            return
        if lit_lens is None:
            self.fixed(final=True)
        else:
            assert len(lit_lens) == 286 and len(dist_lens) == 30
            assert sum(2.0 ** -l for l in lit_lens if l) == 1.0 and sum(2.0 ** -l for l in dist_lens if l) == 1.0
            self.dynamic(lit_lens, dist_lens, final=True)

    # ---- bits ----
    def bits(self, v, n):   # n bits of v, least significant first
        self.acc |= (v & ((1 << n) - 1)) << self.nbits
        self.nbits += n
        while self.nbits >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.nbits -= 8

    def code(self, c, n):   # a Huffman code: most significant bit first
        self.bits(int(format(c, "0%db" % n)[::-1], 2), n)

    def bitpos(self):
        return len(self.out) * 8 + self.nbits

    def align(self):
        if self.nbits: self.bits(0, 8 - self.nbits)

    # ---- blocks ----
    def _open(self, kind, final, btype):
        self.blocks.append((kind, len(self.data), self.bitpos()))
        self.log.append(("block", kind, int(bool(final)), self.bitpos()))
        self.bits(1 if final else 0, 1)
        self.bits(btype, 2)

    def stored(self, data, final=False, length=None, nlen=None):
        """a stored block (3.2.4) of `data`; length / nlen override what LEN / NLEN say"""
        self._open("stored", final, 0)
        self.align()
        length = len(data) if length is None else length
        self.out += struct.pack("<HH", length, (length ^ 0xFFFF) if nlen is None else nlen)
        self.out += data
        self.data += data

    def fixed(self, final=False):
        self._open("fixed", final, 1)
        self.lit, self.dist = self.canonical(FIXED_LIT), self.canonical(FIXED_DIST)   # (286, 287, 30 and 31 have codes: sym() / dsym() can write them)

    def dynamic(self, lit_lens, dist_lens, final=False, clc=None, tokens=None, hclen=None, hlit=None, hdist=None, codes=True):
        """a dynamic block's header: HLIT = len(lit_lens), HDIST = len(dist_lens) (or what hlit / hdist say), the code-length code `clc`
        ({symbol: bits}) in HCLEN entries, and the code lengths as `tokens`: 0..15, (16, rep), (17, rep), (18, rep).  Without tokens every
        length is sent as itself; without clc those take four bits each (HCLEN 19) or, if the tokens hold repeats, clc_for()'s code.
        codes=False: the lengths are no usable code (a reject case): the block's symbol codes are not set up"""
        self._open("dynamic", final, 2)
        plain = tokens is None
        if plain:
            tokens = list(lit_lens) + list(dist_lens)
        if clc is None:
            clc = {s: 4 for s in range(16)} if plain else clc_for(tokens)
            if plain and hclen is None: hclen = 19
        cl = [clc.get(s, 0) for s in range(19)]
        if hclen is None:
            hclen = max([4] + [i + 1 for i, s in enumerate(CLC_ORDER) if cl[s]])
        self.bits((len(lit_lens) if hlit is None else hlit) - 257, 5)
        self.bits((len(dist_lens) if hdist is None else hdist) - 1, 5)
        self.bits(hclen - 4, 4)
        for s in CLC_ORDER[:hclen]:
            self.bits(cl[s], 3)
        self.log.append(("header", len(lit_lens), len(dist_lens), hclen, dict(clc)))
        self.cl_tokens = list(tokens)
        if tokens:
            cc = self.canonical(cl)
            for t in tokens:
                if isinstance(t, tuple):
                    s, rep = t
                    self.code(*cc[s])
                    base, n = {16: (3, 2), 17: (3, 3), 18: (11, 7)}[s]
                    assert 0 <= rep - base < (1 << n)
                    self.bits(rep - base, n)
                else:
                    self.code(*cc[t])
        if codes:
            self.lit, self.dist = self.canonical(lit_lens), self.canonical(dist_lens)
        else:
            self.lit, self.dist = {}, {}

    def end_block(self):
        self.sym(256)

    # ---- tokens ----
    def sym(self, s):   # a literal/length symbol's code, nothing else
        c, n = self.lit[s]
        self.code(c, n)
        self.lit_bits[n] += 1
        return n

    def dsym(self, s):
        c, n = self.dist[s]
        self.code(c, n)
        self.dist_bits[n] += 1
        return n

    def literal(self, b):
        self.sym(b)
        self.data.append(b)
        self.log.append(("lit", b))

    def match(self, length, dist, check=True):
        """check=False: the distance may reach back further than there is output (the member is then no valid one)"""
        assert 3 <= length <= 258 and 1 <= dist <= 32768 and (not check or dist <= len(self.data))
        ls = max(i for i in range(29) if self.LBASE[i] <= length) if length < 258 else 28
        nl = self.sym(257 + ls)
        self.bits(length - self.LBASE[ls], self.LEXTRA[ls])
        ds = max(i for i in range(30) if self.DBASE[i] <= dist)
        nd = self.dsym(ds)
        self.bits(dist - self.DBASE[ds], self.DEXTRA[ds])
        self.pairs.add((nl <= KZ_LIT_BITS, nd <= KZ_DIST_BITS))
        self.matches.append((len(self.blocks) - 1, len(self.data), length, dist))
        self.log.append(("match", length, dist, nl, nd, len(self.data)))
        if dist > len(self.data):
            self.valid = False
            return
        for _ in range(length):
            self.data.append(self.data[-dist])

    def literals(self, values):
        for b in values: self.literal(int(b))

    def dist_in(self, lo, hi, rng):
        """a distance in [lo, hi] that the block's distance code can express and the output so far allows, or None"""
        hi = min(hi, len(self.data), 32768)
        spans = []
        for s in self.dist:
            if s > 29: continue
            a, b = max(lo, self.DBASE[s]), min(hi, self.DBASE[s] + (1 << self.DEXTRA[s]) - 1)
            if a <= b: spans.append((a, b))
        if not spans: return None
        a, b = spans[int(rng.integers(0, len(spans)))]
        return int(rng.integers(a, b + 1))

    def len_in(self, lo, hi, rng):
        """a match length in [lo, hi] that the block's literal/length code can express"""
        spans = []
        for i in range(29):
            if 257 + i not in self.lit: continue
            a, b = max(lo, self.LBASE[i]), min(hi, 257 if i == 27 else self.LBASE[i] + (1 << self.LEXTRA[i]) - 1)
            if a <= b: spans.append((a, b))
        a, b = spans[int(rng.integers(0, len(spans)))]
        return int(rng.integers(a, b + 1))

    def pad_fixed_to(self, byte):
        """a fixed block of one-byte literals that ends where the next block's header then starts in payload byte `byte`"""
        n = -((self.bitpos() + 10 - byte * 8) // 8)
        assert n >= 0
        self.fixed()
        for i in range(n): self.literal(i % 144)   # (literals 0..143: eight bits each)
        self.end_block()
        assert self.bitpos() // 8 == byte

    # ---- results ----
    def payload(self):
        self.align()
        return bytes(self.out)

    def finish(self):
        self.end_block()
        data, comp = bytes(self.data), self.payload()
        assert zlib.decompress(comp, -15) == data
        return bgzf_member(comp, len(data), zlib.crc32(data) & 0xFFFFFFFF), data

    def dump(self):
        """the token list, one per line (what to read kz_inflate.hip against when it gets a member wrong)"""
        return "\n".join(" ".join(str(x) for x in t) for t in self.log)


def rle(lens, use=(16, 17, 18)):
    """a list of code lengths as 3.2.7's tokens, with the repeat symbols in `use`"""
    out, i = [], 0
    while i < len(lens):
        v, n = lens[i], 1
        while i + n < len(lens) and lens[i + n] == v: n += 1
        i += n
        if v == 0:
            while n >= 11 and 18 in use:
                r = min(n, 138)
                out.append((18, r)); n -= r
            while n >= 3 and 17 in use:
                r = min(n, 10)
                out.append((17, r)); n -= r
        if n and (v != 0 or 16 in use or n < 3):
            out.append(v); n -= 1
            while n >= 3 and 16 in use:
                r = min(n, 6)
                out.append((16, r)); n -= r
        out += [v] * n
    return out


def expand(tokens):
    """the lengths a token list stands for, and for every token the range of indices it fills"""
    lens, spans = [], []
    for t in tokens:
        if isinstance(t, tuple):
            v = lens[-1] if t[0] == 16 else 0
            spans.append((len(lens), len(lens) + t[1]))
            lens += [v] * t[1]
        else:
            spans.append((len(lens), len(lens) + 1))
            lens.append(t)
    return lens, spans


def clc_for(tokens):
    """a complete code-length code over the symbols the tokens use: the most frequent ones a bit shorter"""
    freq = Counter(t[0] if isinstance(t, tuple) else t for t in tokens)
    syms = [s for s, _ in freq.most_common()]
    if len(syms) == 1: syms.append(0 if syms[0] else 1)   # (a code of one symbol is incomplete: not allowed here)
    b = max(1, (len(syms) - 1).bit_length())
    short = (1 << b) - len(syms)
    return {s: (b - 1 if i < short else b) for i, s in enumerate(syms)}


# The deep code: literals at 9 bits, length symbols on codes of every length 2..15, end-of-block at 15; distance symbols, near and far
# alike, on codes of every length 1..15.  kz's primary tables resolve 9 and 8 bits, the host's 11 and 8.
DEEP_LIT = [9] * 256 + [0] * 30
for _s, _l in zip((257, 258, 259, 260, 261, 262, 263, 264, 284, 285, 270, 280, 265, 256, 266), list(range(2, 15)) + [15, 15]):
    DEEP_LIT[_s] = _l
DEEP_DIST = [0] * 30
for _s, _l in zip((0, 29, 1, 20, 2, 18, 3, 25, 10, 28, 16, 17, 19, 22, 27, 24), list(range(1, 16)) + [15]):
    DEEP_DIST[_s] = _l
assert sum(2.0 ** -l for l in DEEP_LIT if l) == 1.0 and sum(2.0 ** -l for l in DEEP_DIST if l) == 1.0
DEEP_TOKENS = rle(DEEP_LIT + DEEP_DIST)
DEEP_FAST_LEN = [(3, 10)]                                               # 257..264: 2..9 bits
DEEP_SLOW_LEN = [(227, 257), (258, 258), (23, 26), (115, 130), (11, 12), (13, 14)]   # 284, 285, 270, 280, 265, 266: 10..15 bits
DEEP_FAST_DIST = [0, 29, 1, 20, 2, 18, 3, 25]
DEEP_SLOW_DIST = [10, 28, 16, 17, 19, 22, 27, 24]


def deep(f, final=False):
    f.dynamic(DEEP_LIT, DEEP_DIST, final=final, tokens=DEEP_TOKENS)


def _dist_of_symbol(f, s, rng):
    lo = f.DBASE[s]
    return min(int(rng.integers(lo, lo + (1 << f.DEXTRA[s]))), len(f.data))


def deep_member(seed, n_lits=34000, size=60000):
    """random literals, then matches whose length code is fast and slow for kz, each behind a distance code that is fast and slow, the
    slow symbols taken in turn, a few literals between"""
    rng = np.random.default_rng(seed)
    f = TokenDeflate(open_block=False)
    deep(f, final=True)
    f.literals(rng.integers(0, 256, n_lits, dtype=np.uint8))
    k = 0
    while len(f.data) + 258 + 3 <= size:
        slow_len, slow_dist = bool(k & 1), bool(k & 2)
        lo, hi = DEEP_SLOW_LEN[(k >> 2) % len(DEEP_SLOW_LEN)] if slow_len else DEEP_FAST_LEN[0]
        syms = [s for s in (DEEP_SLOW_DIST if slow_dist else DEEP_FAST_DIST) if f.DBASE[s] <= len(f.data)]
        s = syms[(k >> 2) % len(syms)] if slow_dist else syms[int(rng.integers(0, len(syms)))]
        f.match(int(rng.integers(lo, hi + 1)), _dist_of_symbol(f, s, rng))
        f.literals(rng.integers(0, 256, int(rng.integers(0, 4)), dtype=np.uint8))
        k += 1
    f.end_block()
    return f


STORED_LENS = (0, 1, 3, 5, 255, 257, 1023, 1025, 1500, 2049)   # odd ones, and both sides of kz's 1 KiB window


def _huffman_behind_stored(f, rng, start, length):
    """tokens of an open Huffman block that follows the stored block [start, start + length): matches whose source begins inside the
    stored bytes, matches whose source begins before them (the copy runs across the stored block), then near and far ones anywhere"""
    f.literals(rng.integers(0, 256, int(rng.integers(0, 3)), dtype=np.uint8))
    for _ in range(2):
        cur = len(f.data)
        if length:
            d = f.dist_in(cur - (start + length) + 1, cur - start, rng)
            if d: f.match(f.len_in(3, 40, rng), d)
        cur = len(f.data)
        d = f.dist_in(cur - start + 1, cur - start + 64, rng) or f.dist_in(cur - start + 1, cur - start + 1100, rng)
        if d: f.match(f.len_in(3, 258, rng), d)
        f.literals(rng.integers(0, 256, int(rng.integers(0, 3)), dtype=np.uint8))
    for _ in range(int(rng.integers(4, 30))):
        lo, hi = ((1, KZ_NEAR), (KZ_NEAR + 1, 4000))[int(rng.integers(0, 2))]
        d = f.dist_in(lo, hi, rng)
        if d: f.match(f.len_in(*[(3, 10), (11, 64), (65, 130), (131, 258)][int(rng.integers(0, 4))], rng), d)
        f.literals(rng.integers(0, 256, int(rng.integers(0, 5)), dtype=np.uint8))


def mixed_member(seed):
    """3..9 blocks: a Huffman block of literals first (so that far matches have something to reach), then stored blocks of the listed lengths,
    each followed by a Huffman block in the fixed or the deep code.  Every fourth seed pads so that such a header starts just before a
    multiple of 512 in the payload, every fourth just behind one"""
    rng = np.random.default_rng(seed)
    f = TokenDeflate(open_block=False)
    pairs = int(rng.integers(1, 4 if seed % 4 < 2 else 5))   # (the padded ones hold a block more)
    lens = [int(x) for x in rng.choice(STORED_LENS, pairs)]
    if not any(l & 1 for l in lens): lens[int(rng.integers(0, pairs))] = int(rng.choice([1, 3, 5, 255, 257, 1023, 1025, 2049]))
    kinds = ["fixed" if (l & 1 and i == [x & 1 for x in lens].index(1)) else str(rng.choice(["fixed", "deep"])) for i, l in enumerate(lens)]
    (deep if rng.integers(0, 2) else TokenDeflate.fixed)(f)
    f.literals(rng.integers(0, 256, int(rng.integers(700, 1600)), dtype=np.uint8))
    f.end_block()
    for i, (l, kind) in enumerate(zip(lens, kinds)):
        start = len(f.data)
        f.stored(rng.integers(0, 256, l, dtype=np.uint8).tobytes())
        if i == 0 and seed % 4 < 2:
            at = f.bitpos() // 8 + 16
            f.pad_fixed_to(((at + 511) & ~511) + (-3 if seed % 4 == 0 else 2))
        last = i == pairs - 1
        (deep if kind == "deep" else TokenDeflate.fixed)(f, final=last and pairs > 1)
        _huffman_behind_stored(f, rng, start, l)
        f.end_block()
    if pairs == 1:   # (at least three blocks)
        f.fixed(final=True)
        f.literals(rng.integers(0, 256, 3, dtype=np.uint8)); f.match(258, f.dist_in(KZ_NEAR + 1, 2000, rng))
        f.end_block()
    assert 3 <= len(f.blocks) <= 9
    return f


def tiny_member(seed):
    rng = np.random.default_rng(seed)
    f = TokenDeflate(open_block=False)
    for _ in range(299):
        k = int(rng.integers(0, 3))
        if k == 0:
            f.fixed(); f.literal(int(rng.integers(0, 256))); f.end_block()
        elif k == 1:
            f.fixed(); f.end_block()
        else:
            f.stored(rng.integers(0, 256, int(rng.integers(0, 5)), dtype=np.uint8).tobytes())
    f.stored(b"", final=True)
    return f


# ---- headers ----
CLC_7BIT = {8: 1, 0: 2, 9: 3, 7: 4, 5: 5, 4: 6, 16: 7, 18: 7}
# a code with lengths 4, 5, 7, 8, 9 and 0 only: what CLC_7BIT can say
SEVEN_LIT = [4] * 4 + [5] * 8 + [7] * 16 + [8] * 32 + [9] * 124 + [0] * 72 + [9] * 4
SEVEN_DIST = [4] * 8 + [5] * 16


def _h_min_header(rng):
    f = TokenDeflate(open_block=False)
    f.dynamic([0] + [8] * 256, [0], final=True, clc={0: 1, 8: 2, 18: 2})   # HCLEN 5, HLIT 257, HDIST 1, no distance code, 255 literals
    f.literals(rng.integers(1, 256, 900, dtype=np.uint8))
    f.end_block()
    return f


def _h_seven_bit(rng):
    f = TokenDeflate(open_block=False)
    f.dynamic(SEVEN_LIT, SEVEN_DIST, final=True, clc=CLC_7BIT, tokens=rle(SEVEN_LIT + SEVEN_DIST, use=(16, 18)))
    f.literals(rng.integers(0, 184, 1200, dtype=np.uint8))
    for _ in range(200):
        f.match(int(rng.integers(3, 6)), f.dist_in(1, 4096, rng))
        f.literals(rng.integers(0, 184, int(rng.integers(0, 4)), dtype=np.uint8))
    f.end_block()
    return f


def _h_sixteen_across(rng):
    lit = [8] * 144 + [9] * 112 + [7] * 4 + [6] * 8 + [5] * 2   # HLIT 270: ..., 5, 5 | 5, 5, 5, ...
    dist = [5] * 12 + [4] * 10
    assert sum(2.0 ** -l for l in lit) == 1.0 and sum(2.0 ** -l for l in dist) == 1.0
    f = TokenDeflate(open_block=False)
    f.dynamic(lit, dist, final=True, tokens=rle(lit + dist))
    f.literals(rng.integers(0, 256, 1500, dtype=np.uint8))
    for _ in range(150):
        f.match(int(rng.integers(3, 15)), f.dist_in(1, 1500, rng))
        f.literal(int(rng.integers(0, 256)))
    f.end_block()
    return f


def _h_eighteen_138(rng):
    lit = [6] * 32 + [7] * 62 + [0] * 162 + [7] * 2   # 162 zeros: 18 x 138, then 18 x 24
    dist = [0, 0, 2, 2, 2, 2]
    assert sum(2.0 ** -l for l in lit if l) == 1.0
    f = TokenDeflate(open_block=False)
    f.dynamic(lit, dist, final=True, tokens=rle(lit + dist))
    f.literals(rng.integers(0, 94, 800, dtype=np.uint8))
    for _ in range(60):
        f.match(3, f.dist_in(3, 8, rng))
        f.literal(int(rng.integers(0, 94)))
    f.end_block()
    return f


def _h_lone_distance(rng, dist_lens):
    f = TokenDeflate(open_block=False)
    f.dynamic(DEEP_LIT, dist_lens, final=True, tokens=rle(DEEP_LIT + dist_lens))
    f.literals(rng.integers(0, 256, 120, dtype=np.uint8))
    for k in range(80):
        lo, hi = (DEEP_SLOW_LEN[k % 6] if k & 1 else DEEP_FAST_LEN[0])
        f.match(int(rng.integers(lo, hi + 1)), f.dist_in(1, 32768, rng))
        f.literals(rng.integers(0, 256, int(rng.integers(0, 3)), dtype=np.uint8))
    f.end_block()
    return f


def _h_eob_alone():
    f = TokenDeflate(open_block=False)
    lit = [0] * 256 + [1]
    f.dynamic(lit, [0], final=True, tokens=rle(lit + [0]))
    f.end_block()
    return f


# ---- extremes ----
def _open(kind, final=True):
    f = TokenDeflate(open_block=False)
    (deep if kind == "deep" else TokenDeflate.fixed)(f, final=final)
    return f


def _x_far(kind, rng, what):
    f = _open(kind)
    f.literals(rng.integers(0, 256, 32768, dtype=np.uint8))
    if what == "258x2":
        f.match(258, 32768); f.match(258, 32768)
    else:
        f.match(3, 32768); f.literal(7); f.match(3, 32768)
    f.literals(rng.integers(0, 256, 5, dtype=np.uint8))
    f.end_block()
    return f


def _x_run(kind, rng):
    f = _open(kind)
    for _ in range(6):
        f.literal(int(rng.integers(0, 256)))
        f.match(258, 1)
    f.match(258, 1)
    f.end_block()
    return f


def _x_reach(kind, pos, length, rng, excess=0):
    """`pos` literals, then a match whose distance is the output position (excess 0: the member's first byte) or one more"""
    f = _open(kind)
    f.literals(rng.integers(0, 256, pos, dtype=np.uint8))
    f.match(length, pos + excess, check=False)
    f.literals(rng.integers(0, 256, 4, dtype=np.uint8))
    f.end_block()
    return f


# (kind, position, length): in the fixed code kz's tables resolve the whole match (the step's check); in the deep code a 10-bit-or-longer
# length code, or a distance code beyond 8 bits, stops the chain in front of it (the stop-token path's check)
REACH = [("fixed", 1, 3), ("fixed", 5, 4), ("fixed", 300, 258), ("fixed", 700, 9),
         ("deep", 24676, 5), ("deep", 24676, 258), ("deep", 40, 7), ("deep", 40, 24), ("deep", 20000, 6), ("deep", 20000, 120)]


def _reject_header(rng, **kw):
    """a dynamic header that no decoder may get past, with bytes behind it that are not the reason"""
    f = TokenDeflate(open_block=False)
    f.dynamic(final=True, codes=False, **kw)
    f.out += rng.integers(0, 256, 40, dtype=np.uint8).tobytes()
    return f


@functools.lru_cache(maxsize=1)
def _build():
    cases, writers = [], {}

    def add(label, f, ulen=None, payload=None, valid=True):
        payload = f.payload() if payload is None else payload
        assert label not in writers and (f.valid or not valid)
        writers[label] = f
        if valid:
            cases.append(("V-" + label, payload, len(f.data), bytes(f.data)))
        else:
            cases.append(("R-" + label, payload, len(f.data) if ulen is None else ulen, None))

    # ---------------- valid ----------------
    for seed in range(6):
        add("deep/%d" % seed, deep_member(100 + seed))
    for seed in range(28):
        add("mixed/%d" % seed, mixed_member(200 + seed))
    for seed in range(3):
        add("tiny/%d" % seed, tiny_member(300 + seed))
    rng = np.random.default_rng(400)
    add("header/hclen5-hlit257-hdist1-no-distance-code", _h_min_header(rng))
    add("header/7-bit-code-length-code", _h_seven_bit(rng))
    add("header/16-across-the-boundary", _h_sixteen_across(rng))
    add("header/18x138", _h_eighteen_138(rng))
    add("header/lone-distance-code/sym0", _h_lone_distance(rng, [1]))
    add("header/lone-distance-code/sym4", _h_lone_distance(rng, [0] * 4 + [1]))
    add("header/lone-distance-code/sym10", _h_lone_distance(rng, [0] * 10 + [1]))
    add("header/end-of-block-alone", _h_eob_alone())
    for kind in ("fixed", "deep"):
        add("extreme/258x2@32768/%s" % kind, _x_far(kind, rng, "258x2"))
        add("extreme/3@32768/%s" % kind, _x_far(kind, rng, "3"))
        add("extreme/258@1/%s" % kind, _x_run(kind, rng))
    for kind, pos, length in REACH:
        add("extreme/distance=position/%s/%d/len%d" % (kind, pos, length), _x_reach(kind, pos, length, rng))
    for i, f in enumerate((deep_member(500, 900, 2500), mixed_member(501), _x_run("fixed", rng))):
        add("extreme/trailing-garbage/%d" % i, f, payload=f.payload() + rng.integers(0, 256, 1 + 50 * i, dtype=np.uint8).tobytes())

    # ---------------- reject ----------------
    rng = np.random.default_rng(600)
    tail = lambda n: rng.integers(0, 256, n, dtype=np.uint8).tobytes()   # noqa: E731
    f = TokenDeflate(open_block=False)
    f.bits(1, 1); f.bits(3, 2); f.out += tail(30)
    add("block-type-3", f, ulen=10, valid=False)
    f = TokenDeflate(open_block=False)
    f.fixed(); f.literals(tail(20)); f.end_block(); f.bits(0, 1); f.bits(3, 2); f.out += tail(30)
    add("block-type-3/second-block", f, valid=False)
    for i, nlen in enumerate((0x0000, 100 ^ 0xFFFF ^ 0x0100)):
        f = TokenDeflate(open_block=False)
        f.fixed(); f.literals(tail(7)); f.end_block()
        f.stored(tail(100), final=True, nlen=nlen)
        add("stored/nlen-wrong/%d" % i, f, valid=False)
    f = TokenDeflate(open_block=False)
    f.stored(tail(50), final=True, length=100)
    add("stored/len-past-the-payload", f, ulen=100, valid=False)
    f = TokenDeflate(open_block=False)
    f.fixed(); f.literals(tail(3)); f.end_block(); f.stored(tail(600), final=True, length=601)
    add("stored/len-one-past-the-payload", f, ulen=604, valid=False)
    f = TokenDeflate(open_block=False)   # (a stored block's header of which only LEN is there)
    f.fixed(); f.literals(tail(9)); f.end_block(); f.bits(1, 1); f.bits(0, 2); f.align(); f.out += b"\x00\x00"
    add("stored/header-cut", f, valid=False)

    lit8 = [8] * 256
    add("header/16-first", _reject_header(rng, lit_lens=lit8 + [8], dist_lens=[0], clc={16: 1, 8: 2, 0: 2}, tokens=[(16, 3)] + [8] * 200), valid=False)
    add("header/repeat-past-the-end/18", _reject_header(rng, lit_lens=[0] + lit8, dist_lens=[0], clc={0: 1, 8: 2, 18: 2}, tokens=[0] + [8] * 250 + [(18, 11)]), valid=False)
    add("header/repeat-past-the-end/16", _reject_header(rng, lit_lens=[0] + lit8, dist_lens=[0], clc={0: 1, 8: 2, 16: 2}, tokens=[0] + [8] * 253 + [(16, 6)]), valid=False)
    add("header/repeat-past-the-end/17", _reject_header(rng, lit_lens=[0] + lit8, dist_lens=[0], clc={0: 1, 8: 2, 17: 2}, tokens=[0] + [8] * 256 + [(17, 3)]), valid=False)
    add("header/no-end-of-block-code", _reject_header(rng, lit_lens=lit8 + [0], dist_lens=[0], tokens=rle(lit8 + [0, 0])), valid=False)
    add("header/literal-set-over-subscribed", _reject_header(rng, lit_lens=lit8 + [8], dist_lens=[0], tokens=rle(lit8 + [8, 0])), valid=False)
    add("header/literal-set-incomplete", _reject_header(rng, lit_lens=[0] + [8] * 254 + [0, 8], dist_lens=[0], tokens=rle([0] + [8] * 254 + [0, 8, 0])), valid=False)
    add("header/literal-set-one-code-of-two-bits", _reject_header(rng, lit_lens=[0] * 256 + [2], dist_lens=[0], tokens=rle([0] * 256 + [2, 0])), valid=False)
    add("header/distance-set-over-subscribed", _reject_header(rng, lit_lens=[0] + lit8, dist_lens=[1, 1, 1], tokens=rle([0] + lit8 + [1, 1, 1])), valid=False)
    add("header/distance-set-incomplete", _reject_header(rng, lit_lens=[0] + lit8, dist_lens=[1, 2], tokens=rle([0] + lit8 + [1, 2])), valid=False)
    add("header/code-length-code-over-subscribed", _reject_header(rng, lit_lens=[0] + lit8, dist_lens=[0], clc={0: 1, 8: 1, 18: 1}, tokens=[]), valid=False)
    add("header/code-length-code-incomplete", _reject_header(rng, lit_lens=[0] + lit8, dist_lens=[0], clc={0: 1, 8: 2}, tokens=[]), valid=False)
    add("header/code-length-code-one-code", _reject_header(rng, lit_lens=[0] + lit8, dist_lens=[0], clc={8: 1}, tokens=[]), valid=False)
    add("header/code-length-code-empty", _reject_header(rng, lit_lens=[0] + lit8, dist_lens=[0], clc={}, tokens=[]), valid=False)
    add("header/hlit-287", _reject_header(rng, lit_lens=[0] + lit8, dist_lens=[0], hlit=287, clc={0: 1, 8: 2, 18: 2}, tokens=[0] + [8] * 256 + [(18, 31)]), valid=False)
    add("header/hdist-31", _reject_header(rng, lit_lens=[0] + lit8, dist_lens=[0], hdist=31, clc={0: 1, 8: 2, 18: 2}, tokens=[0] + [8] * 256 + [(18, 31)]), valid=False)
    # incomplete distance sets in blocks that are otherwise in order: nothing but the header is a reason to refuse them
    for name, dl, use in (("lone-distance-code-of-two-bits/sym0", [2], False), ("lone-distance-code-of-two-bits/sym0/used", [2], True),
                          ("lone-distance-code-of-two-bits/sym5/used", [0] * 5 + [2], True), ("lone-distance-code-of-fifteen-bits", [0, 15], True),
                          ("distance-set-incomplete/unused", [1, 2], False), ("distance-set-incomplete/used", [0, 1, 0, 3, 3], True)):
        f = TokenDeflate(open_block=False)
        f.dynamic(DEEP_LIT, dl, final=True, tokens=rle(DEEP_LIT + dl))
        f.literals(tail(60))
        if use: f.match(9, f.dist_in(1, 60, rng)); f.literals(tail(5))
        f.end_block()
        add("header/" + name, f, valid=False)

    for s in (286, 287):
        f = _open("fixed")
        f.literals(tail(10)); f.sym(s); f.literals(tail(10)); f.end_block()
        add("fixed/symbol-%d" % s, f, valid=False)
    for s in (30, 31):
        f = _open("fixed")
        f.literals(tail(40)); f.sym(257); f.dsym(s); f.literals(tail(10)); f.end_block()
        add("fixed/distance-%d" % s, f, ulen=53, valid=False)
    for kind, pos, length in REACH:
        add("distance=position+1/%s/%d/len%d" % (kind, pos, length), _x_reach(kind, pos, length, rng, excess=1), ulen=pos + length + 4, valid=False)
    for slow in (0, 1):   # the bit pattern a lone one-bit distance code leaves unassigned, behind a fast and behind a slow length code
        f = TokenDeflate(open_block=False)
        f.dynamic(DEEP_LIT, [1], final=True, tokens=rle(DEEP_LIT + [1]))
        f.literals(tail(30)); f.match(5, 1); f.sym(270 if slow else 258)
        if slow: f.bits(1, 2)
        f.bits(1, 1); f.literals(tail(10)); f.end_block()
        add("lone-distance-code/unassigned-pattern/%s" % ("slow" if slow else "fast"), f, ulen=30 + 5 + (24 if slow else 4) + 10, valid=False)
        f = TokenDeflate(open_block=False)
        f.dynamic(DEEP_LIT, [0], final=True, tokens=rle(DEEP_LIT + [0]))
        f.literals(tail(30)); f.sym(270 if slow else 258)
        if slow: f.bits(1, 2)
        f.bits(0, 1); f.literals(tail(10)); f.end_block()
        add("match-without-a-distance-code/%s" % ("slow" if slow else "fast"), f, ulen=30 + (24 if slow else 4) + 10, valid=False)
    for kind in ("fixed", "deep"):
        f = _open(kind)
        f.literals(tail(500)); f.match(120, 300); f.literals(tail(3)); f.end_block()
        add("ulen/one-more/%s" % kind, f, ulen=len(f.data) + 1, valid=False)
        g = _open(kind)
        g.literals(tail(500)); g.match(120, 300); g.literals(tail(3)); g.end_block()
        add("ulen/one-less-ended-by-a-literal/%s" % kind, g, ulen=len(g.data) - 1, valid=False)
        g = _open(kind)
        g.literals(tail(500)); g.match(240, 300); g.end_block()
        add("ulen/ends-inside-a-match/%s" % kind, g, ulen=len(g.data) - 100, valid=False)
    g = tiny_member(301)
    add("ulen/one-more/tiny", g, ulen=len(g.data) + 1, valid=False)
    g = mixed_member(207)
    add("ulen/one-less/mixed", g, ulen=len(g.data) - 1, valid=False)

    # truncations: inside the header, the code lengths, the symbols, and the last byte
    f = _open("fixed")
    f.literals(tail(900))
    for _ in range(100):
        f.match(int(rng.integers(3, 259)), f.dist_in(1, 900, rng)); f.literals(tail(int(rng.integers(0, 4))))
    f.end_block()
    full = f.payload()
    for cut in list(range(0, len(full), 37)) + [len(full) - 1]:
        g = TokenDeflate(open_block=False); g.data = f.data
        add("truncated/fixed@%d" % cut, g, payload=full[:cut], valid=False)
    f = deep_member(601, 900, 2600)
    full = f.payload()
    for cut in list(range(0, len(full), 23)) + [len(full) - 1]:
        g = TokenDeflate(open_block=False); g.data = f.data
        add("truncated/deep@%d" % cut, g, payload=full[:cut], valid=False)
    writers["truncated/deep"] = f
    return tuple(cases), writers


def corpus():
    """[(label, payload, ulen, want)]: want is the expected bytes of a valid case ("V-..."), None for a reject ("R-...")"""
    return list(_build()[0])


def writer(label):
    """the TokenDeflate that wrote a case (label without its V- / R- prefix): its bookkeeping, and dump() for its token list"""
    return _build()[1][label]


def writers(prefix):
    return {k: v for k, v in _build()[1].items() if k.startswith(prefix)}


def interleaved(cases):
    """valid and reject cases in turn, so that every valid member has a rejected neighbour; what is left of the longer list at the end"""
    v = [c for c in cases if c[3] is not None]
    r = [c for c in cases if c[3] is None]
    out = []
    for i in range(max(len(v), len(r))):
        if i < len(r): out.append(r[i])
        if i < len(v): out.append(v[i])
    return out
