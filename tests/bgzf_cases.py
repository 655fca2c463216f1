"""BGZF blocks for the inflate tests, made with Python's zlib: every level / window / memLevel / strategy zlib offers, over
data of many kinds, plus corrupt and hand-crafted hostile blocks, and members written token by token (fixed_block,
stored_block) that sit on the seams of the device inflater's window."""
import struct
import zlib

import numpy as np

MAX_IN = 0xff00
EOF_BLOCK = bytes([0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 0x42, 0x43, 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0])
STRATEGIES = [zlib.Z_DEFAULT_STRATEGY, zlib.Z_FILTERED, zlib.Z_HUFFMAN_ONLY, zlib.Z_RLE, zlib.Z_FIXED]


def member(payload, data_crc, isize):
    """A BGZF member around a raw DEFLATE payload."""
    bsize = 18 + len(payload) + 8
    assert bsize <= 65536
    return (bytes([0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 0x42, 0x43, 2, 0]) + struct.pack("<H", bsize - 1) + payload +
            struct.pack("<II", data_crc & 0xffffffff, isize & 0xffffffff))


def deflate_raw(data, level=6, wbits=-15, mem=8, strategy=zlib.Z_DEFAULT_STRATEGY):
    c = zlib.compressobj(level, zlib.DEFLATED, wbits, mem, strategy)
    return c.compress(data) + c.flush()


def block(data, level=6, wbits=-15, mem=8, strategy=zlib.Z_DEFAULT_STRATEGY):
    payload = deflate_raw(data, level, wbits, mem, strategy)
    if 18 + len(payload) + 8 > 65536:                        # incompressible bytes that a fixed code would grow: stored
        payload = deflate_raw(data, 0, wbits, 9, strategy)
    return member(payload, zlib.crc32(data), len(data))


def bgzf(data, size=MAX_IN, level=6, eof=True, **kw):
    """A whole BGZF stream of data cut every `size` bytes."""
    out = [block(data[i:i + size], level, **kw) for i in range(0, len(data), size)]
    return b"".join(out) + (EOF_BLOCK if eof else b"")


def sam_like(rng, n):
    lines, total = [], 0
    while total < n:
        L = int(rng.randint(50, 151))
        seq = "".join("ACGT"[x] for x in rng.randint(0, 4, L))
        qual = "".join(chr(33 + int(x)) for x in rng.randint(2, 41, L))
        s = f"r{rng.randint(1 << 30)}\t{rng.choice([99, 147, 83, 163])}\tchr{rng.randint(1, 23)}\t{rng.randint(1, 1 << 28)}\t60\t{L}M\t=\t{rng.randint(1, 1 << 28)}\t{rng.randint(-500, 500)}\t{seq}\t{qual}\tNM:i:0\n"
        lines.append(s); total += len(s)
    return "".join(lines).encode()[:n]


def data_kinds(rng, n):
    """(name, bytes) of length n."""
    dna = bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), n))
    runs = bytearray()
    while len(runs) < n:
        runs += bytes([int(rng.randint(0, 256))]) * int(rng.randint(1, 600))
    period = bytes(rng.randint(0, 256, 37, dtype=np.uint8)) * (n // 37 + 1)
    far = bytes(rng.randint(0, 256, 32768, dtype=np.uint8))
    far = (far + far + far)[:n]                              # matches at distance 32 768
    return [("zeros", bytes(n)), ("random", bytes(rng.randint(0, 256, n, dtype=np.uint8))), ("dna", dna), ("sam", sam_like(rng, n)),
            ("runs", bytes(runs[:n])), ("period37", period[:n]), ("far", far),
            ("text", (b"the quick brown fox jumps over the lazy dog " * (n // 44 + 1))[:n])]


def zlib_blocks(rng, n_random=0):
    """The parameter grid over the data kinds, then n_random blocks with random parameters."""
    cases = []
    for size in (0, 1, 2, 258, 5000, MAX_IN):
        for name, d in data_kinds(rng, size):
            for level in range(10):
                cases.append((d, dict(level=level)))
            for wbits in (-9, -12, -15):
                for strat in STRATEGIES:
                    cases.append((d, dict(level=9, wbits=wbits, mem=int(rng.randint(1, 10)), strategy=strat)))
    # 258-byte matches at distance 1 and 32 768
    cases.append((b"\x41" * MAX_IN, dict(level=9)))
    r = bytes(rng.randint(0, 256, 32768, dtype=np.uint8))
    cases.append(((r + r)[:MAX_IN], dict(level=9)))
    pool = [d for _, d in data_kinds(rng, 2 * MAX_IN)]
    for _ in range(n_random):
        size = int(rng.choice([rng.randint(0, 64), rng.randint(0, 4096), rng.randint(0, MAX_IN + 1)]))
        src = pool[int(rng.randint(len(pool)))]
        at = int(rng.randint(0, len(src) - size + 1))
        d = src[at:at + size]
        cases.append((d, dict(level=int(rng.randint(0, 10)), wbits=-int(rng.randint(9, 16)), mem=int(rng.randint(1, 10)),
                              strategy=STRATEGIES[int(rng.randint(len(STRATEGIES)))])))
    return [(block(d, **kw), d) for d, kw in cases]


class Bits:
    """LSB-first bit writer for hand-made DEFLATE streams."""
    def __init__(self):
        self.v, self.n = 0, 0

    def put(self, val, nb):
        self.v |= (val & ((1 << nb) - 1)) << self.n
        self.n += nb
        return self

    def put_rev(self, code, nb):                 # a Huffman code, most significant bit first
        for i in range(nb - 1, -1, -1):
            self.put((code >> i) & 1, 1)
        return self

    def bytes(self):
        return self.v.to_bytes((self.n + 7) // 8, "little")


def dynamic_header(cl_lens, lens, nlen, ndist):
    """A dynamic block header: code-length code cl_lens (19 lengths by symbol), then the nlen + ndist lengths written
    as literal code-length symbols (no repeats)."""
    order = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
    b = Bits().put(1, 1).put(2, 2).put(nlen - 257, 5).put(ndist - 1, 5).put(19 - 4, 4)
    for s in order:
        b.put(cl_lens[s], 3)
    codes = canonical(cl_lens)
    for x in lens:
        if x not in codes:
            return b
        b.put_rev(*codes[x])
    return b


def canonical(lens):
    codes, code = {}, 0
    for L in range(1, 16):
        for s, l in enumerate(lens):
            if l == L:
                codes[s] = (code, L)
                code += 1
        code <<= 1
    return codes


def crafted_bad_blocks():
    """Hand-made members every inflater must refuse: (name, bytes)."""
    out = []
    flat5 = [5] * 19                                        # 19 codes of 5 bits: an incomplete code-length code
    cl4 = [4] * 16 + [0] * 3                                # 16 codes of 4 bits: complete, symbols 0-15
    # the code-length code over-subscribed / incomplete
    out.append(("cl_oversubscribed", dynamic_header([1] * 19, [], 257, 1)))
    out.append(("cl_incomplete", dynamic_header(flat5, [], 257, 1)))
    out.append(("cl_empty", dynamic_header([0] * 19, [], 257, 1)))
    # literal/length lengths over-subscribed (286 codes of 1 bit), incomplete (two codes of 2 bits)
    out.append(("ll_oversubscribed", dynamic_header(cl4, [1] * 286 + [1], 286, 1)))
    inc = [0] * 257; inc[65] = 2; inc[256] = 2
    out.append(("ll_incomplete", dynamic_header(cl4, inc + [1], 257, 1)))
    noeob = [8] * 256 + [0]
    out.append(("ll_no_eob", dynamic_header(cl4, noeob + [1], 257, 1)))
    # distance code over-subscribed
    ok_ll = [8] * 226 + [9] * 60                          # 226 * 2 + 60 = 512 slots of 9 bits: a complete code
    out.append(("dist_oversubscribed", dynamic_header(cl4, ok_ll + [1, 1, 1], 286, 3)))
    # a repeat (symbol 16) with nothing before it
    cl16 = [5] * 16 + [1, 0, 0]                            # 16 codes of 5 bits and symbol 16 in 1 bit: complete
    b = dynamic_header(cl16, [], 257, 1)
    out.append(("repeat_first", b.put_rev(*canonical(cl16)[16]).put(0, 2)))
    # a fixed block with a match before any output (distance too far back)
    fixed = Bits().put(1, 1).put(1, 2)
    fixed.put_rev(0b0000001, 7)                            # length symbol 257 (length 3)
    fixed.put_rev(0, 5)                                    # distance symbol 0 (distance 1)
    fixed.put_rev(0, 7)                                    # end of block
    out.append(("dist_too_far", fixed))
    # one literal then a match of distance 2
    f2 = Bits().put(1, 1).put(1, 2).put_rev(0x30 + 65, 8).put_rev(0b0000001, 7).put_rev(1, 5).put_rev(0, 7)
    out.append(("dist_too_far_2", f2))
    # fixed literal/length 286 and distance 30
    out.append(("fixed_sym_286", Bits().put(1, 1).put(1, 2).put_rev(0b11000110, 8)))
    out.append(("fixed_dist_30", Bits().put(1, 1).put(1, 2).put_rev(0x30 + 65, 8).put_rev(0b0000001, 7).put_rev(30, 5).put_rev(0, 7)))
    # a stored block whose LEN and NLEN disagree, a stored block longer than the payload, block type 3
    out.append(("stored_nlen", Bits().put(1, 1).put(0, 2).put(0, 5).put(4, 16).put(0xfffa, 16).put(0x64636261, 32)))
    out.append(("stored_short", Bits().put(1, 1).put(0, 2).put(0, 5).put(100, 16).put(0xffff ^ 100, 16).put(0x64636261, 32)))
    out.append(("btype3", Bits().put(1, 1).put(3, 2).put(0, 13)))
    # no final block: the stream runs off the end
    out.append(("no_final", Bits().put(0, 1).put(1, 2).put_rev(0, 7)))
    res = []
    for name, b in out:
        payload = b.bytes() if isinstance(b, Bits) else b
        res.append((name, member(payload, 0, 4)))
    return res


# ---- hand-made streams for the seams of the device inflater's window (WaveSink of mgx_bgzf_inflate.hip) -------------------
_LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
_LEN_EXTRA = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
_DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193,
              12289, 16385, 24577]
_DIST_EXTRA = [0, 0, 0, 0] + [e for e in range(1, 14) for _ in (0, 1)]
TOK, WIN = 512, 4096                                          # kTok, kWin of the kernel: a window is expanded at 512 tokens or 4096 bytes


def _fixed_sym(b, s):
    if s < 144:
        b.put_rev(0x30 + s, 8)
    elif s < 256:
        b.put_rev(0x190 + s - 144, 9)
    elif s < 280:
        b.put_rev(s - 256, 7)
    else:
        b.put_rev(0xc0 + s - 280, 8)


def fixed_block(tokens, last, b=None):
    """A fixed-Huffman block (RFC 1951 3.2.6) of tokens ("L", byte) and ("M", len, dist), appended to the bit stream b.
    Nothing is checked but the ranges a code exists for: a distance may reach back past the output."""
    b = Bits() if b is None else b
    b.put(1 if last else 0, 1).put(1, 2)
    for t in tokens:
        if t[0] == "L":
            _fixed_sym(b, t[1])
            continue
        _, ln, dist = t
        assert 3 <= ln <= 258 and 1 <= dist <= 32768
        i = 28 if ln == 258 else max(k for k in range(28) if _LEN_BASE[k] <= ln)
        _fixed_sym(b, 257 + i)
        b.put(ln - _LEN_BASE[i], _LEN_EXTRA[i])
        j = max(k for k in range(30) if _DIST_BASE[k] <= dist)
        b.put_rev(j, 5)
        b.put(dist - _DIST_BASE[j], _DIST_EXTRA[j])
    _fixed_sym(b, 256)
    return b


def stored_block(data, last, b=None):
    b = Bits() if b is None else b
    b.put(1 if last else 0, 1).put(0, 2)
    b.put(0, -b.n % 8)
    b.put(len(data), 16).put(len(data) ^ 0xffff, 16)
    return b.put(int.from_bytes(data, "little"), 8 * len(data))


def lits(n, salt=0):
    return [("L", (i * 37 + i // 256 * 11 + salt) & 0xff) for i in range(n)]


def produced(tokens):
    return sum(1 if t[0] == "L" else t[1] for t in tokens)


def fill(n, salt=0, period=29):
    """tokens for n bytes: a short literal prefix, 258-byte matches over it, the rest"""
    out = lits(min(n, period), salt)
    left = n - len(out)
    while left >= 258 + 3 or left == 258:
        out.append(("M", 258, period)); left -= 258
    if left > 258:                                               # 259 or 260: leave a match of 3 or 4
        out.append(("M", 256, period)); left -= 256
    if left >= 3:
        out.append(("M", left, period)); left = 0
    return out + lits(left, salt + 1)


def windows(blocks):
    """The windows the kernel's sink expands for blocks ("F", tokens) / ("S", bytes): [(start in the output, tokens, bytes)]"""
    out, w0, nt, wb = [], 0, 0, 0
    for kind, x in blocks:
        if kind == "S":
            if nt:
                out.append((w0, nt, wb))
            w0, nt, wb = w0 + wb + len(x), 0, 0
            continue
        assert kind == "F"
        for t in x:
            nt += 1; wb += 1 if t[0] == "L" else t[1]
            if nt == TOK or wb >= WIN:
                out.append((w0, nt, wb)); w0, nt, wb = w0 + wb, 0, 0
    return out + ([(w0, nt, wb)] if nt else [])


def to_window_start(tokens):
    """tokens + literals up to the next point at which the sink's window is empty"""
    tokens = list(tokens)
    while True:
        w = windows([("F", tokens)])
        if sum(x[2] for x in w) == produced(tokens) and (not w or w[-1][1] == TOK or w[-1][2] >= WIN):
            return tokens
        tokens.append(("L", (len(tokens) * 5 + 1) & 0xff))


def assemble(blocks):
    """-> the raw DEFLATE payload of blocks ("F", tokens) / ("S", bytes) / ("Z", a Bits holding one non-final block)"""
    b = Bits()
    for i, (kind, x) in enumerate(blocks):
        last = i == len(blocks) - 1
        if kind == "F":
            fixed_block(x, last, b)
        elif kind == "S":
            stored_block(x, last, b)
        else:
            assert not last
            b.put(x.v, x.n)
    return b.bytes()


def dynamic_block_bits(data, before, after):
    """zlib's level-9 dynamic block for `data` as bits, not final, cut to its exact length.  zlib pads its last byte with
    up to 7 zero bits; the length is the one at which the block, set between two fixed blocks, decodes to the whole."""
    raw = deflate_raw(data, 9)
    assert raw[0] & 7 == 5                                       # BFINAL, BTYPE 10: one dynamic block
    want = bytes(t[1] for t in before) + data + bytes(t[1] for t in after)
    for cut in range(8):
        z = Bits()
        z.v, z.n = int.from_bytes(raw, "little") & ~1, 8 * len(raw) - cut
        z.v &= (1 << z.n) - 1
        try:
            d = zlib.decompressobj(-15)
            if d.decompress(assemble([("F", before), ("Z", z), ("F", after)])) == want and d.eof:
                return z
        except zlib.error:
            pass
    raise AssertionError("no cut of zlib's block decodes")


def _member_of(blocks, isize=None, flip_last=False):
    payload = assemble(blocks)
    d = zlib.decompressobj(-15)
    want = d.decompress(payload)                                 # the reference: zlib's own inflate of the payload
    assert d.eof and not d.unused_data
    crc = zlib.crc32(want[:-1] + bytes([want[-1] ^ 1])) if flip_last else zlib.crc32(want)
    return member(payload, crc, len(want) if isize is None else isize), want


def window_seam_cases():
    """(name, member, want): single members whose tokens are placed on the seams of the device sink -- the token and byte
    limits of a window, sources across a window's start, link chains, block kinds in one member, output lengths around the
    64-way CRC split.  want is zlib's inflate of the payload; the windows a case is meant to produce are asserted here."""
    cases = []

    def add(name, blocks, expect=None):
        if expect is not None:
            assert expect(windows(blocks)), (name, windows(blocks)[:6])
        m, want = _member_of(blocks)
        cases.append((name, m, want))

    # token count: a window of exactly 512 literals, one less, one more, and the same at the second window
    for n in (511, 512, 513, 1023, 1024, 1025):
        add(f"lit{n}", [("F", lits(n, n))], lambda w, n=n: [x[1] for x in w] == [TOK] * (n // TOK) + [n % TOK] * (n % TOK > 0))
    # window bytes: the fullest window (4095 + 258 cells), exactly 4096, 4096 reached by a 3-byte match
    pre = lits(37) + [("M", 258, 37)] * 15
    assert produced(pre) == 3907
    add("win4353", [("F", pre + [("M", 188, 37), ("M", 258, 100)] + lits(5, 3))], lambda w: w[0] == (0, 54, WIN + 257) and w[1][0] == WIN + 257)
    add("win4096", [("F", pre + [("M", 189, 37)] + lits(5, 3) + [("M", 30, 4000)])], lambda w: w[0] == (0, 53, WIN) and w[1][0] == WIN)
    add("win4093+3", [("F", pre + [("M", 186, 37), ("M", 3, 1)] + lits(5, 3) + [("M", 30, 4099)])], lambda w: w[0] == (0, 54, WIN))
    # the source of a match across the window's start: the first window is 512 literals
    first = lits(TOK, 9)
    at_start = lambda w: w[0] == (0, TOK, TOK) and w[1][0] == TOK                # noqa: E731
    add("src_before_periodic", [("F", first + [("M", 100, 5)] + lits(3))], at_start)                 # dist < len, every byte read back
    add("src_mixed_periodic", [("F", first + lits(2, 1) + [("M", 50, 7)] + lits(3))], at_start)        # dist < len, tstart < dist
    add("src_dist_eq_len", [("F", first + [("M", 20, 20)] + lits(2, 1) + [("M", 9, 9)])], at_start)
    add("src_1_before", [("F", first + lits(4, 1) + [("M", 3, 5), ("M", 200, 300)])], at_start)        # dist > len: 1 byte before the window
    add("src_2_before", [("F", first + lits(4, 1) + [("M", 4, 6), ("M", 258, 259)])], at_start)
    far = to_window_start(lits(40, 2) + [("M", 258, 40)] * 128)
    assert produced(far) >= 32768
    add("src_32768_before", [("F", far + lits(1, 5) + [("M", 10, 32768), ("M", 258, 32768)])],
        lambda w: any(x[0] == produced(far) for x in w))
    # link chains
    add("chain_dist1", [("F", lits(1, 65) + [("M", 258, 1)] * 16)], lambda w: w == [(0, 17, 1 + 16 * 258)])
    for d in (2, 3, 7):
        add(f"chain_dist{d}", [("F", lits(d, d) + [("M", max(d, 3), d)] * 500 + lits(2))], lambda w, d=d: w == [(0, 502 + d, d + 500 * max(d, 3) + 2)])
    add("chain_three_windows", [("F", lits(1, 66) + [("M", 258, 1)] * 50 + lits(1) + [("M", 258, 2)] * 3)], lambda w: len(w) >= 4)
    # block kinds in one member
    some = lits(100, 4) + [("M", 40, 60)]
    sbytes = bytes((i * 89 + 7) & 0xff for i in range(200))
    add("fixed_stored_fixed", [("F", some), ("S", sbytes), ("F", [("M", 250, 260), ("L", 1), ("M", 30, 450)])],
        lambda w: w == [(0, 101, 140), (340, 3, 281)])
    add("stored_with_tokens_pending", [("F", lits(10, 8)), ("S", sbytes[:50]), ("F", [("M", 58, 58)])], lambda w: w[0] == (0, 10, 10))
    add("stored_empty_not_last", [("F", some), ("S", b""), ("F", [("M", 100, 140)] + lits(3))], lambda w: w[1][0] == 140)
    add("stored_empty_last", [("F", some), ("S", b"")])
    add("stored_empty_first", [("S", b""), ("F", some)])
    add("stored_only_empty", [("S", b"")])
    for n in (1, 63, 64, 65):
        add(f"stored{n}_then_match", [("F", lits(20, n)), ("S", sbytes[:n]), ("F", [("M", 30, n + 10), ("M", 258, n + 40)])])
    add("final_empty_fixed", [("F", some), ("F", [])])
    text = b"".join(b"line %d of the dynamic block, with some text to code\n" % (i * i) for i in range(60))
    before, after = lits(300, 6), lits(5, 7)
    z = dynamic_block_bits(text, before, after)
    add("fixed_dynamic_fixed", [("F", before), ("Z", z), ("F", after + [("M", 258, len(text) + 100), ("M", 100, 4)])])
    # output length: the CRC's 64 lanes and the x^(8n) shift
    for n in (0, 1, 63, 64, 65, 127, 4095, 4096, 4097, 65535, 65536):
        add(f"isize{n}", [("F", fill(n, n))])
        assert len(cases[-1][2]) == n and len(cases[-1][1]) < 4000
    assert len({c[0] for c in cases}) == len(cases)
    return cases


def window_seam_hostile():
    """(name, member, status): members the inflater must refuse with this status (bgzf_inflate_core.h: 11 distance too far
    back, 12 output longer than ISIZE, 14 CRC mismatch), each at a seam of the window."""
    out = []
    payload = fixed_block(lits(TOK, 9) + lits(2, 1) + [("M", 10, TOK + 3)] + lits(4), True).bytes()      # one byte before the output
    out.append(("dist_too_far_across_window", member(payload, 0, TOK + 16), 11))
    toks = lits(37) + [("M", 258, 37)] * 15 + [("M", 188, 37)]
    assert produced(toks) == WIN - 1 and windows([("F", toks)]) == [(0, 53, WIN - 1)]
    good, want = _member_of([("F", toks + [("M", 257, 100)])])
    payload = fixed_block(toks + [("M", 258, 100)], True).bytes()                                  # ISIZE + 1 bytes, over the window's end
    out.append(("overflow_across_window", member(payload, zlib.crc32(want), len(want)), 12))
    m, want = _member_of([("F", fill(4094, 3) + lits(3, 8))], flip_last=True)                     # lane 63 covers bytes 4095 and 4096
    assert len(want) == 4097
    out.append(("crc_last_lane", m, 14))
    return out


def mutate(rng, blk):
    """A corrupted copy of a member: bit flips in the payload or trailer, a truncated payload, or random payload bytes."""
    b = bytearray(blk)
    kind = int(rng.randint(4))
    if kind == 0 and len(b) > 26:
        for _ in range(int(rng.randint(1, 4))):
            i = int(rng.randint(18, len(b)))
            b[i] ^= 1 << int(rng.randint(8))
    elif kind == 1 and len(b) > 26:
        cut = int(rng.randint(18, len(b) - 8))
        b = b[:cut] + b[-8:]
        b[16:18] = struct.pack("<H", len(b) - 1)
    elif kind == 2 and len(b) > 26:
        n = len(b) - 26
        b[18:18 + n] = bytes(rng.randint(0, 256, n, dtype=np.uint8))
    else:
        i = int(rng.randint(18, max(19, len(b))))           # a flip in the first DEFLATE bytes: block types and headers
        if i < len(b):
            b[min(i, 18 + int(rng.randint(0, 4)))] ^= 1 << int(rng.randint(8))
    return bytes(b)


def case_file(path, pairs):
    """pairs: (block, want bytes or None) -> the driver's case file."""
    with open(path, "wb") as f:
        for blk, want in pairs:
            f.write(struct.pack("<I", len(blk))); f.write(blk)
            if want is None:
                f.write(struct.pack("<I", 0xFFFFFFFF))
            else:
                f.write(struct.pack("<I", len(want))); f.write(want)


def walk(stream):
    """Python's own view of the BGZF blocks of a stream: [(offset, isize, crc)], stop offset."""
    out, at = [], 0
    while at + 18 <= len(stream):
        h = stream[at:at + 18]
        if h[:3] != b"\x1f\x8b\x08" or not (h[3] & 4) or h[10:16] != b"\x06\x00BC\x02\x00":
            break
        bs = struct.unpack_from("<H", h, 16)[0] + 1
        if at + bs > len(stream):
            break
        crc, isize = struct.unpack_from("<II", stream, at + bs - 8)
        out.append((at, isize, crc))
        at += bs
    return out, at
