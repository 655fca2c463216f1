"""BGZF blocks for the inflate tests, made with Python's zlib: every level / window / memLevel / strategy zlib offers, over
data of many kinds, plus corrupt and hand-crafted hostile blocks."""
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
