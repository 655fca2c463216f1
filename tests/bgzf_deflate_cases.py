"""Instruments and inputs for the seam tests of the device BGZF compressor (k_bgzf_deflate, csrc/mgx_bgzf.hip), pure
Python and numpy: a strict token-level inflater that shows what a block's header and tokens ARE, package-merge for what
a length limit costs, the member check, and generators built from the kernel's own constants.  What a test claims the
kernel reached is read from the bytes it emitted, never from the kernel."""
import struct
import zlib

import numpy as np

MAX_IN = 0xff00
# the kernel's geometry (mgx_bgzf.hip): 64-position chunks, match windows of kWin = 896 positions (14 wavefronts), groups of kGrp = 4
# windows = 3584 positions = 56 chunks (kGrpPos, kGrpChunks); the longest match and the farthest distance are deflate_rules.h's
K_CHUNK, K_WIN, K_GRP_POS, K_MAX_MATCH, K_MAX_DIST = 64, 896, 4 * 896, 258, 32768
# the knob values under which the cost rule drops every match of at most 16 bytes (its literal price is at most
# 255 * len <= 4080 = 16 * 255), so that data without a repeated 17-byte substring comes out as literals only
LITERAL_ONLY_ENV = {"MGX_BGZF_COST_BASE": "255", "MGX_BGZF_COST_RLE": "255"}

CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145,
             8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0] + [e for e in range(1, 14) for _ in (0, 1)]


class InflateError(ValueError):
    pass


# ---- the strict token-level inflater -------------------------------------------------------------------------------
def _table(lens, kind):
    """Decoding table of a canonical code: entry [next maxl bits, LSB first] = (symbol, length).  Refuses what zlib's
    inflate_table refuses: an over-subscribed code, and an incomplete one unless it is a literal/length or distance
    code of a single 1-bit symbol (or a distance code with no symbol at all)."""
    used = sorted((l, s) for s, l in enumerate(lens) if l)
    kraft = sum(1 << (15 - l) for l, _ in used)
    if kraft > 1 << 15:
        raise InflateError(kind + " code over-subscribed")
    if kraft < 1 << 15 and not (kind != "cl" and (not used and kind == "dist" or len(used) == 1 and used[0][0] == 1)):
        raise InflateError(kind + " code incomplete")
    maxl = used[-1][0] if used else 0
    tab = [None] * (1 << maxl)
    code, prev = 0, 0
    for l, s in used:
        code <<= l - prev
        prev = l
        rev = int(format(code, "0%db" % l)[::-1], 2)
        tab[rev::1 << l] = [(s, l)] * (1 << (maxl - l))
        code += 1
    return tab, maxl


_FIXED_LL = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
_FIXED_D = [5] * 32


def inflate_tokens(payload):
    """Raw DEFLATE -> (bytes, blocks, payload bytes used).  A block is a dict: btype, and for a dynamic block hlit, hdist,
    hclen, cl_lens (19, by symbol), cl_syms [(symbol, extra)], ll_lens, d_lens; tokens: a literal (int) or (length,
    distance).  Raises InflateError on anything zlib's inflate refuses."""
    data = bytes(payload)
    end = len(data)
    pos, acc, n = 0, 0, 0
    out = bytearray()
    blocks = []

    def take(k):
        nonlocal pos, acc, n
        while n < k:
            if pos >= end:
                raise InflateError("the stream runs off the end of the payload")
            acc |= data[pos] << n
            pos += 1
            n += 8
        v = acc & ((1 << k) - 1)
        acc >>= k
        n -= k
        return v

    def symbol(tab, maxl):
        nonlocal pos, acc, n
        while n < maxl and pos < end:
            acc |= data[pos] << n
            pos += 1
            n += 8
        e = tab[acc & ((1 << maxl) - 1)] if maxl else None
        if e is None or e[1] > n:
            raise InflateError("no such code" if e is None else "the stream runs off the end of the payload")
        acc >>= e[1]
        n -= e[1]
        return e[0]

    final = 0
    while not final:
        final = take(1)
        blk = {"btype": take(2), "tokens": []}
        blocks.append(blk)
        if blk["btype"] == 3:
            raise InflateError("block type 3")
        if blk["btype"] == 0:
            pos -= n >> 3                                    # back to the byte boundary: whole unread bytes return
            acc, n = 0, 0
            ln, nln = take(16), take(16)
            if ln != nln ^ 0xffff:
                raise InflateError("stored LEN and NLEN disagree")
            if pos + ln > end:
                raise InflateError("stored block longer than the payload")
            out += data[pos:pos + ln]
            blk["tokens"] = list(data[pos:pos + ln])
            pos += ln
            continue
        if blk["btype"] == 1:
            ll_lens, d_lens = _FIXED_LL, _FIXED_D
        else:
            hlit, hdist, hclen = take(5) + 257, take(5) + 1, take(4) + 4
            if hlit > 286 or hdist > 30:
                raise InflateError("too many length or distance symbols")
            cl_lens = [0] * 19
            for s in CL_ORDER[:hclen]:
                cl_lens[s] = take(3)
            ctab, cmax = _table(cl_lens, "cl")
            lens, syms = [], []
            while len(lens) < hlit + hdist:
                s = symbol(ctab, cmax)
                if s < 16:
                    syms.append((s, 0))
                    lens.append(s)
                    continue
                if s == 16 and not lens:
                    raise InflateError("repeat with nothing before it")
                ex = take(2 if s == 16 else 3 if s == 17 else 7)
                syms.append((s, ex))
                lens += [lens[-1] if s == 16 else 0] * (ex + (3 if s < 18 else 11))
            if len(lens) > hlit + hdist:
                raise InflateError("code lengths overrun HLIT + HDIST")
            ll_lens, d_lens = lens[:hlit], lens[hlit:]
            if not ll_lens[256]:
                raise InflateError("no end-of-block code")
            blk.update(hlit=hlit, hdist=hdist, hclen=hclen, cl_lens=cl_lens, cl_syms=syms, ll_lens=ll_lens, d_lens=d_lens)
        ltab, lmax = _table(ll_lens, "ll")
        dtab, dmax = _table(d_lens, "dist")
        tokens = blk["tokens"]
        while True:
            s = symbol(ltab, lmax)
            if s < 256:
                out.append(s)
                tokens.append(s)
                continue
            if s == 256:
                break
            if s > 285:
                raise InflateError("literal/length symbol %d" % s)
            length = LEN_BASE[s - 257] + take(LEN_EXTRA[s - 257])
            ds = symbol(dtab, dmax)
            if ds > 29:
                raise InflateError("distance symbol %d" % ds)
            dist = DIST_BASE[ds] + take(DIST_EXTRA[ds])
            if dist > len(out):
                raise InflateError("distance beyond the output so far")
            at = len(out) - dist
            if dist >= length:
                out += out[at:at + length]
            else:
                out += (out[at:] * (length // dist + 1))[:length]
            tokens.append((length, dist))
    return bytes(out), blocks, pos - (n >> 3)


def dist_symbol(dist):
    return max(s for s in range(30) if DIST_BASE[s] <= dist)


def token_histograms(tokens):
    """Literal/length (286, end-of-block counted) and distance (30) symbol counts of a token list."""
    ll, d = [0] * 286, [0] * 30
    ll[256] = 1
    for t in tokens:
        if isinstance(t, tuple):
            ll[max(s for s in range(29) if LEN_BASE[s] <= t[0]) + 257] += 1
            d[dist_symbol(t[1])] += 1
        else:
            ll[t] += 1
    return ll, d


def kraft(lens):
    """The Kraft sum of a length list in units of 2^-15: a complete code gives exactly 1 << 15."""
    return sum(1 << (15 - l) for l in lens if l)


def runs(lens):
    """[(value, run length)] of a list."""
    out = []
    for v in lens:
        if out and out[-1][0] == v:
            out[-1][1] += 1
        else:
            out.append([v, 1])
    return [tuple(r) for r in out]


def run_encodings(lens, cl_syms):
    """The header's code-length symbols cut at the runs of the length list they spell: [(value, run length, start index,
    [(symbol, extra)])].  A symbol repeats one value, so none straddles two runs."""
    out, k, at = [], 0, 0
    for v, r in runs(lens):
        got, enc = 0, []
        while got < r:
            s, ex = cl_syms[k]
            k += 1
            enc.append((s, ex))
            got += 1 if s < 16 else ex + (3 if s < 18 else 11)
        assert got == r, (v, r, enc)
        out.append((v, r, at, enc))
        at += r
    assert k == len(cl_syms)
    return out


# ---- package-merge ----------------------------------------------------------------------------------------------------
def limited_cost(freqs, limit):
    """The least total bits of any prefix code for the non-zero counts with no code longer than `limit` (package-merge:
    the 2n - 2 cheapest items of the last merged list).  One symbol costs one bit each time, as in DEFLATE."""
    w = sorted(f for f in freqs if f)
    n = len(w)
    if n < 2:
        return sum(w)
    assert n <= 1 << limit
    cur = w
    for _ in range(limit - 1):
        packages = [cur[i] + cur[i + 1] for i in range(0, len(cur) - 1, 2)]
        cur = sorted(w + packages)[:2 * n - 2]
    return sum(cur[:2 * n - 2])


# ---- the member check ---------------------------------------------------------------------------------------------------
def check_member(block, want):
    """What check_blocks of test_bgzf_gpu.py asks of a block, and two bounds on its size."""
    block, want = bytes(block), bytes(want)
    assert block[:4] == b"\x1f\x8b\x08\x04" and block[10:16] == b"\x06\x00BC\x02\x00"       # gzip + BGZF extra field
    assert struct.unpack("<H", block[16:18])[0] + 1 == len(block)
    d = zlib.decompressobj(-15)
    got = d.decompress(block[18:-8]) + d.flush()
    assert d.eof and d.unused_data == b""
    assert got == want
    crc, isize = struct.unpack("<II", block[-8:])
    assert crc == zlib.crc32(want) and isize == len(want)
    assert len(block) <= 65536
    assert len(block) <= len(want) + 5 + 26
    return True


def btype(block):
    return (block[18] >> 1) & 3


def split_blocks(out, out_off):
    out = bytes(out)
    return [out[int(out_off[i]):int(out_off[i + 1])] for i in range(len(out_off) - 1)]


def offsets_of(pieces):
    return np.concatenate([[0], np.cumsum([len(p) for p in pieces])]).astype(np.uint64)


# ---- literal-only data --------------------------------------------------------------------------------------------------
def literal_only_ok(data):
    """True if no match longer than 16 bytes exists in data: no 17-byte substring occurs twice (overlapping occurrences
    count) and no byte repeats 17 times in a row."""
    a = np.frombuffer(bytes(data), dtype=np.uint8)
    if len(a) < 17:
        return True
    eq = np.concatenate([[0], (a[1:] == a[:-1]).astype(np.int64)])
    reset = np.where(eq == 0, np.arange(len(a)), 0)
    run = np.arange(len(a)) - np.maximum.accumulate(reset) + 1                   # length of the run that ends here
    if run.max() >= 17:
        return False
    win = np.ascontiguousarray(np.lib.stride_tricks.sliding_window_view(a, 17)).view(np.dtype((np.void, 17))).ravel()
    return len(np.unique(win)) == len(win)


def shuffled_literal_only(counts, seed):
    """Bytes with the given count per byte value {value: count}, shuffled; seeds are tried until literal_only_ok.
    Returns (bytes, seed used)."""
    base = np.concatenate([np.full(c, v, dtype=np.uint8) for v, c in sorted(counts.items())])
    for s in range(seed, seed + 200):
        d = np.random.RandomState(s).permutation(base).tobytes()
        if literal_only_ok(d):
            return d, s
    raise AssertionError("no seed gives literal-only data")


def dyadic_counts(ll_lens):
    """{byte value: 2^(K - length)} for a planned literal length list (index 256 = end-of-block, which has count 1 and so the
    longest length K).  The histogram is dyadic and sums to 2^K: its Huffman lengths are the planned ones whatever the
    tie-breaking."""
    assert len(ll_lens) == 257
    k = max(ll_lens)
    assert ll_lens[256] == k and kraft(ll_lens) == 1 << 15
    return {v: 1 << (k - l) for v, l in enumerate(ll_lens[:256]) if l}


def lens_from_segments(segments):
    """[(length, count)] -> the 257 planned lengths."""
    lens = [l for l, c in segments for _ in range(c)]
    assert len(lens) == 257, len(lens)
    return lens


FIB = [1, 1]
while len(FIB) < 24:
    FIB.append(FIB[-1] + FIB[-2])            # FIB[k - 1] = F_k


def case_a(seed=0):
    """Literal/length code past 15 bits: byte values 0..20 with counts F2..F22 (46 366 bytes); with end-of-block the histogram
    is F1..F22, whose Huffman tree is a chain 21 deep."""
    data, _ = shuffled_literal_only({v: FIB[v + 1] for v in range(21)}, seed)
    return data


# case B: the lengths of the 82 used byte values (end-of-block is the 34th symbol of 10 bits)
CASE_B_MULTISET = {2: 1, 3: 1, 5: 13, 6: 8, 8: 5, 9: 21, 10: 33}
CASE_B_CL_HISTOGRAM = {10: 34, 9: 21, 5: 13, 6: 8, 8: 5, 18: 3, 1: 2, 3: 1, 2: 1}


def case_b(seed=0):
    """Code-length code past 7 bits -> (bytes, planned ll_lens).  Layout of the 257 lengths: 28 used, 58 zeros, 28 used, 58 zeros,
    26 used, 58 zeros, end-of-block; the used lengths shuffled until no four neighbours are equal (no symbol 16)."""
    pool = [l for l, c in sorted(CASE_B_MULTISET.items()) for _ in range(c)]
    rng = np.random.RandomState(seed)
    while True:
        used = [int(x) for x in rng.permutation(pool)]
        parts = [used[:28], used[28:56], used[56:]]
        if all(r < 4 for part in parts for _, r in runs(part)):
            break
    lens = parts[0] + [0] * 58 + parts[1] + [0] * 58 + parts[2] + [0] * 58 + [10]
    data, _ = shuffled_literal_only(dyadic_counts(lens), seed)
    return data, lens


def header_histogram(ll_lens, d_lens=(1, 1)):
    """The code-length symbol counts of a header whose zero runs are all 11..138 long and whose other runs are shorter than 4."""
    h = {}
    for v, r in runs(list(ll_lens) + list(d_lens)):
        if v == 0:
            assert 11 <= r <= 138
            h[18] = h.get(18, 0) + 1
        else:
            assert r < 4
            h[v] = h.get(v, 0) + r
    return h


# ---- case C: header runs ------------------------------------------------------------------------------------------------
def _zero_run_plan(z):
    """21 used byte values around a zero run of z (139..141): a run of 10 fours, the zero run, five fours and 5, 6, .., 10."""
    tail = 256 - 10 - z - 11
    return lens_from_segments([(4, 10), (0, z), (4, 5), (5, 1), (6, 1), (7, 1), (8, 1), (9, 1), (10, 1), (0, tail), (10, 1)])


HEADER_PLANS = {
    # non-zero runs of 2, 3, 4, 7, 8 and 10 between zero runs of 1, 2, 3, 10, 11 and 138
    "runs": lens_from_segments([(2, 2), (0, 1), (4, 3), (0, 2), (5, 4), (0, 3), (7, 7), (0, 10), (6, 8), (0, 11), (11, 10), (0, 138),
                                (9, 1), (0, 55), (11, 2)]),
    "zeros139": _zero_run_plan(139),
    "zeros140": _zero_run_plan(140),
    "zeros141": _zero_run_plan(141),
}
FAR_PERIOD = 24577            # the least distance of distance symbol 29


def header_cases(seed=0):
    """[(name, bytes, planned ll_lens or None)] for a compressor under LITERAL_ONLY_ENV.
      runs, zeros139..141   literal-only dyadic blocks that spell HEADER_PLANS
      fib15                 counts F2..F16 over 15 byte values: lengths 15, 15, 14, .., 1 without any limiting, so code-length
                            symbol 15 is used and HCLEN is 19
      zeros258              a literal and eight 258-byte matches at distance 1: symbol 285 (HLIT = 286) has half the weight and one
                            bit, and the distance lengths 1, 1 continue its run
      far                   64-valued random bytes of period FAR_PERIOD: its matches lie FAR_PERIOD back (HDIST = 30).  It cannot
                            be small; the hash table keeps one position per value, so only about one position in e^6 finds it."""
    out = []
    for k, (name, lens) in enumerate(HEADER_PLANS.items()):
        data, _ = shuffled_literal_only(dyadic_counts(lens), seed + 1000 * k)
        out.append((name, data, lens))
    fib, _ = shuffled_literal_only({3 * v + 1: FIB[v + 1] for v in range(15)}, seed)
    lens = [0] * 257
    for v in range(15):
        lens[3 * v + 1] = 15 - v if v else 15
    lens[256] = 15
    out.append(("fib15", fib, lens))
    out.append(("zeros258", bytes(1 + 8 * 258), None))
    rng = np.random.RandomState(seed)
    prefix = rng.randint(0, 64, FAR_PERIOD, dtype=np.uint8).tobytes()
    out.append(("far", (prefix * 2)[:40000], None))
    return out


HEADER_COVERAGE = (
    [("symbol", s, e) for s, e in ((17, 0), (17, 7), (18, 0), (18, 127), (16, 0), (16, 3))] +
    [("zero run", 139, ((18, 127), (0, 0))), ("zero run", 140, ((18, 127), (0, 0), (0, 0))), ("zero run", 141, ((18, 127), (17, 0))),
     ("zero run", 1, ((0, 0),)), ("zero run", 2, ((0, 0), (0, 0)))] +
    [("non-zero run", r) for r in (2, 3, 4, 7, 8, 10)] +
    [("run crosses into the distance lengths",), ("hlit", 257), ("hlit", 286), ("hdist", 2), ("hdist", 30), ("two hclen values",)])


def header_coverage(headers):
    """What of HEADER_COVERAGE a set of decoded dynamic-block headers (dicts of inflate_tokens) contains."""
    seen, hclen = set(), set()
    for h in headers:
        hclen.add(h["hclen"])
        seen.add(("hlit", h["hlit"]))
        seen.add(("hdist", h["hdist"]))
        for s, e in h["cl_syms"]:
            seen.add(("symbol", s, e))
        for v, r, at, enc in run_encodings(h["ll_lens"] + h["d_lens"], h["cl_syms"]):
            if v == 0:
                seen.add(("zero run", r, tuple(enc)))
            else:
                seen.add(("non-zero run", r))
                if at < h["hlit"] < at + r:
                    seen.add(("run crosses into the distance lengths",))
    if len(hclen) >= 2:
        seen.add(("two hclen values",))
    return seen


def planned_header(ll_lens):
    """The header fields a literal-only block with these planned lengths must show, whatever the compressor: HLIT 257,
    distance lengths 1, 1, and the runs of the list (a header's symbols are cut at the runs).  Used on the CPU to show that
    the plans contain the runs the coverage table asks for."""
    return runs(list(ll_lens) + [1, 1])


# ---- case D: distance and length edges ---------------------------------------------------------------------------------
PERIODS = [1, 2, 3, 4, 5, 7, 63, 64, 65, 255, 256, 257, 258, 259, 895, 896, 897, 3583, 3584, 3585, 32767, 32768, 32769, 32770]
ZERO_RUN_STARTS = [62, 63, 64, 65]
ZERO_RUN_LENGTHS = [2, 3, 4, 63, 64, 65, 257, 258, 259, 260, 261, 516, 517]


def periodic_pieces(seed=0):
    """[(P, bytes)]: a random prefix of P bytes repeated to 65 280 bytes (P >= 895) or 9 000."""
    rng = np.random.RandomState(seed)
    out = []
    for p in PERIODS:
        n = MAX_IN if p >= 895 else 9000
        prefix = rng.randint(0, 256, p, dtype=np.uint8).tobytes()
        out.append((p, (prefix * (n // p + 1))[:n]))
    return out


def nonzero_random(rng, n):
    return rng.randint(1, 256, n, dtype=np.uint8).tobytes()


def zero_run_pieces(seed=0):
    """[((k, r), bytes)]: k random non-zero bytes, r zeros, 40 random non-zero bytes."""
    rng = np.random.RandomState(seed)
    return [((k, r), nonzero_random(rng, k) + bytes(r) + nonzero_random(rng, 40)) for k in ZERO_RUN_STARTS for r in ZERO_RUN_LENGTHS]


# ---- the geometry grid --------------------------------------------------------------------------------------------------
GRID_LENGTHS = (list(range(10)) + [63, 64, 65, 127, 128, 129] + list(range(257, 263)) + [895, 896, 897, 898] +
                [3583, 3584, 3585, 3841, 3842, 3843, 7167, 7168, 7169] + [65279, 65280])
GRID_KINDS = ["bam_like", "four_values", "period300", "zeros1", "zeros4", "zeros64", "zeros300"]


def bam_like(rng, n_bytes):
    """Bytes with the statistics of BAM records (as bam_like of test_bgzf_gpu.py, on a RandomState)."""
    parts, total, k = [], 0, 0
    while total < n_bytes:
        l_seq = 151
        name = f"SYN:1:FC:1:{1100 + k % 40}:{(k * 37) % 20000}:{(k * 91) % 20000}".encode() + b"\0"
        core = struct.pack("<iiBBHHHiiii", k % 25, 1000 + 3 * k, len(name), int(rng.randint(0, 61)), 4681, 1, 99, l_seq, k % 25, 1300 + 3 * k, 450)
        seq = rng.randint(0, 256, (l_seq + 1) // 2, dtype=np.uint8).tobytes()
        q = np.repeat(rng.choice([2, 11, 25, 37], size=40, p=[0.05, 0.1, 0.25, 0.6]), rng.randint(1, 9, 40))[:l_seq]
        q = np.pad(q, (0, l_seq - len(q)), constant_values=37).astype(np.uint8).tobytes()
        rec = core + name + struct.pack("<I", l_seq << 4) + seq + q + b"NMC\x01MDZ151\0RGZgroup1\0ASC\x97XSC\x00"
        parts.append(struct.pack("<i", len(rec)) + rec)
        total += len(rec) + 4
        k += 1
    return b"".join(parts)[:n_bytes]


def grid_content(kind, source, n):
    """n bytes of a kind, cut from that kind's 65 280-byte source; zerosT: the last T bytes are zero."""
    if kind.startswith("zeros"):
        t = min(n, int(kind[5:]))
        return source[:n - t] + bytes(t)
    return source[:n]


def grid_sources(seed=0):
    rng = np.random.RandomState(seed)
    period = rng.randint(0, 256, 300, dtype=np.uint8).tobytes()
    src = {"bam_like": bam_like(rng, MAX_IN), "four_values": rng.randint(0, 4, MAX_IN, dtype=np.uint8).tobytes(),
           "period300": (period * (MAX_IN // 300 + 1))[:MAX_IN]}
    for t in (1, 4, 64, 300):
        src["zeros%d" % t] = nonzero_random(rng, MAX_IN)
    return src


def geometry_grid(kinds, seed=0):
    """Pieces of every GRID_LENGTHS x kinds x (start offset & 3), with filler pieces of 1-3 bytes that steer the start:
    (pieces, [(length, kind) or None for a filler])."""
    src = grid_sources(seed)
    rng = np.random.RandomState(seed + 1)
    pieces, tags, at = [], [], 0
    for kind in kinds:
        for n in GRID_LENGTHS:
            for align in range(4):
                fill = (align - at) & 3
                if fill:
                    pieces.append(nonzero_random(rng, fill))
                    tags.append(None)
                    at += fill
                pieces.append(grid_content(kind, src[kind], n))
                tags.append((n, kind))
                at += n
    return pieces, tags


def alignments_seen(pieces, tags):
    """{length: set of start offset & 3} of the tagged pieces, from the offsets the compressor is given."""
    off = offsets_of(pieces)
    seen = {}
    for i, tag in enumerate(tags):
        if tag is not None:
            seen.setdefault(tag[0], set()).add(int(off[i]) & 3)
    return seen


# ---- stored or dynamic --------------------------------------------------------------------------------------------------
def stored_sweep(seed=0):
    """2 000 random bytes followed by t zeros, t = 0..80.  A dynamic block saves next to nothing on the literals and spends some
    fifty bytes on its header; the zeros cost it three bytes however many they are (zlib -9 turns dynamic at t = 51 on these)."""
    rng = np.random.RandomState(seed)
    head = rng.randint(0, 256, 2000, dtype=np.uint8).tobytes()
    return [head + bytes(t) for t in range(81)]


def repeated_byte_sweep():
    return [b"\x5a" * n for n in range(1, 41)]


# ---- the pieces whose bytes must depend on their content only -------------------------------------------------
def content_only_pieces(seed=0):
    """About 60 pieces from the crafted blocks and the grid, large and tiny interleaved, some contents several times."""
    src = grid_sources(seed)
    per = dict(periodic_pieces(seed))
    zr = dict(zero_run_pieces(seed))
    big = [case_a(seed), per[32768], per[3584], per[897], per[7], per[1], src["bam_like"], src["four_values"], src["period300"],
           grid_content("zeros300", src["zeros300"], MAX_IN), bytes(MAX_IN), case_b(seed)[0],
           stored_sweep(seed)[0], stored_sweep(seed)[80], zr[(63, 258)], zr[(64, 517)]] + [d for _, d, _ in header_cases(seed)]
    tiny = []
    for n in (0, 1, 2, 3, 5, 9, 63, 64, 65, 129, 257, 258, 259, 262, 895, 896, 897, 3583, 3584, 3585, 3842, 7168):
        tiny.append(src["bam_like"][:n] if n % 2 else src["period300"][:n])
    pieces = []
    for i in range(max(len(big), len(tiny))):
        if i < len(big):
            pieces.append(big[i])
        if i < len(tiny):
            pieces.append(tiny[i])
        if i % 4 == 3:
            pieces.append(big[i % len(big) - 3])             # equal content again, later and at another offset
            pieces.append(tiny[i - 2])
    return pieces
