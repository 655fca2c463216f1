"""Test data for BAM input (tests/test_bam_host.py, test_bam_gpu.py, test_cli_bam_gpu.py): a spec-based BAM encoder over the
record dicts of sam_spec.parse_sam_line (SAMv1 4.2), the synthetic record set the compressed-SAM tests use, an edge list
for the key rules, seam and decoy inputs for the device index (dependent_decoys: misses that need several repair rounds,
with the index's guess rule restated to assert the layout), and mutations for the sanitizer run.  Test infrastructure
only."""
import struct

import numpy as np

import sam_spec

_AUX_FMT = {"c": "<b", "C": "<B", "s": "<h", "S": "<H", "i": "<i", "I": "<I", "f": "<f"}


def encode_aux(aux):
    out = b""
    for tag, typ, val in aux:
        out += tag.encode()
        if typ == "A":
            out += b"A" + val.encode()
        elif typ in _AUX_FMT:
            out += typ.encode() + struct.pack(_AUX_FMT[typ], val)
        elif typ in "ZH":
            out += typ.encode() + (val if isinstance(val, bytes) else val.encode()) + b"\0"
        else:                                                    # "B" + subtype
            out += b"B" + typ[1].encode() + struct.pack("<I", len(val)) + b"".join(struct.pack(_AUX_FMT[typ[1]], v) for v in val)
    return out


def encode_record(r):
    name = r["qname"].encode() + b"\0"
    seq = r["seq"]
    codes = [sam_spec.SEQ_CODES.index(c) for c in seq] + [0]
    seq4 = bytes(codes[i] << 4 | codes[i + 1] for i in range(0, len(seq), 2))
    beg, end = sam_spec.ref_span(r)
    bn = sam_spec.reg2bin(beg, end) if beg >= 0 else 4680
    body = struct.pack("<iiBBHHHiiii", r["tid"], r["pos"], len(name), r["mapq"], bn, len(r["cigar"]), r["flag"], len(seq), r["mtid"], r["mpos"], r["tlen"])
    body += name + struct.pack(f"<{len(r['cigar'])}I", *r["cigar"]) + seq4 + bytes(r["qual"]) + encode_aux(r["aux"])
    return struct.pack("<i", len(body)) + body


def encode_header(text, refs):
    t = text.encode()
    out = b"BAM\x01" + struct.pack("<i", len(t)) + t + struct.pack("<i", len(refs))
    for name, ln in refs:
        out += struct.pack("<i", len(name) + 1) + name.encode() + b"\0" + struct.pack("<i", ln)
    return out


def encode_bam(text, refs, recs):
    """-> (the inflated BAM bytes, offset of the first record, offset of every record)"""
    head = encode_header(text, refs)
    parts, at, p = [head], [], len(head)
    for r in recs:
        b = encode_record(r)
        at.append(p); parts.append(b); p += len(b)
    return b"".join(parts), len(head), np.array(at, dtype=np.uint64)


def raw_arrays(recs, target_len):
    """the mgx_raw_records_t arrays (pkg.sortdedup.pack) of record dicts"""
    off = lambda xs: np.concatenate([[0], np.cumsum([len(x) for x in xs])]).astype(np.uint64)  # noqa: E731
    cat = lambda xs, dt: np.concatenate([np.asarray(x, dtype=dt) for x in xs]) if sum(len(x) for x in xs) else np.zeros(0, dt)  # noqa: E731
    return dict(n_records=len(recs), flag=np.array([r["flag"] for r in recs], dtype=np.uint16),
                tid=np.array([r["tid"] for r in recs], dtype=np.int32), pos=np.array([r["pos"] for r in recs], dtype=np.int64),
                cigar_off=off([r["cigar"] for r in recs]), cigar=cat([r["cigar"] for r in recs], np.uint32),
                qual_off=off([r["qual"] for r in recs]), qual=cat([r["qual"] for r in recs], np.uint8),
                qname_off=off([r["qname"] for r in recs]), qname=np.frombuffer("".join(r["qname"] for r in recs).encode(), dtype=np.uint8).copy(),
                n_targets=len(target_len), target_len=np.asarray(target_len, dtype=np.uint64))


_SYNTH = {}


def synthetic(synth, tmp_dir):
    """The input of tests/test_cli_compressed_gpu.py as (SAM path, header text, refs, record dicts, BAM bytes, first, offsets)."""
    if "v" not in _SYNTH:
        from test_cli_gpu import make_sam
        raw = synth.gen_sortdedup_raw(6000, 77, n_contigs=3, contig_len=200000, dup_rate=0.3)
        p = str(tmp_dir / "synthetic.sam")
        make_sam(raw, p)
        text, refs, recs = sam_spec.parse_sam_text(open(p).read())
        data, first, at = encode_bam(text, refs, recs)
        _SYNTH["v"] = (p, text, refs, recs, data, first, at)
    return _SYNTH["v"]


def rec(qname, flag=0, tid=0, pos=1000, cigar=(), l_seq=None, qual=None, aux=(), mapq=30):
    cigar = list(cigar)
    if l_seq is None:
        l_seq = sum(c >> 4 for c in cigar if (c & 15) in (0, 1, 4, 7, 8)) if cigar else 20
    qual = [30] * l_seq if qual is None else list(qual)
    assert len(qual) == l_seq
    return dict(qname=qname, flag=flag, tid=tid, pos=pos, mapq=mapq, cigar=cigar, mtid=tid if flag & 1 else -1, mpos=pos + 50 if flag & 1 else -1,
                tlen=0, seq="ACGT" * (l_seq // 4) + "ACGT"[:l_seq % 4], qual=qual, aux=[list(a) for a in aux])


def C(text):
    """CIGAR text -> BAM operations"""
    out, num = [], ""
    for ch in text:
        if ch.isdigit():
            num += ch
        else:
            out.append(int(num) << 4 | sam_spec.CIGAR_OPS.index(ch)); num = ""
    return out


EDGE_REFS = [("chrA", 100000), ("chrB", 50000)]


def edge_records():
    """Every edge of the key rules, each as a single and inside a pair (forward + reverse mate), names kept apart by
    plain separator records."""
    shapes = [
        dict(cigar=[]), dict(cigar=C("5S10S")), dict(cigar=C("3H4S20M")), dict(cigar=C("3H4S20M5S2H")), dict(cigar=C("20M2D5M3N4M6S")),
        dict(cigar=C("10M"), l_seq=0, qual=[]), dict(cigar=C("7M")), dict(cigar=[], l_seq=0, qual=[]), dict(cigar=C("9M"), qual=[255] * 9),
        dict(cigar=C("2000M"), qual=[40] * 2000), dict(cigar=C("21M"), qual=[14, 15] * 10 + [0]),
        dict(tid=-1, pos=-1, cigar=[]), dict(tid=1, pos=-1, cigar=C("8M")), dict(tid=-1, pos=5, cigar=C("4S4M")),
        dict(cigar=C("30S100N"), l_seq=30),                     # the long-CIGAR placeholder's shape, no CG tag: taken as it stands
        dict(cigar=C("1=1X1I1P1M")),
    ]
    names = ["m:1:fc:2:1101:1500:2000", "m:fc:2:1101:1500:2000", "a:b:c:d:e", "m:1:fc:2:1101:1500:2000:9", "a::b:1:2:3:4", "a::b::c:11:22:33::",
             "m:1:fc:2:11x1:1500:2000", "m:1:fc:2:1101:+15:2000", "m:1:fc:2:1101: 15:-20", "m:1:fc:2:1101:1500:1234567890123456789",
             "m:1:fc:2:1101:1500:123456789012345678", "m:1:fc:2:70000:65536:65535", "q", "n" * 254, "abc", "abcd", "abc", ":::::::", "1:2:3:4:5:6", "m:1:fc:2:1101:1500:99999999999999999999"]
    out = []
    sep = lambda: rec(f"sep{len(out)}", cigar=C("5M"))          # noqa: E731
    for i, sh in enumerate(shapes):
        nm = names[i % 12]
        out.append(rec(f"single{i}:" + nm, **sh)); out.append(sep())
        out.append(rec(f"pair{i}:" + nm, flag=0x1 | 0x40, **sh)); out.append(rec(f"pair{i}:" + nm, flag=0x1 | 0x80 | 0x10, **sh)); out.append(sep())
    for nm in names:
        out.append(rec(nm, cigar=C("12M")))                     # as a single; "abc" / "abcd" / "abc" sit side by side here
    out.append(sep())
    for nm in names:
        out.append(rec(nm, flag=0x1 | 0x40, cigar=C("3S12M"))); out.append(rec(nm, flag=0x1 | 0x80 | 0x10, cigar=C("12M3S")))
        out.append(rec(nm, flag=0x1 | 0x100, cigar=C("12M")))   # an ignorable record inside the name group
    return out


def seam_records(tile=256):
    """(refs, record dicts, what each case places at a tile boundary) for tile 256: a start exactly on a boundary, block_size
    straddling one by 1, 2 and 3 bytes, a 5000-byte record over 19 tiles without a start, 38-byte records back to back."""
    refs = EDGE_REFS
    recs, at = [], len(encode_header("", refs))
    first = at

    def add(r):
        nonlocal at
        recs.append(r); at += len(encode_record(r))

    def pad_to(target_mod):
        """a record whose end lies at `target_mod` modulo the tile (its Z tag is sized for it)"""
        base = rec(f"pad{len(recs)}", cigar=C("10M"), aux=[("XP", "Z", "")])
        need = (target_mod - (at + len(encode_record(base)))) % tile
        base["aux"] = [["XP", "Z", "p" * need]]
        add(base)
        assert at % tile == target_mod % tile

    for straddle in (0, 1, 2, 3):
        pad_to(-straddle)                                      # the next record starts `straddle` bytes before a boundary
        add(rec(f"seam{straddle}", cigar=C("15M")))
        add(rec("plain", cigar=C("15M")))
    add(rec("long", cigar=C("15M"), aux=[("XL", "Z", "L" * 5000)]))
    for i in range(60):
        add(dict(qname="s", flag=0, tid=0, pos=i, mapq=0, cigar=[], mtid=-1, mpos=-1, tlen=0, seq="", qual=[], aux=[]))
    add(rec("last", cigar=C("15M")))
    assert len(encode_record(recs[-2])) == 38
    return refs, recs, first


def decoy_bam(pad, in_b_tag=False):
    """Records whose Z (or B,C) payload holds two consecutive well-formed fake records, `pad` bytes after the tag's start."""
    refs = EDGE_REFS
    fake = b"".join(encode_record(rec(f"fake{i}", cigar=C("20M"), tid=i)) for i in range(2))
    assert b"\0" in fake                                       # a Z tag cannot hold it as text: it is laid down as bytes below
    recs = []
    for k in range(6):
        r = rec(f"host{k}", cigar=C("25M"))
        payload = b"p" * pad + fake + b"q" * (300 + 37 * k)
        if in_b_tag:
            r["aux"] = [["XD", "BC", list(payload)]]
        else:
            r["aux"] = [["XD", "Z", payload]]
        recs.append(r)
    return refs, recs


MAX_RECORD = 1 << 28                                             # MGX_BAM_MAX_RECORD


def _fixed_ok(data, c, n_ref):
    """check_fixed and, with n_ref given, plausible (bam_record_core.h) of the 36 bytes at c -> (block_size, l_read_name) or None"""
    bs, tid, pos = struct.unpack_from("<iii", data, c)
    l_name = data[c + 12]
    n_cigar = struct.unpack_from("<H", data, c + 16)[0]
    l_seq, ntid, npos = struct.unpack_from("<iii", data, c + 20)
    if not 32 <= bs <= MAX_RECORD or l_name < 1 or l_seq < 0 or 32 + l_name + 4 * n_cigar + (l_seq + 1) // 2 + l_seq > bs:
        return None
    if n_ref is not None and not (-1 <= tid < n_ref and -1 <= ntid < n_ref and pos >= -1 and npos >= -1):
        return None
    return bs, l_name


def guess_hit(data, n, c, n_ref):
    """The index kernel's guess rule for a record start at c, restated: check_fixed, plausible, the record inside the
    data, the name's NUL, and follower_ok of what comes behind it."""
    if c + 36 > n:
        return False
    f = _fixed_ok(data, c, n_ref)
    if f is None or f[0] > n - c - 4 or data[c + 36 + f[1] - 1] != 0:
        return False
    at = c + 4 + f[0]
    if n - at < 4:
        return True
    if not 32 <= struct.unpack_from("<i", data, at)[0] <= MAX_RECORD:
        return False
    return n - at < 36 or _fixed_ok(data, at, n_ref) is not None


def first_hits(data, first, n_ref, tile, n_tiles):
    """What each of the first n_tiles tiles is walked from: None before `first`, `first` in its own tile, else the lowest
    offset of the tile that passes the guess rule (None: no guess)."""
    n, out = len(data), []
    for t in range(n_tiles):
        base = t * tile
        if base + tile <= first:
            out.append(None)
        elif first >= base:
            out.append(first)
        else:
            out.append(next((c for c in range(base, base + tile) if guess_hit(data, n, c, n_ref)), None))
    return out


def chain_exit(data, entry, end):
    """The chain walked from `entry` to `end` as the tile walk does it -> (exit, records, stopped by the data)"""
    n, o, cnt = len(data), entry, 0
    while o < end:
        if n - o < 4:
            return o, cnt, True
        bs = struct.unpack_from("<i", data, o)[0]
        f = _fixed_ok(data, o, None) if 32 <= bs <= n - o - 4 else None
        if f is None or data[o + 36 + f[1] - 1] != 0:
            return o, cnt, True
        o += 4 + bs; cnt += 1
    return o, cnt, False


def dependent_decoys(tile, k, lead=3, tail=3, every=1, leak=False, pad=7, extra=()):
    """Misses of the index's guess that depend on each other -> (refs, data, first, record offsets, decoy tiles).

    One record of exactly `tile` bytes starts in every tile, 56 bytes before its end, so each tile's true entry is the exit
    of the tile before it and no tile holds a second start.  A record's Z payload lies wholly in the next tile, in front
    of that tile's record; in the k tiles lead, lead + every, ... it holds two consecutive well-formed fake records (as
    decoy_bam), so the lowest offset of the tile that passes the guess rule is the first fake.  What follows the second
    fake is filler: the walk from the guess stops there, short of the tile's true start, and nothing it leaves says where
    the next tile is entered.  With every == 1 the run can therefore be repaired only one tile per stitch pass; with
    every == 2 a tile that guesses right follows each miss and the misses are independent.
    leak: the second fake's block_size carries the wrong chain to a filler offset in the next tile instead, so that the
    stitch hands a WRONG entry to the tile after the next.
    The regular part ends with a 38-byte record inside the last tile (a last tile without a record start would itself be
    a miss and cost a round); `extra` record dicts follow it and are not part of the asserted layout.
    Asserted here, on the CPU, by the restated guess rule: in each decoy tile the first hit is the fake and the walk from
    it does not reach the true chain; in every other tile the first hit is the true start."""
    assert tile >= 256 and lead >= 1 and every >= 1
    refs = EDGE_REFS
    s = tile - 56
    head = encode_header("", refs)
    fakes = [bytearray(encode_record(rec(f"fake{i}", cigar=C("8M"), tid=i))) for i in range(2)]
    if leak:
        fakes[1][:4] = struct.pack("<i", tile + len(fakes[1]) + 12)
    fake = bytes(fakes[0] + fakes[1])
    decoys = [lead + every * i for i in range(k)]
    n_regular = (decoys[-1] if decoys else lead) + 1 + tail       # tiles with a full-size record
    recs, fake_at = [], {}
    r = rec("pad", cigar=C("10M"), aux=[("XP", "Z", b"")])
    r["aux"][0][2] = b"p" * (s - len(head) - len(encode_record(r)))
    recs.append(r)
    for j in range(n_regular):
        r = rec(f"r{j:05d}", cigar=C("10M"), pos=1000 + j, aux=[("XD", "Z", b"")])
        body = bytearray(b"p" * (tile - len(encode_record(r))))
        payload_at = j * tile + s + len(encode_record(r)) - 1
        assert payload_at > (j + 1) * tile and len(body) > pad + len(fake) + 40
        if j + 1 in decoys:                                      # this record's payload is the front of tile j + 1
            body[pad:pad + len(fake)] = fake
            fake_at[j + 1] = payload_at + pad
        r["aux"][0][2] = bytes(body)
        recs.append(r)
    recs.append(dict(qname="s", flag=0, tid=0, pos=7, mapq=0, cigar=[], mtid=-1, mpos=-1, tlen=0, seq="", qual=[], aux=[]))
    recs += list(extra)
    data, first, at = encode_bam("", refs, recs)
    assert first == len(head) and [int(a) % tile for a in at[1:n_regular + 2]] == [s] * (n_regular + 1)
    starts = {int(a) // tile: int(a) for a in at[1:n_regular + 2]}
    hits = first_hits(data, first, len(refs), tile, n_regular + 1)
    for t in range(1, n_regular + 1):
        if t in decoys:
            assert hits[t] == fake_at[t] < starts[t] and data[fake_at[t]:fake_at[t] + len(fake)] == fake, (t, hits[t], fake_at[t])
            ex, cnt, stopped = chain_exit(data, hits[t], (t + 1) * tile)
            assert cnt == 2 and ex != starts[t + 1] and stopped != leak, (t, ex, cnt, stopped)
            if leak:
                assert (t + 1) * tile < ex < starts[t + 1] and not guess_hit(data, len(data), ex, len(refs))
        else:
            assert hits[t] == starts[t], (t, hits[t], starts[t])
    assert hits[0] == first
    return refs, data, first, at, decoys


def mutate(rng, data, first):
    """one corrupted copy of BAM bytes: byte flips, a truncation, or a length field overwritten"""
    b = bytearray(data)
    kind = rng.randint(4)
    if kind == 0:
        for _ in range(int(rng.randint(1, 6))):
            b[int(rng.randint(len(b)))] ^= 1 << int(rng.randint(8))
    elif kind == 1:
        del b[int(rng.randint(len(b))):]
    elif kind == 2:
        p = int(rng.randint(first, len(b) - 4))
        b[p:p + 4] = struct.pack("<i", int(rng.choice([-1, 0, 31, 32, 33, 1 << 28, (1 << 28) + 1, 0x7fffffff, -0x80000000, int(rng.randint(0, 4000))])))
    else:
        p = int(rng.randint(0, max(1, min(len(b) - 4, first + 64))))
        b[p:p + 4] = struct.pack("<i", int(rng.choice([-1, 0, 1, 0x7fffffff, int(rng.randint(0, 100000))])))
    return bytes(b)
