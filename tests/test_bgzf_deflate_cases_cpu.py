"""The instruments and generators of the BGZF deflate seam tests (bgzf_deflate_cases.py), checked without a GPU: the token-level
inflater against zlib, package-merge against brute force, and every precondition the GPU tests build on."""
import itertools
import zlib

import numpy as np
import pytest

import bgzf_cases as bc
import bgzf_deflate_cases as dc


def test_inflate_tokens_agrees_with_zlib():
    """every block of the inflate suite's grid up to 5 000 bytes and of its 200 random ones, and four full-size blocks: the same
    bytes out and the same number of payload bytes consumed (three bytes of junk follow the payload)"""
    blocks = bc.zlib_blocks(np.random.RandomState(7), n_random=200)
    small = [(b, d) for b, d in blocks if len(d) <= 5000]
    full = [(b, d) for b, d in blocks if len(d) == dc.MAX_IN]
    picked = small + [full[k] for k in (201, 200, 3 * 25 + 6, 4 * 25 + 9)]      # 258-byte matches 32 768 and 1 back; sam and runs, level 6 and 9
    assert len(small) > 1000 and len(picked) == len(small) + 4
    btypes = set()
    for blk, want in picked:
        payload = blk[18:-8] + b"\xa5\x5a\xff"
        d = zlib.decompressobj(-15)
        assert d.decompress(payload) + d.flush() == want and d.eof
        got, info, used = dc.inflate_tokens(payload)
        assert got == want
        assert used == len(payload) - len(d.unused_data)
        btypes.update(b["btype"] for b in info)
        n_out = sum(t[0] if isinstance(t, tuple) else 1 for b in info for t in b["tokens"])
        assert n_out == len(want)
    assert btypes == {0, 1, 2}


def test_inflate_tokens_refuses_the_crafted_bad_blocks():
    for name, blk in bc.crafted_bad_blocks():
        with pytest.raises(dc.InflateError):
            dc.inflate_tokens(blk[18:-8])
            pytest.fail(name + " was accepted")


def test_inflate_tokens_refuses_overrun_and_bad_counts():
    cl = [4] * 16 + [0, 0, 0]
    overrun = bc.dynamic_header([3, 3, 3, 3, 3, 3, 3, 0] + [0] * 10 + [3], [1] * 6, 257, 1)       # symbols 0..6 and 18, 3 bits each
    codes = bc.canonical([3, 3, 3, 3, 3, 3, 3, 0] + [0] * 10 + [3])
    for _ in range(2):
        overrun.put_rev(*codes[18]).put(127, 7)                      # 6 + 138 + 138 lengths for HLIT + HDIST = 258
    with pytest.raises(dc.InflateError, match="overrun"):
        dc.inflate_tokens(overrun.bytes() + bytes(8))
    many = bc.Bits().put(1, 1).put(2, 2).put(30, 5).put(0, 5).put(15, 4)                          # HLIT = 287
    with pytest.raises(dc.InflateError, match="too many"):
        dc.inflate_tokens(many.bytes() + bytes(40))
    # a complete header whose only literal/length code is end-of-block in one bit: accepted, as zlib accepts it
    one = bc.dynamic_header(cl, [0] * 256 + [1] + [0], 257, 1).put_rev(0, 1)
    assert zlib.decompressobj(-15).decompress(one.bytes()) == b""
    assert dc.inflate_tokens(one.bytes())[0] == b""


def brute_force_cost(freqs, limit):
    best = None
    for lens in itertools.product(range(1, limit + 1), repeat=len(freqs)):
        if sum(1 << (limit - l) for l in lens) <= 1 << limit:
            c = sum(f * l for f, l in zip(freqs, lens))
            best = c if best is None or c < best else best
    return best


def test_limited_cost_against_brute_force():
    rng = np.random.RandomState(5)
    cases = [[1, 1], [1, 1, 2, 3, 5, 8], [1, 2, 4, 8, 16, 32], [7, 7, 7, 7, 7], [1, 1, 1, 1, 1, 1], [1, 100, 100, 100]]
    cases += [[int(x) for x in rng.randint(1, 60, n)] for n in (2, 3, 4, 5, 6, 6, 6) for _ in range(3)]
    for f in cases:
        for limit in range(3 if len(f) > 4 else 2 if len(f) > 2 else 1, 6):
            assert dc.limited_cost(f, limit) == brute_force_cost(f, limit), (f, limit)
        assert dc.limited_cost(f, 40) == dc.limited_cost(f, 5) == dc.limited_cost(f + [0, 0], 5)        # 6 symbols never need more than 5 bits
    assert dc.limited_cost([], 15) == 0 and dc.limited_cost([9], 15) == 9


def test_literal_only_check():
    rng = np.random.RandomState(1)
    base = rng.randint(0, 256, 4000, dtype=np.uint8)
    assert dc.literal_only_ok(base.tobytes())
    a = base.copy(); a[3000:3017] = a[100:117]                       # a 17-byte substring twice
    assert not dc.literal_only_ok(a.tobytes())
    a = base.copy(); a[3000:3016] = a[100:116]; a[3016] = a[116] ^ 1      # 16 bytes twice: still literal-only
    assert dc.literal_only_ok(a.tobytes())
    a = base.copy(); a[500:517] = 9; a[499] = 8; a[517] = 8           # a run of exactly 17: no 17-byte substring twice, refused all the same
    assert not dc.literal_only_ok(a.tobytes())
    a = base.copy(); a[500:516] = 9; a[499] = 8; a[516] = 8
    assert dc.literal_only_ok(a.tobytes())
    assert dc.literal_only_ok(b"") and dc.literal_only_ok(bytes(16)) and not dc.literal_only_ok(bytes(17))


def byte_histogram(data):
    return [int(x) for x in np.bincount(np.frombuffer(data, dtype=np.uint8), minlength=256)] + [1]


def test_case_a_forces_the_15_bit_limit():
    data = dc.case_a()
    h = byte_histogram(data)
    assert len(data) == 46366 and sorted(x for x in h if x) == sorted(dc.FIB[:22])
    assert dc.literal_only_ok(data)
    assert dc.limited_cost(h, 40) == 121367 and dc.limited_cost(h, 15) == 121373
    assert dc.limited_cost(h, 21) == dc.limited_cost(h, 40) < dc.limited_cost(h, 20)          # the unlimited depth is 21


def test_case_b_forces_the_7_bit_limit():
    data, lens = dc.case_b()
    h = byte_histogram(data)
    assert len(data) == 1023 and sum(1 for x in h[:256] if x) == 82 and sum(h) == 1024
    assert all(c == (1 << (10 - lens[v]) if lens[v] else 0) for v, c in enumerate(h))       # dyadic: the Huffman lengths are the planned ones
    assert dc.kraft(lens) == 1 << 15 and lens[256] == 10
    assert dc.literal_only_ok(data)
    zeros = [(v, r) for v, r in dc.runs(lens) if v == 0]
    assert zeros == [(0, 58)] * 3 and all(r < 4 for v, r in dc.runs(lens) if v)
    cl = dc.header_histogram(lens)
    assert cl == dc.CASE_B_CL_HISTOGRAM
    assert dc.limited_cost(cl.values(), 40) == 220 and dc.limited_cost(cl.values(), 7) == 221


def test_header_plans_contain_the_runs_the_coverage_asks_for():
    cases = dc.header_cases()
    zero_runs, other_runs = set(), set()
    for name, data, lens in cases:
        assert len(data) <= 4096 or name == "far"
        if lens is None:
            continue
        h = byte_histogram(data)
        k = max(lens)
        assert dc.literal_only_ok(data), name
        if name == "fib15":
            assert sorted(x for x in h if x) == sorted(dc.FIB[:16])
            assert dc.limited_cost(h, 15) == dc.limited_cost(h, 40) < dc.limited_cost(h, 14)     # 15 bits deep with no limit applied
            assert dc.limited_cost(h, 40) == sum(c * l for c, l in zip(h, lens))
        else:
            assert all(c == (1 << (k - lens[v]) if lens[v] else 0) for v, c in enumerate(h)), name
        for v, r in dc.planned_header(lens):
            (zero_runs if v == 0 else other_runs).add(r)
    assert zero_runs >= {1, 2, 3, 10, 11, 138, 139, 140, 141}
    assert other_runs >= {2, 3, 4, 7, 8, 10}
    far = dict((n, d) for n, d, _ in cases)["far"]
    assert far[dc.FAR_PERIOD:] == far[:len(far) - dc.FAR_PERIOD] and dc.dist_symbol(dc.FAR_PERIOD) == 29
    assert dc.literal_only_ok(far[:dc.FAR_PERIOD + 16])             # nothing but the period to match


def test_header_coverage_reads_a_header():
    """the coverage table on a header made by hand: runs cut at the right places, the crossing run seen"""
    lens = [3] * 4 + [0] * 141 + [3] * 4 + [0] * 107 + [2]          # 257 lengths
    cl_syms = [(3, 0), (16, 0), (18, 127), (17, 0), (3, 0), (3, 0), (3, 0), (3, 0), (18, 96), (2, 0), (2, 0), (2, 0)]
    h = dict(hlit=257, hdist=2, hclen=18, ll_lens=lens, d_lens=[2, 2], cl_syms=cl_syms)
    seen = dc.header_coverage([h])
    assert {("zero run", 141, ((18, 127), (17, 0))), ("non-zero run", 4), ("non-zero run", 3), ("run crosses into the distance lengths",),
            ("symbol", 16, 0), ("hlit", 257), ("hdist", 2)} <= seen
    assert ("two hclen values",) not in seen and ("non-zero run", 2) not in seen


def test_distance_and_length_pieces():
    per = dc.periodic_pieces()
    assert [p for p, _ in per] == dc.PERIODS
    for p, d in per:
        assert len(d) == (dc.MAX_IN if p >= 895 else 9000) and d[p:] == d[:len(d) - p]
    assert {1, dc.K_CHUNK, dc.K_MAX_MATCH, dc.K_WIN, dc.K_GRP_POS, dc.K_MAX_DIST, dc.K_MAX_DIST + 1} <= set(dc.PERIODS)
    zr = dc.zero_run_pieces()
    assert len(zr) == 4 * 13
    for (k, r), d in zr:
        a = np.frombuffer(d, dtype=np.uint8)
        assert len(d) == k + r + 40 and not a[k:k + r].any() and a[:k].all() and a[k + r:].all()


def test_geometry_grid_reaches_every_alignment():
    total = 0
    for kinds in (dc.GRID_KINDS[:3], dc.GRID_KINDS[3:]):
        pieces, tags = dc.geometry_grid(kinds)
        assert len(pieces) <= 1024                                       # one internal batch: offsets are taken from the call's first byte
        assert all(len(p) <= dc.MAX_IN for p in pieces)
        seen = dc.alignments_seen(pieces, tags)
        assert sorted(seen) == sorted(dc.GRID_LENGTHS) and all(s == {0, 1, 2, 3} for s in seen.values())
        assert {k for t in tags if t for k in [t[1]]} == set(kinds)
        for p, t in zip(pieces, tags):
            if t and t[1].startswith("zeros") and t[0]:
                z = min(t[0], int(t[1][5:]))
                assert p[-z:] == bytes(z) and (len(p) == z or p[-z - 1] != 0)
        total += sum(len(p) for p in pieces)
    assert total < 8 << 20
    for n in (0, dc.K_CHUNK, 2 * dc.K_CHUNK, dc.K_MAX_MATCH, dc.K_WIN, dc.K_GRP_POS, dc.K_GRP_POS + dc.K_MAX_MATCH, 2 * dc.K_GRP_POS, dc.MAX_IN):
        assert {n - 1, n, n + 1} <= set(dc.GRID_LENGTHS) or n in (0, dc.K_GRP_POS + dc.K_MAX_MATCH, dc.MAX_IN)
    assert {3841, 3842, 3843, 65279, 65280} <= set(dc.GRID_LENGTHS)


def test_sweeps_and_content_only_pieces():
    sw = dc.stored_sweep()
    assert [len(p) for p in sw] == [2000 + t for t in range(81)] and all(p[:2000] == sw[0] and not any(p[2000:]) for p in sw)
    assert [len(p) for p in dc.repeated_byte_sweep()] == list(range(1, 41))
    pieces = dc.content_only_pieces()
    assert 50 <= len(pieces) <= 70 and all(len(p) <= dc.MAX_IN for p in pieces)
    assert len(set(pieces)) <= len(pieces) - 6                        # equal contents repeated
    sizes = [len(p) for p in pieces]
    assert sum(1 for a, b in zip(sizes, sizes[1:]) if (a > 8000) != (b > 8000)) >= 20       # large and tiny interleaved
