"""k_bgzf_deflate at the seams of its own constants (inputs and instruments: bgzf_deflate_cases.py): the 15- and 7-bit code
length limits, the run-length coded header, the distance cap and the 258-byte match, the pipeline's chunk / window / group
boundaries at every source alignment, LDS reuse from block to block, the stored / dynamic decision and the CRC combination.
Every block must be a valid BGZF member that inflates to its input; what a case claims to have reached -- a limited code, a
header symbol, a distance -- is read from the emitted bytes with a strict token-level inflater."""
import pytest

import bgzf_deflate_cases as dc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def comp(pkg):
    c = pkg.BgzfCompressor(0)
    yield c
    c.close()


def compressor_under(pkg, env):
    """A compressor created under knob values (they are read when it is created)."""
    with pytest.MonkeyPatch.context() as mp:
        for k, v in env.items():
            mp.setenv(k, v)
        return pkg.BgzfCompressor(0)


@pytest.fixture(scope="module")
def lit_comp(pkg):
    """every match of at most 16 bytes dropped: data without a repeated 17-byte substring becomes literals only"""
    c = compressor_under(pkg, dc.LITERAL_ONLY_ENV)
    yield c
    c.close()


def compress(c, pieces):
    out, out_off = c.compress(b"".join(pieces) or b"\0", dc.offsets_of(pieces))
    blocks = dc.split_blocks(out, out_off)
    assert len(blocks) == len(pieces) and int(out_off[-1]) == len(out)
    return blocks


def decode(block, want):
    """check_member, then the one DEFLATE block of the member as the token-level inflater sees it"""
    dc.check_member(block, want)
    got, info, used = dc.inflate_tokens(block[18:-8])
    assert got == bytes(want) and used == len(block) - 26 and len(info) == 1
    return info[0]


def matches(tokens):
    return [t for t in tokens if isinstance(t, tuple)]


@pytest.fixture(scope="module")
def block_a(lit_comp):
    """case A: byte counts F2..F22; with end-of-block the histogram is F1..F22 and every optimal code is 21 bits deep"""
    data = dc.case_a()
    assert dc.literal_only_ok(data) and len(data) == 46366
    return decode(compress(lit_comp, [data])[0], data)


@pytest.fixture(scope="module")
def block_b(lit_comp):
    """case B: a header whose symbol counts are Fibonacci numbers: the unlimited code-length code is 8 bits deep"""
    data, lens = dc.case_b()
    assert dc.literal_only_ok(data) and dc.header_histogram(lens) == dc.CASE_B_CL_HISTOGRAM
    return decode(compress(lit_comp, [data])[0], data), lens


def test_literal_length_code_is_limited_to_15_bits(block_a):
    """the block is literals only, its observed histogram forces the limit, and the emitted code is complete and within it:
    huff_build repaired the counts per length"""
    b = block_a
    assert b["btype"] == 2 and not matches(b["tokens"])
    ll, _ = dc.token_histograms(b["tokens"])
    assert sorted(x for x in ll if x) == sorted(dc.FIB[:22])
    best15, best = dc.limited_cost(ll, 15), dc.limited_cost(ll, 40)
    bits = sum(c * l for c, l in zip(ll, b["ll_lens"]))
    print(f"case A: longest code {max(b['ll_lens'])} bits; token bits {bits}, package-merge optimum at 15 bits {best15}: "
          f"ratio {bits / best15:.5f} (unlimited optimum {best})")
    assert best15 > best                                             # the limit was binding: every unlimited optimum is too deep
    assert max(b["ll_lens"]) <= 15
    assert dc.kraft(b["ll_lens"]) == 1 << 15
    assert bits >= best15


def test_limited_literal_length_code_is_15_bits_deep(block_a):
    """a code that the limit binds is as deep as the limit allows (the first limiter halved all counts until the rebuilt code fitted,
    which left this one 11 bits deep; the repair of the counts per length keeps it at 15: 121 433 token bits against the 121 373
    of the best 15-bit code)"""
    assert max(block_a["ll_lens"]) == 15


def test_code_length_code_is_limited_to_7_bits(block_b):
    """literals only, the planned lengths, the planned header symbols -- whose histogram forces the limit -- and a complete
    code-length code within it"""
    b, lens = block_b
    assert b["btype"] == 2 and not matches(b["tokens"])
    assert b["ll_lens"] == lens and b["d_lens"] == [1, 1]
    hist = {}
    for s, _ in b["cl_syms"]:
        hist[s] = hist.get(s, 0) + 1
    assert hist == dc.CASE_B_CL_HISTOGRAM
    bits = sum(c * b["cl_lens"][s] for s, c in hist.items())
    print(f"case B: longest code-length code {max(b['cl_lens'])} bits; header symbol bits {bits}, optimum at 7 bits "
          f"{dc.limited_cost(hist.values(), 7)}, unlimited {dc.limited_cost(hist.values(), 40)}")
    assert dc.limited_cost(hist.values(), 7) > dc.limited_cost(hist.values(), 40)      # the limit was binding
    assert max(b["cl_lens"]) <= 7
    assert dc.kraft(b["cl_lens"]) == 1 << 15
    assert all((b["cl_lens"][s] != 0) == (s in hist) for s in range(19))


def test_limited_code_length_code_is_7_bits_deep(block_b):
    """the same for the code-length code (5 bits deep under the first limiter; now 7, at the optimal 221 header symbol bits)"""
    assert max(block_b[0]["cl_lens"]) == 7


def test_header_runs(lit_comp):
    """the seams of the run arithmetic (symbols 16, 17, 18), a run that continues into the distance lengths, and the trimming
    of HLIT, HDIST and HCLEN, collected from the decoded headers of one batch"""
    cases = dc.header_cases()
    blocks = compress(lit_comp, [d for _, d, _ in cases])
    headers = []
    for (name, data, lens), blk in zip(cases, blocks):
        b = decode(blk, data)
        assert b["btype"] == 2, name
        headers.append(b)
        if lens is not None:
            assert dc.literal_only_ok(data), name
            assert not matches(b["tokens"]) and b["ll_lens"] == lens and b["d_lens"] == [1, 1], name
        assert dc.kraft(b["ll_lens"]) == 1 << 15 and dc.kraft(b["cl_lens"]) == 1 << 15, name
    seen = dc.header_coverage(headers)
    missing = [e for e in dc.HEADER_COVERAGE if e not in seen]
    assert not missing, missing


def expected_run_matches(r):
    """a zero run of r after a non-zero byte: its first zero is a literal, the other r - 1 are distance-1 matches of up to 258;
    what is left below 3 bytes is literals (the runs of the sweep leave 0, 1, 2 or more than 16)"""
    rest, out = r - 1, []
    while rest >= 3:
        out.append((min(rest, 258), 1))
        rest -= out[-1][0]
    return out


def test_distance_and_length_edges(comp):
    """periods around every constant up to the distance cap, and zero runs around the wavefront's 64 positions"""
    per, zr = dc.periodic_pieces(), dc.zero_run_pieces()
    pieces = [d for _, d in per] + [d for _, d in zr]
    blocks = compress(comp, pieces)
    decoded = [decode(blk, d) for blk, d in zip(blocks, pieces)]
    distances, lengths, only_symbol = set(), set(), set()
    for b in decoded:
        m = matches(b["tokens"])
        distances.update(d for _, d in m)
        lengths.update(l for l, _ in m)
        syms = {dc.dist_symbol(d) for _, d in m}
        if len(syms) == 1:
            only_symbol.add(min(next(iter(syms)), 1))                        # 0: symbol 0 alone; 1: another symbol alone
            assert sum(1 for l in b["d_lens"] if l) == 2                      # huff_build gave the lone symbol a partner
    assert max(distances) <= dc.K_MAX_DIST
    missing = [name for name, ok in [("distance 32768", 32768 in distances), ("length 257", 257 in lengths), ("length 258", 258 in lengths),
                                     ("a block whose only distance symbol is 0", 0 in only_symbol),
                                     ("a block whose only distance symbol is not 0", 1 in only_symbol)] if not ok]
    assert not missing, missing
    for (p, _), b in zip(per, decoded):
        if p > dc.K_MAX_DIST:
            assert b["btype"] == 0 or not matches(b["tokens"]), p
        elif p >= 895:
            far = {d for _, d in matches(b["tokens"])}
            assert far <= {p} and (far or p > 3585), p                       # random bytes: nothing to match but the period
    for ((k, r), data), b in zip(zr, decoded[len(per):]):
        if r >= 63:                                                           # shorter runs are the cost rule's to take or leave
            assert matches(b["tokens"]) == expected_run_matches(r), (k, r)
            assert b["tokens"][:k + 1] == list(data[:k + 1]), (k, r)


def test_geometry_grid_at_every_alignment(comp):
    """piece lengths on the chunk, match, window, group and block boundaries x seven kinds of content x the four source
    alignments; n = 0 and n % 64 == 0 check the CRC combination through CRC-32 and ISIZE"""
    for kinds in (dc.GRID_KINDS[:3], dc.GRID_KINDS[3:]):
        pieces, tags = dc.geometry_grid(kinds)
        assert len(pieces) <= 1024
        seen = dc.alignments_seen(pieces, tags)
        assert sorted(seen) == sorted(dc.GRID_LENGTHS) and all(s == {0, 1, 2, 3} for s in seen.values()), seen
        for i, (blk, p) in enumerate(zip(compress(comp, pieces), pieces)):
            try:
                dc.check_member(blk, p)
            except AssertionError as e:
                raise AssertionError(f"piece {i}: {tags[i]}, {len(p)} bytes") from e


@pytest.mark.parametrize("backwards", [False, True])
def test_a_block_depends_on_its_content_only(comp, pkg, backwards):
    """each piece alone at offset 0 against the same piece inside a batch that ONE workgroup walks (MGX_BGZF_GRID=1: every block
    inherits the LDS of the one before -- hash heads, match tables, masks, header words, counts, the parse carry)"""
    pieces = dc.content_only_pieces()
    if backwards:
        pieces = pieces[::-1]
    alone = {}
    for p in pieces:
        if p not in alone:
            alone[p] = compress(comp, [p])[0]
            dc.check_member(alone[p], p)
    one = compressor_under(pkg, {"MGX_BGZF_GRID": "1"})
    try:
        batch = compress(one, pieces)
    finally:
        one.close()
    differ = [(i, len(p)) for i, (blk, p) in enumerate(zip(batch, pieces)) if blk != alone[p]]
    assert not differ, differ


def test_stored_or_dynamic(comp):
    """the decision payload >= n + 5 at its boundary, read from BTYPE"""
    pieces = dc.stored_sweep() + dc.repeated_byte_sweep()
    before = comp.stats()["n_stored"]
    blocks = compress(comp, pieces)
    kinds = []
    for blk, p in zip(blocks, pieces):
        dc.check_member(blk, p)
        kinds.append(dc.btype(blk))
        assert kinds[-1] in (0, 2)
        if kinds[-1] == 2:
            assert len(blk) - 26 < len(p) + 5
        else:
            assert len(blk) == len(p) + 5 + 26
    assert {0, 2} == set(kinds[:81]), "both outcomes in the sweep of zero tails"
    print("stored (0) / dynamic (2) over t = 0..80:", "".join(map(str, kinds[:81])), " over n = 1..40:", "".join(map(str, kinds[81:])))
    assert comp.stats()["n_stored"] - before == kinds.count(0)
