"""BAM input on the device (mgx_bam_scan: the tiled record index and the key kernel) against the host functions that define
it: record offsets, keys with their redo bits, `next`, error code and message are equal on ordinary data at several tile
sizes, at every cut of the input, across tile seams, with decoy records inside tag payloads (where the guesses are wrong
and the re-walk must repair them), with misses that depend on each other (the later repair rounds, the serial finish and
the stitch's step boundary, each with the number of rounds the schedule must take), and on corrupt chains."""
import ctypes
import errno
import os
import struct

import numpy as np
import pytest

import bam_cases as bm

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def scanner(pkg):
    sc = pkg.BamScanner(0)
    yield sc
    sc.close()


@pytest.fixture(scope="module")
def synthetic(synth, tmp_path_factory):
    return bm.synthetic(synth, tmp_path_factory.mktemp("bamgpu"))


@pytest.fixture
def tile():
    def set_tile(v):
        if v is None:
            os.environ.pop("MGX_BAM_TILE", None)
        else:
            os.environ["MGX_BAM_TILE"] = str(v)
    yield set_tile
    os.environ.pop("MGX_BAM_TILE", None)


def compare(pkg, sc, data, first, n_ref, n=None):
    """device == host for data[:n] from `first`; returns the device statistics"""
    try:
        want = pkg.bam.walk_host(data, first, n)
    except pkg.bam.BamDataError as e:
        with pytest.raises(pkg.bam.BamDataError) as g:
            sc.scan(data, first, n_ref, n)
        assert (str(g.value), g.value.n_records, g.value.next) == (str(e), e.n_records, e.next)
        return sc.stats()
    off, keys, nxt = sc.scan(data, first, n_ref, n)
    assert nxt == want[1] and np.array_equal(off, want[0]), (first, n)
    assert keys.tobytes() == pkg.bam.keys_host(data, off, rules_only=True).tobytes(), (first, n)
    st = sc.stats()
    assert st["n_redo"] == int((keys["redo"] != 0).sum())
    return st


@pytest.mark.parametrize("size", [256, 1024, 4096, 16384, None])
def test_synthetic_set_at_every_tile_size(pkg, scanner, synthetic, tile, size):
    _, _, refs, recs, data, first, at = synthetic
    tile(size)
    st = compare(pkg, scanner, data, first, len(refs))
    assert st["n_tiles"] == -(-len(data) // (size or 16384))
    print(f"tile {size}: {st}")
    assert st["n_tiles_rewalked"] * 100 <= st["n_tiles"], st       # the re-walk is not what makes ordinary data pass
    for f in (int(at[7]), int(at[-1]), len(data), len(data) + 1, len(data) + 5000):
        compare(pkg, scanner, data, f, len(refs))
    # every cut of the input in a window that holds two record ends: block_size cut after 1, 2 and 3 bytes, the fixed
    # part cut, the name cut, the exact end
    k = 100
    assert at[k + 2] - at[k] < 600
    for n in range(int(at[k]) - 20, int(at[k]) + 580):
        compare(pkg, scanner, data, first, len(refs), n)
    compare(pkg, scanner, data, int(at[k - 3]), len(refs), int(at[k]) + 2)
    compare(pkg, scanner, b"", 0, len(refs))


def test_seams_at_tile_256(pkg, scanner, tile):
    refs, recs, first = bm.seam_records(256)
    data, f2, at = bm.encode_bam("", refs, recs)
    assert f2 == first
    by = {r["qname"]: int(a) for r, a in zip(recs, at)}
    assert [by[f"seam{s}"] % 256 for s in (0, 1, 2, 3)] == [0, 255, 254, 253]
    assert at[recs.index(next(r for r in recs if r["qname"] == "long")) + 1] - by["long"] > 19 * 256
    tile(256)
    st = compare(pkg, scanner, data, first, len(refs))
    for n in (by["seam1"] + 1, by["seam2"] + 2, by["seam3"] + 3, by["seam3"] + 4, by["long"] + 2000, len(data) - 1):
        compare(pkg, scanner, data, first, len(refs), n)
    for f in (by["seam0"], by["seam3"], by["long"], by["last"]):
        compare(pkg, scanner, data, f, len(refs))


@pytest.mark.parametrize("in_b_tag", [False, True])
def test_decoys_inside_tag_payloads(pkg, scanner, tile, in_b_tag):
    tile(256)
    rewalked = 0
    for pad in range(256):
        refs, recs = bm.decoy_bam(pad, in_b_tag)
        data, first, _ = bm.encode_bam("", refs, recs)
        st = compare(pkg, scanner, data, first, len(refs))
        rewalked += st["n_tiles_rewalked"]
    assert rewalked > 0


# ---- repair rounds ---------------------------------------------------------------------------------------------------
# bam_cases.dependent_decoys lays down misses that depend on each other.  What the schedule of mgx_bam.hip does with a
# dependent run of k tiles, read from k_bam_stitch:
#   * a pass marks the first tile whose guess disagrees with the verified chain and gives it its true entry; behind it the
#     pass is optimistic and takes the NEXT tile's guess (a fake) for true.  The walk from a fake stops at the filler
#     behind the second fake with a status, which ends the pass (S.done): nothing further is marked.  So each pass
#     repairs exactly one tile of the run, and n_rounds counts the passes that marked something.
#   * k <= 3: passes 1..k mark, pass k + 1 (at the latest the fourth) marks nothing and accepts: n_rounds == k, and
#     n_tiles_rewalked == k.
#   * k >= 4: all four passes mark, the fourth leaves the frontier at the run's fourth tile, and k_bam_finish walks from
#     there and counts as one more round: n_rounds == 5.  A pass that marks is always followed by another pass or by the
#     finish, so 4 cannot occur.
N_REF = len(bm.EDGE_REFS)


def rounds_of_a_run(k):
    return k if k <= 3 else 5


@pytest.mark.parametrize("k", [0, 1, 2, 3, 4, 5, 12])
def test_dependent_run_is_repaired_one_tile_per_round(pkg, scanner, tile, k):
    _, data, first, at, decoys = bm.dependent_decoys(256, k)
    assert len(decoys) == k
    tile(256)
    st = compare(pkg, scanner, data, first, N_REF)
    print(f"k {k}: {st}")
    assert st["n_rounds"] == rounds_of_a_run(k), st
    if k <= 3:
        assert st["n_tiles_rewalked"] == k, st
    else:                                                        # four marked tiles, then the finish from the fourth to the end
        assert st["n_tiles_rewalked"] == 4 + (st["n_tiles"] - decoys[3]), st


def test_twelve_independent_misses_take_one_round(pkg, scanner, tile):
    _, data, first, at, decoys = bm.dependent_decoys(256, 12, every=2)
    tile(256)
    st = compare(pkg, scanner, data, first, N_REF)
    assert st["n_rounds"] == 1 and st["n_tiles_rewalked"] >= 12, st


@pytest.mark.parametrize("k,rounds", [(2, 3), (3, 3), (12, 5)])
def test_wrong_chain_that_leaks_into_the_next_tile(pkg, scanner, tile, k, rounds):
    """leak=True: the walk from a fake does not stop but leaves its tile at a filler offset x of the next one.  Pass 1
    marks the run's first tile, takes the second's fake for true and hands its exit x to the third tile as an entry: that
    tile is re-walked from a WRONG entry (the walk from x stops at once), and again from the true one when the frontier
    reaches it.  With k == 2 the third tile is the first that guessed right: the wrong entry spoils it, so it costs a
    round of its own (3 rounds); with k == 3 it is the run's last tile and the count stays 3."""
    _, data, first, at, decoys = bm.dependent_decoys(256, k, leak=True)
    tile(256)
    st = compare(pkg, scanner, data, first, N_REF)
    assert st["n_rounds"] == rounds and st["n_tiles_rewalked"] > k, st


def finish_tail():
    """what follows a run of 12 in the finish tests: a long record over 19 tiles, hosts of further decoys, 60 records of 38
    bytes back to back, plain records"""
    tail = [bm.rec("long", cigar=bm.C("15M"), aux=[("XL", "Z", "L" * 5000)])]
    tail += bm.decoy_bam(11)[1][:3] + bm.decoy_bam(200, in_b_tag=True)[1][:3]
    tail += [dict(qname="s", flag=0, tid=0, pos=i, mapq=0, cigar=[], mtid=-1, mpos=-1, tlen=0, seq="", qual=[], aux=[]) for i in range(60)]
    tail += [bm.rec(f"plain{i}:1:fc:2:1101:{i}:77", cigar=bm.C("30M")) for i in range(8)]
    return tail


def test_the_serial_finish_behind_a_run_of_twelve(pkg, scanner, tile):
    """Everything here lies behind the frontier that the fourth pass leaves, so k_bam_finish finds it: its slot writes (60
    starts in a tile and a half), the tiles a long record spans, decoys it must not look at, the end of the data, cut
    records, invalid records, and a record array that is one too short."""
    refs, data, first, at, decoys = bm.dependent_decoys(256, 12, extra=finish_tail())
    tile(256)
    n_rec = len(at)
    st = compare(pkg, scanner, data, first, N_REF)                     # a clean end at n
    assert st["n_rounds"] == 5 and st["n_tiles_rewalked"] > 12, st
    long_at = int(at[-(60 + 8 + 6 + 1)])
    assert long_at > (decoys[-1] + 1) * 256 and int(at[-(60 + 8 + 6)]) - long_at > 19 * 256
    for j in (-3, -30, -(60 + 8 + 6 + 1)):                             # a plain record, one of the 38-byte ones, the long one
        o = int(at[j])
        for n in (o + 2, o + 20, o + 37):                            # cut inside block_size, the fixed part, the name
            st = compare(pkg, scanner, data, first, N_REF, n)
            assert st["n_rounds"] == 5, (j, n, st)
    o = int(at[-4])
    assert data[o + 12] > 2 and data[o + 36 + data[o + 12] - 1] == 0
    for name, (p, b) in {"bs31": (o, struct.pack("<i", 31)), "name0": (o + 12, b"\0"), "no_nul": (o + 36 + data[o + 12] - 1, b"x")}.items():
        bad = bytearray(data)
        bad[p:p + len(b)] = b
        with pytest.raises(pkg.bam.BamDataError) as e:
            scanner.scan(bytes(bad), first, N_REF)
        assert f"offset {o}:" in str(e.value) and e.value.n_records == n_rec - 4 and e.value.next == o, (name, str(e.value))
        st = compare(pkg, scanner, bytes(bad), first, N_REF)          # text, n_records and next equal the host's
        assert st["n_rounds"] == 5, (name, st)
        compare(pkg, scanner, data, first, N_REF)                      # the context is usable afterwards
    for t in (decoys[1], decoys[5], decoys[-1]):                 # `first` = the record that starts inside tile t of the run
        assert int(at[t + 1]) // 256 == t
        st = compare(pkg, scanner, data, int(at[t + 1]), N_REF)
        assert t == decoys[-1] or st["n_rounds"] == 5, (t, st)      # at least six tiles of the run are left behind `first`
    # a record array one too short: -E2BIG, and nothing is written to the caller's arrays
    d = np.frombuffer(data, dtype=np.uint8)
    cap = n_rec - 1
    off = np.full(cap + 64, 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
    keys = np.full((cap + 64) * 32, 0xA5, dtype=np.uint8)
    cnt, nxt = ctypes.c_uint64(), ctypes.c_uint64()
    rc = scanner.lib.mgx_bam_scan(scanner.h, d.ctypes.data_as(ctypes.c_void_p), len(d), first, N_REF, cap, off.ctypes.data_as(ctypes.c_void_p),
                                  keys.ctypes.data_as(ctypes.c_void_p), ctypes.byref(cnt), ctypes.byref(nxt))
    assert rc == -errno.E2BIG and f"{n_rec} records" in scanner.lib.mgx_last_error().decode()
    assert (off[cap:] == 0xA5A5A5A5A5A5A5A5).all() and (keys[cap * 32:] == 0xA5).all()
    assert scanner.stats()["n_rounds"] == 5
    off2, keys2, _ = scanner.scan(data, first, N_REF, max_records=n_rec)     # exactly enough
    assert np.array_equal(off2, at)
    compare(pkg, scanner, data, first, N_REF)


@pytest.mark.parametrize("leak", [False, True])
@pytest.mark.parametrize("start", [254, 255, 256])
def test_run_of_three_across_the_stitch_step(pkg, scanner, tile, start, leak):
    """The stitch takes 256 tiles per step.  A run that starts at tile 254, 255 or 256 puts its marked tile, the optimistic
    tile behind it and the tile behind that on either side of the step: S.cur is carried over as the pass's end (start
    254, the status of the fake walk in tile 255), as `none` (start 255: tile 255 marked, the next guess taken at the
    top of the step) or, with leak, as the optimistic exit of tile 255 that tile 256 is then marked against."""
    _, data, first, at, decoys = bm.dependent_decoys(256, 3, lead=start, leak=leak)
    assert decoys == [start, start + 1, start + 2]
    tile(256)
    st = compare(pkg, scanner, data, first, N_REF)
    assert st["n_rounds"] == 3 and st["n_tiles"] > 258, st
    assert st["n_tiles_rewalked"] == (4 if leak else 3), st


@pytest.mark.parametrize("leak", [False, True])
def test_run_of_twelve_across_the_stitch_step(pkg, scanner, tile, leak):
    """the frontier (tile 254) and the start of the finish lie in the stitch's first step, the run's end in the second"""
    _, data, first, at, decoys = bm.dependent_decoys(256, 12, lead=251, leak=leak)
    tile(256)
    st = compare(pkg, scanner, data, first, N_REF)
    assert st["n_rounds"] == 5 and decoys[3] == 254 and decoys[-1] == 262, st
    compare(pkg, scanner, data, first, N_REF, int(at[259]) + 20)       # the finish ends inside the run, in the second step


def test_dependent_run_at_the_default_tile(pkg, scanner, tile):
    _, data, first, at, decoys = bm.dependent_decoys(16384, 5)
    tile(None)
    st = compare(pkg, scanner, data, first, N_REF)
    assert st["n_rounds"] == 5 and st["n_tiles"] == -(-len(data) // 16384), st
    _, data, first, at, decoys = bm.dependent_decoys(16384, 3, leak=True)
    st = compare(pkg, scanner, data, first, N_REF)
    assert st["n_rounds"] == 3, st


def test_edge_list(pkg, scanner, tile):
    recs = bm.edge_records()
    data, first, _ = bm.encode_bam("@HD\tVN:1.6\n", bm.EDGE_REFS, recs)
    for size in (256, None):
        tile(size)
        st = compare(pkg, scanner, data, first, len(bm.EDGE_REFS))
        assert st["n_redo"] >= 10
    off, keys, _ = scanner.scan(data, first, len(bm.EDGE_REFS))
    assert pkg.bam.keys_redo(data, off, keys).tobytes() == pkg.bam.keys_host(data, off).tobytes()


def test_fifty_megabytes_at_the_default_tile(pkg, scanner, synthetic):
    _, _, refs, recs, data, first, at = synthetic
    big = data + data[first:] * 15
    st = compare(pkg, scanner, big, first, len(refs))
    assert st["n_tiles"] > 3000 and st["n_tiles_rewalked"] * 100 <= st["n_tiles"], st
    print(f"{len(big)} bytes, {16 * len(recs)} records: {st}")


def test_corrupt_records_in_mid_chain(pkg, scanner, synthetic, tile):
    _, _, refs, recs, data, first, at = synthetic
    o = int(at[len(at) // 2])
    edits = {"bs31": (o, struct.pack("<i", 31)), "negative": (o, struct.pack("<i", -7)), "parts": (o, struct.pack("<i", 40)), "name0": (o + 12, b"\0")}
    for size in (256, None):
        tile(size)
        for name, (p, b) in edits.items():
            bad = bytearray(data)
            bad[p:p + len(b)] = b
            with pytest.raises(pkg.bam.BamDataError) as e:
                scanner.scan(bytes(bad), first, len(refs))
            assert f"offset {o}:" in str(e.value) and e.value.n_records == len(at) // 2 and e.value.next == o, (name, str(e.value))
            compare(pkg, scanner, bytes(bad), first, len(refs))
        compare(pkg, scanner, data, first, len(refs))               # the context is usable afterwards
