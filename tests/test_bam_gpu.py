"""BAM input on the device (mgx_bam_scan: the tiled record index and the key kernel) against the host functions that define
it: record offsets, keys with their redo bits, `next`, error code and message are equal on ordinary data at several tile
sizes, at every cut of the input, across tile seams, with decoy records inside tag payloads (where the guesses are wrong
and the re-walk must repair them), and on corrupt chains."""
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
