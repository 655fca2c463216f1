"""SAM text input on the device (include/mgx_sam.h: mgx_sam_batch_*, mgx_sam_encode) against the same rule set on the host
(mgx_sam_encode_rules, which tests/test_sam_encode_host.py holds to the command-line tool's parser): line offsets and
lengths, rec_off, the BAM bytes, the keys with their redo and same_qname bits, counts and stats are equal -- over the
reference's SAM files, the synthetic set, the edge list, the seams of the line finder's tiles and of the lane groups,
capacity limits and mutated text.  And mgx_bgzf_store_put_device: records put from device memory are emitted as those
put from the host."""
import ctypes
import gzip
import os

import numpy as np
import pytest

from conftest import ROOT
import bam_cases as bm
import sam_cases as sc

pytestmark = pytest.mark.gpu


def vector_files():
    z = np.load(os.path.join(ROOT, "tests", "golden", "sam_vectors.npz"))
    return [(k[4:], bytes(z[k])) for k in z.files if k.startswith("sam:")]


def assert_same(dev, host, what=""):
    assert dev.line_off.tolist() == host.line_off.tolist(), what
    assert dev.line_len.tolist() == host.line_len.tolist(), what
    assert dev.rec_off.tolist() == host.rec_off.tolist(), what
    assert dev.n_declined == host.n_declined, what
    for f in host.keys.dtype.names:
        bad = np.nonzero(dev.keys[f] != host.keys[f])[0]
        assert len(bad) == 0, (what, f, bad[:5].tolist(), dev.keys[f][bad[:5]].tolist(), host.keys[f][bad[:5]].tolist())
    if dev.bam.tobytes() != host.bam.tobytes():
        d = int(np.nonzero(dev.bam != host.bam)[0][0])
        line = int(np.searchsorted(host.rec_off, d, side="right")) - 1
        raise AssertionError(f"{what}: BAM bytes differ first at {d} (line {line}, byte {d - int(host.rec_off[line])} of its record)")


@pytest.fixture(scope="module")
def enc(pkg):
    e = pkg.SamEncoder(sc.NAMES)
    yield e
    e.close()


@pytest.fixture(scope="module")
def synthetic(pkg, synth, tmp_path_factory):
    syn = bm.synthetic(synth, tmp_path_factory.mktemp("samgpu"))
    names, body = sc.sam_body(open(syn[0], "rb").read())
    return names, body, pkg.sam.encode_rules(names, body, max_lines=len(syn[3]))


def test_reference_vectors_one_submit_each(pkg):
    for name, text in vector_files():
        names, body = sc.sam_body(text)
        e = pkg.SamEncoder(names)
        host = pkg.sam.encode_rules(names, body)
        assert_same(e.encode(body), host, name)
        st = e.stats()
        assert (st["n_lines"], st["n_declined"], st["bytes_in"], st["bytes_out"]) == (len(host.keys), host.n_declined, len(body), len(host.bam)), name
        e.close()


def test_synthetic_set_one_submit(pkg, synthetic):
    names, body, host = synthetic
    e = pkg.SamEncoder(names)
    dev = e.encode(body, max_lines=len(host.keys))
    assert_same(dev, host)
    assert dev.n_declined == 0 and len(dev.keys) >= 6000
    st = e.stats()
    assert st["n_lines"] == len(host.keys) and st["bytes_out"] == len(host.bam) and st["n_tiles"] == len(body) // 16384 + 1
    assert st["ms_lines"] > 0 and st["ms_encode"] > 0 and st["ms_keys"] > 0
    e.close()


def test_submits_cut_at_every_line_end_of_a_window(pkg, synthetic):
    names, body, _ = synthetic
    off, ln = pkg.sam.lines_host(body)
    e = pkg.SamEncoder(names)
    first = 1000
    window = body[int(off[first]):int(off[first + 20])]
    b = e.batch(len(window), 20)
    for k in range(1, 21):                                           # one batch, twenty submits of growing length
        text = body[int(off[first]):int(off[first + k])]
        assert_same(b.run(text), pkg.sam.encode_rules(names, text), k)
        assert_same(b.run(text[:-1]), pkg.sam.encode_rules(names, text[:-1]), (k, "no newline"))
    b.close(); e.close()


def padded(prefix_len, newline_at, i):
    """a line that starts at prefix_len and whose '\\n' lands at offset newline_at"""
    base = sc.mk(qname=b"pad%d" % i, aux=[b"XP:Z:"])
    need = newline_at - prefix_len - len(base)
    assert need >= 0
    return base + b"p" * need + b"\n"


def seam_text(T):
    """every seam event at tile size T, each asserted where it is built"""
    seam = lambda t: (len(t) + 100) // T + 1                         # noqa: E731  the next seam with room for a padded line in front
    t = sc.ordinary(0) + b"\n"
    k = seam(t)
    t += padded(len(t), k * T - 1, 1)                                # a '\n' is the last byte of a tile
    assert t[k * T - 1:k * T] == b"\n"
    t += sc.ordinary(1) + b"\n"
    k = seam(t)
    t += padded(len(t), k * T, 2)                                    # a '\n' is the first byte of a tile
    assert t[k * T:k * T + 1] == b"\n" and len(t) == k * T + 1
    t += sc.ordinary(2) + b"\n"
    k = seam(t)
    t += padded(len(t), k * T - 1, 3)[:-1] + b"\r\n"                 # '\r' ends a tile, '\n' starts the next
    assert t[k * T - 1:k * T + 1] == b"\r\n"
    t += sc.ordinary(3) + b"\r\n"
    k = seam(t)
    start = len(t)
    t += padded(start, (k + 2) * T + 40, 4)                          # a line over three tiles (declined where longer than the staging limit)
    assert (len(t) - 1) // T - start // T >= 3
    k = seam(t)
    t += padded(len(t), k * T - 1, 5)
    t += b"\n" * (T // 2) + b"\r\n" * (T // 4)                       # a tile of empty lines only
    assert len(t) == (k + 1) * T and set(t[k * T:]) <= {10, 13}
    t += sc.ordinary(4) + b"\n"
    k = seam(t)
    t += padded(len(t), k * T - 1, 6)                                # the text ends exactly at a seam
    assert len(t) % T == 0
    return t


@pytest.mark.parametrize("tile", [256, None])
def test_tile_seams_of_the_line_finder(pkg, monkeypatch, tile):
    if tile is None:
        monkeypatch.delenv("MGX_SAM_TILE", raising=False)
    else:
        monkeypatch.setenv("MGX_SAM_TILE", str(tile))
    T = tile or 16384
    text = seam_text(T)
    e = pkg.SamEncoder(sc.NAMES)
    for name, t in (("ends at a seam", text), ("ends without a newline", text[:-1]), ("a last line without newline", text + sc.ordinary(9)),
                    ("ends in CR", text[:-1] + b"\r"), ("one byte into a tile", text + b"\n")):
        host = pkg.sam.encode_rules(sc.NAMES, t)
        assert_same(e.encode(t, max_lines=len(host.keys)), host, (T, name))
        assert e.stats()["n_tiles"] == len(t) // T + 1
    monkeypatch.setenv("MGX_SAM_TILE", "300")
    with pytest.raises(pkg.MgxError, match="MGX_SAM_TILE"):
        e.encode(b"x\n")
    e.close()


@pytest.fixture(scope="module")
def long_body(pkg, synthetic):
    """the synthetic alignment text, repeated until it has more than 4097 lines and 4096 tiles of 256 bytes, and its line starts"""
    names, body, _ = synthetic
    off, _ = pkg.sam.lines_host(body)
    while len(off) <= 4097 or len(body) < 4096 * 256:
        body = body + body
        off, _ = pkg.sam.lines_host(body)
    return names, body, off


@pytest.mark.parametrize("count", [4095, 4096, 4097])
def test_line_counts_at_the_seams_of_the_record_scan(pkg, long_body, count):
    """4096 sizes are one workgroup's chunk of the scan over the records: the chunk one short, met and passed, with max_lines
    (the scan's bound) equal to the count; one line more than max_lines is E2BIG"""
    names, body, off = long_body
    text = body[:int(off[count])]
    host = pkg.sam.encode_rules(names, text, max_lines=count)
    assert len(host.keys) == count
    e = pkg.SamEncoder(names)
    assert_same(e.encode(text, max_lines=count), host, count)
    with pytest.raises(pkg.MgxError, match="-7"):                    # E2BIG
        e.encode(text, max_lines=count - 1)
    e.close()


@pytest.mark.parametrize("tiles,rest", [(4095, 255), (4096, 0), (4097, 1)])
def test_tile_counts_at_the_seams_of_the_tile_scan(pkg, monkeypatch, long_body, tiles, rest):
    """the scan over the tiles' counts at its chunk of 4096: text cut at a line end and padded with newlines (which the line
    finder skips) to a byte length that gives exactly that many tiles of 256 bytes"""
    monkeypatch.setenv("MGX_SAM_TILE", "256")
    names, body, off = long_body
    n = (tiles - 1) * 256 + rest
    assert n // 256 + 1 == tiles and n <= len(body)
    cut = int(off[np.searchsorted(off, n, side="right") - 1])        # the last line start at or before n: the text ends in front of it
    text = body[:cut] + b"\n" * (n - cut)
    assert len(text) == n
    host = pkg.sam.encode_rules(names, text)
    assert len(host.keys) > 1000
    e = pkg.SamEncoder(names)
    assert_same(e.encode(text, max_lines=len(host.keys)), host, tiles)
    assert e.stats()["n_tiles"] == tiles
    e.close()


def test_edge_list_and_lane_group_seams(pkg, enc):
    edges = sc.edge_lines()
    mixed = []
    for i, (label, line) in enumerate(edges):
        mixed += [sc.ordinary(i), line]
    mixed.append(sc.ordinary(999))
    text = sc.framed(mixed)
    host = pkg.sam.encode_rules(sc.NAMES, text)
    dev = enc.encode(text, max_lines=len(host.keys))
    assert_same(dev, host)
    by_label = {label: 2 * i + 1 for i, (label, _) in enumerate(edges)}
    size = np.diff(host.rec_off.astype(np.int64))
    # the staging limit: at it encoded, one byte over it declined, and the line behind it unharmed (assert_same above)
    assert size[by_label["stage-1"]] > 0 and size[by_label["stage+0"]] > 0 and size[by_label["stage+1"]] == 0 and size[by_label["stage+1"] + 1] > 0
    assert all(size[by_label[f"lseq{n}"]] > 0 for n in (127, 128, 129, 255, 256, 257)) and all(size[by_label[f"Z{n}"]] > 0 for n in (7, 8, 9, 127, 128, 129))
    b = enc.batch(max(len(l) for _, l in edges) + 2, 4)
    for label, line in edges:                                        # each alone
        assert_same(b.run(line + b"\n"), pkg.sam.encode_rules(sc.NAMES, line + b"\n"), label)
    b.close()


def test_empty_input_newlines_only_and_one_line(pkg, enc):
    for text in (b"", b"\n", b"\n\n\r\n\n", b"\r", sc.ordinary(1), sc.ordinary(1) + b"\n", b"\n" + sc.ordinary(1) + b"\r\n", b"x", b"x\n"):
        host = pkg.sam.encode_rules(sc.NAMES, text)
        assert_same(enc.encode(text), host, text[:20])
        assert_same(enc.encode(text, max_lines=len(host.keys)), host, text[:20])


def test_max_records_met_and_exceeded(pkg, enc):
    lines = [sc.ordinary(i) for i in range(40)]
    text = sc.framed(lines)
    b = enc.batch(len(text), 40)
    host = pkg.sam.encode_rules(sc.NAMES, text)
    assert_same(b.run(text), host, "exactly met")
    b.close()
    b = enc.batch(len(text), 39)
    with pytest.raises(pkg.MgxError, match="-7"):                    # E2BIG
        b.run(text)
    short = sc.framed(lines[:39])
    assert_same(b.run(short), pkg.sam.encode_rules(sc.NAMES, short), "after E2BIG")
    b.close()
    with pytest.raises(pkg.MgxError, match="-7"):
        enc.encode(text, max_lines=40, out_capacity=len(host.bam) - 1)
    assert_same(enc.encode(text, max_lines=40, out_capacity=len(host.bam)), host, "room exactly")


def test_mutated_text_is_declined_not_mangled_and_nothing_is_written_past_the_total(pkg, enc):
    """Damaged text as a user can produce it: the device equals the rules (lines are declined, not mangled), and of the
    device buffer for the records only the bytes the scan counted are written: the rest, and 16 guard bytes behind its
    capacity, keep the pattern they were filled with."""
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipMemset.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t]
    hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    rng = np.random.RandomState(12)
    base = sc.framed([sc.ordinary(i) for i in range(8)] + sc.random_lines(rng, 8))
    cap, max_records = len(base) + 8, 40
    b = enc.batch(cap, max_records)
    room = pkg.sam.out_bound(max_records, cap) + 16
    everything = np.zeros(room, dtype=np.uint8)
    n_declined = 0
    for i in range(300):
        text = sc.mutate(rng, base)
        host = pkg.sam.encode_rules(sc.NAMES, text)
        if len(host.keys) > max_records:
            continue
        assert hip.hipMemset(b.device_records(), 0xA5, room) == 0 and hip.hipDeviceSynchronize() == 0
        dev = b.run(text)
        assert_same(dev, host, i)
        assert hip.hipMemcpy(everything.ctypes.data, b.device_records(), room, 2) == 0
        n_out = int(host.rec_off[-1])
        assert everything[:n_out].tobytes() == host.bam.tobytes() and (everything[n_out:] == 0xA5).all(), i
        n_declined += dev.n_declined
    assert n_declined > 100
    b.close()


def test_store_put_device_emits_what_put_emits(pkg, synthetic):
    names, body, _ = synthetic
    off, _ = pkg.sam.lines_host(body)
    text = body[:int(off[1500])]
    e = pkg.SamEncoder(names)
    b = e.batch(len(text), 1500)
    r = b.run(text, fetch=False)
    assert len(r.bam) == 0 and len(r.keys) == 1500 and r.n_declined == 0
    host = pkg.sam.encode_rules(names, text)
    length = (np.diff(r.rec_off.astype(np.int64)) - 4).astype(np.uint32)
    order = np.random.RandomState(3).permutation(1500).astype(np.uint32)
    dup = (np.arange(1500) % 7 == 0).astype(np.uint8)
    streams = []
    for device in (True, False):
        store = pkg.BgzfStore(e)
        at = store.put_device(b.device_records(), int(r.rec_off[-1])) if device else store.put(host.bam)
        blocks, _, uoff = store.emit(order, dup, np.uint64(at) + r.rec_off[:-1] + np.uint64(4), length)
        streams.append((gzip.decompress(blocks + pkg.bgzf.EOF_BLOCK), uoff.tolist()))
        store.close()
    assert streams[0] == streams[1] and len(streams[0][0]) == len(host.bam)
    b.close(); e.close()
