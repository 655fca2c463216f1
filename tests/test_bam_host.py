"""BAM input on the host (include/mgx_bam.h: mgx_bam_parse_header, mgx_bam_walk_host, mgx_bam_keys_host, mgx_bam_pack_keys)
against an independent reading of the format (sam_spec) and against mgx_sortdedup_pack on the parsed arrays of the same
records.  No device."""
import gzip
import os
import struct

import numpy as np
import pytest

from conftest import ROOT
import bam_cases as bm
import sam_spec


def htslib_bams():
    z = np.load(os.path.join(ROOT, "tests", "golden", "sam_vectors.npz"))
    return [(k, gzip.decompress(z[k].tobytes())) for k in ("bin:range.bam", "bin:colons.bam")]


@pytest.fixture(scope="module")
def inputs(synth, tmp_path_factory):
    s = bm.synthetic(synth, tmp_path_factory.mktemp("bamhost"))
    return htslib_bams() + [("synthetic", s[4])]


def test_header_equals_the_spec_reading(pkg, inputs):
    for name, data in inputs:
        assert pkg.bam.parse_header(data) == sam_spec.decode_bam_header(data), name
    # trailing NULs of the text are dropped, the reference list is the binary one (the text may disagree)
    data = bm.encode_header("@SQ\tSN:other\tLN:5\n\0\0\0", [("chrA", 7)])
    assert pkg.bam.parse_header(data) == ("@SQ\tSN:other\tLN:5\n", [("chrA", 7)], len(data))


def test_header_partial_for_every_prefix(pkg):
    data = bm.encode_header("@HD\tVN:1.6\n", [("chrA", 100000), ("b", 5), ("chrLongerName", 1 << 30)])
    want = sam_spec.decode_bam_header(data)
    for n in range(len(data)):
        assert pkg.bam.parse_header(data[:n]) is None, n
    assert pkg.bam.parse_header(data) == want
    assert pkg.bam.parse_header(data + b"\x10\0\0") == want      # what follows the header is not looked at


def test_header_with_2000_references(pkg):
    refs = [(f"contig_{i:05d}_{'x' * (i % 40)}", 1000 + i) for i in range(2000)]
    data = bm.encode_header("@HD\tVN:1.6\n", refs) + b"rest"
    text, got, first = pkg.bam.parse_header(data)
    assert got == refs and first == len(data) - 4 and text == "@HD\tVN:1.6\n"
    assert pkg.bam.parse_header(data[:len(data) // 2]) is None


def test_header_errors(pkg):
    good = bm.encode_header("@HD\n", [("chrA", 10)])
    neg = struct.pack("<i", -1)
    cases = {"magic": b"BAM\x02" + good[4:], "text": b"SAM\x01" + good[4:], "short_magic": b"BA\x01",
             "l_text": good[:4] + neg + good[8:], "n_ref": good[:12] + neg + good[16:], "l_name": good[:16] + neg + good[20:],
             "l_name_0": good[:16] + struct.pack("<i", 0) + good[20:]}
    for name, data in cases.items():
        with pytest.raises(pkg.MgxError) as e:
            pkg.bam.parse_header(data)
        assert "-84" in str(e.value), (name, str(e.value))       # EILSEQ
        assert ("not BAM" in str(e.value)) == (name in ("magic", "text", "short_magic")), (name, str(e.value))


def test_walk_equals_the_spec_reading(pkg, inputs):
    for name, data in inputs:
        first = sam_spec.decode_bam_header(data)[2]
        want = [r["at"] for r in sam_spec.decode_bam_records(data, first)]
        off, nxt = pkg.bam.walk_host(data, first)
        assert off.tolist() == want and nxt == len(data), name
        assert len(off) > 0


def test_walk_at_every_cut_and_first(pkg, inputs):
    name, data = inputs[-1]
    first = sam_spec.decode_bam_header(data)[2]
    at = np.array([r["at"] for r in sam_spec.decode_bam_records(data, first)], dtype=np.int64)
    ends = np.append(at[1:], len(data))
    k = len(at) // 2
    assert ends[k + 1] - at[k] < 600                             # two record ends inside the window
    for n in range(int(at[k]) - 20, int(at[k]) + 580):
        off, nxt = pkg.bam.walk_host(data, first, n)
        cnt = int(np.searchsorted(ends, n, side="right"))       # the records that end at or before n
        assert off.tolist() == at[:cnt].tolist() and nxt == (int(ends[cnt - 1]) if cnt else first), n
    for f in (int(at[0]), int(at[7]), int(at[-1])):
        off, nxt = pkg.bam.walk_host(data, f)
        assert off.tolist() == at[at >= f].tolist() and nxt == len(data)
    for f in (len(data), len(data) + 1, len(data) + 1000):
        off, nxt = pkg.bam.walk_host(data, f)
        assert len(off) == 0 and nxt == f
    off, nxt = pkg.bam.walk_host(b"", 0)
    assert len(off) == 0 and nxt == 0


def test_walk_names_the_corrupt_record_and_its_rule(pkg, inputs):
    name, data = inputs[-1]
    first = sam_spec.decode_bam_header(data)[2]
    data = data[:first + 20000]
    at = pkg.bam.walk_host(data, first)[0].tolist()
    k = len(at) // 2
    o = at[k]
    l_qn = data[o + 12]
    edits = {"block_size is not": (o, struct.pack("<i", 31)), "block_size is not ": (o, struct.pack("<i", -5)), "l_read_name is 0": (o + 12, b"\0"),
             "l_seq is negative": (o + 20, struct.pack("<i", -1)), "longer than block_size": (o, struct.pack("<i", 40)),
             "does not end with NUL": (o + 36 + l_qn - 1, b"x")}
    for msg, (p, b) in edits.items():
        bad = bytearray(data)
        bad[p:p + len(b)] = b
        with pytest.raises(pkg.bam.BamDataError) as e:
            pkg.bam.walk_host(bytes(bad), first)
        assert f"offset {o}:" in str(e.value) and msg.strip() in str(e.value), (msg, str(e.value))
        assert e.value.n_records == k and e.value.next == o


def check_pack(pkg, refs, recs, data, first):
    off, nxt = pkg.bam.walk_host(data, first)
    assert len(off) == len(recs) and nxt == len(data)
    keys = pkg.bam.keys_host(data, off)
    assert not keys["redo"].any()
    tl = [ln for _, ln in refs]
    got = pkg.bam.pack_keys(keys, tl)
    want = pkg.sortdedup.pack(bm.raw_arrays(recs, tl))
    assert got[0].tobytes() == want[0].tobytes() and np.array_equal(got[1], want[1]) and got[2] == want[2]
    assert [int(e) for e in keys["end"]] == [sam_spec.ref_span(r)[1] for r in recs]
    same = [int(i > 0 and recs[i]["qname"] == recs[i - 1]["qname"]) for i in range(len(recs))]
    assert keys["same_qname"].tolist() == same
    return keys, got


def test_keys_and_pack_equal_sortdedup_pack_on_the_synthetic_set(pkg, synth, tmp_path):
    _, _, refs, recs, data, first, _ = bm.synthetic(synth, tmp_path)
    keys, (packed, _, _) = check_pack(pkg, refs, recs, data, first)
    assert (packed["mate"] != 0xFFFFFFFF).sum() > 1000 and (keys["y"] != 0).any()


def test_keys_and_pack_on_the_htslib_sam_files(pkg):
    z = np.load(os.path.join(ROOT, "tests", "golden", "sam_vectors.npz"))
    n = 0
    for key in z.files:
        if not key.startswith("sam:"):
            continue
        text, refs, recs = sam_spec.parse_sam_text(bytes(z[key]).decode())
        if not refs:
            assert key == "sam:ce#unmap.sam"                     # the one file without @SQ lines
            continue
        data, first, _ = bm.encode_bam(text, refs, recs)
        check_pack(pkg, refs, recs, data, first)
        n += 1
    assert n == 13


def test_keys_and_pack_on_the_edge_list(pkg):
    recs = bm.edge_records()
    data, first, _ = bm.encode_bam("@HD\tVN:1.6\n", bm.EDGE_REFS, recs)
    keys, (packed, idx, _) = check_pack(pkg, bm.EDGE_REFS, recs, data, first)
    by_name = {recs[int(idx[k])]["qname"]: packed[k] for k in range(len(recs)) if recs[int(idx[k])]["flag"] == 0}
    assert by_name["m:1:fc:2:1101:+15:2000"]["x"] == 15 and by_name["m:1:fc:2:1101:1500:99999999999999999999"]["y"] == 0xFFFF      # strtol's answers
    assert by_name["m:1:fc:2:1101:1500:1234567890123456789"]["y"] == 1234567890123456789 & 0xFFFF
    assert by_name["m:1:fc:2:1101:1500:123456789012345678"]["y"] == 123456789012345678 & 0xFFFF
    assert (keys["score"] == (2000 * 40) & 0xFFFF).any()
    # tid >= n_ref is an error, and so is a key still marked redo
    with pytest.raises(pkg.MgxError, match="tid 1 out of range"):
        pkg.bam.pack_keys(keys, [100000])
    marked = keys.copy(); marked["redo"][3] = 1
    with pytest.raises(pkg.MgxError, match="redo"):
        pkg.bam.pack_keys(marked, [100000, 50000])


def test_long_cigar_placeholder_with_a_cg_tag_is_refused(pkg):
    plain = bm.rec("r1", cigar=bm.C("30S100N"), l_seq=30)
    tagged = bm.rec("r2", cigar=bm.C("30S100N"), l_seq=30, aux=[("NM", "C", 3), ("XZ", "Z", "text"), ("CG", "BI", [10 << 4, 5 << 4 | 2])])
    other = bm.rec("r3", cigar=bm.C("30S100N"), l_seq=30, aux=[("CG", "Bs", [1, 2]), ("XB", "Bf", [1.5])])       # not B,I: not the long-CIGAR tag
    data, first, at = bm.encode_bam("", bm.EDGE_REFS, [plain, other])
    assert not pkg.bam.keys_host(data, at)["redo"].any()
    data, first, at = bm.encode_bam("", bm.EDGE_REFS, [plain, tagged])
    with pytest.raises(pkg.MgxError) as e:
        pkg.bam.keys_host(data, at)
    assert f"offset {int(at[1])}" in str(e.value) and "CG" in str(e.value)


def test_pack_keys_on_several_threads(pkg, synth, tmp_path, monkeypatch):
    """From 200 000 records on the pairing loop cuts the input at name-group boundaries for several threads."""
    _, _, refs, recs, data, first, _ = bm.synthetic(synth, tmp_path)
    monkeypatch.setenv("MGX_PACK_THREADS", "5")
    big = data + data[first:] * 16
    off, nxt = pkg.bam.walk_host(big, first)
    assert len(off) == 17 * len(recs) > 200000
    keys = pkg.bam.keys_host(big, off)
    tl = [ln for _, ln in refs]
    got = pkg.bam.pack_keys(keys, tl)
    raw = bm.raw_arrays(recs, tl)
    rep = dict(raw, n_records=17 * len(recs))
    for k in ("flag", "tid", "pos", "cigar", "qual", "qname"):
        rep[k] = np.tile(raw[k], 17)
    for k in ("cigar_off", "qual_off", "qname_off"):
        o = raw[k].astype(np.uint64)
        rep[k] = np.concatenate([o[:-1] + np.uint64(i) * o[-1] for i in range(17)] + [np.array([17 * int(o[-1])], dtype=np.uint64)])
    want = pkg.sortdedup.pack(rep)
    assert got[0].tobytes() == want[0].tobytes() and np.array_equal(got[1], want[1]) and got[2] == want[2]


@pytest.mark.parametrize("kw", [dict(tile=256, k=0), dict(tile=256, k=1), dict(tile=256, k=12), dict(tile=256, k=12, every=2),
                                dict(tile=256, k=3, leak=True), dict(tile=256, k=3, lead=255), dict(tile=256, k=12, lead=251, leak=True),
                                dict(tile=16384, k=5), dict(tile=16384, k=3, leak=True)], ids=lambda kw: "-".join(f"{k}{v}" for k, v in kw.items()))
def test_dependent_decoy_layout(pkg, kw):
    """The inputs of the device index's repair-round tests (test_bam_gpu.py): the builder asserts, by the guess rule
    restated in Python, that exactly the decoy tiles guess a fake and that the walk from it misses the true chain; here the
    host walk finds the records the builder laid down, so the bytes are a valid chain and the fakes are not on it."""
    refs, data, first, at, decoys = bm.dependent_decoys(**kw)
    assert len(decoys) == kw["k"] and decoys == sorted(set(decoys))
    off, nxt = pkg.bam.walk_host(data, first)
    assert np.array_equal(off, at) and nxt == len(data)
    assert pkg.bam.parse_header(data)[2] == first
    # the guess rule's restatement against the host's own validity: every true start passes it, no filler byte does
    for o in at[1:-1]:
        assert bm.guess_hit(data, len(data), int(o), len(refs))
    assert not bm.guess_hit(data, len(data), int(at[1]) + 1, len(refs))
