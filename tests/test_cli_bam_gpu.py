"""The sortmardup CLI on BAM input (-b: BGZF inflated, records found and keyed on the device): the BAM and the BAI must be
byte-identical to the run on the same records as SAM text, under every output mode, BGZF block size and level, through
stdin, over many small inflate batches (seam records, seam name groups), at the smallest index tile and with the host
knob; htslib's own BAM files come out sorted and marked as the oracle says; everything that is not BAM, or is broken BAM,
exits 1 with a message that names the cause."""
import gzip
import os
import struct
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from test_cli_gpu import build_cli
import bam_cases as bm
import bgzf_cases as bc
import sam_spec

pytestmark = pytest.mark.gpu
TIMEOUT = 300


def run(args, stdin=None, env=None, timeout=TIMEOUT):
    return subprocess.run([build_cli()] + args, stdin=stdin, capture_output=True, text=True, timeout=timeout, env=dict(os.environ, **(env or {})))


def outputs(tmp_path, inp, mode="device", extra=(), stdin=False, env=None, tag="o"):
    bam = str(tmp_path / f"{tag}.out.bam")                     # never the input's path: the tool unlinks its output first
    args = ["-O", bam, "-t", "4", "-z", mode] + list(extra)
    res = run(args, stdin=open(inp, "rb"), env=env) if stdin else run(args + ["-I", inp], env=env)
    assert res.returncode == 0, (tag, res.returncode, res.stderr[-3000:])
    return open(bam, "rb").read(), open(bam + ".bai", "rb").read(), res


def records_without_dup(data):
    """the record bytes of inflated BAM, the duplicate flag cleared, sorted"""
    out = []
    for r in sam_spec.decode_bam_records(data, sam_spec.decode_bam_header(data)[2]):
        b = bytearray(data[r["at"]:r["at"] + 4 + struct.unpack_from("<i", data, r["at"])[0]])
        b[19] &= 0xFB                                            # 0x400 of the flag at bytes 18-19
        out.append(bytes(b))
    return sorted(out)


def write(path, data):
    with open(path, "wb") as f:
        f.write(data)
    return str(path)


@pytest.fixture(scope="module")
def synthetic(synth, tmp_path_factory):
    return bm.synthetic(synth, tmp_path_factory.mktemp("clibam"))


@pytest.mark.parametrize("mode", ["device", "pinned", "zlib"])
def test_bam_input_gives_the_bam_and_bai_of_the_sam_run(tmp_path, synthetic, mode):
    sam, text, refs, recs, data, first, at = synthetic
    want_bam, want_bai, _ = outputs(tmp_path, sam, mode, ["-s", "200000"], tag="sam")
    if mode == "device":
        # the test encoder against the product's: the records the SAM run wrote are the encoder's, bar 0x400
        head = bm.encode_header(text, refs)
        mine = sorted(bytes(bytearray(x[:19]) + bytes([x[19] & 0xFB]) + x[20:]) for x in (bm.encode_record(r) for r in recs))
        assert records_without_dup(gzip.decompress(want_bam)) == mine and data[:first] == head
    cases = [(f"l{level}_{size}", bc.bgzf(data, size=size, level=level), ["-s", "200000"], None) for size in (1024, 16384, 65280) for level in (0, 1, 6)]
    small = {"MGX_CLI_INFLATE_BATCH": "262144"}
    blocks4k = bc.bgzf(data, size=4000, level=1)
    cases += [("batches_t1", blocks4k, ["-s", "20000", "-t", "1"], small), ("batches_t4", blocks4k, ["-s", "20000", "-t", "4"], small),
              ("tile256", bc.bgzf(data, size=16384, level=1), ["-s", "200000"], {"MGX_BAM_TILE": "256"}),
              ("tile256_batches", blocks4k, ["-s", "20000"], dict(small, MGX_BAM_TILE="256")),
              ("host", bc.bgzf(data, size=16384, level=1), ["-s", "200000"], {"MGX_CLI_BAM": "host"}),
              ("host_batches", blocks4k, ["-s", "20000"], dict(small, MGX_CLI_BAM="host")),
              ("host_inflate", blocks4k, ["-s", "20000"], dict(small, MGX_CLI_INFLATE="host"))]
    if mode != "device":
        # the output mode takes over behind the ingest: one compressed and one stored-only block shape, and every case that
        # changes how the ingest cuts and keys (many batches on 1 and 4 threads, the smallest tile, the host walk)
        cases = [c for c in cases if c[0] in ("l6_16384", "l0_65280", "batches_t1", "batches_t4", "tile256", "tile256_batches", "host_batches")]
    for name, blob, extra, env in cases:
        inp = write(tmp_path / "in.bam", blob)
        bam, bai, res = outputs(tmp_path, inp, mode, ["-b"] + extra, env=env, tag=name)
        assert bam == want_bam and bai == want_bai, name
        assert "EOF" not in res.stderr, (name, res.stderr)
    inp = write(tmp_path / "stdin.bam", bc.bgzf(data, size=16384, level=6))
    bam, bai, _ = outputs(tmp_path, inp, mode, ["-b", "-s", "200000"], stdin=True, tag="stdin")
    assert bam == want_bam and bai == want_bai
    inp = write(tmp_path / "noeof.bam", bc.bgzf(data, size=20000, level=1, eof=False))
    bam, bai, res = outputs(tmp_path, inp, mode, ["-b", "-s", "200000"], tag="noeof")
    assert bam == want_bam and bai == want_bai and "no EOF block" in res.stderr


def test_htslib_bam_files(tmp_path, sd_oracle):
    from test_cli_gpu import raw_from_recs
    z = np.load(os.path.join(ROOT, "tests", "golden", "sam_vectors.npz"))
    for key in ("bin:range.bam", "bin:colons.bam"):
        inp = write(tmp_path / "in.bam", z[key].tobytes())
        raw_bam, bai, _ = outputs(tmp_path, inp, extra=["-b"], tag="hts")
        src = gzip.decompress(z[key].tobytes())
        text, refs, p0 = sam_spec.decode_bam_header(src)
        recs = sam_spec.decode_bam_records(src, p0)
        out = gzip.decompress(raw_bam)
        otext, orefs, q0 = sam_spec.decode_bam_header(out)
        got = sam_spec.decode_bam_records(out, q0)
        assert (otext, orefs) == (text, refs) and len(got) == len(recs) > 0, key
        orecs, idx, L = sd_oracle.pack(raw_from_recs([dict(r, qual=np.asarray(r["qual"], dtype=np.uint8)) for r in recs], [r[1] for r in refs]))
        order, dup, _ = sd_oracle.run(L, orecs)
        for k, g in enumerate(got):                              # the oracle's order and duplicate flags, every field unchanged
            want = recs[idx[order[k]]]
            assert g["flag"] == want["flag"] | (0x400 if dup[order[k]] else 0), (key, k)
            assert {f: g[f] for f in g if f not in ("at", "flag")} == {f: want[f] for f in want if f not in ("at", "flag")}, (key, k)
        coord = [(g["tid"] if g["tid"] >= 0 else 1 << 30, g["pos"]) for g in got]
        assert coord == sorted(coord), key
        sam_spec.check_index(raw_bam, bai)


def test_other_accepted_inputs(tmp_path, synthetic):
    sam, text, refs, recs, data, first, at = synthetic
    inp = write(tmp_path / "in.bam", bc.bgzf(data, size=30000, level=1))
    once, once_bai, _ = outputs(tmp_path, inp, extra=["-b"], tag="once")
    # the tool's own output, fed back: the records are the same, already in order and marked
    again, again_bai, _ = outputs(tmp_path, str(tmp_path / "once.out.bam"), extra=["-b"], tag="again")
    a, b = gzip.decompress(once), gzip.decompress(again)
    assert sam_spec.decode_bam_header(a) == sam_spec.decode_bam_header(b)
    assert records_without_dup(a) == records_without_dup(b)
    sam_spec.check_index(again, again_bai)
    # a header and no record
    inp = write(tmp_path / "empty.bam", bc.bgzf(data[:first], size=500, level=6))
    bam, bai, res = outputs(tmp_path, inp, extra=["-b"], tag="empty")
    assert sam_spec.decode_bam_header(gzip.decompress(bam)) == (text, refs, first) and "0 alignment records" in res.stdout
    # a header of 2000 references over 1 KB blocks, records behind it
    many = [(f"contig_{i:05d}", 5000 + i) for i in range(2000)]
    mrecs = [bm.rec(f"r{i // 2}", flag=0x1 | (0x40 if i % 2 == 0 else 0x80 | 0x10), tid=(i * 37) % 2000, pos=(i * 13) % 4000, cigar=bm.C("3S40M")) for i in range(400)]
    mdata, mfirst, _ = bm.encode_bam("@HD\tVN:1.6\n", many, mrecs)
    assert mfirst > 30000
    inp = write(tmp_path / "many.bam", bc.bgzf(mdata, size=1024, level=6))
    bam, bai, _ = outputs(tmp_path, inp, extra=["-b"], tag="many")
    out = gzip.decompress(bam)
    assert sam_spec.decode_bam_header(out)[1] == many and len(sam_spec.decode_bam_records(out, sam_spec.decode_bam_header(out)[2])) == 400
    sam_spec.check_index(bam, bai)
    # a header that spans inflate batches (1.2 MB of text, batches of 1 MB inflated)
    long_text = "@HD\tVN:1.6\n" + "".join(f"@CO\t{i:06d} {'x' * 90}\n" for i in range(12000))
    hdata, hfirst, _ = bm.encode_bam(long_text, bm.EDGE_REFS, mrecs[:0] + [bm.rec(f"h{i // 2}", flag=0x1 | (0x40 if i % 2 == 0 else 0x80), cigar=bm.C("30M")) for i in range(100)])
    assert hfirst > (1 << 20)
    inp = write(tmp_path / "longhead.bam", bc.bgzf(hdata, size=65280, level=1))
    bam, bai, _ = outputs(tmp_path, inp, extra=["-b"], env={"MGX_CLI_INFLATE_BATCH": "262144"}, tag="longhead")
    out = gzip.decompress(bam)
    assert sam_spec.decode_bam_header(out) == (long_text, bm.EDGE_REFS, hfirst) and len(sam_spec.decode_bam_records(out, hfirst)) == 100
    # more (tiny) records in a batch than its device arrays are made for: the batch is walked on the host instead
    tiny = [dict(qname=f"t{i // 2}", flag=0, tid=0, pos=i, mapq=0, cigar=[], mtid=-1, mpos=-1, tlen=0, seq="", qual=[], aux=[]) for i in range(40000)]
    tdata, _, _ = bm.encode_bam("", bm.EDGE_REFS, tiny)
    inp = write(tmp_path / "tiny.bam", bc.bgzf(tdata, size=65280, level=1))
    bam, bai, _ = outputs(tmp_path, inp, extra=["-b"], env={"MGX_CLI_INFLATE_BATCH": "262144"}, tag="tiny")
    out = gzip.decompress(bam)
    assert len(sam_spec.decode_bam_records(out, sam_spec.decode_bam_header(out)[2])) == len(tiny)


def test_refusals(tmp_path, synthetic):
    sam, text, refs, recs, data, first, at = synthetic
    sam_text = open(sam, "rb").read()
    whole = bc.bgzf(data, size=16384, level=1)
    blocks, _ = bc.walk(whole)
    cut = blocks[len(blocks) // 2][0]                            # whole blocks, and an EOF block: the stream ends inside a record
    out_of_range = bytearray(data)
    struct.pack_into("<i", out_of_range, int(at[len(at) // 3]) + 4, len(refs))
    cases = {
        "bam_without_b": (whole, [], "BAM"),
        "sam_text": (sam_text, ["-b"], "not BAM"),
        "bgzf_sam": (bc.bgzf(sam_text, size=16384), ["-b"], "not BAM"),
        "gzip_bam": (gzip.compress(data), ["-b"], "not BAM"),
        "cut_record": (whole[:cut] + bc.EOF_BLOCK, ["-b"], "truncated"),
        "cut_block": (whole[:cut + 100], ["-b"], "truncated"),
        "cut_header": (bc.bgzf(data[:first - 3], size=100), ["-b"], "truncated"),
        "tid": (bc.bgzf(bytes(out_of_range), size=16384, level=1), ["-b"], f"tid {len(refs)} out of range"),
    }
    assert sum(isize for _, isize, _ in blocks[:len(blocks) // 2]) not in set(int(a) for a in at)      # cut_record ends inside a record
    for name, (blob, extra, msg) in cases.items():
        inp = write(tmp_path / f"{name}.in", blob)
        for stdin in (False, True):
            args = ["-O", str(tmp_path / "x.bam"), "-t", "4"] + extra
            res = run(args, stdin=open(inp, "rb")) if stdin else run(args + ["-I", inp])
            assert res.returncode == 1, (name, stdin, res.returncode, res.stderr[-2000:])
            assert msg in res.stderr, (name, stdin, res.stderr[-2000:])
    # a record longer than an inflate batch holds
    long_rec = bm.rec("long", cigar=bm.C("10M"), aux=[("XL", "Z", "L" * 60000)])
    ldata, _, _ = bm.encode_bam("", bm.EDGE_REFS, [bm.rec("a", cigar=bm.C("10M"))] + [dict(long_rec, aux=[["XL", "Z", "L" * 60000]] * 20)])
    inp = write(tmp_path / "long.bam", bc.bgzf(ldata, size=65280, level=1))
    res = run(["-b", "-I", inp, "-O", str(tmp_path / "x.bam")], env={"MGX_CLI_INFLATE_BATCH": "262144"})
    assert res.returncode == 1 and "longer than an inflate batch holds" in res.stderr, (res.returncode, res.stderr[-2000:])


@pytest.mark.parametrize("where", ["inside_a_batch", "last_record"])
def test_cg_tag_record_is_refused_by_its_offset_in_the_stream(tmp_path, where):
    """a long-CIGAR record (placeholder CIGAR + CG:B,I tag), in a slice cut in place from a batch and in the owned slice
    that carries the input's last name group: one offset, in the uncompressed stream, whichever batch holds it"""
    recs = [bm.rec(f"r{i // 2}", flag=0x1 | (0x40 if i % 2 == 0 else 0x80 | 0x10), pos=100 + i, cigar=bm.C("3S40M"), aux=[("XZ", "Z", "z" * 150)]) for i in range(6000)]
    long_cigar = bm.rec("longcigar", pos=7000, cigar=bm.C("30S100N"), l_seq=30, aux=[("CG", "BI", bm.C("10M70000N20M"))])
    k = 4500 if where == "inside_a_batch" else len(recs)
    recs.insert(k, long_cigar)
    data, _, at = bm.encode_bam("@HD\tVN:1.6\n", bm.EDGE_REFS, recs)
    assert int(at[k]) > (1 << 20) and len(data) > int(at[k]) + (1 << 18) * (where == "inside_a_batch")     # not in the first batch (1 MB inflated)
    inp = write(tmp_path / "cg.bam", bc.bgzf(data, size=16384, level=1))
    for env in ({}, {"MGX_CLI_BAM": "host"}):
        res = run(["-b", "-I", inp, "-O", str(tmp_path / "x.bam"), "-t", "4", "-s", "20000"], env=dict(env, MGX_CLI_INFLATE_BATCH="262144"), timeout=120)
        assert res.returncode == 1, (res.returncode, res.stderr[-2000:])
        assert f"offset {int(at[k])} of the uncompressed stream" in res.stderr and "CG tag" in res.stderr, res.stderr[-2000:]


@pytest.mark.parametrize("threads", [1, 4])
def test_corrupt_block_size_deep_in_a_multi_batch_input_exits(tmp_path, synthetic, threads):
    sam, text, refs, recs, data, first, at = synthetic
    o = int(at[int(len(at) * 0.8)])
    for env in ({}, {"MGX_CLI_BAM": "host"}):
        for bs in (31, -1, 40):
            bad = bytearray(data)
            struct.pack_into("<i", bad, o, bs)
            inp = write(tmp_path / "bad.bam", bc.bgzf(bytes(bad), size=4000, level=1))
            res = run(["-b", "-I", inp, "-O", str(tmp_path / "x.bam"), "-t", str(threads), "-s", "20000"], env=dict(env, MGX_CLI_INFLATE_BATCH=str(256 << 10)), timeout=120)
            assert res.returncode == 1, (bs, res.returncode, res.stderr[-2000:])
            assert f"offset {o} " in res.stderr and "corrupt" in res.stderr, (bs, res.stderr[-2000:])


def test_records_longer_than_a_block_through_every_output_mode(tmp_path):
    """Records just over one BGZF block, of about two and of more than two (a Z tag of 65 300, 131 000 and 140 000 bytes) among
    short ones: each output mode cuts them across blocks in its own way (SAMv1 4.1), holds the same stream and indexes it."""
    recs = [bm.rec(f"q{i:02d}", tid=i % 2, pos=500 + 37 * i, cigar=bm.C("30M")) for i in range(60)]
    for k, n in ((7, 65300), (30, 131000), (52, 140000)):
        recs[k]["aux"] = [["XL", "Z", "L" * n]]
    data, first, _ = bm.encode_bam("@HD\tVN:1.6\n", bm.EDGE_REFS, recs)
    inp = write(tmp_path / "long.bam", bc.bgzf(data, size=65280, level=1))
    want = sorted(bm.encode_record(r) for r in recs)             # (no flag has 0x400, and no record here is another's duplicate)
    assert sum(len(x) > 0xff00 for x in want) == 3 and sum(len(x) > 2 * 0xff00 for x in want) == 2
    streams = {}
    for mode in ("device", "pinned", "zlib"):
        bam, bai, _ = outputs(tmp_path, inp, mode, ["-b"], tag=mode)
        streams[mode] = gzip.decompress(bam)
        assert records_without_dup(streams[mode]) == want, mode
        assert all(isize <= 0xff00 for _, _, isize in sam_spec.bgzf_blocks(bam)), mode
        assert sam_spec.check_index(bam, bai) == len(recs), mode
    assert streams["device"] == streams["pinned"] == streams["zlib"] and streams["zlib"][:first] == data[:first]
