"""The sortmardup CLI on compressed SAM (BGZF inflated on the device, plain gzip with zlib on the host): the BAM and the
BAI must be byte-identical to the run on the plain text, under -z device and -z zlib, for BGZF of several levels and
block sizes, plain gzip (one member and concatenated members), BGZF followed by a plain member, no EOF block, compressed
stdin, htslib's SAM files and an input of a million records cut into many small slices; truncated, corrupt and BAM input
exits non-zero with a message."""
import gzip
import os
import subprocess
import zlib

import numpy as np
import pytest

from conftest import ROOT
from test_cli_gpu import build_cli, make_sam
import bgzf_cases as bc

pytestmark = pytest.mark.gpu


def run(args, stdin=None, env=None, timeout=600):
    res = subprocess.run([build_cli()] + args, stdin=stdin, capture_output=True, text=True, timeout=timeout,
                         env=dict(os.environ, **(env or {})))
    return res


def outputs(tmp_path, inp, mode, extra=(), stdin=False, env=None, tag="o"):
    bam = str(tmp_path / f"{tag}.bam")
    args = ["-O", bam, "-t", "4", "-z", mode] + list(extra)
    res = run(args, stdin=open(inp, "rb"), env=env) if stdin else run(args + ["-I", inp], env=env)
    assert res.returncode == 0, res.stderr
    return open(bam, "rb").read(), open(bam + ".bai", "rb").read(), res


def write(path, data):
    with open(path, "wb") as f:
        f.write(data)
    return str(path)


@pytest.fixture(scope="module")
def sam_text(tmp_path_factory, synth):
    d = tmp_path_factory.mktemp("csam")
    raw = synth.gen_sortdedup_raw(6000, 77, n_contigs=3, contig_len=200000, dup_rate=0.3)
    p = str(d / "in.sam")
    make_sam(raw, p)
    return p, open(p, "rb").read()


def variants(text):
    rng = np.random.RandomState(5)
    out = []
    for level in (1, 6, 9):
        for size in (1024, 16384, bc.MAX_IN):
            out.append((f"bgzf_l{level}_{size}", bc.bgzf(text, size=size, level=level)))
    out.append(("gzip", gzip.compress(text)))
    cuts = sorted(rng.randint(1, len(text), 6))
    parts = [text[a:b] for a, b in zip([0] + cuts, cuts + [len(text)])]
    out.append(("gzip_members", b"".join(gzip.compress(p, 6) for p in parts)))
    half = len(text) // 2
    out.append(("bgzf_then_gzip", bc.bgzf(text[:half], size=9000, eof=False) + gzip.compress(text[half:])))
    out.append(("bgzf_no_eof", bc.bgzf(text, size=20000, eof=False)))
    return out


@pytest.mark.parametrize("mode", ["device", "zlib"])
def test_compressed_inputs_give_the_same_bam_and_bai(tmp_path, sam_text, mode):
    sam, text = sam_text
    want_bam, want_bai, _ = outputs(tmp_path, sam, mode, ["-s", "200000"], tag="plain")
    for name, data in variants(text):
        inp = write(tmp_path / f"{name}.sam.gz", data)
        bam, bai, res = outputs(tmp_path, inp, mode, ["-s", "200000"], tag=name)
        assert bam == want_bam and bai == want_bai, name
        if name == "bgzf_no_eof":
            assert "no EOF block" in res.stderr
        elif name.startswith("bgzf"):
            assert "EOF" not in res.stderr, (name, res.stderr)
    # compressed stdin, BGZF and plain gzip
    for name, data in (("stdin_bgzf", bc.bgzf(text, size=16384)), ("stdin_gzip", gzip.compress(text))):
        inp = write(tmp_path / f"{name}.gz", data)
        bam, bai, _ = outputs(tmp_path, inp, mode, ["-s", "200000"], stdin=True, tag=name)
        assert bam == want_bam and bai == want_bai, name
    # batches of 256 KB compressed: about eight batches through the source's four, each reused once its text is parsed
    inp = write(tmp_path / "small_batches.sam.gz", bc.bgzf(text, size=4000, level=6))
    bam, bai, _ = outputs(tmp_path, inp, mode, ["-s", "100000"], env={"MGX_CLI_INFLATE_BATCH": str(256 << 10)}, tag="small_batches")
    assert bam == want_bam and bai == want_bai


def test_host_inflate_knob_gives_the_same_output(tmp_path, sam_text):
    sam, text = sam_text
    want_bam, want_bai, _ = outputs(tmp_path, sam, "device", tag="plain")
    inp = write(tmp_path / "in.sam.gz", bc.bgzf(text, size=4000, level=6))
    bam, bai, _ = outputs(tmp_path, inp, "device", env={"MGX_CLI_INFLATE": "host"}, tag="host")
    assert bam == want_bam and bai == want_bai


def test_htslib_sam_files_compressed(tmp_path):
    z = np.load(os.path.join(ROOT, "tests", "golden", "sam_vectors.npz"))
    n = 0
    for key in z.files:
        if not key.startswith("sam:"):
            continue
        text = bytes(z[key])
        sam = write(tmp_path / "in.sam", text)
        res = run(["-I", sam, "-O", str(tmp_path / "p.bam"), "-t", "3"])
        if res.returncode != 0:
            continue                                     # not a file the tool takes as text either (no @SQ lines)
        want = open(tmp_path / "p.bam", "rb").read(), open(tmp_path / "p.bam.bai", "rb").read()
        for name, data in (("bgzf", bc.bgzf(text, size=512)), ("gzip", gzip.compress(text))):
            inp = write(tmp_path / "in.sam.gz", data)
            res = run(["-I", inp, "-O", str(tmp_path / "c.bam"), "-t", "3"])
            assert res.returncode == 0, (key, name, res.stderr)
            assert (open(tmp_path / "c.bam", "rb").read(), open(tmp_path / "c.bam.bai", "rb").read()) == want, (key, name)
        n += 1
    assert n >= 5


def test_million_records_in_small_slices(tmp_path, pkg):
    recs, _ = pkg.synth.gen_sortdedup_packed_fast(1_000_000, 0x5EED0042, n_contigs=4, contig_len=20_000_000)
    sam = str(tmp_path / "big.sam")
    pkg.synth.write_sam_from_packed(sam, recs, n_contigs=4, contig_len=20_000_000)
    del recs
    text = open(sam, "rb").read()
    want_bam, want_bai, _ = outputs(tmp_path, sam, "device", ["-s", "1000000"], tag="plain")
    # BGZF of the text made on the device (quick at this size), blocks of 16 KB, batches of 4 MB compressed: dozens of
    # inflate batches pipeline through the source's four, every one reused many times
    comp = pkg.BgzfCompressor(0)
    blocks, _ = comp.compress(np.frombuffer(text, dtype=np.uint8), block=16384)
    comp.close()
    inp = write(tmp_path / "big.sam.gz", bytes(blocks) + bc.EOF_BLOCK)
    assert len(blocks) > 20 * (4 << 20)
    del text
    bam, bai, res = outputs(tmp_path, inp, "device", ["-s", "1000000"], env={"MGX_CLI_INFLATE_BATCH": str(4 << 20)}, tag="gz")
    n_slices = int(res.stdout.split(" slices")[0].split()[-1])
    assert n_slices > 100
    assert bam == want_bam and bai == want_bai


@pytest.mark.parametrize("threads", [1, 4])
def test_parse_error_deep_in_a_multi_batch_input_exits(tmp_path, sam_text, threads):
    """A SAM line the parser refuses, 80 % into an input of many small inflate batches: the tool exits non-zero with the
    parse error (the slices still queued hold inflate batches; the reader must not wait for them to come free)."""
    _, text = sam_text
    lines = text.split(b"\n")
    k = int(len(lines) * 0.8)
    assert not lines[k].startswith(b"@")
    lines[k] = b"broken\trecord"
    inp = write(tmp_path / "bad.sam.gz", bc.bgzf(b"\n".join(lines), size=4000, level=1))
    res = run(["-I", inp, "-O", str(tmp_path / "x.bam"), "-t", str(threads), "-s", "20000"],
              env={"MGX_CLI_INFLATE_BATCH": str(256 << 10)}, timeout=120)
    assert res.returncode == 1, (res.returncode, res.stderr[-2000:])
    assert "SAM parse error" in res.stderr and "broken" in res.stderr, res.stderr[-2000:]


def test_bad_input_exits_with_a_message(tmp_path, sam_text):
    sam, text = sam_text
    s = bc.bgzf(text, size=16384)
    cases = {
        "truncated_bgzf": s[:len(s) // 2 + 7],
        "truncated_gzip": gzip.compress(text)[:len(text) // 8],
        "bad_crc": None,
        "bam": None,
    }
    blocks, _ = bc.walk(s)
    b = bytearray(s)
    o = blocks[5][0]
    bs = int.from_bytes(s[o + 16:o + 18], "little") + 1
    b[o + bs - 8] ^= 0x10                                     # the CRC of block 5
    cases["bad_crc"] = bytes(b)
    z = np.load(os.path.join(ROOT, "tests", "golden", "sam_vectors.npz"))
    cases["bam"] = z["bin:range.bam"].tobytes()
    want = {"truncated_bgzf": "truncated", "truncated_gzip": "truncated", "bad_crc": "CRC", "bam": "BAM"}
    for name, data in cases.items():
        inp = write(tmp_path / f"{name}.gz", data)
        res = run(["-I", inp, "-O", str(tmp_path / "x.bam"), "-t", "4"])
        assert res.returncode not in (0, -6, -11, 134, 139), (name, res.returncode, res.stderr)
        assert want[name] in res.stderr, (name, res.stderr)
    # the bad CRC through host zlib as well
    res = run(["-I", str(tmp_path / "bad_crc.gz"), "-O", str(tmp_path / "x.bam")], env={"MGX_CLI_INFLATE": "host"})
    assert res.returncode == 1 and "corrupt" in res.stderr, res.stderr
