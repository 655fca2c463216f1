"""The sortmardup CLI with MGX_CLI_SAM=device (SAM text encoded on the device, include/mgx_sam.h): BAM and BAI are
byte-identical to the default run -- the synthetic SAM as a file and on stdin, plain and BGZF-compressed, under -z device,
-z pinned and -z zlib, with one and four threads and with hundreds of small slices; with float tags added to some lines
(declined by the device, encoded by the host parser in their place); on htslib's SAM files -- and a malformed line exits 1
with the default path's message."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from test_cli_compressed_gpu import outputs, run, sam_text, write  # noqa: F401  (sam_text: the module's fixture, used here too)
import bgzf_cases as bc

pytestmark = pytest.mark.gpu

DEVICE = {"MGX_CLI_SAM": "device", "MGX_CLI_TRACE": "1"}
TRACE = re.compile(r"sam device: (\d+) lines encoded on the device, (\d+) declined")


def counts(res):
    m = TRACE.search(res.stderr)
    assert m, res.stderr[-2000:]
    return int(m.group(1)), int(m.group(2))


@pytest.mark.parametrize("mode", ["device", "pinned", "zlib"])
def test_same_bam_and_bai_as_the_default(tmp_path, sam_text, mode):  # noqa: F811
    sam, text = sam_text
    n_lines = sum(1 for l in text.split(b"\n") if l and not l.startswith(b"@"))
    gz = write(tmp_path / "in.sam.gz", bc.bgzf(text, size=16384))
    want_bam, want_bai, res = outputs(tmp_path, sam, mode, tag="default")
    assert "sam device" not in res.stderr
    assert outputs(tmp_path, sam, mode, env={"MGX_CLI_SAM": "host"}, tag="host")[:2] == (want_bam, want_bai)
    legs = [("file", sam, [], False), ("stdin", sam, [], True), ("bgzf", gz, [], False), ("bgzf_stdin", gz, [], True), ("t1", sam, ["-t", "1"], False),
            ("small_slices", sam, ["-s", "6000"], False), ("bgzf_small_slices", gz, ["-s", "6000"], False)]
    for name, inp, extra, stdin in legs:
        bam, bai, res = outputs(tmp_path, inp, mode, extra, stdin=stdin, env=DEVICE, tag=name)
        assert bam == want_bam and bai == want_bai, name
        assert counts(res) == (n_lines, 0), name
        if "small" in name:
            assert int(res.stdout.split(" slices")[0].split()[-1]) > 200


def test_declined_lines_are_encoded_by_the_host_in_their_place(tmp_path, sam_text):  # noqa: F811
    _, text = sam_text
    lines = text.split(b"\n")
    n_float = 0
    for i, l in enumerate(lines):
        if l and not l.startswith(b"@") and i % 7 == 3:
            lines[i] = l + b"\tXF:f:%d.5\tXG:B:f,1.5,-2" % (i % 9)
            n_float += 1
    n_lines = sum(1 for l in lines if l and not l.startswith(b"@"))
    sam = write(tmp_path / "float.sam", b"\n".join(lines))
    for mode in ("device", "zlib"):
        want_bam, want_bai, _ = outputs(tmp_path, sam, mode, ["-s", "50000"], tag="default")
        bam, bai, res = outputs(tmp_path, sam, mode, ["-s", "50000"], env=DEVICE, tag="dev")
        assert bam == want_bam and bai == want_bai, mode
        assert counts(res) == (n_lines - n_float, n_float) and n_float > 500


def test_htslib_sam_files(tmp_path):
    z = np.load(os.path.join(ROOT, "tests", "golden", "sam_vectors.npz"))
    n = declined = 0
    for key in z.files:
        if not key.startswith("sam:"):
            continue
        sam = write(tmp_path / "in.sam", bytes(z[key]))
        res = run(["-I", sam, "-O", str(tmp_path / "p.bam"), "-t", "3"])
        dev = run(["-I", sam, "-O", str(tmp_path / "d.bam"), "-t", "3"], env=DEVICE)
        assert dev.returncode == res.returncode, (key, dev.stderr)
        if res.returncode != 0:
            assert dev.stderr.strip().splitlines()[-1] == res.stderr.strip().splitlines()[-1], key      # not a file the tool takes (no @SQ lines)
            continue
        for ext in ("", ".bai"):
            assert open(tmp_path / ("p.bam" + ext), "rb").read() == open(tmp_path / ("d.bam" + ext), "rb").read(), key
        declined += counts(dev)[1]
        n += 1
    assert n >= 5 and declined >= 1


@pytest.mark.parametrize("threads", [1, 4])
def test_a_malformed_line_exits_with_the_default_message(tmp_path, sam_text, threads):  # noqa: F811
    _, text = sam_text
    lines = text.split(b"\n")
    k = int(len(lines) * 0.8)
    lines[k] = b"broken\trecord"
    for name, data in (("plain", b"\n".join(lines)), ("bgzf", bc.bgzf(b"\n".join(lines), size=4000, level=1))):
        inp = write(tmp_path / f"bad_{name}.sam", data)
        args = ["-I", inp, "-O", str(tmp_path / "x.bam"), "-t", str(threads), "-s", "20000"]
        want = run(args, timeout=120)
        got = run(args, env={"MGX_CLI_SAM": "device"}, timeout=120)
        assert want.returncode == 1 and got.returncode == 1, (name, got.returncode, got.stderr[-2000:])
        assert got.stderr.strip().splitlines()[-1] == want.stderr.strip().splitlines()[-1] == "SAM parse error: fewer than 11 fields at: broken\trecord", (name, got.stderr[-500:])
