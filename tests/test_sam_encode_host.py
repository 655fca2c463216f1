"""SAM text input on the host (include/mgx_sam.h: mgx_sam_lines_host, mgx_sam_encode_rules, mgx_sam_encode_host) against
the definition of the result, samtext::parse_record_into of the command-line tool (through tests/cpp/sam_encode_driver.cpp):
encode_host gives its bytes line for line, encode_rules gives them on every line it accepts, and it declines exactly what
an independent predicate written from the documented list declines.  The same functions run as a stand-alone program under
AddressSanitizer + UBSan over the same inputs and over every truncation of the edge lines.  No device."""
import os
import struct
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import bam_cases as bm
import sam_cases as sc

PKGDIR = sc.PKGDIR


@pytest.fixture(scope="module")
def ref_lib():
    return sc.build_driver()


def vector_files():
    z = np.load(os.path.join(ROOT, "tests", "golden", "sam_vectors.npz"))
    return [(k[4:], bytes(z[k])) for k in z.files if k.startswith("sam:")]


def check_text(pkg, ref_lib, names, text, max_line=0, expect_host_ok=None):
    """both host encoders against the definition on one text -> (lines, declined flags, the rules' Encoded)"""
    lines = sc.split_lines(text)
    rec_off, ok, want = sc.reference(ref_lib, names, text)
    assert len(ok) == len(lines)
    off, ln = pkg.sam.lines_host(text)
    assert [bytes(text[int(o):int(o) + int(n)]) for o, n in zip(off, ln)] == lines
    r = pkg.sam.encode_rules(names, text, max_line=max_line, max_lines=len(lines))
    assert r.line_off.tolist() == off.tolist() and r.line_len.tolist() == ln.tolist()
    sizes = np.diff(r.rec_off.astype(np.int64))
    dec = sizes == 0
    assert r.n_declined == int(dec.sum()) and np.array_equal((r.keys["redo"] & 4) != 0, dec)
    want_dec = np.array([sc.declined(l, names, max_line or sc.MAX_LINE) for l in lines], dtype=bool)
    assert np.array_equal(dec, want_dec), [(lines[i][:120], bool(dec[i])) for i in np.nonzero(dec != want_dec)[0][:5]]
    for i in np.nonzero(~dec)[0]:
        assert ok[i], lines[i][:120]                              # what the rules accept, the parser accepts
        got = r.bam[int(r.rec_off[i]):int(r.rec_off[i + 1])].tobytes()
        assert got == want[int(rec_off[i]):int(rec_off[i + 1])].tobytes(), lines[i][:120]
        assert len(got) <= 36 + 2 * len(lines[i])
    same = [i > 0 and lines[i].split(b"\t")[0] == lines[i - 1].split(b"\t")[0] for i in range(len(lines))]
    assert r.keys["same_qname"].tolist() == [int(s) for s in same]
    if ok.all():
        h = pkg.sam.encode_host(names, text, max_lines=len(lines))
        assert h.rec_off.tolist() == rec_off.tolist() and h.bam.tobytes() == want.tobytes()
        assert not (h.keys["redo"] & 4).any()
        if not max_line:                                             # encode_host declines by the device's limit
            assert h.n_declined == r.n_declined
        acc = np.nonzero(~dec)[0]
        assert np.array_equal(h.keys[acc], r.keys[acc])
    else:
        with pytest.raises(pkg.sam.SamDataError) as e:
            pkg.sam.encode_host(names, text, max_lines=len(lines))
        assert e.value.line == int(np.nonzero(ok == 0)[0][0]) and " at: " in str(e.value)
    if expect_host_ok is not None:
        assert bool(ok.all()) == expect_host_ok
    return lines, dec, r


def test_reference_vectors(pkg, ref_lib):
    n_lines, declined = 0, []
    for name, text in vector_files():
        names, body = sc.sam_body(text)
        lines, dec, _ = check_text(pkg, ref_lib, names, body, expect_host_ok=True)
        n_lines += len(lines)
        declined += [(name, lines[i]) for i in np.nonzero(dec)[0]]
    assert n_lines == 263
    # the one line with float tags (F0:f .. F6:f; the file's B arrays are all integer); nothing else of the reference's own test files is left to the host
    assert len(declined) == 1 and declined[0][0] == "auxf#values.sam" and b"\tF0:f:-1\t" in declined[0][1], declined


def test_synthetic_set_is_encoded_whole(pkg, ref_lib, synth, tmp_path_factory):
    syn = bm.synthetic(synth, tmp_path_factory.mktemp("samhost"))
    names, body = sc.sam_body(open(syn[0], "rb").read())
    lines, dec, r = check_text(pkg, ref_lib, names, body, expect_host_ok=True)
    assert len(lines) == len(syn[3]) >= 6000 and not dec.any()
    # the keys are those of BAM input for the same records
    off = r.rec_off[:-1]
    want = pkg.bam.keys_host(r.bam, off, rules_only=True)
    got = r.keys.copy(); got["same_qname"] = 0; want["same_qname"] = 0
    assert np.array_equal(got, want)


def test_edge_list_each_alone_and_between_ordinary_lines(pkg, ref_lib):
    edges = sc.edge_lines()
    n_dec = 0
    for label, line in edges:
        for max_line in (0, sc.LONG):
            lines, dec, _ = check_text(pkg, ref_lib, sc.NAMES, line + b"\n", max_line=max_line)
            assert len(lines) == 1, label
            n_dec += int(dec[0])
    assert n_dec > 40
    mixed = []
    for i, (label, line) in enumerate(edges):
        mixed += [sc.ordinary(i), line]
    mixed.append(sc.ordinary(999))
    for max_line in (0, sc.LONG):
        check_text(pkg, ref_lib, sc.NAMES, sc.framed(mixed), max_line=max_line)
    # the same with only the lines the full parser takes: encode_host completes every declined one
    _, ok, _ = sc.reference(ref_lib, sc.NAMES, b"\n".join(mixed))
    good = [l for l, k in zip(mixed, ok) if k]
    lines, dec, _ = check_text(pkg, ref_lib, sc.NAMES, sc.framed(good) + good[0], expect_host_ok=True)      # no final newline
    assert dec.any() and not dec.all()


def test_twin_names_take_the_lowest_index(pkg):
    r = pkg.sam.encode_rules(sc.NAMES, sc.mk(rname=b"twin", rnext=b"c1") + b"\n")
    tid, = struct.unpack_from("<i", r.bam, 4)
    mtid, = struct.unpack_from("<i", r.bam, 24)
    assert (tid, mtid) == (2, 0)


def test_framing(pkg, ref_lib):
    a, b = sc.ordinary(1), sc.ordinary(2)
    for text in (b"", b"\n", b"\r\n", b"\n\n\r\n\r", b"\r", a, a + b"\n", a + b"\r\n" + b, b"\n" + a + b"\r", a + b"\r\r\n" + b + b"\n\n", b"\r\r\n", a + b"\n\r\n\n" + b):
        check_text(pkg, ref_lib, sc.NAMES, text)
    assert len(pkg.sam.lines_host(b"\r\r\n")[0]) == 1              # one CR is dropped, the other is the line


def test_size_bound_at_its_worst_cases(pkg, ref_lib):
    edges = dict(sc.edge_lines())
    for label in ("bound_cigar", "bound_Bi"):
        line = edges[label]
        r = pkg.sam.encode_rules(sc.NAMES, line, max_line=sc.LONG)
        size = int(r.rec_off[1])
        assert r.n_declined == 0 and 36 + 2 * len(line) - 64 <= size <= 36 + 2 * len(line), (label, size, len(line))
        assert pkg.sam.encode_rules(sc.NAMES, line).n_declined == 1      # too long for the device: declined under its limit


def test_random_lines_from_the_edge_list(pkg, ref_lib):
    rng = np.random.RandomState(5)
    lines = sc.random_lines(rng, 3000)
    _, dec, _ = check_text(pkg, ref_lib, sc.NAMES, sc.framed(lines))
    assert 300 < dec.sum() < 2700


def test_capacity_errors(pkg):
    text = sc.framed([sc.ordinary(i) for i in range(5)])
    with pytest.raises(pkg.MgxError, match="-7"):                  # E2BIG
        pkg.sam.encode_rules(sc.NAMES, text, max_lines=4)
    with pytest.raises(pkg.MgxError, match="-7"):
        pkg.sam.encode_rules(sc.NAMES, text, max_lines=5, out_capacity=300)
    assert len(pkg.sam.encode_rules(sc.NAMES, text, max_lines=5).keys) == 5


# ---- the same host code under AddressSanitizer + UBSan, as a program of its own ---------------------------------------
SAN_SRC = [sc.DRIVER_SRC] + [os.path.join(PKGDIR, "csrc", f) for f in ("sam_host.cpp", "mgx_common.cpp", os.path.join("cli", "sam_text.cpp"))]
SAN_ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")


@pytest.fixture(scope="module")
def san_driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("samsan") / "driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-DSAM_DRIVER_MAIN", "-I", os.path.join(ROOT, "include"), "-I", sc.CLI] + SAN_SRC + ["-o", exe])
    return exe


def run_san(exe, mode, path):
    res = subprocess.run([exe, mode, path], capture_output=True, text=True, env=SAN_ENV, timeout=900)
    assert res.returncode == 0 and "ERROR: AddressSanitizer" not in res.stderr and "runtime error" not in res.stderr, res.stdout[-2000:] + res.stderr[-4000:]
    return dict(zip(res.stdout.split()[0::2], map(int, res.stdout.split()[1::2])))


def write_cases(path, names, cases):
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(names)) + b"".join(struct.pack("<I", len(n)) + n for n in names))
        for c in cases:
            f.write(struct.pack("<I", len(c)) + c)


def test_sanitized_host_code_on_the_same_inputs(san_driver, tmp_path, synth):
    rng = np.random.RandomState(6)
    edges = [l for _, l in sc.edge_lines()]
    cases = [l + b"\n" for l in edges] + [sc.framed(sc.random_lines(rng, 500))]
    base = sc.framed([sc.ordinary(i) for i in range(6)] + sc.random_lines(rng, 6))
    cases += [sc.mutate(rng, base) for _ in range(300)]
    p = str(tmp_path / "edges.bin")
    write_cases(p, sc.NAMES, cases)
    c = run_san(san_driver, "cases", p)
    assert c["cases"] == len(cases) and c["mismatches"] == 0 and c["declined"] > 100 and c["rejected"] > 50, c
    for name, text in vector_files():
        names, body = sc.sam_body(text)
        write_cases(p, names, [body])
        c = run_san(san_driver, "cases", p)
        assert c["mismatches"] == 0 and c["rejected"] == 0, (name, c)
    syn = bm.synthetic(synth, tmp_path)
    names, body = sc.sam_body(open(syn[0], "rb").read())
    write_cases(p, names, [body])
    c = run_san(san_driver, "cases", p)
    assert c == dict(cases=1, lines=len(syn[3]), declined=0, rejected=0, mismatches=0), c


def test_sanitized_host_code_on_every_truncation(san_driver, tmp_path):
    short = [l for _, l in sc.edge_lines() if len(l) < 400]
    p = str(tmp_path / "trunc.bin")
    write_cases(p, sc.NAMES, [sc.ordinary(3) + b"\n" + l + b"\r\n" for l in short])
    c = run_san(san_driver, "trunc", p)
    assert c["cases"] == sum(len(sc.ordinary(3)) + len(l) + 4 for l in short) and c["mismatches"] == 0, c


def test_the_header_is_c99(tmp_path, pkg):
    """include/mgx_sam.h as tests/test_headers_are_c.py holds the other headers: plain C99, and a C program links with it alone"""
    pkg.native.load()
    src = tmp_path / "abi.c"
    src.write_text("""
#include "mgx_sam.h"
#include <stdio.h>
int main(void) {
    mgx_sam_table_t* t = 0; mgx_sam_stats_t st; uint64_t n = 9; (void)st;
    const uint8_t names[] = "c1"; const uint32_t off[2] = {0, 2};
    if (mgx_sam_table_create(1, names, off, &t)) return 3;
    if (mgx_sam_lines_host((const uint8_t*)"a\\n\\nb", 4, 0, 0, 0, &n) || n != 2) return 4;
    mgx_sam_table_destroy(t);
    printf("%d %llu\\n", MGX_SAM_MAX_LINE, (unsigned long long)MGX_SAM_OUT_BOUND(1, 10));
    return 0;
}
""")
    exe = tmp_path / "abi"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(src), "-L", PKGDIR, "-lmgx",
                           "-Wl,-rpath," + PKGDIR, "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.split() == ["2048", "56"], out.stdout + out.stderr
