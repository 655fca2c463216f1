"""The LDS emission table's layout (csrc/pairhmm_etab.h) on the CPU: tests/cpp/pairhmm_etab_driver.cpp, built with -Werror under
AddressSanitizer + UBSan, prints the layout for RPL 1..16 x CODES {4, 5} x {pair, quad layout} and replays the kernels' table build
and column loads on a heap block of exactly the wavefront's bytes.  This file checks what it prints against what the kernels and the
host rely on, restated here:
  * a wavefront's table takes ceil(RPL / 2) * CODES * 512 bytes in either layout (pairhmm_plan.h's lds_bytes, test_pairhmm_plan_host.py);
  * a 16-byte read is 16-byte aligned (a misaligned ds_read_b128 stalls), and the reads of a column deliver every row once;
  * LDS banks: 64 of 4 bytes; ds_read_b128 is served in four groups of 16 lanes, {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31} and the
    same + 32, ds_read_b64 in the two halves of 32 lanes.  Within every group all dwords fall on distinct banks whatever code each
    lane asks for: the code strides are multiples of 256 bytes, so the bank does not depend on the code.
No GPU, nothing loaded into Python."""
import os
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "fast-genomic-data-processing_amd", "csrc")
B128_GROUPS = [list(range(0, 4)) + list(range(12, 16)) + list(range(20, 28)), list(range(4, 12)) + list(range(16, 20)) + list(range(28, 32))]
B128_GROUPS += [[lane + 32 for lane in g] for g in B128_GROUPS]
B64_GROUPS = [list(range(32)), list(range(32, 64))]
KEYS = [(rpl, codes, quads) for rpl in range(1, 17) for codes in (4, 5) for quads in (0, 1)]
# the fp32 kernels that exist: pick_kernel<float, 4 | 5> and the strip-mined class (64 lanes x 16 rows, five codes)
F32 = [(g, r) for g in (4, 8) for r in range(1, 9)] + [(16, r) for r in range(1, 13)] + [(64, r) for r in range(4, 17)]


@pytest.fixture(scope="module")
def layouts(tmp_path_factory):
    exe = os.path.join(str(tmp_path_factory.mktemp("pairhmm_etab")), "pairhmm_etab_san")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                           "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "pairhmm_etab_driver.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1")
    res = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=600)
    assert res.returncode == 0 and not res.stderr, res.stdout[-1000:] + res.stderr[-4000:]
    out = dict(layout={}, reads={}, off={}, sim={}, cls={})
    for ln in res.stdout.splitlines():
        kind, *v = ln.split()
        v = [int(x) for x in v]
        key = tuple(v[:3])
        if kind == "layout":
            out["layout"][key] = dict(bytes=v[3], n_reads=v[4], n_quads=v[5])
        elif kind == "read":
            out["reads"].setdefault(key, []).append(dict(k=v[3], offset=v[4], bytes=v[5], code_stride=v[6], row0=v[7]))
        elif kind == "off":
            out["off"][key + (v[3], v[4])] = v[5:]
        elif kind == "sim":
            out["sim"][key] = v[3]
        elif kind == "class":
            out["cls"][key] = v[3]
    return out


def test_driver_covers_every_layout(layouts):
    assert sorted(layouts["layout"]) == sorted(KEYS) == sorted(layouts["sim"])
    assert all(bad == 0 for bad in layouts["sim"].values())          # the kernels' stores and loads, replayed: every value where it belongs


@pytest.mark.parametrize("rpl,codes,quads", KEYS)
def test_offsets_are_injective_and_inside(layouts, rpl, codes, quads):
    size = -(-rpl // 2) * codes * 512
    assert layouts["layout"][(rpl, codes, quads)]["bytes"] == size and size % 16 == 0
    seen = set()
    for row in range(2 * -(-rpl // 2)):
        for code in range(codes):
            offs = layouts["off"][(rpl, codes, quads, row, code)]
            assert len(offs) == 64
            for o in offs:
                assert 0 <= o and o + 4 <= size and o % 4 == 0
            seen.update(offs)
    assert len(seen) == 2 * -(-rpl // 2) * codes * 64 == size // 4      # injective, and no byte is left over


@pytest.mark.parametrize("rpl,codes,quads", KEYS)
def test_read_list(layouts, rpl, codes, quads):
    L, reads = layouts["layout"][(rpl, codes, quads)], layouts["reads"][(rpl, codes, quads)]
    assert [r["k"] for r in reads] == list(range(L["n_reads"]))
    assert L["n_quads"] == (rpl // 4 if quads else 0) and L["n_reads"] == -(-rpl // 2) - L["n_quads"]
    assert [r["bytes"] for r in reads] == [16] * L["n_quads"] + [8] * (L["n_reads"] - L["n_quads"])          # the quad tables come first
    delivered = []
    for r in reads:
        assert r["code_stride"] == 64 * r["bytes"] and r["code_stride"] % 256 == 0
        if r["bytes"] == 16:
            assert r["offset"] % 16 == 0
        for t in range(r["bytes"] // 4):
            row = r["row0"] + t
            if r["bytes"] == 16:
                assert row < rpl                                        # only full quads: a three-row quad would be read as ds_read_b96
            if row >= rpl:
                continue
            delivered.append(row)
            for code in range(codes):
                want = [r["offset"] + code * r["code_stride"] + lane * r["bytes"] + 4 * t for lane in range(64)]
                assert layouts["off"][(rpl, codes, quads, row, code)] == want
                if r["bytes"] == 16:
                    assert all((w - 4 * t) % 16 == 0 for w in want)
    assert delivered == list(range(rpl))                                # every row exactly once


@pytest.mark.parametrize("rpl,codes,quads", KEYS)
def test_bank_rule(layouts, rpl, codes, quads):
    for r in layouts["reads"][(rpl, codes, quads)]:
        groups = B128_GROUPS if r["bytes"] == 16 else B64_GROUPS
        assert sorted(lane for g in groups for lane in g) == list(range(64))
        dwords = r["bytes"] // 4
        # the bank does not depend on the code ...
        for code in range(1, codes):
            for t in range(dwords):
                row = r["row0"] + t
                a0, a = layouts["off"][(rpl, codes, quads, row, 0)], layouts["off"][(rpl, codes, quads, row, code)]
                assert [(x // 4) % 64 for x in a0] == [(x // 4) % 64 for x in a]
        # ... so one assignment of codes to lanes stands for all of them
        for g in groups:
            banks = [(layouts["off"][(rpl, codes, quads, r["row0"] + t, lane % codes)][lane] // 4) % 64 for lane in g for t in range(dwords)]
            assert len(set(banks)) == len(banks) == len(g) * dwords


def test_which_class_takes_which_layout(layouts):
    cls = layouts["cls"]
    for G, rpl in F32:
        for codes in (4, 5):
            want = rpl % 4 == 0                                          # only classes without a trailing pair table: DESIGN.md 3.2
            assert cls[(G, rpl, codes)] == int(want), (G, rpl, codes)
    assert cls[(16, 8, 4)] == 1                                          # the headline class: two quads, no pair
    assert layouts["layout"][(8, 4, 1)] == dict(bytes=8192, n_reads=2, n_quads=2)
    # the sizes the plan test fixes: RPL 3 as 4 rows, 5 and 6 as 6 rows, 8 as two quads
    assert [layouts["layout"][(r, 4, 1)]["bytes"] for r in (3, 5, 6, 8)] == [4096, 6144, 6144, 8192]
