"""The seam inputs of tests/sortdedup_cases.py without a GPU: their constants equal the kernel file's, their
expectations and the numpy restatement of the marking agree with the CPU oracle bit for bit, and the host router around
the oracle reproduces the single-shard result -- the proof that what tests/test_sortdedup_seams_gpu.py expects does
not come from the code under test.  Also: the ctypes mirror of mgx_sortdedup_stats_t cannot drift from the header."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import sortdedup_cases as sc
from conftest import ROOT
from test_shard_cpu import sharded

CASES = sc.all_cases()
IDS = [c.name for c in CASES]
_WANT = {}


def oracle_of(sd_oracle, case):
    """the oracle's answer for a case, computed once"""
    if case.name not in _WANT:
        _WANT[case.name] = sd_oracle.run(case.L, case.recs)
    return _WANT[case.name]


def test_constants_equal_the_kernel_source():
    src = sc.source_constants()
    for name in ("WALK_CAP", "HUGE_RUN", "NEAR_SPAN", "IND_TILE", "TILE_KEYS", "BUILD_BLOCK", "L_PACKED_PAIR", "L_PACKED_COORD"):
        assert getattr(sc, name) == src[name], name
    assert src["NEAR_SCORE_BITS"] == 16                              # the near key's layout as `expected` restates it
    assert src["FIND_ITEMS"] * 256 == sc.TILE_KEYS == max(sc.H_EDGES)  # k_find_runs' workgroup edge is family H's


def test_every_row_of_the_threshold_table_has_a_case_on_both_sides():
    by = {c.name: c.expect for c in CASES}
    both = lambda field, names: {by[n][field] for n in names}      # noqa: E731
    assert {c.expect["n_long_near"] > 0 for c in CASES if c.name.startswith("A-near")} == {True}
    assert both("n_pipeline_runs", ("B-huge", "B-huge+1")) == {1, 2}
    assert both("near_by_position", ("B-huge", "B-huge+1", "A-near1-exact")) == {0, 1}
    assert both("bitmap_tiled", [n for n in by if n.startswith("E-")]) == {0, 1}
    fa = [n for n in by if n.startswith("F-")]
    assert {(by[n]["packed_coord"], by[n]["packed_pair"]) for n in fa} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    assert both("n_builds", fa) == {1, 2}
    assert {c.expect["n_radix_passes"] for c in sc.family_g()} == {1, 2, 3, 4}
    c = by["C-seam"]
    assert 0 < c["n_near"] < c["n_double"]


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_restatement_and_oracle_agree(case, sd_oracle):
    order, dup, counts = oracle_of(sd_oracle, case)
    assert np.array_equal(sc.restate(case.L, case.recs), dup)
    assert np.array_equal(order, np.argsort(case.recs["coord"], kind="stable").astype(np.uint32))
    assert (case.expect["n_double"], case.expect["n_single"]) == (int(counts[0]), int(counts[1]))
    assert len(case.recs) == case.expect["n_records"]


@pytest.mark.parametrize("case", [c for c in CASES if c.L < 2**32], ids=[c.name for c in CASES if c.L < 2**32])
def test_router_over_the_oracle_equals_the_single_shard(case, pkg, sd_oracle):
    want_order, want_dup, _ = oracle_of(sd_oracle, case)
    for k_shards in (2, 3):
        order, dup, _ = sharded(pkg, lambda r, k, sh: sd_oracle.run_shard(case.L, sh), case.L, case.recs, k_shards)
        assert np.array_equal(order, want_order), k_shards
        assert np.array_equal(dup, want_dup), k_shards


def test_the_ctypes_stats_struct_is_the_header_s(tmp_path, pkg):
    """a size mismatch would let the library write past the ctypes buffer"""
    st = pkg.native.SortDedupStats
    first, last = "n_near", "pad2_"
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "mgx_sortdedup.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu\\n", sizeof(mgx_sortdedup_stats_t), offsetof(mgx_sortdedup_stats_t, pad_), '
                   f'offsetof(mgx_sortdedup_stats_t, {first}), offsetof(mgx_sortdedup_stats_t, {last})); return 0; }}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    size, off_pad, off_first, off_last = map(int, subprocess.check_output([str(exe)], text=True).split())
    assert size == ctypes.sizeof(st)
    assert (off_pad, off_first, off_last) == (st.pad_.offset, getattr(st, first).offset, getattr(st, last).offset)
    assert off_pad == 92 and off_first == 96                         # the fields from before the path counters keep their offsets
    assert st._fields_[-1][0] == last and [f for f, _ in st._fields_].index(first) == [f for f, _ in st._fields_].index("pad_") + 1
