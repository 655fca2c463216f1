"""The device sort / mark-duplicate pipeline on the seam inputs of tests/sortdedup_cases.py (run with -m gpu): order and
duplicate flags equal the CPU oracle's bit for bit, and the path counters of mgx_sortdedup_stats_t equal what the case
expects -- so a case meant for the workgroup-per-run kernel that was quietly handled by the per-lane walk, or a fallback
that never fired, fails.  tests/test_sortdedup_seams_cpu.py shows that the expectations do not come from the device."""
import numpy as np
import pytest

import sortdedup_cases as sc
from test_shard_cpu import sharded
from test_shard_gpu import device_shard

pytestmark = pytest.mark.gpu

_WANT = {}


def oracle_of(sd_oracle, case):
    """the oracle's answer for a case, computed once"""
    if case.name not in _WANT:
        _WANT[case.name] = sd_oracle.run(case.L, case.recs)
    return _WANT[case.name]


def set_env(monkeypatch, case):
    monkeypatch.delenv(sc.ENV_EXACT, raising=False)
    for k, v in case.env.items():
        monkeypatch.setenv(k, v)


def check(engine, sd_oracle, monkeypatch, case):
    set_env(monkeypatch, case)
    want_order, want_dup, counts = oracle_of(sd_oracle, case)
    order, dup = engine.sort_mark(case.L, case.recs)
    assert np.array_equal(order, want_order), case.name
    assert np.array_equal(dup, want_dup), case.name
    st = engine.stats()
    assert (st["n_double"], st["n_single"], st["n_dup_records"]) == tuple(int(c) for c in counts), case.name
    assert {k: st[k] for k in case.expect} == case.expect, case.name


def check_sharded(pkg, engine, sd_oracle, monkeypatch, case, k_shards=3):
    set_env(monkeypatch, case)
    want_order, want_dup, _ = oracle_of(sd_oracle, case)
    order, dup, _ = sharded(pkg, device_shard(engine), case.L, case.recs, k_shards)
    assert np.array_equal(order, want_order), case.name
    assert np.array_equal(dup, want_dup), case.name


def by_name(cases):
    return dict(argvalues=cases, ids=[c.name for c in cases])


@pytest.mark.parametrize("case", **by_name(sc.family_a()))
def test_run_length_ladder(pkg, sd_engine, sd_oracle, monkeypatch, case):
    check(sd_engine, sd_oracle, monkeypatch, case)
    if case.L < 2**32:
        check_sharded(pkg, sd_engine, sd_oracle, monkeypatch, case)


@pytest.mark.parametrize("case", **by_name(sc.family_b()))
def test_huge_run_seam(sd_engine, sd_oracle, monkeypatch, case):
    check(sd_engine, sd_oracle, monkeypatch, case)


@pytest.mark.parametrize("case", **by_name(sc.family_c()))
def test_near_far_seam_and_degenerate_pairs(pkg, sd_engine, sd_oracle, monkeypatch, case):
    check(sd_engine, sd_oracle, monkeypatch, case)
    check_sharded(pkg, sd_engine, sd_oracle, monkeypatch, case)


@pytest.mark.parametrize("k", range(len(sc.family_d()) // 2), ids=[c.name for c in sc.family_d()[0::2]])
def test_bitmap_tiles(pkg, sd_engine, sd_oracle, monkeypatch, k):
    with_pairs, singles_only = sc.family_d()[2 * k], sc.family_d()[2 * k + 1]
    check(sd_engine, sd_oracle, monkeypatch, with_pairs)
    check(sd_engine, sd_oracle, monkeypatch, singles_only)       # right after it: no bit of the pairs may survive
    check_sharded(pkg, sd_engine, sd_oracle, monkeypatch, with_pairs)
    check_sharded(pkg, sd_engine, sd_oracle, monkeypatch, singles_only)


@pytest.mark.parametrize("case", **by_name(sc.family_e()))
def test_tiled_atomic_switch(pkg, sd_engine, sd_oracle, monkeypatch, case):
    check(sd_engine, sd_oracle, monkeypatch, case)
    check_sharded(pkg, sd_engine, sd_oracle, monkeypatch, case)


@pytest.mark.parametrize("case", **by_name(sc.family_f()))
def test_key_widths(sd_engine, sd_oracle, monkeypatch, case):
    check(sd_engine, sd_oracle, monkeypatch, case)


def test_key_maxima_on_either_side_of_a_byte_boundary(sd_engine, sd_oracle, monkeypatch):
    for case in sc.family_f_powers():
        check(sd_engine, sd_oracle, monkeypatch, case)


@pytest.mark.parametrize("case", **by_name(sc.family_g()))
def test_record_sort_alone(sd_engine, sd_oracle, monkeypatch, case):
    check(sd_engine, sd_oracle, monkeypatch, case)
    order, dup = sd_engine.results()
    assert np.array_equal(order, np.argsort(case.recs["coord"], kind="stable").astype(np.uint32))
    assert not dup.any()
    st = sd_engine.stats()
    assert st["n_radix_passes"] == (st["key_bits_coord"] + 7) // 8 == st["n_key_hist_launches"] + 1


@pytest.mark.parametrize("case", **by_name(sc.family_h()))
def test_run_heads_on_the_edges_of_the_run_search(sd_engine, sd_oracle, monkeypatch, case):
    check(sd_engine, sd_oracle, monkeypatch, case)


@pytest.mark.parametrize("case", **by_name(sc.family_i()))
def test_mates_that_are_not_neighbours(pkg, sd_engine, sd_oracle, monkeypatch, case):
    check(sd_engine, sd_oracle, monkeypatch, case)
    check_sharded(pkg, sd_engine, sd_oracle, monkeypatch, case)


def test_engine_reuse(pkg, sd_oracle, monkeypatch):
    """one fresh engine, input after input: the huge-run fallback and the wide keys of one input do not stick"""
    eng = pkg.SortDedupEngine(0)
    try:
        for case in sc.family_k():
            check(eng, sd_oracle, monkeypatch, case)
    finally:
        eng.close()
