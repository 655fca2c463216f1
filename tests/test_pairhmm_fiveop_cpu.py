"""The five-operation fp32 PairHMM cell on the host (tools/cell_emulator.cpp, form 4): values against the oracle
within the tolerance of the GPU tests, the float-first decision, and the two deferral rules -- the static one against its
restatement in numpy, the dynamic one on a hand-made test case whose x overflows."""
import numpy as np
import pytest

from pairhmm_fiveop_cases import (DYNAMIC, FIVE, HAP_N, STATIC, THRESHOLD, emulate, has_n, overflowing_pair, static_rule,
                                  whole_quality_range)
from test_pairhmm_oracle import TOL


def against_oracle(oracle, d):
    want, wused = oracle.batch(d)
    got, used, way = emulate(d)
    f32 = (used == 0) & (wused == 0)
    err = np.abs(got[f32] - want[f32])
    print(f"n {len(want)}  fp32 in both {int(f32.sum())}  max |d log10| {err.max(initial=0.0):.3e}  ways {np.bincount(way, minlength=5).tolist()}")
    assert f32.sum() > len(want) // 2
    assert err.max(initial=0.0) <= TOL
    clear = np.isinf(want) | (np.abs(want - THRESHOLD) > 2 * TOL)
    assert np.array_equal(used[clear], wused[clear])
    return way


def test_headline_shape(oracle, synth):
    d = synth.gen_pairhmm_pairs_fast(2048, 0x5EED0001, r_range=(128, 128), h_range=(256, 256))
    way = against_oracle(oracle, d)
    assert (way == FIVE).all()


def test_every_narrow_length(oracle, synth):
    d = synth.gen_pairhmm_pairs(4000, 0x5EED0005, r_range=(1, 192), h_range=(1, 300))
    way = against_oracle(oracle, d)
    assert (way == FIVE).sum() >= 3990 and np.isin(way, (FIVE, DYNAMIC)).all()


@pytest.fixture(scope="module")
def wide(synth):
    return whole_quality_range(synth, 1500)


def test_whole_quality_range(oracle, wide):
    way = against_oracle(oracle, wide)
    assert min((way == w).sum() for w in (FIVE, STATIC, DYNAMIC, HAP_N)) > 0


def test_static_rule_fires_exactly_where_a_row_divides_by_zero(wide):
    """pMM == 0 or a gap-continuation byte of 0 in the read; a haplotype with an N is on the second launch's list anyway."""
    _, _, way = emulate(wide)
    bad, isn = static_rule(wide), has_n(wide)
    assert np.array_equal(way == HAP_N, isn)
    assert np.array_equal(way == STATIC, bad & ~isn)
    assert (bad & ~isn).sum() > 50 and (~bad & ~isn).sum() > 50      # the data holds both kinds (5 % of the bases have ins = del = 0)
    # and with gap-continuation bytes of 0 only (ins / del qualities at which pMM > 0)
    d = dict(wide, ins=np.full_like(wide["ins"], 40), dele=np.full_like(wide["dele"], 40))
    gcp = d["gcp"].copy()
    gcp[::97] = 0
    d["gcp"] = gcp
    _, _, way = emulate(d)
    bad = static_rule(d)
    assert np.array_equal(way == STATIC, bad & ~isn) and 0 < (bad & ~isn).sum() < (~isn).sum()


def test_overflow_of_x_is_deferred_and_still_right(oracle):
    d = overflowing_pair()
    want, wused = oracle.batch(d)
    got, used, way = emulate(d)
    assert way[0] == DYNAMIC
    assert wused[0] == 0 and used[0] == 0 and abs(got[0] - want[0]) <= TOL
