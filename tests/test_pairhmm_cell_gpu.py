"""GPU tests of the fp32 6-operation PairHMM cell (X^ = g'X as in the scaled form, Y carried as y = Y / pMY of its own
row): headline-shaped data, the whole 7-bit quality range (pMM = 0, pGAPM = 0), strip-mined reads, batch composition, and the
fp64 tier, which keeps its own forms."""
import ctypes
import os

import numpy as np
import pytest

from pairhmm_f64_cases import assert_fp64_tier_close
from pairhmm_fiveop_cases import with_qualities
from test_pairhmm_oracle import assert_log10_close

pytestmark = pytest.mark.gpu


def run(engine, d):
    b = engine.batch(d)
    b.run()
    out, used = b.results(with_flags=True)
    st = b.stats()
    b.close()
    return out, used, st


def test_headline_shape_vs_oracle(engine, oracle, synth):
    d = synth.gen_pairhmm_pairs_fast(8192, 0x5EED0001, r_range=(128, 128), h_range=(256, 256))
    want, wused = oracle.batch(d)
    out, used, _ = run(engine, d)
    assert_log10_close(out, want)
    assert (used != wused).sum() <= 4


@pytest.mark.parametrize("gcp", [(1, 127), (0, 127), (1, 3)])
def test_whole_quality_range_vs_oracle(engine, oracle, synth, gcp):
    """Qualities 0-127 in every field, ins = del = 0 on some bases; gap-continuation bytes from 1 (pYY = 0.79, the
    largest y / M ratio of the 6-operation form) upwards, or including 0 (the wavefront takes the plain form)."""
    d = synth.gen_pairhmm_pairs(6000, 0xC311 + gcp[0] + gcp[1], r_range=(1, 128), h_range=(1, 256), hap_n_rate=0.01)
    d = with_qualities(d, 7 + gcp[1], gcp=gcp)
    want, wused = oracle.batch(d)
    out, used, _ = run(engine, d)
    assert_log10_close(out, want)
    assert (used != wused).sum() <= 3


@pytest.mark.parametrize("r_range,h_range,n", [((1025, 2048), (300, 1200), 24), ((1025, 1100), (1, 60), 30)])
def test_strip_reads_with_varied_qualities(pkg, engine, oracle, synth, r_range, h_range, n):
    """Strip-mined reads: the boundary row carries (M, X^, y) and lane 0 of a later strip takes pMY of the previous
    strip's last read row."""
    d = synth.gen_pairhmm_pairs(n, 0x571 + n, r_range=r_range, h_range=h_range, random_read_rate=0.0)
    d = with_qualities(d, n, qual=(20, 45), ins=(1, 70), dele=(1, 70), gcp=(1, 40), zero_ins_del_rate=0.01)
    want, wused = oracle.batch(d)
    out, used, _ = run(engine, d)
    assert_log10_close(out, want)
    assert (used != wused).sum() <= 1
    eng64 = pkg.PairHMMEngine(0, flags=pkg.pairhmm.FORCE_DOUBLE)
    out64, used64, _ = run(eng64, d)
    eng64.close()
    assert used64.all()
    assert_log10_close(out64, want)
    assert_fp64_tier_close(d, out64, "strip kernel, forced, varied qualities")


def test_batch_composition_with_varied_qualities(engine, synth):
    """The same bits for a test case whatever else is in the batch, over every class of lane-group width and rows per
    lane, with per-base ins / del qualities that differ from row to row (pMY of the row above enters the cell)."""
    d = synth.gen_pairhmm_pairs(8000, 0xC0DE, r_range=(1, 700), h_range=(1, 400))
    d = with_qualities(d, 3, qual=(6, 60), ins=(1, 80), dele=(1, 80), gcp=(1, 60))
    full = engine.compute(d)
    rng = np.random.RandomState(1)
    for _ in range(3):
        idx = np.sort(rng.choice(8000, 1700, replace=False))
        sub = dict(d, pair_read=d["pair_read"][idx], pair_hap=d["pair_hap"][idx])
        assert np.array_equal(engine.compute(sub), full[idx])


def test_force_double_with_varied_qualities_matches_fp64_oracle(pkg, synth):
    """The fp64 tier keeps its scaled 7-operation form: FORCE_DOUBLE against the oracle's fp64 recurrence."""
    from conftest import ROOT
    d = synth.gen_pairhmm_pairs(3000, 0xD0B1, r_range=(1, 300), h_range=(1, 300), random_read_rate=0.0)
    d = with_qualities(d, 11, qual=(6, 45), ins=(6, 60), dele=(6, 60), gcp=(1, 60), zero_ins_del_rate=0.0)
    eng = pkg.PairHMMEngine(0, flags=pkg.pairhmm.FORCE_DOUBLE)
    out, used, _ = run(eng, d)
    eng.close()
    assert used.all()
    olib = ctypes.CDLL(os.path.join(ROOT, "oracle", "libpairhmm_oracle.so"))
    olib.ph_oracle_init()
    olib.ph_oracle_prob_f64.restype = ctypes.c_double
    ro, ho = d["read_off"].astype(np.int64), d["hap_off"].astype(np.int64)
    P = lambda a, o: ctypes.c_void_p(a.ctypes.data + int(o))  # noqa: E731
    log10_init = np.log10(np.ldexp(1.0, 1020))
    for i in range(0, 3000, 11):
        R, H = int(ro[i + 1] - ro[i]), int(ho[i + 1] - ho[i])
        v = olib.ph_oracle_prob_f64(R, P(d["bases"], ro[i]), P(d["qual"], ro[i]), P(d["ins"], ro[i]),
                                    P(d["dele"], ro[i]), P(d["gcp"], ro[i]), H, P(d["hap_bases"], ho[i]))
        if v == 0.0:                               # R far above H: the fp64 likelihood underflows in both
            assert out[i] == -np.inf
        else:
            assert abs(out[i] - (np.log10(v) - log10_init)) < 1e-9
